"""Where the errors are, at the DATASET's own size on MI355X: boundary IoU (Cheng et al., CVPR 2021:
IoU restricted to the pixels within distance d of each mask's own contour) and trimap mIoU (mIoU
restricted to a band of width d around the ground-truth boundaries), from one fused integer kernel
over a predicted and a ground-truth label map (include/mdil_boundary.h).  Every count is exact.

    python -m mdil_ss_amd.boundary --state model_best_....pth.tar --num-classes 20 20 27 --task 0 \
        --dataset cityscapes [--cs-datadir ...] [--ratio 0.02 | --widths 1 2 4 8] --score [--json FILE] \
        [--out DIR]
    python -m mdil_ss_amd.boundary --pred MAPS --num-classes 20 20 27 --task 0 --dataset cityscapes --score

The prediction is the full-size label map of ``mdil_ss_amd.fullres`` (``--state``), or the
``<stem>_label.png`` files in train ids that ``predict`` / ``fullres`` / ``ensemble`` wrote
(``--pred DIR``: this is how an ensemble's maps get a boundary score).  ``--ratio R`` is the
published metric: one width d = max(1, round(R * diagonal)) per image size; ``--widths`` are
absolute pixels.  ``--out`` writes ``<stem>_boundary.png``: the band of the ground truth, green
where the prediction is right and red where it is wrong, over grey."""
import functools
import math
import os

import torch

from . import _boundary_lib
from . import _head_common as hc
from . import _labelsize_common as ls
from . import _report_common as rc
from ._labelsize_common import read_label_png  # noqa: F401  (public here)
from .fullres import iou_rule

_FN, _PATH = "boundary_count", "boundary"
_chk = functools.partial(hc.chk, _FN, _PATH)
COUNTERS = ("target_hist", "pred_hist", "both_hist", "confusion", "bad_targets", "bad_preds")
DEFAULT_RATIO = 0.02


def check_widths(widths):
    """-> the widths as a list of ints: 1 to 8 strictly increasing integers in [1, 128]."""
    try:
        w = [int(v) for v in widths]
    except (TypeError, ValueError):
        raise RuntimeError(f"mdil {_FN}: widths must be integers, got {widths!r}") from None
    if not 1 <= len(w) <= _boundary_lib.MAX_WIDTHS:
        raise RuntimeError(f"mdil {_FN}: {len(w)} widths (supported: 1 to {_boundary_lib.MAX_WIDTHS})")
    if any(v < 1 or v > _boundary_lib.MAX_WIDTH for v in w) or any(b <= a for a, b in zip(w, w[1:])):
        raise RuntimeError(f"mdil {_FN}: widths must be strictly increasing within [1, {_boundary_lib.MAX_WIDTH}], "
                           f"got {w}")
    return w


def ratio_width(ratio, height, width):
    """The published band width of an image: max(1, round(ratio * diagonal))."""
    d = max(1, int(round(ratio * math.sqrt(height * height + width * width))))
    if d > _boundary_lib.MAX_WIDTH:
        raise RuntimeError(f"mdil boundary: ratio {ratio} of a {height} x {width} image is a width of {d} pixels "
                           f"(supported: up to {_boundary_lib.MAX_WIDTH}); give a smaller ratio or absolute widths")
    return d


def new_counters(nc, nb, dev):
    """The six int64 counters of ``boundary_count`` for ``nc`` classes and ``nb`` bins, zeroed, on ``dev``."""
    shapes = counter_shapes(nc, nb)
    return {k: torch.zeros(shapes[k], dtype=torch.int64, device=dev) for k in COUNTERS}


def counter_shapes(nc, nb):
    return {"target_hist": (nc, nb), "pred_hist": (nc, nb), "both_hist": (nc, nb), "confusion": (nb, nc, nc),
            "bad_targets": (1,), "bad_preds": (1,)}


def workspace_bytes(N, H, W):
    need = _boundary_lib.load().mdil_boundary_workspace_bytes(N, H, W)
    if need < 0:
        raise RuntimeError(f"mdil {_FN}: maps [{N},{H},{W}] are outside the supported sizes (H, W up to "
                           f"{_boundary_lib.MAX_SIZE}, 2^40 pixels)")
    return need


def boundary_count(pred, target, nc, widths, *, ignore_index=-1, counters, workspace=None, dist=False):
    """Counts the pixels of ``pred`` and ``target`` (u8 [N,H,W] label maps on the device, train ids)
    INTO ``counters`` -- a dict of the six int64 device tensors of ``new_counters(nc, len(widths) + 1,
    device)``, accumulated into, never cleared -- by class and by the bin of their distance to the
    contour of their own region (include/mdil_boundary.h), on the current stream.
    ``workspace``: u8, at least ``workspace_bytes(N, H, W)`` bytes on the device (allocated when None).
    -> (dist_pred, dist_target): u8 [N,H,W] with min(d, widths[-1] + 1), or (None, None) without ``dist``."""
    import ctypes as C
    lib = _boundary_lib.load()
    _chk(pred, "pred", torch.uint8)
    _chk(target, "target", torch.uint8)
    if pred.dim() != 3 or pred.numel() == 0 or pred.shape != target.shape or pred.device != target.device:
        raise RuntimeError(f"mdil {_FN}: expects two uint8 label maps [N,H,W] of one size on one device (got pred "
                           f"{tuple(pred.shape)} on {pred.device}, target {tuple(target.shape)} on {target.device})")
    nc = int(nc)
    if not _boundary_lib.MIN_CLASSES <= nc <= _boundary_lib.MAX_CLASSES:
        raise RuntimeError(f"mdil {_FN}: {nc} classes (supported: {_boundary_lib.MIN_CLASSES} to "
                           f"{_boundary_lib.MAX_CLASSES})")
    w = check_widths(widths)
    hc.check_ignore_index(_FN, ignore_index)
    N, H, W = pred.shape
    c = rc.check_counters(_FN, counters, COUNTERS)
    missing = [k for k in COUNTERS if c[k] is None]
    if missing:
        raise RuntimeError(f"mdil {_FN}: counters {missing} are missing; all of {list(COUNTERS)} are needed (int64, on "
                           "the device; they are accumulated into)")
    shapes = counter_shapes(nc, len(w) + 1)
    hc.check_tables(_FN, _PATH, pred.device, torch.int64, tuple((c[k], k, shapes[k]) for k in COUNTERS))
    need = workspace_bytes(N, H, W)
    with torch.no_grad(), torch.cuda.device(pred.device):
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=pred.device)
        else:
            _chk(workspace, "workspace", torch.uint8)
            if workspace.device != pred.device or workspace.numel() < need:
                raise RuntimeError(f"mdil {_FN}: workspace must hold {need} bytes on {pred.device} (got "
                                   f"{workspace.numel()} on {workspace.device})")
        dp = torch.empty_like(pred) if dist else None
        dt = torch.empty_like(pred) if dist else None
        _boundary_lib.check(
            lib.mdil_boundary_count(pred.data_ptr(), target.data_ptr(), N, H, W, nc, (C.c_int * len(w))(*w), len(w),
                                    int(ignore_index), workspace.data_ptr(), workspace.numel(), hc.ptr(dp), hc.ptr(dt),
                                    *(c[k].data_ptr() for k in COUNTERS),
                                    torch.cuda.current_stream(pred.device).cuda_stream),
            "mdil_boundary_count")
    return dp, dt


def score(counters, nc, ignore_index, widths):
    """The report of int64 host counters (the shapes of ``counter_shapes``): per width the boundary
    IoU -- B / (T + P - B + 1e-15) on the histograms summed over the bins up to that width -- and the
    trimap mIoU -- the ``iouEval`` rule on the confusion matrices summed likewise --, then the
    interior mIoU (the last bin alone) and the ordinary mIoU (every bin).  Float64 on the host; the
    ignore class is left out exactly as ``fullres.ConfusionMeter.iou`` leaves it out."""
    rule = functools.partial(iou_rule, nc, ignore_index)
    T, P, B = (counters[k].double().cumsum(1) for k in ("target_hist", "pred_hist", "both_hist"))
    conf = counters["confusion"].double()
    C = conf.cumsum(0)

    def of_matrix(m):
        return rule(m.diagonal(), m.sum(0), m.sum(1))

    def entry(pair):
        return {"mean": float(pair[0]), "classes": [float(v) for v in pair[1]]}

    out = {"widths": list(widths), "boundary_iou": [], "trimap_iou": []}
    for k in range(len(widths)):
        out["boundary_iou"].append(entry(rule(B[:, k], P[:, k], T[:, k])))
        out["trimap_iou"].append(entry(of_matrix(C[k])))
    out["interior_iou"] = entry(of_matrix(conf[-1]))
    full = of_matrix(C[-1])
    out.update(mIoU=float(full[0]), iou_classes=[float(v) for v in full[1]], pixels=int(conf.sum()))
    out["counters"] = {k: counters[k].tolist() for k in COUNTERS}
    return out


class BoundaryMeter:
    """Boundary IoU and trimap mIoU of full-size predictions, counted on the device by the fused
    kernel.  ``widths``: absolute band widths in pixels; ``ratio``: the published metric, one width
    per call from the maps' diagonal (two bins whose meaning is the same across image sizes);
    neither: ``ratio`` = 0.02."""

    def __init__(self, nc, ignore_index, widths=None, ratio=None):
        if widths is not None and ratio is not None:
            raise RuntimeError("mdil BoundaryMeter: give widths or ratio, not both")
        self.nc, self.ignore_index = int(nc), int(ignore_index)
        self.widths = None if widths is None else check_widths(widths)
        self.ratio = None if widths is not None else float(DEFAULT_RATIO if ratio is None else ratio)
        if self.ratio is not None and not self.ratio > 0.0:
            raise RuntimeError(f"mdil BoundaryMeter: ratio {ratio} must be positive")
        self.nb = 2 if self.widths is None else len(self.widths) + 1
        self.tensors, self.used = {}, []

    def add(self, *source, target=None, dist=False):
        """``add(pred, target)`` with two u8 [N,H,W] label maps in train ids on the device, or
        ``add(model, images, task, target=t)`` / ``add(features, weight, bias, target=t)``, which first
        run ``fullres.fullres_head`` for the label map of ``target``'s size.
        -> (pred, dist_pred, dist_target); the distance maps are None without ``dist``."""
        (pred,), target = ls.label_maps(("BoundaryMeter", _FN, _PATH), source, target)
        N, H, W = pred.shape
        widths = self.widths if self.widths is not None else [ratio_width(self.ratio, H, W)]
        if not self.tensors:
            self.tensors = new_counters(self.nc, self.nb, pred.device)
        need = workspace_bytes(N, H, W)
        ws = self.tensors.get("workspace")
        if ws is None or ws.numel() < need:
            self.tensors["workspace"] = torch.empty(need, dtype=torch.uint8, device=pred.device)
        dp, dt = boundary_count(pred, target, self.nc, widths, ignore_index=self.ignore_index,
                                counters={k: self.tensors[k] for k in COUNTERS},
                                workspace=self.tensors["workspace"], dist=dist)
        if self.widths is None and widths[0] not in self.used:
            self.used.append(widths[0])
        return pred, dp, dt

    def counters(self):
        """The six counters as int64 host tensors; raises when a target or a prediction outside
        [0, nc) (other than an ignored target) was met."""
        if not self.tensors:
            shapes = counter_shapes(self.nc, self.nb)
            return {k: torch.zeros(shapes[k], dtype=torch.int64) for k in COUNTERS}
        rc.refuse_bad_pixels("BoundaryMeter", self.nc, self.ignore_index, self.tensors["bad_targets"],
                             self.tensors["bad_preds"])
        return {k: self.tensors[k].cpu() for k in COUNTERS}

    def report(self):
        """``score`` of what was added.  With ``ratio`` the one entry of ``widths`` is None and
        ``widths_used`` lists the pixel widths the image sizes met so far gave."""
        widths = self.widths if self.widths is not None else [None]
        out = score(self.counters(), self.nc, self.ignore_index, widths)
        if self.widths is None:
            out.update(ratio=self.ratio, widths_used=sorted(self.used))
        return out


# ------------------------------------------------------------------------------------------ CLI
GREY, RIGHT, WRONG = (128, 128, 128), (0, 200, 0), (220, 0, 0)


def band_image(pred, target, dist_target, width):
    """u8 [N,H,W,3] on the device: the pixels within ``width`` of the target's contours coloured by
    whether the prediction is right, over grey."""
    band = dist_target <= width
    img = torch.tensor(GREY, dtype=torch.uint8, device=pred.device).repeat(*pred.shape, 1)
    img[band & (pred == target)] = torch.tensor(RIGHT, dtype=torch.uint8, device=pred.device)
    img[band & (pred != target)] = torch.tensor(WRONG, dtype=torch.uint8, device=pred.device)
    return img


def main(args):
    _refusals(args)
    rc.refuse_task(args.task, args.num_classes)
    dev, nc, models, folders = ls.load_predictors(args)
    meter = BoundaryMeter(nc, nc - 1, widths=args.widths, ratio=None if args.widths else args.ratio)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    data = ls.open_data(args, nc)
    with hc.png_pool() as pool:
        png = hc.PngWriter(pool, args.out)
        for run in ls.label_runs(data, pool, dev, args.batch_size, models, args.task, folders, png):
            pred, _, dt = meter.add(*run.sources, target=run.target, dist=bool(args.out))
            if args.out:
                width = meter.widths[-1] if meter.widths is not None else ratio_width(meter.ratio, *pred.shape[1:])
                run.write("_boundary.png", band_image(pred, run.target, dt, width).cpu().numpy())
    report = ls.report_header(args, data[0], png)
    report.update(meter.report())
    if args.score:
        shown = report["widths"] if meter.widths is not None else [f"{meter.ratio:g} of the diagonal"]
        print(f"{report['dataset']} (task {args.task}) at the labels' own size: mIoU {report['mIoU'] * 100:.2f} %  "
              f"interior mIoU {report['interior_iou']['mean'] * 100:.2f} %  over {report['pixels']} pixels")
        for k, w in enumerate(shown):
            print(f"width {w}: boundary IoU {report['boundary_iou'][k]['mean'] * 100:.2f} %  trimap mIoU "
                  f"{report['trimap_iou'][k]['mean'] * 100:.2f} %")
    return hc.score_report(report, None, args)


def _refusals(args):
    """Raise a RuntimeError that names why this combination of flags is refused."""
    ls.refuse_idle(args)
    ls.refuse_json_without_score(args)
    ls.refuse_sources(args)
    if args.widths is not None:
        check_widths(args.widths)
    elif not args.ratio > 0.0:
        raise RuntimeError("--ratio must be positive")
    ls.refuse_data(args)


def build_parser():
    p = ls.add_flags(hc.RefusingParser(_refusals, description="boundary IoU and trimap mIoU at the dataset's own size "
                                                              "from a checkpoint or from label maps already written"),
                     label_maps=False, required=("num_classes", "task"), pred=True,
                     out_help="write <stem>_boundary.png at the image's own size into this folder")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--ratio", type=float, default=DEFAULT_RATIO,
                   help="band width as a share of the image diagonal, the published metric (default %(default)s)")
    g.add_argument("--widths", type=int, nargs="+", help="band widths in pixels instead: 1 to 8 increasing values up "
                                                         "to 128")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
