"""Label maps refined against the image on MI355X: a local fully-connected CRF on the head's softmax
(Kraehenbuehl & Koltun 2011, truncated to a dilated window as in Teichmann & Cipolla 2018, Potts
compatibility), a fixed number of parallel mean-field steps, fused with ``output_conv`` -- the logits
are never stored and no ``[N, nc, K, H, W]`` unfold of the probabilities is ever built
(include/mdil_refine.h).

    python -m mdil_ss_amd.refine --state model_best_....pth.tar --num-classes 20 20 --task 1 \
        --images DIR --out DIR [--colour] [--confidence]
    python -m mdil_ss_amd.refine --state model_best_....pth.tar --num-classes 20 20 --task 1 \
        --dataset cityscapes --subset val --score --json FILE [--out DIR]

``--out`` writes ``<stem>_label.png`` in train ids, the files ``boundary --pred`` and ``segments --pred``
read; ``--score`` reports the mIoU of the plain argmax beside that of the refined labels.  The
default parameters are DenseCRF's usual ones carried to [0, 1] colours and a 21-pixel reach; they
have NOT been tuned on real data."""
import math
import os
from typing import NamedTuple

import torch

from . import _head_common as hc
from . import _refine_lib
from . import _report_common as rc

_FN, _PATH = "refine_head", "refinement"


class RefineParams(NamedTuple):
    """``iterations`` T mean-field steps (0: plain prediction) over a window of ``radius`` r taps at
    ``dilation`` d each way; the appearance kernel ``w_appearance`` exp(-|dp|^2 / 2 theta_alpha^2 -
    |dI|^2 / 2 theta_beta^2) and the smoothness kernel ``w_smooth`` exp(-|dp|^2 / 2 theta_gamma^2),
    each normalised by the sum of its spatial factor over the window.  Untuned defaults."""
    iterations: int = 5
    radius: int = 5
    dilation: int = 2
    w_appearance: float = 3.0
    w_smooth: float = 1.0
    theta_alpha: float = 8.0
    theta_beta: float = 0.05
    theta_gamma: float = 3.0


DEFAULTS = RefineParams()
_RANGES = (("iterations", 0, _refine_lib.MAX_ITERATIONS), ("radius", 1, _refine_lib.MAX_RADIUS),
           ("dilation", 1, _refine_lib.MAX_DILATION))


def check_params(params, fn=_FN):
    """-> a RefineParams inside the library's limits (None: the defaults)."""
    if params is None:
        return DEFAULTS
    if not isinstance(params, RefineParams):
        raise RuntimeError(f"mdil {fn}: params must be a RefineParams, got {type(params).__name__}")
    for name, lo, hi in _RANGES:
        v = getattr(params, name)
        if not isinstance(v, int) or isinstance(v, bool) or not lo <= v <= hi:
            raise RuntimeError(f"mdil {fn}: {name} {v!r} outside [{lo}, {hi}]")
    for name in ("theta_alpha", "theta_beta", "theta_gamma"):
        v = getattr(params, name)
        if not isinstance(v, (int, float)) or not math.isfinite(v) or not v > 0:
            raise RuntimeError(f"mdil {fn}: {name} {v!r} must be finite and > 0")
    for name in ("w_appearance", "w_smooth"):
        v = getattr(params, name)
        if not isinstance(v, (int, float)) or not math.isfinite(v) or not v >= 0:
            raise RuntimeError(f"mdil {fn}: {name} {v!r} must be finite and >= 0")
    return params


def workspace_bytes(N, H, W, nc, iterations):
    """Bytes of device workspace ``refine_head`` needs for features [N,H,W,16]."""
    lib = _refine_lib.load()
    need = lib.mdil_refine_workspace_bytes(int(N), int(H), int(W), int(nc), int(iterations))
    if need < 0:
        raise RuntimeError(f"mdil_refine_workspace_bytes failed: {lib.mdil_refine_last_error().decode()}")
    return need


def refine_head(features, weight, bias, image, params=None, *, want_confidence=False, want_q=False, target=None,
                ignore_index=-1, confusion=None, bad_targets=None, changed=None, workspace=None):
    """``output_conv`` + softmax + ``params.iterations`` mean-field steps guided by ``image`` + argmax,
    on NHWC decoder features [N,H,W,16], the ``ConvTranspose2d(16, nc, 2, 2)`` parameters
    (2 <= nc <= 32) and the network's own input ``image`` f32 [N,3,2H,2W] in [0, 1], on the current
    stream.  -> (label u8 [N,2H,2W], confidence f32 [N,2H,2W] or None, Q f32 [N,2H,2W,nc] or None).

    With ``target`` (u8 [N,2H,2W], device) the pixels are counted INTO ``confusion`` (i64 [2,nc,nc]:
    plane 0 the plain argmax, plane 1 the refined label; row = target) and targets >= nc other than
    ``ignore_index`` into ``bad_targets`` (i64 [1]); ``changed`` (i64 [1]) gains the pixels whose
    refined label differs from the plain one.  All three are accumulated into, never cleared.
    ``workspace``: a uint8 device tensor of at least ``workspace_bytes(...)`` (default: allocated here)."""
    lib = _refine_lib.load()
    p = check_params(params)
    for t, name in ((features, "features"), (weight, "weight"), (bias, "bias"), (image, "image")):
        hc.chk(_FN, _PATH, t, name)
    x, w, b = features, weight, bias
    nc = hc.check_params(_FN, w, b, x)
    N, H, W = x.shape[0], x.shape[1], x.shape[2]
    hc.check_classes(_FN, _refine_lib, nc, x, w, b)
    if tuple(image.shape) != (N, 3, 2 * H, 2 * W) or image.device != x.device:
        raise RuntimeError(f"mdil {_FN}: image must be float32 [{N}, 3, {2 * H}, {2 * W}] on {x.device}, the network's "
                           f"own input (got {tuple(image.shape)} on {image.device})")
    dev = x.device
    hc.check_tables(_FN, _PATH, dev, torch.uint8, ((target, "target", (N, 2 * H, 2 * W)),))
    if target is None:
        if confusion is not None or bad_targets is not None:
            raise RuntimeError(f"mdil {_FN}: confusion / bad_targets given without a target")
    elif confusion is None or bad_targets is None:
        raise RuntimeError(f"mdil {_FN}: a target needs confusion (int64 [2,nc,nc]) and bad_targets (int64 [1]) on "
                           "the device; they are accumulated into")
    hc.check_tables(_FN, _PATH, dev, torch.int64, ((confusion, "confusion", (2, nc, nc)),
                                                    (bad_targets, "bad_targets", (1,)), (changed, "changed", (1,))))
    hc.check_ignore_index(_FN, ignore_index)
    need = workspace_bytes(N, H, W, nc, p.iterations)
    if workspace is not None:
        hc.chk(_FN, _PATH, workspace, "workspace", torch.uint8)
        if workspace.device != dev or workspace.numel() < need:
            raise RuntimeError(f"mdil {_FN}: workspace must hold {need} bytes on {dev} (got {workspace.numel()} on "
                               f"{workspace.device})")
    with torch.no_grad(), torch.cuda.device(dev):
        if workspace is None and need:
            workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        label = torch.empty(N, 2 * H, 2 * W, dtype=torch.uint8, device=dev)
        conf = torch.empty(N, 2 * H, 2 * W, dtype=torch.float32, device=dev) if want_confidence else None
        q = torch.empty(N, 2 * H, 2 * W, nc, dtype=torch.float32, device=dev) if want_q else None
        _refine_lib.check(
            lib.mdil_refine_head(x.data_ptr(), w.data_ptr(), b.data_ptr(), image.data_ptr(), N, H, W, nc,
                                 p.iterations, p.radius, p.dilation, p.w_appearance, p.w_smooth, p.theta_alpha,
                                 p.theta_beta, p.theta_gamma, hc.ptr(workspace) if need else None,
                                 workspace.numel() if need else 0, label.data_ptr(), hc.ptr(conf), hc.ptr(q),
                                 hc.ptr(target), int(ignore_index), hc.ptr(confusion), hc.ptr(bad_targets),
                                 hc.ptr(changed), torch.cuda.current_stream(dev).cuda_stream),
            "mdil_refine_head")
    return label, conf, q


def refine(model, images, task, params=None, **kw):
    """Refined label (and confidence / Q) maps of ``images`` [N,3,H,W] for ``task``: the model's
    decoder features, then ``refine_head`` with that task's ``output_conv`` parameters and the
    images themselves as the guide."""
    check_params(params, "refine")
    if not isinstance(images, torch.Tensor) or not images.is_cuda:
        raise RuntimeError("mdil refine: images must be a float32 [N,3,H,W] device tensor; there is no CPU fallback "
                           f"in the {_PATH} path")
    model.eval()
    with torch.no_grad():
        feat = model.features(images, task)
        w, b = model.head_params(task)
        return refine_head(feat.contiguous(), w.detach(), b.detach(), images.contiguous(), params, **kw)


class RefineMeter:
    """Both confusion matrices (plain argmax and refined labels against one target), the targets out
    of range and the count of pixels the refinement changed, kept on the device across batches."""

    def __init__(self, nc, ignore_index):
        self.nc, self.ignore_index = int(nc), int(ignore_index)
        self.confusion = self.bad_targets = self.changed = None
        self.pixels = 0

    def add(self, model, images, task, params=None, target=None, **kw):
        """-> what ``refine`` returns for the batch; ``target`` u8 [N,H,W] on the device or None."""
        dev = images.device
        if self.changed is None:
            self.confusion = torch.zeros(2, self.nc, self.nc, dtype=torch.int64, device=dev)
            self.bad_targets = torch.zeros(1, dtype=torch.int64, device=dev)
            self.changed = torch.zeros(1, dtype=torch.int64, device=dev)
        if target is not None:
            kw.update(target=target, ignore_index=self.ignore_index, confusion=self.confusion,
                      bad_targets=self.bad_targets)
        out = refine(model, images, task, params, changed=self.changed, **kw)
        self.pixels += out[0].numel()
        return out

    def report(self):
        """-> dict: mIoU and per-class IoU (fullres.py's ``iou_rule``) of both planes, the confusion
        planes, ``changed``, ``changed_share``, ``bad_targets``, ``pixels``."""
        from .fullres import iou_rule
        planes = torch.zeros(2, self.nc, self.nc, dtype=torch.int64) if self.confusion is None else self.confusion.cpu()
        out = {"pixels": self.pixels, "changed": 0 if self.changed is None else int(self.changed.item()),
               "bad_targets": 0 if self.bad_targets is None else int(self.bad_targets.item())}
        out["changed_share"] = out["changed"] / max(1, self.pixels)
        for k, name in enumerate(("plain", "refined")):
            m = planes[k].double()
            miou, per_class = iou_rule(self.nc, self.ignore_index, m.diagonal(), m.sum(0), m.sum(1))
            out[f"mIoU_{name}"] = float(miou)
            out[f"iou_classes_{name}"] = [float(v) for v in per_class]
            out[f"confusion_{name}"] = planes[k].tolist()
        return out


# ------------------------------------------------------------------------------------------ CLI
def params_of(args):
    return RefineParams(args.iterations, args.radius, args.dilation, args.w_appearance, args.w_smooth,
                        args.theta_alpha, args.theta_beta, args.theta_gamma)


def main(args):
    _refusals(args)
    rc.refuse_task(args.task, args.num_classes)
    params = params_of(args)
    dev, nc, model = hc.load_model(args.state, args.num_classes, args.task)
    palette = None
    if args.colour:
        from .predict import default_palette
        palette = default_palette(nc).to(dev)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    meter = RefineMeter(nc, nc - 1)
    images_seen = 0
    with hc.png_pool() as pool:
        png = hc.PngWriter(pool, args.out)
        for stems, images, target in rc.image_or_dataset_batches(args, nc, pool, dev, args.score, bool(args.out)):
            label, conf, _ = meter.add(model, images, args.task, params, target, want_confidence=args.confidence)
            images_seen += len(stems)
            if not args.out:
                continue
            planes = [label.unsqueeze(3)]
            if palette is not None:
                planes.append(palette[label.long()])
            if conf is not None:
                planes.append(conf.mul(255.0).round_().nan_to_num_(0.0).clamp_(0.0, 255.0).to(torch.uint8).unsqueeze(3))
            host = (torch.cat(planes, 3) if len(planes) > 1 else planes[0]).cpu().numpy()
            png.wait()                         # the batch before this one: bounds what is in flight
            for k, stem in enumerate(stems):
                png.submit(host[k, :, :, 0], f"{stem}_label.png")
                c = 1
                if palette is not None:
                    png.submit(host[k, :, :, 1:4], f"{stem}_colour.png")
                    c = 4
                if conf is not None:
                    png.submit(host[k, :, :, c], f"{stem}_conf.png")
        png.wait()
    report = {"dataset": rc.source_name(args),
              "task": args.task, "images": images_seen, "written": png.written, "params": params._asdict()}
    scored = meter.report()
    report.update({k: scored[k] for k in ("pixels", "changed", "changed_share")})
    print(f"{report['dataset']} (task {args.task}): {images_seen} images, the refinement changed "
          f"{report['changed_share'] * 100:.2f} % of {report['pixels']} pixels")
    if args.score:
        report.update(scored)
        print(f"mIoU plain {scored['mIoU_plain'] * 100:.2f} %  refined {scored['mIoU_refined'] * 100:.2f} %  "
              f"({scored['bad_targets']} targets out of range)")
        print("per-class IoU plain:   " + " ".join(f"{v * 100:.2f}" for v in scored["iou_classes_plain"]))
        print("per-class IoU refined: " + " ".join(f"{v * 100:.2f}" for v in scored["iou_classes_refined"]))
    if args.out:
        print(f"{len(png.written)} maps written to {args.out}")
    if args.json:
        hc.write_json(report, args.json)
    return report


def _refusals(args):
    """Raise a RuntimeError that names why this combination of flags is refused."""
    if sum(bool(v) for v in (args.images, args.dataset, args.synthetic)) != 1:
        raise RuntimeError("give one source of images: --images DIR, --dataset cityscapes|BDD|IDD or --synthetic N")
    if args.score and args.images:
        raise RuntimeError("--score needs labels: give --dataset or --synthetic N, not --images")
    if args.json and not args.score:
        raise RuntimeError("--json writes the score: it needs --score")
    if not args.out and not args.score:
        raise RuntimeError("nothing to do: give --out DIR, --score or both")
    if (args.colour or args.confidence) and not args.out:
        raise RuntimeError("--colour and --confidence need --out DIR")
    if min(args.height, args.width, args.batch_size) < 1 or args.synthetic < 0:
        raise RuntimeError("sizes and --batch-size must be positive")
    check_params(params_of(args), "refine")


def build_parser():
    p = hc.RefusingParser(_refusals, description="label maps refined against the image by mean-field steps of a local "
                                                 "CRF, from a checkpoint")
    p.add_argument("--state", required=True, help="checkpoint written by the trainers (or by the reference)")
    p.add_argument("--num-classes", type=int, nargs="+", required=True)
    p.add_argument("--task", type=int, required=True, help="which task's decoder predicts")
    p.add_argument("--images", help="folder of .jpg / .png images (searched recursively)")
    rc.add_data_flags(p, dataset_help="a labelled dataset instead (for --score)",
                      synthetic_help="N procedural images instead (labelled)")
    p.add_argument("--out", help="write <stem>_label.png (8-bit train ids) here")
    p.add_argument("--colour", action="store_true", help="also write <stem>_colour.png")
    p.add_argument("--confidence", action="store_true", help="also write <stem>_conf.png = round(255 p)")
    p.add_argument("--score", action="store_true", help="mIoU of the plain and of the refined labels")
    p.add_argument("--json", help="write the report here")
    d = DEFAULTS
    p.add_argument("--iterations", type=int, default=d.iterations, help="mean-field steps, 0 to 16 (default %(default)s)")
    p.add_argument("--radius", type=int, default=d.radius, help="window taps each way, 1 to 5 (default %(default)s)")
    p.add_argument("--dilation", type=int, default=d.dilation, help="pixels between taps, 1 to 4 (default %(default)s)")
    p.add_argument("--w-appearance", type=float, default=d.w_appearance, help="default %(default)s")
    p.add_argument("--w-smooth", type=float, default=d.w_smooth, help="default %(default)s")
    p.add_argument("--theta-alpha", type=float, default=d.theta_alpha, help="appearance kernel, pixels (default %(default)s)")
    p.add_argument("--theta-beta", type=float, default=d.theta_beta, help="appearance kernel, colour in [0, 1] (default %(default)s)")
    p.add_argument("--theta-gamma", type=float, default=d.theta_gamma, help="smoothness kernel, pixels (default %(default)s)")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
