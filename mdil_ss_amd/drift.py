"""Drift report on MI355X: the model BEFORE an incremental step next to the model AFTER it, the
comparison the step-2 loss itself makes through its KD term.  Both ``output_conv``, both softmaxes,
the per-pixel KL divergence, both argmaxes, the class-transition counts and the retained /
forgotten / gained counts come from one fused kernel straight from the two decoders' 16-channel
features, so neither logit tensor is stored (include/mdil_drift.h).

    python -m mdil_ss_amd.drift --before CKPT --before-num-classes 20 \
        --after CKPT --after-num-classes 20 20 --task 0 \
        (--dataset cityscapes|BDD|IDD [--subset val] | --synthetic N) \
        [--report] [--score] [--json FILE] [--out DIR [--kl-max 1.0] [--labels]] \
        [--height 512 --width 1024 --batch-size 6]

``--report`` prints the label-free half: how often the two models agree, the mean KL divergence
(overall and per class of the "before" label), the KD loss as the step-2 trainer logs it, and the
largest class transitions.  ``--score`` brings the labels in (the validation transform, labels at
the network's size) and adds mIoU before / after by the reference's ``iouEval`` rule and the
per-class forgotten / gained rates.  ``--out`` writes ``<stem>_change.png`` (RGB, CHANGE_PALETTE
applied to the change codes), ``<stem>_kl.png`` (L, ``round(255 min(kl, kl_max) / kl_max)``) and,
with ``--labels``, ``<stem>_before_label.png`` and ``<stem>_after_label.png`` (train ids)."""
import functools
import os

import numpy as np
import torch

from . import _drift_lib
from . import _head_common as hc
from . import _report_common as rc
from .fullres import ConfusionMeter

_FN, _PATH = "drift_head", "drift"
_chk = functools.partial(hc.chk, _FN, _PATH)

# change code -> colour: 0 both right (without a target: labels equal), 1 forgotten (without a
# target: labels differ), 2 gained, 3 both wrong with the same class, 4 both wrong with different
# classes, 255 pixel not counted
CHANGE_PALETTE = {0: (70, 70, 70), 1: (220, 50, 47), 2: (60, 170, 80), 3: (235, 200, 60), 4: (200, 110, 30),
                  255: (0, 0, 0)}
OUTCOMES = ("both_right", "forgotten", "gained", "both_wrong")
_COUNTERS = ("transition", "confusion_a", "confusion_b", "outcome", "bad_targets", "sums", "workspace")


def workspace_bytes(N, H, W, nc):
    """Bytes of workspace ``drift_head`` needs to fill ``sums`` for features [N,H,W,16]."""
    n = _drift_lib.load().mdil_drift_workspace_bytes(int(N), int(H), int(W), int(nc))
    if n < 0:
        raise RuntimeError(f"mdil {_FN}: no workspace size for N {N}, H {H}, W {W}, {nc} classes")
    return n


def drift_head(feat_a, w_a, b_a, feat_b, w_b, b_b, *, target=None, ignore_index=-1, labels=False, kl=False,
               change=False, counters=None):
    """Two heads compared on NHWC decoder features [N,H,W,16] (``feat_a`` of the model before,
    ``feat_b`` of the model after) and their ``ConvTranspose2d(16, nc, 2, 2)`` parameters,
    2 <= nc <= 32, on the current stream.  -> dict with ``label_a``, ``label_b`` (u8 [N,2H,2W], with
    ``labels``), ``kl`` (f32 [N,2H,2W], with ``kl``) and ``change`` (u8 [N,2H,2W], with ``change``:
    the codes of CHANGE_PALETTE); what was not asked for is None.

    ``target`` (u8 [N,2H,2W], device, train ids) decides which pixels are counted (< nc and not
    ``ignore_index``).  ``counters``: a dict of device tensors that are ADDED to, never cleared, any
    of ``transition``, ``confusion_a``, ``confusion_b`` (i64 [nc,nc]), ``outcome`` (i64 [nc,4]),
    ``bad_targets`` (i64 [1]) and ``sums`` (f64 [nc+1]), the last with ``workspace`` (f64, at least
    ``workspace_bytes(N, H, W, nc)`` bytes).  ``confusion_a``, ``confusion_b`` and ``outcome`` need a
    target."""
    lib = _drift_lib.load()
    for t, name in ((feat_a, "feat_a"), (w_a, "w_a"), (b_a, "b_a"), (feat_b, "feat_b"), (w_b, "w_b"), (b_b, "b_b")):
        _chk(t, name)
    nc = hc.check_params(_FN, w_a, b_a, feat_a)
    if hc.check_params(_FN, w_b, b_b, feat_b) != nc or feat_a.shape != feat_b.shape:
        raise RuntimeError(f"mdil {_FN}: the two models must agree in N, H, W and nc (got features "
                           f"{tuple(feat_a.shape)} and {tuple(feat_b.shape)}, {nc} and {w_b.shape[1]} classes)")
    hc.check_classes(_FN, _drift_lib, nc, feat_a, w_a, b_a, "feat_a")
    hc.check_classes(_FN, _drift_lib, nc, feat_a, w_b, b_b, "feat_a")
    dev = feat_a.device
    if feat_b.device != dev:
        raise RuntimeError(f"mdil {_FN}: feat_a on {dev}, feat_b on {feat_b.device}")
    N, H, W = feat_a.shape[0], feat_a.shape[1], feat_a.shape[2]
    hc.check_tables(_FN, _PATH, dev, torch.uint8, ((target, "target", (N, 2 * H, 2 * W)),))
    hc.check_ignore_index(_FN, ignore_index)
    c = rc.check_counters(_FN, counters, _COUNTERS)
    hc.check_tables(_FN, _PATH, dev, torch.int64,
                    ((c["transition"], "transition", (nc, nc)), (c["confusion_a"], "confusion_a", (nc, nc)),
                     (c["confusion_b"], "confusion_b", (nc, nc)), (c["outcome"], "outcome", (nc, 4)),
                     (c["bad_targets"], "bad_targets", (1,))))
    hc.check_tables(_FN, _PATH, dev, torch.float64, ((c["sums"], "sums", (nc + 1,)),))
    if target is None and any(c[k] is not None for k in ("confusion_a", "confusion_b", "outcome")):
        raise RuntimeError(f"mdil {_FN}: confusion_a / confusion_b / outcome given without a target")
    ws, ws_bytes = rc.check_workspace(_FN, _PATH, dev, c, lambda: workspace_bytes(N, H, W, nc))
    with torch.no_grad(), torch.cuda.device(dev):
        def new(want, dtype):
            return torch.empty(N, 2 * H, 2 * W, dtype=dtype, device=dev) if want else None
        out = {"label_a": new(labels, torch.uint8), "label_b": new(labels, torch.uint8), "kl": new(kl, torch.float32),
               "change": new(change, torch.uint8)}
        _drift_lib.check(
            lib.mdil_drift_head(feat_a.data_ptr(), w_a.data_ptr(), b_a.data_ptr(), feat_b.data_ptr(), w_b.data_ptr(),
                                b_b.data_ptr(), N, H, W, nc, hc.ptr(target), int(ignore_index), hc.ptr(out["label_a"]),
                                hc.ptr(out["label_b"]), hc.ptr(out["kl"]), hc.ptr(out["change"]),
                                hc.ptr(c["transition"]), hc.ptr(c["confusion_a"]), hc.ptr(c["confusion_b"]),
                                hc.ptr(c["outcome"]), hc.ptr(c["bad_targets"]), hc.ptr(c["sums"]), ws, ws_bytes,
                                torch.cuda.current_stream(dev).cuda_stream),
            "mdil_drift_head")
    return out


def compare(model_a, model_b, images, task, **kw):
    """``drift_head`` on ``images`` [N,3,H,W] for ``task``: the decoder features and that task's
    ``output_conv`` parameters of ``model_a`` (before) and ``model_b`` (after), both in eval mode."""
    model_a.eval()
    model_b.eval()
    with torch.no_grad():
        fa, fb = model_a.features(images, task), model_b.features(images, task)
        (wa, ba), (wb, bb) = model_a.head_params(task), model_b.head_params(task)
        return drift_head(fa.contiguous(), wa.detach(), ba.detach(), fb.contiguous(), wb.detach(), bb.detach(), **kw)


class DriftMeter:
    """Owns the counters, the sums and the workspace of a comparison over many batches; the first
    ``add`` decides whether it is scored against targets."""

    def __init__(self, nc, ignore_index):
        self.nc, self.ignore_index = int(nc), int(ignore_index)
        self.tensors = None
        self.scored = None
        self.pixels = 0                      # ALL output pixels seen: what kd_loss is a mean over

    def _counters(self, dev, scored, N, H, W):
        nc = self.nc
        if self.tensors is None:
            self.scored = scored
            z = functools.partial(torch.zeros, dtype=torch.int64, device=dev)
            self.tensors = {"transition": z(nc, nc), "bad_targets": z(1),
                            "sums": torch.zeros(nc + 1, dtype=torch.float64, device=dev)}
            if scored:
                self.tensors.update(confusion_a=z(nc, nc), confusion_b=z(nc, nc), outcome=z(nc, 4))
        elif scored != self.scored:
            raise RuntimeError("mdil DriftMeter.add: every call must come with a target, or none")
        rc.grow_workspace(self.tensors, workspace_bytes(N, H, W, nc), dev)
        return self.tensors

    def add(self, *source, target=None, **kw):
        """``add(model_a, model_b, images, task)`` or ``add(feat_a, w_a, b_a, feat_b, w_b, b_b)``,
        with ``target=t`` (u8 [N,2H,2W] train ids on the device) when scoring.  -> ``drift_head``'s dict."""
        if not isinstance(source[0], torch.nn.Module):
            _chk(source[0], "feat_a")
        fn, dev, N, H, W = rc.meter_source("DriftMeter", _PATH, source, 2, compare, drift_head, "feat_a")
        kw.update(target=target, ignore_index=self.ignore_index,
                  counters=self._counters(dev, target is not None, N, H, W))
        out = fn(*source, **kw)
        self.pixels += N * 4 * H * W
        return out

    def host(self):
        """The counters on the host: int64 matrices, float64 sums; raises when a target outside
        [0, nc) (other than the ignore index) was met."""
        if self.tensors is None:
            return {"transition": torch.zeros(self.nc, self.nc, dtype=torch.int64),
                    "sums": torch.zeros(self.nc + 1, dtype=torch.float64)}
        rc.refuse_bad_targets("DriftMeter", self.tensors, self.nc, self.ignore_index)
        return {k: v.cpu() for k, v in self.tensors.items() if k not in ("workspace", "bad_targets")}

    def report(self, top=10):
        return drift_report(self.nc, pixels=self.pixels, ignore_index=self.ignore_index, top=top, **self.host())


def _rate(num, den):
    return [float(n) / float(d) if d else None for n, d in zip(num.tolist(), den.tolist())]


def drift_report(nc, transition, sums, pixels, confusion_a=None, confusion_b=None, outcome=None, ignore_index=-1,
                 top=10):
    """From the integer matrices and the sums to the report; runs on the host alone.

    ``transition`` i64 [nc,nc] (row = label before, column = label after), ``sums`` f64 [nc+1],
    ``pixels``: ALL output pixels seen (N * 2H * 2W summed over the calls).  -> dict:
    ``agreement`` trace / total of the transition matrix; ``mean_kl`` the sum of the class sums over
    the counted pixels, ``kl_classes`` each class sum over that class's counted pixels (None for a
    class without pixels; the class is the target with the confusion matrices, else the label
    before); ``kd_loss`` = sums[nc] / (pixels * nc), what the step-2 trainer logs as KLD;
    ``top_transitions`` the largest off-diagonal entries as [from, to, pixels].  With the three target
    matrices also ``mIoU_before``, ``mIoU_after``, ``mIoU_change``, ``iou_before``, ``iou_after``,
    ``iou_change`` (``ConfusionMeter.iou``, the iouEval rule) and per target class ``forgotten`` /
    ``gained``: the share of its counted pixels that only the model before / only the model after
    got right."""
    t = torch.as_tensor(transition, dtype=torch.int64)
    s = torch.as_tensor(sums, dtype=torch.float64)
    if tuple(t.shape) != (nc, nc) or tuple(s.shape) != (nc + 1,):
        raise RuntimeError(f"mdil drift_report: expected transition [{nc},{nc}] and sums [{nc + 1}] "
                           f"(got {tuple(t.shape)} and {tuple(s.shape)})")
    scored = [m is not None for m in (confusion_a, confusion_b, outcome)]
    if any(scored) and not all(scored):
        raise RuntimeError("mdil drift_report: confusion_a, confusion_b and outcome come together")
    total = int(t.sum())
    per_class = torch.as_tensor(confusion_a, dtype=torch.int64).sum(1) if all(scored) else t.sum(1)
    off = t.clone()
    off.fill_diagonal_(0)
    order = sorted(((int(off[i, j]), i, j) for i in range(nc) for j in range(nc) if off[i, j] > 0),
                   key=lambda e: (-e[0], e[1], e[2]))
    report = {
        "classes": nc, "pixels": int(pixels), "counted_pixels": total,
        "agreement": float(t.diagonal().sum()) / total if total else None,
        "mean_kl": float(s[:nc].sum()) / total if total else None,
        "kl_classes": _rate(s[:nc], per_class),
        "kd_loss": float(s[nc]) / (int(pixels) * nc) if pixels else None,
        "top_transitions": [[i, j, n] for n, i, j in order[:top]],
        "transition": t.tolist(),
    }
    if all(scored):
        ca, cb = (torch.as_tensor(m, dtype=torch.int64) for m in (confusion_a, confusion_b))
        o = torch.as_tensor(outcome, dtype=torch.int64)
        meter = ConfusionMeter(nc, ignore_index)
        (ma, ia), (mb, ib) = meter.iou(ca), meter.iou(cb)
        rows = o.sum(1)
        report.update(mIoU_before=float(ma), mIoU_after=float(mb), mIoU_change=float(mb - ma),
                      iou_before=[float(v) for v in ia], iou_after=[float(v) for v in ib],
                      iou_change=[float(v) for v in ib - ia], forgotten=_rate(o[:, 1], rows),
                      gained=_rate(o[:, 2], rows), outcome=o.tolist(), confusion_before=ca.tolist(),
                      confusion_after=cb.tolist())
    return report


# ------------------------------------------------------------------------------------------ CLI
def change_colours(change):
    """u8 [...] change codes -> u8 [..., 3] by CHANGE_PALETTE (host arrays)."""
    lut = np.zeros((256, 3), dtype=np.uint8)
    for code, rgb in CHANGE_PALETTE.items():
        lut[code] = rgb
    return lut[change]


def kl_bytes(kl, kl_max):
    """f32 kl map (device) -> u8 ``round(255 min(kl, kl_max) / kl_max)``; a NaN gives 0."""
    return kl.clamp(max=kl_max).mul(255.0 / kl_max).round_().nan_to_num_(0.0).clamp_(0.0, 255.0).to(torch.uint8)


def main(args):
    _refusals(args)
    dev, nc, before = hc.load_model(args.before, args.before_num_classes, args.task)
    _, _, after = hc.load_model(args.after, args.after_num_classes, args.task)
    reporting = args.report or args.score
    meter = DriftMeter(nc, nc - 1 if args.score else -1) if reporting else None
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    n_items = 0
    with hc.png_pool() as pool:
        png = hc.PngWriter(pool, args.out)
        for stems, images, target in rc.batches(args, nc, dev, score=args.score, unique_stems=True):
            n_items += len(stems)
            kw = dict(labels=bool(args.out and args.labels), kl=bool(args.out), change=bool(args.out))
            if meter is not None:
                out = meter.add(before, after, images, args.task, target=target, **kw)
            else:
                out = compare(before, after, images, args.task, **kw)
            if not args.out:
                continue
            host = {"change": change_colours(out["change"].cpu().numpy()),
                    "kl": kl_bytes(out["kl"], args.kl_max).cpu().numpy()}
            if args.labels:
                host.update(before_label=out["label_a"].cpu().numpy(), after_label=out["label_b"].cpu().numpy())
            png.wait()                         # the batch before this one: bounds what is in flight
            for k, stem in enumerate(stems):
                for kind, arr in host.items():
                    png.submit(arr[k], f"{stem}_{kind}.png")
        png.wait()
    report = {"dataset": "synthetic" if args.synthetic else args.dataset, "task": args.task, "images": n_items,
              "written": png.written}
    if meter is not None:
        report.update(meter.report())
        what = f"{report['dataset']} (task {args.task}), before -> after"
        print(f"{what}: agreement {report['agreement'] * 100:.2f} %  mean KL {report['mean_kl']:.6f}  "
              f"KD loss {report['kd_loss']:.6f}  over {report['counted_pixels']} pixels")
        print("largest transitions (from, to, pixels): " + " ".join(f"{i}->{j}:{n}" for i, j, n in report["top_transitions"]))
        if args.score:
            print(f"mIoU {report['mIoU_before'] * 100:.2f} % -> {report['mIoU_after'] * 100:.2f} % "
                  f"({report['mIoU_change'] * 100:+.2f})")
            print("per-class IoU change: " + " ".join(f"{v * 100:+.2f}" for v in report["iou_change"]))
            print("forgotten: " + " ".join("-" if v is None else f"{v * 100:.2f}" for v in report["forgotten"]))
            print("gained:    " + " ".join("-" if v is None else f"{v * 100:.2f}" for v in report["gained"]))
    if args.out:
        print(f"{len(png.written)} maps written to {args.out}")
    if args.json:
        hc.write_json(report, args.json)
    return report


def _refusals(args):
    """Raise a RuntimeError that names why this combination of flags is refused."""
    rc.refuse_pair(args)
    if not args.report and not args.score and not args.out:
        raise RuntimeError("nothing to do: give --report, --score, --out DIR or several")
    if args.json and not args.report and not args.score:
        raise RuntimeError("--json writes the report: it needs --report or --score")
    if args.labels and not args.out:
        raise RuntimeError("--labels needs --out DIR")
    rc.refuse_data(args)
    if not args.kl_max > 0:
        raise RuntimeError("--kl-max must be positive")


def build_parser():
    p = hc.RefusingParser(_refusals, description="drift report: two checkpoints compared on one task")
    p.add_argument("--before", required=True, help="checkpoint before the incremental step (the teacher)")
    p.add_argument("--before-num-classes", type=int, nargs="+", required=True)
    p.add_argument("--after", required=True, help="checkpoint after it (the student)")
    p.add_argument("--after-num-classes", type=int, nargs="+", required=True)
    p.add_argument("--task", type=int, required=True, help="which task's decoder is compared; both models have it")
    p.add_argument("--report", action="store_true", help="agreement, KL, KD loss and class transitions (no labels)")
    p.add_argument("--score", action="store_true", help="the report with the labels: mIoU before / after, "
                                                        "forgotten and gained rates")
    p.add_argument("--json", help="write the report (with its matrices) here")
    p.add_argument("--out", help="write <stem>_change.png and <stem>_kl.png into this folder")
    p.add_argument("--kl-max", type=float, default=1.0, help="the KL divergence drawn as 255 in <stem>_kl.png")
    p.add_argument("--labels", action="store_true", help="also write <stem>_before_label.png and <stem>_after_label.png")
    rc.add_data_flags(p)
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
