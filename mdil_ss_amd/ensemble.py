"""Multi-scale and flip ensembles ("MS + flip") at the DATASET's own size on MI355X: the image is run
through the network at several scales, each optionally mirrored as well; every view's logits are
un-mirrored, resized to the label size, turned into probabilities and added up, and the argmax of
the sum is written and scored -- one fused kernel straight from the views' 16-channel decoder
features, so no view's logits, resized logits or probabilities are stored
(include/mdil_ensemble.h).

    python -m mdil_ss_amd.ensemble --state model_best_....pth.tar --num-classes 20 20 27 --task 0 \
        --dataset cityscapes [--cs-datadir ...] --scales 0.75 1 1.25 --flip [--mode prob|logit] \
        [--score] [--json FILE] [--out DIR [--colour] [--confidence] [--label-ids cityscapes|FILE.json]]

The flags are those of ``python -m mdil_ss_amd.fullres``.  Each scale's network input is
``8 * round(scale * size / 8)`` (at least 8) per axis, made from the NATIVE-size image by the same PIL
bilinear resize as the scale-1 view; the label keeps its own size and the maps come out at that
size.  ``--confidence`` writes ``<stem>_conf.png``, the 8-bit rounding of 255 x confidence."""
import copy
import json
import math
import os
from argparse import ArgumentParser
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _ensemble_lib
from .fullres import LABEL_IDS, ConfusionMeter, _open, _runs, load_label_ids
from .fullres import _refusals as _fullres_refusals
from .predict import MAX_PNG_THREADS, _save_png, default_palette

MAX_VIEWS = _ensemble_lib.MAX_VIEWS


def _chk(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        got = (f"{t.dtype}, {t.device}, contiguous={t.is_contiguous()}" if isinstance(t, torch.Tensor)
               else type(t).__name__)
        raise RuntimeError(f"mdil ensemble_head: {name} must be a contiguous {str(dtype)[6:]} device tensor "
                           f"(got {got}); there is no CPU fallback in the ensemble path")


def _p(t):
    return None if t is None else t.data_ptr()


def ensemble_head(views, weight, bias, out_size, *, mode="prob", id_map=None, palette=None, confidence=False,
                  target=None, ignore_index=-1, confusion=None, bad_targets=None):
    """The vote of up to 8 views at ``out_size`` = (Ho, Wo) on the current stream.  ``views`` is a
    sequence of ``(features [N,H,W,16] NHWC, mirrored)``: per view ``output_conv`` with the
    ``ConvTranspose2d(16, nc, 2, 2)`` parameters, 2 <= nc <= 32, the un-mirroring and the bilinear
    resize of the logits; ``mode`` "prob" adds the views' softmax, "logit" their logits.
    -> (label u8 [N,Ho,Wo], colour u8 [N,Ho,Wo,3] or None, confidence f32 [N,Ho,Wo] or None).

    ``id_map``, ``palette``, ``target``, ``ignore_index``, ``confusion`` and ``bad_targets`` are those
    of ``fullres_head``; ``confidence=True`` also returns the winner's mean probability ("prob") or
    its softmax of the mean logits ("logit")."""
    lib = _ensemble_lib.load()
    if mode not in _ensemble_lib.MODES:
        raise RuntimeError(f"mdil ensemble_head: mode must be one of {sorted(_ensemble_lib.MODES)}, got {mode!r}")
    try:
        views = [(f, bool(m)) for f, m in views]
    except (TypeError, ValueError):
        raise RuntimeError("mdil ensemble_head: views must be a sequence of (features [N,H,W,16], mirrored)") from None
    if not 1 <= len(views) <= MAX_VIEWS:
        raise RuntimeError(f"mdil ensemble_head: views holds {len(views)} entries (supported: 1 to {MAX_VIEWS})")
    x0, w, b = views[0][0], weight, bias
    for i, (f, _) in enumerate(views):         # the shapes first: they can be judged wherever the tensors live
        if isinstance(f, torch.Tensor) and isinstance(x0, torch.Tensor):
            if f.dim() != 4 or f.shape[3] != 16 or f.numel() == 0:
                raise RuntimeError(f"mdil ensemble_head: views[{i}] must be NHWC features [N,H,W,16] "
                                   f"(got {tuple(f.shape)})")
            if f.shape[0] != x0.shape[0]:
                raise RuntimeError(f"mdil ensemble_head: views[{i}] has N = {f.shape[0]}, views[0] has N = "
                                   f"{x0.shape[0]}: all views share the batch")
    for i, (f, _) in enumerate(views):
        _chk(f, f"views[{i}]")
    _chk(weight, "weight")
    _chk(bias, "bias")
    if w.dim() != 4 or w.shape[0] != 16 or tuple(w.shape[2:]) != (2, 2) or b.numel() != w.shape[1]:
        raise RuntimeError("mdil ensemble_head: expects ConvTranspose2d(16, nc, 2, 2) parameters as weight and bias "
                           f"(got w {tuple(w.shape)}, bias {tuple(b.shape)})")
    for i, (f, _) in enumerate(views):
        if f.device != x0.device:
            raise RuntimeError(f"mdil ensemble_head: views[{i}] on {f.device}, views[0] on {x0.device}")
    N, nc = x0.shape[0], w.shape[1]
    if not _ensemble_lib.MIN_CLASSES <= nc <= _ensemble_lib.MAX_CLASSES:
        raise RuntimeError(f"mdil ensemble_head: {nc} classes (supported: {_ensemble_lib.MIN_CLASSES} to "
                           f"{_ensemble_lib.MAX_CLASSES})")
    if w.device != x0.device or b.device != x0.device:
        raise RuntimeError(f"mdil ensemble_head: views on {x0.device}, weight on {w.device}, bias on {b.device}")
    try:
        Ho, Wo = (int(v) for v in out_size)
    except (TypeError, ValueError):
        raise RuntimeError(f"mdil ensemble_head: out_size must be (height, width), got {out_size!r}") from None
    if not (1 <= Ho <= _ensemble_lib.MAX_SIZE and 1 <= Wo <= _ensemble_lib.MAX_SIZE):
        raise RuntimeError(f"mdil ensemble_head: out_size {Ho} x {Wo} outside [1, {_ensemble_lib.MAX_SIZE}]")
    for t, name, shape in ((id_map, "id_map", (nc,)), (palette, "palette", (nc, 3)), (target, "target", (N, Ho, Wo))):
        if t is not None:
            _chk(t, name, torch.uint8)
            if tuple(t.shape) != shape or t.device != x0.device:
                raise RuntimeError(f"mdil ensemble_head: {name} must be uint8 {list(shape)} on {x0.device} "
                                   f"(got {tuple(t.shape)} on {t.device})")
    if target is None:
        if confusion is not None or bad_targets is not None:
            raise RuntimeError("mdil ensemble_head: confusion / bad_targets given without a target")
    else:
        if confusion is None or bad_targets is None:
            raise RuntimeError("mdil ensemble_head: a target needs confusion (int64 [nc,nc]) and bad_targets "
                               "(int64 [1]) on the device; they are accumulated into")
        for t, name, shape in ((confusion, "confusion", (nc, nc)), (bad_targets, "bad_targets", (1,))):
            _chk(t, name, torch.int64)
            if tuple(t.shape) != shape or t.device != x0.device:
                raise RuntimeError(f"mdil ensemble_head: {name} must be int64 {list(shape)} on {x0.device} "
                                   f"(got {tuple(t.shape)} on {t.device})")
    if not -1 <= int(ignore_index) <= 255:
        raise RuntimeError(f"mdil ensemble_head: ignore_index {ignore_index} outside [-1, 255]")
    table = _ensemble_lib.view_table([(f.data_ptr(), f.shape[1], f.shape[2], m) for f, m in views])
    with torch.no_grad(), torch.cuda.device(x0.device):
        label = torch.empty(N, Ho, Wo, dtype=torch.uint8, device=x0.device)
        colour = None if palette is None else torch.empty(N, Ho, Wo, 3, dtype=torch.uint8, device=x0.device)
        conf = torch.empty(N, Ho, Wo, dtype=torch.float32, device=x0.device) if confidence else None
        _ensemble_lib.check(
            lib.mdil_ensemble_head(table, len(views), w.data_ptr(), b.data_ptr(), N, nc, Ho, Wo,
                                   _ensemble_lib.MODES[mode], _p(id_map), _p(palette), _p(target), int(ignore_index),
                                   label.data_ptr(), _p(colour), _p(conf), _p(confusion), _p(bad_targets),
                                   torch.cuda.current_stream(x0.device).cuda_stream),
            "mdil_ensemble_head")
    return label, colour, conf


def predict_ensemble(model, images, task, out_size, *, scales=(1.0,), flip=False, mode="prob", **kw):
    """The ensemble's maps for ``task`` at ``out_size``.  ``images`` is a list with one [N,3,h_v,w_v]
    device tensor per entry of ``scales``, already resized; each is run through the model's decoder
    features and, with ``flip``, so is the tensor flipped along the width (a mirrored view).  The
    views -- scales ascending in the list, the plain view before the mirrored one -- then go through
    ``ensemble_head`` with that task's ``output_conv`` parameters."""
    if isinstance(images, torch.Tensor):
        images = [images]
    if len(images) != len(scales):
        raise RuntimeError(f"mdil predict_ensemble: {len(images)} image tensors for {len(scales)} scales")
    if len(images) * (2 if flip else 1) > MAX_VIEWS:
        raise RuntimeError(f"mdil predict_ensemble: {len(images) * (2 if flip else 1)} views (at most {MAX_VIEWS})")
    model.eval()
    views = []
    with torch.no_grad():
        for im in images:
            for mirrored in ((False, True) if flip else (False,)):
                src = im.flip(3).contiguous() if mirrored else im
                try:
                    feat = model.features(src, task)
                except RuntimeError as e:
                    if isinstance(im, torch.Tensor) and im.is_cuda:
                        raise RuntimeError(f"mdil predict_ensemble: the eval forward refuses a "
                                           f"{im.shape[2]} x {im.shape[3]} input: {e}") from e
                    raise
                views.append((feat.contiguous(), mirrored))
        w, b = model.head_params(task)
        return ensemble_head(views, w.detach(), b.detach(), out_size, mode=mode, **kw)


class EnsembleMeter(ConfusionMeter):
    """A ConfusionMeter whose ``add`` goes through the ensemble; ``matrix()`` and ``iou()`` are the
    base class's."""

    def add(self, *source, target, **kw):
        """``add(model, images, task, target=t, scales=..., flip=...)`` or
        ``add(views, weight, bias, target=t)``; ``target``: u8 [N,Ho,Wo] train ids on the device,
        which also sets the output size.  -> (label, colour or None, confidence or None)."""
        if not isinstance(target, torch.Tensor) or target.dim() != 3:
            raise RuntimeError("mdil EnsembleMeter.add: target must be a uint8 [N,Ho,Wo] device tensor")
        if self.confusion is None:
            self.confusion = torch.zeros(self.nc, self.nc, dtype=torch.int64, device=target.device)
            self.bad_targets = torch.zeros(1, dtype=torch.int64, device=target.device)
        kw.update(target=target, ignore_index=self.ignore_index, confusion=self.confusion,
                  bad_targets=self.bad_targets)
        fn = predict_ensemble if isinstance(source[0], torch.nn.Module) else ensemble_head
        return fn(*source, tuple(target.shape[1:]), **kw)


# ------------------------------------------------------------------------------------------ CLI
def scaled_size(size, scale):
    """The network's input length for ``scale``: the nearest multiple of 8 (halves up), at least 8."""
    return max(8, 8 * int(math.floor(scale * size / 8 + 0.5)))


def main(args):
    from .models.erfnet_RA_parallel import Net as Net_RAP
    from .trainer_common import _strip
    _refusals(args)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    nb = len(args.num_classes)
    if not 0 <= args.task < nb:
        raise RuntimeError(f"--task {args.task}: the model has tasks 0 to {nb - 1}")
    nc = args.num_classes[args.task]
    model = Net_RAP(args.num_classes, nb, nb - 1)
    saved = torch.load(args.state, map_location="cpu", weights_only=False)
    model.load_state_dict(_strip(saved["state_dict"]), strict=True)
    model.to(dev).eval()
    id_map = load_label_ids(args.label_ids, nc).to(dev) if args.label_ids else None
    palette = default_palette(nc).contiguous().to(dev) if args.colour else None
    meter = EnsembleMeter(nc, nc - 1) if args.score else None
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    # one sampler per scale: the native-size image resized for that scale, as the scale-1 view is
    sizes = [(scaled_size(args.height, s), scaled_size(args.width, s)) for s in args.scales]
    samplers = []
    for h, w_ in sizes:
        a = copy.copy(args)
        a.height, a.width = h, w_
        n_items, stems, sample = _open(a, nc)
        samplers.append(sample)
    written, pending = [], []
    with ThreadPoolExecutor(max_workers=min(MAX_PNG_THREADS, os.cpu_count() or 1)) as pool:
        for i0 in range(0, n_items, args.batch_size):
            idx = range(i0, min(i0 + args.batch_size, n_items))
            jobs = [(k, i) for k in range(len(samplers)) for i in idx]
            items = list(pool.map(lambda ki: samplers[ki[0]](ki[1]), jobs))
            per_scale = [items[k * len(idx):(k + 1) * len(idx)] for k in range(len(samplers))]
            labels = [lab for _, lab in per_scale[0]]
            views = []
            with torch.no_grad():
                for (h, w_), batch in zip(sizes, per_scale):
                    u8 = torch.from_numpy(np.stack([im for im, _ in batch])).to(dev)    # [n,h,w,3] bytes
                    images = u8.permute(0, 3, 1, 2).to(torch.float32).div_(255.0)
                    for mirrored in ((False, True) if args.flip else (False,)):
                        try:
                            feat = model.features(images.flip(3).contiguous() if mirrored else images, args.task)
                        except RuntimeError as e:
                            raise RuntimeError(f"--scales: the eval forward refuses the {h} x {w_} input: {e}") from e
                        views.append((feat.contiguous(), mirrored))
                w, b = (t.detach() for t in model.head_params(args.task))
            maps = []
            # one kernel call per run of images that share a native size
            for s, e in _runs([lab.shape for lab in labels]):
                target = torch.from_numpy(np.stack(labels[s:e])).to(dev)
                part = [(f[s:e], m) for f, m in views]
                kw = dict(mode=args.mode, id_map=id_map, palette=palette, confidence=args.confidence)
                if meter is not None:
                    label, colour, conf = meter.add(part, w, b, target=target, **kw)
                else:
                    label, colour, conf = ensemble_head(part, w, b, tuple(target.shape[1:]), **kw)
                if args.out:
                    conf8 = None if conf is None else conf.mul(255.0).round_().to(torch.uint8).cpu().numpy()
                    maps.append((s, label.cpu().numpy(), None if colour is None else colour.cpu().numpy(), conf8))
            for f in pending:                  # the batch before this one: bounds what is in flight
                f.result()
            pending = []
            for s, label, colour, conf8 in maps:
                for k in range(label.shape[0]):
                    out = [(label[k], f"{stems[idx[s + k]]}_label.png")]
                    if colour is not None:
                        out.append((colour[k], f"{stems[idx[s + k]]}_colour.png"))
                    if conf8 is not None:
                        out.append((conf8[k], f"{stems[idx[s + k]]}_conf.png"))
                    for arr, name in out:
                        path = os.path.join(args.out, name)
                        pending.append(pool.submit(_save_png, np.ascontiguousarray(arr), path))
                        written.append(path)
        for f in pending:
            f.result()
    report = {"dataset": "synthetic" if args.synthetic else args.dataset, "task": args.task, "images": n_items,
              "written": written, "scales": [float(s) for s in args.scales], "flip": bool(args.flip),
              "mode": args.mode}
    if meter is not None:
        matrix = meter.matrix()
        miou, per_class = meter.iou(matrix)
        report.update(mIoU=float(miou), iou_classes=[float(v) for v in per_class], confusion=matrix.tolist(),
                      pixels=int(matrix.sum()))
        what = "scales " + " / ".join(f"{s:g}" for s in args.scales) + (" + flip" if args.flip else "")
        print(f"{report['dataset']} (task {args.task}) at the labels' own size, {what}, {args.mode}: "
              f"mIoU {float(miou) * 100:.2f} %  over {report['pixels']} pixels")
        print("per-class IoU: " + " ".join(f"{float(v) * 100:.2f}" for v in per_class))
    if args.out:
        print(f"{len(written)} maps written to {args.out}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1)
    return report


def _refusals(args):
    """Raise a RuntimeError that names why this combination of flags is refused (before the GPU is
    touched): fullres's own refusals, then those of the ensemble's flags."""
    _fullres_refusals(args)
    scales = list(args.scales)
    if any(not (s > 0 and math.isfinite(s)) for s in scales):
        raise RuntimeError(f"--scales must be positive, got {scales}")
    if len(set(scales)) != len(scales):
        raise RuntimeError(f"--scales holds a duplicate: {scales}")
    nviews = len(scales) * (2 if args.flip else 1)
    if nviews > MAX_VIEWS:
        raise RuntimeError(f"--scales{' with --flip' if args.flip else ''} makes {nviews} views: at most {MAX_VIEWS}")
    if args.confidence and not args.out:
        raise RuntimeError("--confidence needs --out DIR")


class _Parser(ArgumentParser):
    def parse_args(self, *a, **kw):
        args = super().parse_args(*a, **kw)
        try:
            _refusals(args)
        except RuntimeError as e:
            self.error(str(e))
        return args


def build_parser():
    from .dataset import add_datadir_flags
    p = _Parser(description="multi-scale / flip ensemble: label maps and mIoU at the dataset's own size from a "
                            "checkpoint")
    p.add_argument("--state", required=True, help="checkpoint written by the trainers (or by the reference)")
    p.add_argument("--num-classes", type=int, nargs="+", required=True)
    p.add_argument("--task", type=int, required=True, help="which task's decoder predicts")
    p.add_argument("--dataset", choices=("cityscapes", "BDD", "IDD"))
    p.add_argument("--subset", default="val")
    p.add_argument("--synthetic", type=int, default=0, help="N procedural images instead of a dataset")
    p.add_argument("--native-height", type=int, default=1024, help="--synthetic: the labels' own height")
    p.add_argument("--native-width", type=int, default=2048, help="--synthetic: the labels' own width")
    p.add_argument("--height", type=int, default=512, help="the network's input height at scale 1")
    p.add_argument("--width", type=int, default=1024, help="the network's input width at scale 1")
    p.add_argument("--batch-size", type=int, default=6)
    p.add_argument("--scales", type=float, nargs="+", default=[1.0],
                   help="one view per scale; the input is 8 * round(scale * size / 8) per axis")
    p.add_argument("--flip", action="store_true", help="every scale also mirrored")
    p.add_argument("--mode", choices=sorted(_ensemble_lib.MODES), default="prob",
                   help="add the views' probabilities (prob) or their logits (logit)")
    p.add_argument("--score", action="store_true", help="mIoU and per-class IoU against the full-size labels")
    p.add_argument("--json", help="write the score (with the confusion matrix) here")
    p.add_argument("--out", help="write <stem>_label.png at the image's own size into this folder")
    p.add_argument("--colour", action="store_true", help="also write <stem>_colour.png")
    p.add_argument("--confidence", action="store_true", help="also write <stem>_conf.png (255 x confidence)")
    p.add_argument("--label-ids", help=f"label PNGs in the dataset's own ids: one of {sorted(LABEL_IDS)} or a "
                                       "JSON file with one id per class (default: train ids)")
    add_datadir_flags(p)
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
