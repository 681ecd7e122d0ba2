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
import functools
import math
import os

import torch

from . import _ensemble_lib
from . import _head_common as hc
from . import _labelsize_common as ls
from .fullres import ConfusionMeter
from .predict import default_palette

MAX_VIEWS = _ensemble_lib.MAX_VIEWS
_FN, _PATH = "ensemble_head", "ensemble"
_chk = functools.partial(hc.chk, _FN, _PATH)


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
    nc = hc.check_params(_FN, w, b)
    for i, (f, _) in enumerate(views):
        if f.device != x0.device:
            raise RuntimeError(f"mdil ensemble_head: views[{i}] on {f.device}, views[0] on {x0.device}")
    N = x0.shape[0]
    hc.check_classes(_FN, _ensemble_lib, nc, x0, w, b, "views")
    Ho, Wo = hc.check_out_size(_FN, _ensemble_lib, out_size)
    hc.check_scoring(_FN, _PATH, x0.device, N, nc, Ho, Wo, id_map, palette, target, confusion, bad_targets, ignore_index)
    table = _ensemble_lib.view_table([(f.data_ptr(), f.shape[1], f.shape[2], m) for f, m in views])
    with torch.no_grad(), torch.cuda.device(x0.device):
        label = torch.empty(N, Ho, Wo, dtype=torch.uint8, device=x0.device)
        colour = None if palette is None else torch.empty(N, Ho, Wo, 3, dtype=torch.uint8, device=x0.device)
        conf = torch.empty(N, Ho, Wo, dtype=torch.float32, device=x0.device) if confidence else None
        _ensemble_lib.check(
            lib.mdil_ensemble_head(table, len(views), w.data_ptr(), b.data_ptr(), N, nc, Ho, Wo,
                                   _ensemble_lib.MODES[mode], hc.ptr(id_map), hc.ptr(palette), hc.ptr(target),
                                   int(ignore_index), label.data_ptr(), hc.ptr(colour), hc.ptr(conf),
                                   hc.ptr(confusion), hc.ptr(bad_targets),
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
    """A ConfusionMeter whose ``add`` goes through the ensemble:
    ``add(model, images, task, target=t, scales=..., flip=...)`` or ``add(views, weight, bias, target=t)``
    -> (label, colour or None, confidence or None); ``matrix()`` and ``iou()`` are the base class's."""

    def __init__(self, nc, ignore_index):
        super().__init__(nc, ignore_index)
        self._name, self._model_fn, self._head_fn = "EnsembleMeter", predict_ensemble, ensemble_head


# ------------------------------------------------------------------------------------------ CLI
def scaled_size(size, scale):
    """The network's input length for ``scale``: the nearest multiple of 8 (halves up), at least 8."""
    return max(8, 8 * int(math.floor(scale * size / 8 + 0.5)))


def view_heads(sizes, flip):
    """The hook of ``ls.label_runs`` for the ensemble: per input size (one sampler each) the batch's
    images, plain and with ``flip`` mirrored, through the model -> cut(s, e): the one predictor's
    (views of the items s .. e - 1, weight, bias)."""
    def heads(models, task, images, dev):
        (model,), views = models, []
        with torch.no_grad():
            for (h, w_), arrays in zip(sizes, images):
                batch = hc.image_batch(arrays, dev)
                for mirrored in ((False, True) if flip else (False,)):
                    try:
                        feat = model.features(batch.flip(3).contiguous() if mirrored else batch, task)
                    except RuntimeError as e:
                        raise RuntimeError(f"--scales: the eval forward refuses the {h} x {w_} input: {e}") from e
                    views.append((feat.contiguous(), mirrored))
            w, b = (t.detach() for t in model.head_params(task))
        return lambda s, e: [([(f[s:e], m) for f, m in views], w, b)]
    return heads


def main(args):
    _refusals(args)
    dev, nc, model = hc.load_model(args.state, args.num_classes, args.task)
    id_map = ls.load_label_ids(args.label_ids, nc).to(dev) if args.label_ids else None
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
        n_items, stems, sample = ls.open_data(a, nc)
        samplers.append(sample)
    with hc.png_pool() as pool:
        png = hc.PngWriter(pool, args.out)
        for run in ls.label_runs((n_items, stems, samplers), pool, dev, args.batch_size, [model], args.task, png=png,
                                 heads=view_heads(sizes, args.flip)):
            (views, w, b), = run.sources
            kw = dict(mode=args.mode, id_map=id_map, palette=palette, confidence=args.confidence)
            if meter is not None:
                label, colour, conf = meter.add(views, w, b, target=run.target, **kw)
            else:
                label, colour, conf = ensemble_head(views, w, b, tuple(run.target.shape[1:]), **kw)
            if args.out:
                conf8 = None if conf is None else conf.mul(255.0).round_().to(torch.uint8).cpu().numpy()
                run.write("_label.png", label.cpu().numpy())
                run.write("_colour.png", None if colour is None else colour.cpu().numpy())
                run.write("_conf.png", conf8)
    report = dict(ls.report_header(args, n_items, png), scales=[float(s) for s in args.scales], flip=bool(args.flip),
                  mode=args.mode)
    what = "scales " + " / ".join(f"{s:g}" for s in args.scales) + (" + flip" if args.flip else "")
    return hc.score_report(report, meter, args, f", {what}, {args.mode}")


def _refusals(args):
    """Raise a RuntimeError that names why this combination of flags is refused (before the GPU is
    touched): fullres's own refusals, then those of the ensemble's flags."""
    ls.refuse_map_flags(args)
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


def build_parser():
    p = ls.add_flags(hc.RefusingParser(_refusals, description="multi-scale / flip ensemble: label maps and mIoU at the "
                                                             "dataset's own size from a checkpoint"),
                     at_scale_1=" at scale 1")
    p.add_argument("--scales", type=float, nargs="+", default=[1.0],
                   help="one view per scale; the input is 8 * round(scale * size / 8) per axis")
    p.add_argument("--flip", action="store_true", help="every scale also mirrored")
    p.add_argument("--mode", choices=sorted(_ensemble_lib.MODES), default="prob",
                   help="add the views' probabilities (prob) or their logits (logit)")
    p.add_argument("--confidence", action="store_true", help="also write <stem>_conf.png (255 x confidence)")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
