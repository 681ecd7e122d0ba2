"""Label maps and scores at the DATASET's own size on MI355X: ``output_conv`` + bilinear resize of
the logits (half-pixel centres, ``align_corners=False``) + argmax, with the confusion matrix against
the full-size ground truth counted in the same pass -- one fused kernel straight from the decoder's
16-channel features, so neither the logits nor the resized logits are stored
(include/mdil_fullres.h).

    python -m mdil_ss_amd.fullres --state model_best_....pth.tar --num-classes 20 20 27 --task 0 \
        --dataset cityscapes [--cs-datadir ...] [--score] [--json FILE] \
        [--out DIR [--colour] [--label-ids cityscapes|FILE.json]]

The image is resized to ``--height x --width`` for the network (PIL bilinear, as the validation
transform does); the label keeps its own size and the maps come out at that size.  ``--score``
reports mIoU and per-class IoU by the reference's ``iouEval`` rule; ``--out`` writes
``<stem>_label.png`` (train ids, or the dataset's own ids with ``--label-ids``) and, on request,
``<stem>_colour.png``.  ``--synthetic N --native-height Hn --native-width Wn`` does the same on the
procedural dataset drawn at the native size."""
import functools
import os

import torch

from . import _fullres_lib
from . import _head_common as hc
from . import _labelsize_common as ls
from . import _report_common as rc
from ._labelsize_common import LABEL_IDS, load_label_ids, resize_image, synthetic_sample  # noqa: F401  (public here)
from .predict import default_palette

_FN, _PATH = "fullres_head", "full-resolution"
_chk = functools.partial(hc.chk, _FN, _PATH)


def fullres_head(features, weight, bias, out_size, *, id_map=None, palette=None, target=None, ignore_index=-1,
                 confusion=None, bad_targets=None):
    """``output_conv`` + bilinear resize of the logits to ``out_size`` = (Ho, Wo) + argmax on NHWC
    decoder features [N,H,W,16] and the ``ConvTranspose2d(16, nc, 2, 2)`` parameters, 2 <= nc <= 32,
    on the current stream.  -> (label u8 [N,Ho,Wo], colour u8 [N,Ho,Wo,3] or None).

    ``id_map`` (u8 [nc], device): the byte written for each class (default: the class index);
    ``palette`` (u8 [nc,3], device): the colour map is written when given.  With ``target``
    (u8 [N,Ho,Wo], device, train ids) the pixels are counted INTO ``confusion`` (i64 [nc,nc], device;
    row = target, column = predicted train id) and targets >= nc other than ``ignore_index`` into
    ``bad_targets`` (i64 [1], device); both are accumulated into, never cleared."""
    lib = _fullres_lib.load()
    _chk(features, "features")
    _chk(weight, "weight")
    _chk(bias, "bias")
    x, w, b = features, weight, bias
    nc = hc.check_params(_FN, w, b, x)
    N, H, W = x.shape[0], x.shape[1], x.shape[2]
    hc.check_classes(_FN, _fullres_lib, nc, x, w, b)
    Ho, Wo = hc.check_out_size(_FN, _fullres_lib, out_size)
    hc.check_scoring(_FN, _PATH, x.device, N, nc, Ho, Wo, id_map, palette, target, confusion, bad_targets, ignore_index)
    with torch.no_grad(), torch.cuda.device(x.device):
        label = torch.empty(N, Ho, Wo, dtype=torch.uint8, device=x.device)
        colour = None if palette is None else torch.empty(N, Ho, Wo, 3, dtype=torch.uint8, device=x.device)
        _fullres_lib.check(
            lib.mdil_fullres_head(x.data_ptr(), w.data_ptr(), b.data_ptr(), N, H, W, nc, Ho, Wo, hc.ptr(id_map),
                                  hc.ptr(palette), hc.ptr(target), int(ignore_index), label.data_ptr(),
                                  hc.ptr(colour), hc.ptr(confusion), hc.ptr(bad_targets),
                                  torch.cuda.current_stream(x.device).cuda_stream),
            "mdil_fullres_head")
    return label, colour


def predict_fullres(model, images, task, out_size, **kw):
    """Label (and colour) maps of ``images`` [N,3,H,W] for ``task`` at ``out_size``: the model's
    decoder features, then ``fullres_head`` with that task's ``output_conv`` parameters."""
    model.eval()
    with torch.no_grad():
        feat = model.features(images, task)
        w, b = model.head_params(task)
        return fullres_head(feat.contiguous(), w.detach(), b.detach(), out_size, **kw)


class ConfusionMeter:
    """Confusion matrix (row = target, column = prediction) of full-size predictions, counted on
    the device by the fused kernel and scored by the reference's ``iouEval`` rule."""

    def __init__(self, nc, ignore_index):
        self._name, self._model_fn, self._head_fn = "ConfusionMeter", predict_fullres, fullres_head
        self.nc, self.ignore_index = int(nc), int(ignore_index)
        self.confusion = self.bad_targets = None

    def add(self, *source, target, **kw):
        """``add(model, images, task, target=t)`` or ``add(features, weight, bias, target=t)``;
        ``target``: u8 [N,Ho,Wo] train ids on the device, which also sets the output size.
        -> (label, colour or None) of that call."""
        if not isinstance(target, torch.Tensor) or target.dim() != 3:
            raise RuntimeError(f"mdil {self._name}.add: target must be a uint8 [N,Ho,Wo] device tensor")
        if self.confusion is None:
            self.confusion = torch.zeros(self.nc, self.nc, dtype=torch.int64, device=target.device)
            self.bad_targets = torch.zeros(1, dtype=torch.int64, device=target.device)
        kw.update(target=target, ignore_index=self.ignore_index, confusion=self.confusion,
                  bad_targets=self.bad_targets)
        fn = self._model_fn if isinstance(source[0], torch.nn.Module) else self._head_fn
        return fn(*source, tuple(target.shape[1:]), **kw)

    def matrix(self):
        """int64 [nc,nc] on the host; raises when a target outside [0, nc) (other than the ignore
        index) was met."""
        if self.confusion is None:
            return torch.zeros(self.nc, self.nc, dtype=torch.int64)
        rc.refuse_bad_pixels("ConfusionMeter", self.nc, self.ignore_index, self.bad_targets)
        return self.confusion.cpu()

    def iou(self, matrix=None):
        """-> (mean, per_class) in float64: tp = diagonal, fp = column sum - tp, fn = row sum - tp,
        tp / (tp + fp + fn + 1e-15); the ignore class is left out of the classes and of the mean."""
        m = (self.matrix() if matrix is None else matrix).double()
        return iou_rule(self.nc, self.ignore_index, m.diagonal(), m.sum(0), m.sum(1))


def iou_rule(nc, ignore_index, both, predicted, labelled):
    """The ``iouEval`` rule on per-class float64 counts [nc]: ``both`` pixels in the intersection,
    ``predicted`` and ``labelled`` in each of the two sets -> (mean, per_class) of
    both / (union + 1e-15); the ignore class is left out of the classes and of the mean.
    ``ConfusionMeter.iou`` and ``boundary.BoundaryMeter`` score with it."""
    k = nc - 1 if 0 <= ignore_index < nc else nc
    if 0 <= ignore_index < nc - 1:
        raise RuntimeError("mdil ConfusionMeter: the ignore class must be the last one (iouEval's rule)")
    fp, fn = predicted - both, labelled - both
    iou = (both / (both + fp + fn + 1e-15))[:k]
    return iou.mean(), iou


# ------------------------------------------------------------------------------------------ CLI
def main(args):
    ls.refuse_map_flags(args)
    dev, nc, model = hc.load_model(args.state, args.num_classes, args.task)
    id_map = load_label_ids(args.label_ids, nc).to(dev) if args.label_ids else None
    palette = default_palette(nc).contiguous().to(dev) if args.colour else None
    meter = ConfusionMeter(nc, nc - 1) if args.score else None
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    data = ls.open_data(args, nc)
    with hc.png_pool() as pool:
        png = hc.PngWriter(pool, args.out)
        for run in ls.label_runs(data, pool, dev, args.batch_size, [model], args.task, png=png):
            (feat, w, b), = run.sources
            kw = dict(id_map=id_map, palette=palette)
            if meter is not None:
                label, colour = meter.add(feat, w, b, target=run.target, **kw)
            else:
                label, colour = fullres_head(feat, w, b, tuple(run.target.shape[1:]), **kw)
            if args.out:
                run.write("_label.png", label.cpu().numpy())
                run.write("_colour.png", None if colour is None else colour.cpu().numpy())
    return hc.score_report(ls.report_header(args, data[0], png), meter, args)


def build_parser():
    return ls.add_flags(hc.RefusingParser(ls.refuse_map_flags, description="label maps and mIoU at the dataset's own "
                                                                           "size from a checkpoint"))


if __name__ == "__main__":
    main(build_parser().parse_args())
