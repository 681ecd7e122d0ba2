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
import json
import os

import numpy as np
import torch

from . import _fullres_lib
from . import _head_common as hc
from .predict import default_palette

# train id -> the dataset's own label id, the ignore class (last) -> 0
LABEL_IDS = {
    "cityscapes": bytes((7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33, 0)),
}


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
        bad = int(self.bad_targets.item())
        if bad:
            raise RuntimeError(f"mdil ConfusionMeter: {bad} target pixels are outside [0, {self.nc}) and are not the "
                               f"ignore index {self.ignore_index}")
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
def load_label_ids(spec, nc):
    """``--label-ids``: a name in LABEL_IDS or a JSON file with one id per class -> u8 [nc] (host)."""
    if spec in LABEL_IDS:
        ids = list(LABEL_IDS[spec])
    else:
        if not os.path.isfile(spec):
            raise RuntimeError(f"--label-ids {spec}: neither one of {sorted(LABEL_IDS)} nor a JSON file")
        with open(spec) as f:
            ids = json.load(f)
    if not isinstance(ids, list) or len(ids) != nc or any(not isinstance(v, int) or not 0 <= v <= 255 for v in ids):
        raise RuntimeError(f"--label-ids {spec}: expected {nc} integers in [0, 255]")
    return torch.tensor(ids, dtype=torch.uint8)


def resize_image(arr, height, width):
    """uint8 [Hn,Wn,3] -> uint8 [height,width,3], PIL bilinear (the validation transform's image half)."""
    from PIL import Image
    return np.asarray(Image.fromarray(arr).resize((width, height), Image.BILINEAR), dtype=np.uint8)


def synthetic_sample(ds, i, height, width):
    """Item ``i`` of a ProceduralSeg drawn at the native size -> (image u8 [height,width,3] resized
    for the network, label u8 [Hn,Wn] at the native size)."""
    img, lab = ds[i]
    u8 = img.mul(255.0).round_().to(torch.uint8).permute(1, 2, 0).contiguous().numpy()
    return resize_image(u8, height, width), lab[0].to(torch.uint8).numpy()


def _real_sample(ds, i, height, width, nc):
    image, label = ds[i]                                   # PIL, both at their own size
    lab = np.array(label, dtype=np.uint8)
    lab[lab == 255] = nc - 1                               # the validation path's relabel
    return resize_image(np.asarray(image.convert("RGB"), dtype=np.uint8), height, width), lab


def _open(args, nc):
    """-> (number of items, stems, sample(i) -> (image u8 [h,w,3], label u8 [Hn,Wn]))."""
    if args.synthetic:
        from .dataset import ProceduralSeg
        ds = ProceduralSeg(args.synthetic, args.native_height, args.native_width, nc, seed=12 + args.task,
                           domain=args.task)
        return len(ds), [f"synthetic_{j:04d}" for j in range(len(ds))], \
            lambda i: synthetic_sample(ds, i, args.height, args.width)
    from .dataset import _ALIASES, _CLASSES
    key = _ALIASES[args.dataset]
    root = {"cityscapes": args.cs_datadir, "BDD": args.bdd_datadir, "IDD": args.idd_datadir}[key]
    if not os.path.isdir(root):
        raise RuntimeError(f"dataset root for {args.dataset} not found: {root} (set the datadir flag or run with "
                           "--synthetic N)")
    ds = _CLASSES[key](root, None, args.subset)            # co_transform=None: image AND label at their own size
    stems = [os.path.splitext(os.path.basename(f))[0] for f in ds.filenames]
    if len(set(stems)) != len(stems):
        raise RuntimeError(f"image names under {root} are not unique: the outputs would collide")
    return len(ds), stems, lambda i: _real_sample(ds, i, args.height, args.width, nc)


def _runs(shapes):
    """[(start, stop)] of the maximal runs of equal consecutive entries."""
    out, i = [], 0
    for j in range(1, len(shapes) + 1):
        if j == len(shapes) or shapes[j] != shapes[i]:
            out.append((i, j))
            i = j
    return out


def main(args):
    _refusals(args)
    dev, nc, model = hc.load_model(args.state, args.num_classes, args.task)
    id_map = load_label_ids(args.label_ids, nc).to(dev) if args.label_ids else None
    palette = default_palette(nc).contiguous().to(dev) if args.colour else None
    meter = ConfusionMeter(nc, nc - 1) if args.score else None
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    n_items, stems, sample = _open(args, nc)
    with hc.png_pool() as pool:
        png = hc.PngWriter(pool, args.out)
        for i0 in range(0, n_items, args.batch_size):
            idx = range(i0, min(i0 + args.batch_size, n_items))
            items = list(pool.map(sample, idx))
            images = hc.image_batch([im for im, _ in items], dev)
            with torch.no_grad():
                feat = model.features(images, args.task).contiguous()
                w, b = (t.detach() for t in model.head_params(args.task))
            maps = []
            # one kernel call per run of images that share a native size
            for s, e in _runs([lab.shape for _, lab in items]):
                target = torch.from_numpy(np.stack([lab for _, lab in items[s:e]])).to(dev)
                kw = dict(id_map=id_map, palette=palette)
                if meter is not None:
                    label, colour = meter.add(feat[s:e], w, b, target=target, **kw)
                else:
                    label, colour = fullres_head(feat[s:e], w, b, tuple(target.shape[1:]), **kw)
                if args.out:
                    maps.append((s, label.cpu().numpy(), None if colour is None else colour.cpu().numpy()))
            png.wait()                         # the batch before this one: bounds what is in flight
            for s, label, colour in maps:
                for k in range(label.shape[0]):
                    png.submit(label[k], f"{stems[idx[s + k]]}_label.png")
                    if colour is not None:
                        png.submit(colour[k], f"{stems[idx[s + k]]}_colour.png")
        png.wait()
    report = {"dataset": "synthetic" if args.synthetic else args.dataset, "task": args.task, "images": n_items,
              "written": png.written}
    return hc.score_report(report, meter, args)


def _refusals(args):
    """Raise a RuntimeError that names why this combination of flags is refused."""
    if not args.score and not args.out:
        raise RuntimeError("nothing to do: give --score, --out DIR or both")
    if (args.colour or args.label_ids) and not args.out:
        raise RuntimeError("--colour and --label-ids need --out DIR")
    if args.json and not args.score:
        raise RuntimeError("--json writes the score: it needs --score")
    if not args.synthetic and not args.dataset:
        raise RuntimeError("give --dataset cityscapes|BDD|IDD or --synthetic N")
    if args.synthetic and args.dataset:
        raise RuntimeError("--dataset and --synthetic exclude each other")
    if min(args.height, args.width, args.batch_size, args.native_height, args.native_width) < 1:
        raise RuntimeError("sizes and --batch-size must be positive")


def add_flags(p, at_scale_1="", maps=True):
    """The flags of this command line, which ``python -m mdil_ss_amd.ensemble`` shares;
    ``maps=False``: those of ``python -m mdil_ss_amd.boundary``, which writes no label or colour map
    and can score maps already written instead of running a checkpoint."""
    from .dataset import add_datadir_flags
    p.add_argument("--state", required=maps, help="checkpoint written by the trainers (or by the reference)")
    p.add_argument("--num-classes", type=int, nargs="+", required=True)
    p.add_argument("--task", type=int, required=True, help="which task's decoder predicts")
    p.add_argument("--dataset", choices=("cityscapes", "BDD", "IDD"))
    p.add_argument("--subset", default="val")
    p.add_argument("--synthetic", type=int, default=0, help="N procedural images instead of a dataset")
    p.add_argument("--native-height", type=int, default=1024, help="--synthetic: the labels' own height")
    p.add_argument("--native-width", type=int, default=2048, help="--synthetic: the labels' own width")
    p.add_argument("--height", type=int, default=512, help="the network's input height" + at_scale_1)
    p.add_argument("--width", type=int, default=1024, help="the network's input width" + at_scale_1)
    p.add_argument("--batch-size", type=int, default=6)
    p.add_argument("--score", action="store_true", help="mIoU and per-class IoU against the full-size labels")
    p.add_argument("--json", help="write the score (with the confusion matrix) here")
    p.add_argument("--out", help="write <stem>_label.png at the image's own size into this folder" if maps else
                   "write <stem>_boundary.png at the image's own size into this folder")
    if maps:
        p.add_argument("--colour", action="store_true", help="also write <stem>_colour.png")
        p.add_argument("--label-ids", help=f"label PNGs in the dataset's own ids: one of {sorted(LABEL_IDS)} or a "
                                           "JSON file with one id per class (default: train ids)")
    add_datadir_flags(p)
    return p


def build_parser():
    return add_flags(hc.RefusingParser(_refusals, description="label maps and mIoU at the dataset's own size from a "
                                                             "checkpoint"))


if __name__ == "__main__":
    main(build_parser().parse_args())
