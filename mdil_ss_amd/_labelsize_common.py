"""What the label-size drivers (fullres.py, ensemble.py, boundary.py, segments.py, significance.py)
share on top of _head_common.py and _report_common.py: the dataset opened with the labels at their own
size, the batch loop over runs of equal native size with its bounded PNG writing, the step that turns
what a meter's ``add`` was given into checked label maps, and the flags, refusals and report header of
the command lines.  Plain functions; each takes the caller's name where a message carries it, so every
message reads as it always did."""
import json
import os

import numpy as np
import torch

from . import _head_common as hc
from . import _report_common as rc


# ----------------------------------------------------------------------- the data at label size
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


def real_sample(ds, i, height, width, nc):
    image, label = ds[i]                                   # PIL, both at their own size
    lab = np.array(label, dtype=np.uint8)
    lab[lab == 255] = nc - 1                               # the validation path's relabel
    return resize_image(np.asarray(image.convert("RGB"), dtype=np.uint8), height, width), lab


def open_data(args, nc):
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
    return len(ds), stems, lambda i: real_sample(ds, i, args.height, args.width, nc)


def runs(shapes):
    """[(start, stop)] of the maximal runs of equal consecutive entries."""
    out, i = [], 0
    for j in range(1, len(shapes) + 1):
        if j == len(shapes) or shapes[j] != shapes[i]:
            out.append((i, j))
            i = j
    return out


def read_label_png(folder, stem, shape):
    """``<stem>_label.png`` of ``folder`` as u8 [H,W]; its size must be the label's."""
    from PIL import Image
    path = os.path.join(folder, f"{stem}_label.png")
    if not os.path.isfile(path):
        raise RuntimeError(f"--pred {folder}: {stem}_label.png not found")
    with Image.open(path) as im:
        arr = np.array(im)
    if arr.ndim != 2 or arr.dtype != np.uint8:
        raise RuntimeError(f"--pred {folder}: {stem}_label.png is not an 8-bit single-channel label map")
    if arr.shape != tuple(shape):
        raise RuntimeError(f"--pred {folder}: {stem}_label.png is {arr.shape[0]} x {arr.shape[1]}, its label "
                           f"{shape[0]} x {shape[1]}")
    return arr


# ------------------------------------------------------------------------------- the batch loop
def load_predictors(args):
    """``--pred DIR`` or ``--state CHECKPOINT`` -> (device, class count of ``--task``, models, folders)."""
    if args.pred:
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        return dev, args.num_classes[args.task], [], [args.pred]
    dev, nc, model = hc.load_model(args.state, args.num_classes, args.task)
    return dev, nc, [model], []


def model_heads(models, task, images, dev):
    """The hook of ``label_runs`` that every driver but the ensemble uses: the batch's images (one
    sampler) uploaded once and run through every model -> cut(s, e): per model the head's inputs
    (features[s:e], weight, bias) of the items s .. e - 1."""
    batch = hc.image_batch(images[0], dev)
    with torch.no_grad():
        heads = [(m.features(batch, task).contiguous(), *(t.detach() for t in m.head_params(task))) for m in models]
    return lambda s, e: [(feat[s:e], w, b) for feat, w, b in heads]


class Run:
    """The items of a batch that share a native size: ``stems``, ``target`` (u8 [n,Hn,Wn] on the
    device) and one entry of ``sources`` per predictor -- what the hook's cut gives for the models,
    then the label maps (u8 [n,Hn,Wn] on the device) read from each folder.  ``write(suffix, maps)``
    hands back host maps [n,...] to be written as ``<stem><suffix>`` once the batch is through."""

    def __init__(self, stems, target, sources):
        self.stems, self.target, self.sources, self.maps = stems, target, sources, []

    def write(self, suffix, maps):
        if maps is not None:
            self.maps.append((suffix, maps))


def label_runs(data, pool, dev, batch_size, models=(), task=None, folders=(), png=None, heads=model_heads):
    """The loop of the label-size drivers over ``data`` = (number of items, stems, sample) as
    ``open_data`` gives it (``sample``: one sampler, or one per input size): per batch the items are
    sampled on ``pool``, ``heads(models, task, images, dev)`` turns the images (per sampler the batch's
    u8 arrays) into the predictors' inputs, and one ``Run`` is yielded per run of equal native size,
    so a caller makes one kernel call per run.  The maps a caller hands to ``Run.write`` go to ``png``
    (a ``PngWriter``) after the batch's last run, behind a ``wait()`` that bounds what is in flight."""
    n_items, stems, sample = data
    samplers = list(sample) if isinstance(sample, (list, tuple)) else [sample]
    for i0 in range(0, n_items, batch_size):
        idx = range(i0, min(i0 + batch_size, n_items))
        items = list(pool.map(lambda ki: samplers[ki[0]](ki[1]), [(k, i) for k in range(len(samplers)) for i in idx]))
        per_sampler = [items[k * len(idx):(k + 1) * len(idx)] for k in range(len(samplers))]
        labels = [lab for _, lab in per_sampler[0]]
        cut = heads(models, task, [[im for im, _ in part] for part in per_sampler], dev) if models else None
        written = []
        # one run, so one kernel call of the caller's, per stretch of images that share a native size
        for s, e in runs([lab.shape for lab in labels]):
            names = [stems[i] for i in idx[s:e]]
            target = torch.from_numpy(np.stack(labels[s:e])).to(dev)
            sources = cut(s, e) if cut else []
            for folder in folders:
                read = [read_label_png(folder, name, lab.shape) for name, lab in zip(names, labels[s:e])]
                sources.append(torch.from_numpy(np.stack(read)).to(dev))
            run = Run(names, target, sources)
            written.append((names, run.maps))
            yield run
        if png is not None:
            png.wait()                         # the batch before this one: bounds what is in flight
            for names, maps in written:
                for k, name in enumerate(names):
                    for suffix, stack in maps:
                        png.submit(stack[k], name + suffix)
    if png is not None:
        png.wait()


# ------------------------------------------------------------------------------------ the meters
def label_maps(who, source, target, paired=False):
    """What a meter's ``add(*source, target=target)`` was given -> (the predictors' label maps, u8
    [N,H,W] on the device at ``target``'s size, and ``target``).  ``(pred, target)``, ``(model, images,
    task, target=...)`` or ``(features, weight, bias, target=...)``; otherwise (``paired``: two) one
    entry per predictor, each a label map or such a triple, which first goes through
    ``fullres.predict_fullres`` / ``fullres_head``.  ``who`` = (the meter, the entry point, the path):
    how the refusals call the caller."""
    from .fullres import fullres_head, predict_fullres
    meter, fn, path = who
    if not paired and len(source) == 2 and target is None:
        source, target = source[:1], source[1]
    elif not paired and len(source) == 3 and target is not None:
        source = (tuple(source),)
    elif not (len(source) == (2 if paired else 1) and target is not None):
        raise RuntimeError(f"mdil {meter}.add: expects " + (
            "(a, b, target=...), each of a and b a label map, (model, images, task) or (features, weight, bias)"
            if paired else
            "(pred, target), (model, images, task, target=...) or (features, weight, bias, target=...)"))
    if not isinstance(target, torch.Tensor) or target.dim() != 3:
        raise RuntimeError(f"mdil {meter}.add: target must be a uint8 [N,H,W] device tensor")
    hc.chk(fn, path, target, "target", torch.uint8)
    preds = []
    for one in source:
        if isinstance(one, (tuple, list)) and len(one) == 3:
            head = predict_fullres if isinstance(one[0], torch.nn.Module) else fullres_head
            one = head(*one, tuple(target.shape[1:]))[0]
        elif not isinstance(one, torch.Tensor):
            raise RuntimeError(f"mdil {meter}.add: a predictor is a uint8 [N,H,W] label map, (model, images, "
                               "task) or (features, weight, bias)")
        hc.chk(fn, path, one, "pred", torch.uint8)
        if one.shape != target.shape:
            raise RuntimeError(f"mdil {meter}.add: pred {tuple(one.shape)} and target {tuple(target.shape)} must be "
                               "uint8 [N,H,W] maps of one size")
        preds.append(one)
    return preds, target


# -------------------------------------------------------------------------------- command lines
# train id -> the dataset's own label id, the ignore class (last) -> 0
LABEL_IDS = {
    "cityscapes": bytes((7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33, 0)),
}


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


def add_flags(p, *, label_maps=True, required=("state", "num_classes", "task"), pred=False, at_scale_1="",
              out_help="write <stem>_label.png at the image's own size into this folder"):
    """The flags the label-size command lines share; the defaults are those of fullres and ensemble.
    ``label_maps``: the command line writes label maps, so ``--colour`` and ``--label-ids`` exist;
    ``required``: which of "state", "num_classes" and "task" the parser demands; ``pred``: ``--pred DIR``
    exists, label maps already written in place of ``--state``; ``at_scale_1``: appended to the help of
    ``--height`` and ``--width``; ``out_help``: what ``--out`` writes."""
    from .dataset import add_datadir_flags
    p.add_argument("--state", required="state" in required,
                   help="checkpoint written by the trainers (or by the reference)")
    p.add_argument("--num-classes", type=int, nargs="+", required="num_classes" in required)
    p.add_argument("--task", type=int, required="task" in required, help="which task's decoder predicts")
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
    p.add_argument("--out", help=out_help)
    if label_maps:
        p.add_argument("--colour", action="store_true", help="also write <stem>_colour.png")
        p.add_argument("--label-ids", help=f"label PNGs in the dataset's own ids: one of {sorted(LABEL_IDS)} or a "
                                           "JSON file with one id per class (default: train ids)")
    add_datadir_flags(p)
    if pred:
        p.add_argument("--pred", help="score the <stem>_label.png files (train ids) of this folder instead of --state")
    return p


def refuse_idle(args, or_else=""):
    if not args.score and not args.out:
        raise RuntimeError(f"nothing to do: give --score, --out DIR or both{or_else}")


def refuse_json_without_score(args):
    if args.json and not args.score:
        raise RuntimeError("--json writes the score: it needs --score")


def refuse_map_flags(args):
    """The refusals of a command line that writes label maps (fullres; ensemble adds its own)."""
    refuse_idle(args)
    if (args.colour or args.label_ids) and not args.out:
        raise RuntimeError("--colour and --label-ids need --out DIR")
    refuse_json_without_score(args)
    refuse_data(args)


def refuse_sources(args):
    """``--state`` or ``--pred``: one of them."""
    if args.pred and args.state:
        raise RuntimeError("--pred scores maps already written and --state runs a checkpoint: give one of them")
    if not args.pred and not args.state:
        raise RuntimeError("give --state CHECKPOINT or --pred DIR")


def refuse_data(args):
    """``rc.refuse_data`` and the labels' own size."""
    rc.refuse_data(args)
    if min(args.native_height, args.native_width) < 1:
        raise RuntimeError("sizes and --batch-size must be positive")


def report_header(args, n_items, png):
    """How every report but significance's opens; ``hc.score_report`` closes it."""
    return {"dataset": "synthetic" if args.synthetic else args.dataset, "task": args.task, "images": n_items,
            "written": png.written}
