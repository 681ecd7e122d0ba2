"""What the report drivers (drift.py, calibrate.py, similarity.py, boundary.py, pseudo.py, route.py,
segments.py, refine.py, significance.py, openset.py, audit.py, acquire.py, ripu.py) share on top of
_head_common.py: the network-size batch feeders (a dataset, or a folder of images), the counter and
workspace checks of the entry points, the workspace, source and bad-target steps of the meters, the
label tree that audit, acquire and ripu write, and the flags and refusals of the command lines.  Plain
functions; each takes the caller's name where a message carries it, so every message reads as it
always did.  What only the annotator family (audit, acquire, ripu) shares -- its refusals and flags, the
writer of that label tree, the annotated block of the report -- is one level up, in _annotate_common.py; what
the label-size family (fullres, ensemble, boundary, segments, significance) shares -- the data at the labels' own
size, its batch loop, the meters' prologue, its flags and refusals -- likewise, in _labelsize_common.py."""
import os

import torch

from . import _head_common as hc


# ------------------------------------------------------------------------- entry-point checks
def check_counters(fn, counters, known):
    """-> {name: tensor or None} over ``known``; a name outside it is refused."""
    c = dict(counters or {})
    unknown = sorted(set(c) - set(known))
    if unknown:
        raise RuntimeError(f"mdil {fn}: unknown counters {unknown} (known: {list(known)})")
    return {k: c.get(k) for k in known}


def check_workspace(fn, path, dev, c, need):
    """``c["sums"]`` need ``c["workspace"]``, float64 of at least ``need()`` bytes on ``dev``.
    -> (pointer, bytes) for the entry point: (None, 0) without sums."""
    if c["sums"] is None:
        return None, 0
    need, ws = need(), c["workspace"]
    if ws is None:
        raise RuntimeError(f"mdil {fn}: sums need a workspace (float64, {need} bytes) on the device")
    hc.chk(fn, path, ws, "workspace", torch.float64)
    ws_bytes = ws.numel() * 8
    if ws.device != dev or ws_bytes < need:
        raise RuntimeError(f"mdil {fn}: workspace must hold {need} bytes on {dev} (got {ws_bytes} on {ws.device})")
    return ws.data_ptr(), ws_bytes


# -------------------------------------------------------------------------------------- meters
def grow_workspace(tensors, need_bytes, dev):
    """``tensors["workspace"]`` holds at least ``need_bytes``: allocated anew when too small."""
    need = need_bytes // 8
    ws = tensors.get("workspace")
    if ws is None or ws.numel() < need:
        tensors["workspace"] = torch.empty(need, dtype=torch.float64, device=dev)


def meter_source(who, path, source, images_at, on_images, on_features, feat_name):
    """What ``add(*source)`` was given: models with the images at ``source[images_at]``, or NHWC
    features first.  -> (``on_images`` or ``on_features``, device, N, H, W of the features)."""
    if isinstance(source[0], torch.nn.Module):
        images = source[images_at]
        if not isinstance(images, torch.Tensor) or images.dim() != 4:
            raise RuntimeError(f"mdil {who}.add: images must be a float32 [N,3,H,W] device tensor")
        fn, dev, N, H, W = on_images, images.device, images.shape[0], images.shape[2] // 2, images.shape[3] // 2
    else:
        feat = source[0]
        if not isinstance(feat, torch.Tensor) or feat.dim() != 4:
            raise RuntimeError(f"mdil {who}.add: {feat_name} must be NHWC features [N,H,W,16]")
        fn, dev, (N, H, W) = on_features, feat.device, feat.shape[:3]
    if dev.type != "cuda":
        raise RuntimeError(f"mdil {who}.add: inputs must be device tensors; there is no CPU fallback in the "
                           f"{path} path")
    return fn, dev, N, H, W


def refuse_bad_pixels(who, nc, ignore_index, bad_targets, bad_preds=None):
    """A meter's counts (int64 device tensors of one element) of the target pixels outside [0, nc) other than
    the ignore index and, where it keeps one, of the predicted pixels outside [0, nc): either refuses."""
    bad = int(bad_targets.item())
    if bad:
        raise RuntimeError(f"mdil {who}: {bad} target pixels are outside [0, {nc}) and are not the "
                           f"ignore index {ignore_index}")
    bad = 0 if bad_preds is None else int(bad_preds.item())
    if bad:
        raise RuntimeError(f"mdil {who}: {bad} predicted pixels are outside [0, {nc})")


def refuse_bad_targets(who, tensors, nc, ignore_index):
    refuse_bad_pixels(who, nc, ignore_index, tensors["bad_targets"])


# -------------------------------------------------------------------------------- command lines
def batches(args, nc, dev, score=True, unique_stems=False):
    """The validation set at the network's size, from ``--synthetic N`` or ``--dataset`` (opened as
    evaluate.py opens it).  -> (stems, images f32 [n,3,H,W], target u8 [n,H,W] or None without
    ``score``) per batch, on the device.  ``unique_stems``: refuse a dataset whose outputs would collide."""
    bs = args.batch_size
    if args.synthetic:
        from .dataset import ProceduralSeg
        ds = ProceduralSeg(args.synthetic, args.height, args.width, nc, seed=12 + args.task, domain=args.task)
        for i in range(0, len(ds), bs):
            items = [ds[j] for j in range(i, min(i + bs, len(ds)))]
            target = torch.stack([lab[0] for _, lab in items]).to(torch.uint8).to(dev) if score else None
            yield ([f"synthetic_{j:04d}" for j in range(i, i + len(items))],
                   torch.stack([im for im, _ in items]).to(dev), target)
        return
    from . import ops
    from .dataset import open_dataset
    ds = open_dataset(args.dataset, args.subset, args, augment=False)
    names = getattr(ds, "base", ds).filenames
    stems = [os.path.splitext(os.path.basename(f))[0] for f in names]
    if unique_stems and len(set(stems)) != len(stems):
        raise RuntimeError(f"image names of {args.dataset} are not unique: the outputs would collide")
    for i in range(0, len(ds), bs):
        items = [ds[j] for j in range(i, min(i + bs, len(ds)))]
        img, lab, params = (torch.stack([it[k] for it in items]).to(dev) for k in range(3))
        images, labels = ops.augment_batch(img, lab, params, nc)       # no flip, no shift; 255 -> nc - 1
        yield stems[i:i + len(items)], images, labels[:, 0].to(torch.uint8).contiguous() if score else None


def image_or_dataset_batches(args, nc, pool, dev, score=True, unique_stems=False):
    """``--images DIR`` (no targets) or ``batches``.  -> (stems, images f32 [n,3,H,W], target u8 [n,H,W] or
    None) per batch, on the device."""
    if args.images:
        for stems, images in hc.image_batches(args, pool, dev):
            yield stems, images, None
        return
    yield from batches(args, nc, dev, score=score, unique_stems=unique_stems)


def source_name(args):
    """What a report calls its source of images."""
    return "images" if getattr(args, "images", None) else "synthetic" if args.synthetic else args.dataset


def plan_label_tree(args, root):
    """The folders of a label tree under ``root`` (``audit --clean-root``, ``acquire --out-root``), laid out
    as ``--layout`` says, and the label file of every image, in the order of the batches.  A dataset's
    images are linked (``pseudo.plan_tree``); procedural images have no files, so they are written beside
    their labels.  -> (labels' folder, label names, images' folder or None)"""
    from argparse import Namespace
    from . import pseudo as P
    img_dir, lab_dir = P.LAYOUTS[args.layout]
    if args.synthetic:
        images = os.path.join(root, img_dir, args.subset)
        labels = os.path.join(root, lab_dir, args.subset)
        os.makedirs(images, exist_ok=True)
        os.makedirs(labels, exist_ok=True)
        stems = [f"synthetic_{j:04d}" for j in range(args.synthetic)]
        return labels, [P.label_name(args.layout, s) for s in stems], images
    from .dataset import open_dataset
    ds = open_dataset(args.dataset, args.subset, args, augment=False)
    base = getattr(ds, "base", ds)
    plan = Namespace(images=base.images_root, layout=args.layout, out_root=root, subset=args.subset)
    labels, names = P.plan_tree(plan, base.filenames)
    return labels, names, None


def add_data_flags(p, dataset_help=None, synthetic_help="N procedural images instead of a dataset"):
    """--dataset, --subset, --synthetic, --height, --width, --batch-size and the datasets' root folders."""
    from .dataset import add_datadir_flags
    p.add_argument("--dataset", choices=("cityscapes", "BDD", "IDD"), help=dataset_help)
    p.add_argument("--subset", default="val")
    p.add_argument("--synthetic", type=int, default=0, help=synthetic_help)
    p.add_argument("--height", type=int, default=512, help="the network's input height")
    p.add_argument("--width", type=int, default=1024, help="the network's input width")
    p.add_argument("--batch-size", type=int, default=6)
    add_datadir_flags(p)


def refuse_task(task, num_classes, name=""):
    """``name``: "" or which model ("--before ")."""
    if not 0 <= task < len(num_classes):
        raise RuntimeError(f"--task {task}: the {name}model has tasks 0 to {len(num_classes) - 1}")


def refuse_pair(args):
    """--task within both models of a before/after pair, and their heads of one width.  -> that width"""
    refuse_task(args.task, args.before_num_classes, "--before ")
    refuse_task(args.task, args.after_num_classes, "--after ")
    ca, cb = args.before_num_classes[args.task], args.after_num_classes[args.task]
    if ca != cb:
        raise RuntimeError(f"--task {args.task}: {ca} classes before and {cb} after; the heads must agree")
    return ca


def refuse_data(args):
    """--dataset xor --synthetic, and positive sizes."""
    if not args.synthetic and not args.dataset:
        raise RuntimeError("give --dataset cityscapes|BDD|IDD or --synthetic N")
    if args.synthetic and args.dataset:
        raise RuntimeError("--dataset and --synthetic exclude each other")
    if min(args.height, args.width, args.batch_size) < 1 or args.synthetic < 0:
        raise RuntimeError("sizes and --batch-size must be positive")
