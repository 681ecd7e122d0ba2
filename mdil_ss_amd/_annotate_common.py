"""What the annotator family (acquire.py, ripu.py, audit.py) shares on top of _report_common.py: the flags and
refusals of the two acquisition command lines (audit takes the two about its label tree), the path checks, the
opened head, the batch feeder, ``read_labels`` and ``LabelTreeWriter`` for the label trees they read and write,
and the annotated block and ``selection.json`` of the two reports.  Plain functions and one small class; where
a message names a flag or a program the caller passes it, so every message reads as it always did."""
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import _head_common as hc
from . import _report_common as rc


def refuse_head(args, share_of, max_pixels=None):
    """The shared head: one source, positive even sizes (at most ``max_pixels``), something to write, a budget."""
    if sum(bool(v) for v in (args.images, args.dataset, args.synthetic)) != 1:
        raise RuntimeError("give one source of images: --images DIR, --dataset cityscapes|BDD|IDD or --synthetic N")
    if min(args.height, args.width, args.batch_size) < 1 or args.synthetic < 0:
        raise RuntimeError("sizes and --batch-size must be positive")
    if args.height % 2 or args.width % 2:
        raise RuntimeError("--height and --width must be even")
    if max_pixels and args.height * args.width > max_pixels:
        raise RuntimeError(f"--height {args.height} x --width {args.width}: at most 2^24 pixels per image")
    if not (args.json or args.out or args.out_root):
        raise RuntimeError("nothing to do: give --json FILE, --out DIR or --out-root ROOT")
    if not 0.0 < args.budget <= 1.0:
        raise RuntimeError(f"--budget {args.budget} outside (0, 1]: a share of {share_of} pixels")


def refuse_tree(args, flag, root):
    """A label tree under ``root`` (``flag``: --out-root or --clean-root) comes with a layout, and not from IDD."""
    if bool(root) != bool(args.layout):
        raise RuntimeError(f"{flag} and --layout cityscapes|BDD go together")
    if root and args.dataset == "IDD":
        raise RuntimeError(f"{flag} does not take --dataset IDD: its loaders remap level-3 ids, so the label "
                           "files would need the inverse map")


def refuse_rounds(args):
    """The shared tail: what needs labels, the tree's layout, and what goes with an earlier round."""
    if args.images and args.by == "oracle":
        raise RuntimeError("--by oracle needs labels: give --dataset or --synthetic")
    if args.out_root and args.images:
        raise RuntimeError("--out-root writes what an annotator would answer: it needs labels (--dataset or --synthetic); "
                           "with --images give --out DIR")
    refuse_tree(args, "--out-root", args.out_root)
    if (args.previous_root or args.fill_root) and not args.out_root:
        raise RuntimeError("--previous-root and --fill-root are label trees laid out as --out-root lays its own: they need "
                           "--out-root and --layout")
    if args.previous_root and not args.previous:
        raise RuntimeError("--previous-root goes with --previous SEL.json, the selection that tree was written for")


def add_source_flags(p, budget_help):
    """--state to --budget: the checkpoint, the source of images (``--subset`` defaults to train) and the budget."""
    p.add_argument("--state", required=True, help="checkpoint written by the trainers (or by the reference)")
    p.add_argument("--num-classes", type=int, nargs="+", required=True)
    p.add_argument("--task", type=int, required=True, help="which task's decoder predicts")
    p.add_argument("--images", help="folder of unlabelled .jpg / .png images (searched recursively)")
    rc.add_data_flags(p, dataset_help="a labelled dataset instead: the run simulates the annotator",
                      synthetic_help="N procedural images instead (labelled)")
    p.set_defaults(subset="train")
    p.add_argument("--budget", type=float, required=True, help=budget_help)


def add_criterion_flags(p, kinds, criteria, by_help):
    p.add_argument("--kind", choices=kinds, default="entropy", help="the per-pixel uncertainty (default %(default)s)")
    p.add_argument("--by", choices=criteria, default="ripu", help=f"{by_help} (default %(default)s)")
    p.add_argument("--seed", type=int, default=0, help="of --by random (default %(default)s)")


def add_round_flags(p, previous_help, out_help):
    """--previous to --layout: the earlier round, the fill labels and where to write."""
    p.add_argument("--previous", help=f"an earlier round's selection.json: {previous_help}")
    p.add_argument("--previous-root", help="the label tree of that round: its labelled pixels are kept")
    p.add_argument("--fill-root", help="a label tree (pseudo --out-root, say) for the pixels still empty")
    p.add_argument("--json", help="write the report here")
    p.add_argument("--out", help=f"write <stem>_select.png (255 selected, 128 kept, 64 filled) and {out_help} here")
    p.add_argument("--out-root", help="with labels: write a dataset tree the trainers open as --cs-datadir / --bdd-datadir")
    p.add_argument("--layout", choices=("cityscapes", "BDD"), help="the tree --out-root writes")


def open_head(args):
    """Checks the task and the paths of earlier rounds, then opens the checkpoint -> dev, nc, model, the head's w and b,
    size, labelled, ignore (the trainers' relabelled ignore class), ign (the kernels': ignore, or -1 without labels)."""
    rc.refuse_task(args.task, args.num_classes)
    for flag, path, there, what in (("--previous", args.previous, os.path.isfile, "file"),
                                    ("--previous-root", args.previous_root, os.path.isdir, "folder"),
                                    ("--fill-root", args.fill_root, os.path.isdir, "folder")):
        if path and not there(path):
            raise RuntimeError(f"{flag} {path}: no such {what}")
    dev, nc, model = hc.load_model(args.state, args.num_classes, args.task)
    w, b = (t.detach() for t in model.head_params(args.task))
    labelled = not args.images
    return SimpleNamespace(dev=dev, nc=nc, model=model, w=w, b=b, task=args.task, size=(args.height, args.width),
                           labelled=labelled, ignore=nc - 1, ign=nc - 1 if labelled else -1)


def features(head, images):
    with torch.no_grad():
        return head.model.features(images, head.task).contiguous()


def batches(args, head, pool):
    """(stems, images, target or None) per batch on the device, each image of the network's size."""
    for stems, images, target in rc.image_or_dataset_batches(args, head.nc, pool, head.dev, unique_stems=True):
        if tuple(images.shape[2:]) != head.size:
            raise RuntimeError(f"images of {tuple(images.shape[2:])}, expected {head.size}")
        yield stems, images, target


def read_labels(root, layout, subset, names, size, what):
    """The label files ``names`` of a tree written by ``--out-root`` -> u8 [n, Hl, Wl] (host)."""
    from PIL import Image
    from . import pseudo as P
    folder = os.path.join(root, P.LAYOUTS[layout][1], subset)
    maps = []
    for name in names:
        path = os.path.join(folder, name)
        if not os.path.isfile(path):
            raise RuntimeError(f"{what} {root}: no label file {path}")
        with Image.open(path) as im:
            arr = np.array(im, dtype=np.uint8)
        if arr.shape != tuple(size):
            raise RuntimeError(f"{what} {root}: {path} is {arr.shape[0]} x {arr.shape[1]}, the network's labels are "
                               f"{size[0]} x {size[1]}")
        maps.append(arr)
    return torch.from_numpy(np.stack(maps))


class LabelTreeWriter:
    """The files of one run: the maps of ``--out`` (``write_maps``) and the label tree under ``root`` (``flag``:
    --out-root or --clean-root), per image a label file (``names[i]`` for the split's i-th) with 255 for the ignore
    class, and the procedural images beside their labels.  ``images``: how many the split has, where known."""

    def __init__(self, pool, args, flag, root, out, images=None):
        self.flag, self.root, self.seen = flag, root, 0
        labels_dir = self.names = self.images_dir = None
        if root:
            labels_dir, self.names, self.images_dir = rc.plan_label_tree(args, root)
            self._count(images)
        if out:
            os.makedirs(out, exist_ok=True)
        self.maps, self.tree, self.pics = (hc.PngWriter(pool, d) for d in (out, labels_dir, self.images_dir))

    def _count(self, images):
        if self.root and images is not None and len(self.names) != images:
            raise RuntimeError(f"{self.flag}: {len(self.names)} label names for {images} images")

    def wait(self):                                    # the batch before this one: bounds what is in flight
        for png in (self.maps, self.tree, self.pics):
            png.wait()

    def write_maps(self, stems, **maps):
        """``<stem>_<name>.png`` into ``--out`` for every u8 map [n, ...] on the device, name by name per stem."""
        host = {name: m.cpu().numpy() for name, m in maps.items()}
        for j, stem in enumerate(stems):
            for name, arr in host.items():
                self.maps.submit(arr[j], f"{stem}_{name}.png")

    def batch_names(self, rows):
        return [self.names[self.seen + j] for j in rows]

    def earlier_labels(self, args, rows, size, dev):
        """(``--previous-root``'s, ``--fill-root``'s) label maps of the batch's images ``rows``, each None without its flag."""
        return tuple(read_labels(root, args.layout, args.subset, self.batch_names(rows), size, flag).to(dev) if root else None
                     for flag, root in (("--previous-root", args.previous_root), ("--fill-root", args.fill_root)))

    def write_batch(self, stems, images, out, ignore, rows=None):
        """The tree's files of one batch.  ``out``: u8 label maps on the device, of every image of the batch or of
        ``rows`` (ascending places in it; None for no rows) alone: the others get an all-255 file, nothing selected."""
        n = len(stems)
        rows = list(range(n)) if rows is None else rows
        if self.root:
            if rows:
                host = torch.where(out == ignore, torch.full_like(out, 255), out).cpu().numpy()   # the files' own ignore value
                for k, name in enumerate(self.batch_names(rows)):
                    self.tree.submit(host[k], name)
            empty = np.full(tuple(images.shape[2:]), 255, dtype=np.uint8)
            for name in self.batch_names(j for j in range(n) if j not in rows):
                self.tree.submit(empty, name)
            if self.images_dir:
                pics = (images.permute(0, 2, 3, 1) * 255.0).round().clamp(0, 255).to(torch.uint8).cpu().numpy()
                for j, stem in enumerate(stems):
                    self.pics.submit(pics[j], f"{stem}.png")
        self.seen += n

    def close(self):
        """Waits for every file -> the paths written: maps, labels, images."""
        self._count(self.seen)
        self.wait()
        return self.maps.written + self.tree.written + self.pics.written


def given_counts(given, target, nc, ignore):
    """given[c] += the target's pixels of class c (not the ignore class); nothing without a target."""
    if target is not None:
        tl = target.reshape(-1).long()
        given += torch.bincount(tl[(tl < nc) & (tl != ignore)], minlength=nc)


def annotated_block(who, counters, given, nc):
    """The annotated fields of a labelled run's report; refuses targets outside [0, nc)."""
    if int(counters["bad_targets"]):
        raise RuntimeError(f"{who}: {int(counters['bad_targets'])} target pixels are outside [0, {nc})")
    ann, giv = counters["annotated"].tolist(), given.cpu().tolist()
    return dict(annotated=ann, annotated_pixels=sum(ann), given=giv,
                annotated_share_per_class=[a / g if g else 0.0 for a, g in zip(ann, giv)])


def finish(report, written, args, selection=None):
    """``selection.json`` into ``--out-root`` and ``--out``, the paths into the report, the report into ``--json``."""
    for folder in (args.out_root, args.out) if selection else ():
        if folder:
            written.append(os.path.join(folder, "selection.json"))
            hc.write_json(selection, written[-1])
    report["written"] = written
    if written:
        print(f"{len(written)} files written")
    if args.json:
        hc.write_json(report, args.json)
    return report
