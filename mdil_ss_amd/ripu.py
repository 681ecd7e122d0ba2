"""Ripu on MI355X: RIPU's acquisition as published (Xie et al., "Towards Fewer Annotations: Active Learning
via Region Impurity and Prediction Uncertainty", CVPR 2022).  ``mdil_ss_amd.acquire`` ranks the tiles of a
fixed grid; here every pixel is scored by the (2k+1)^2 window CENTRED on it (clipped at the border, nothing
padded) and the best centres are picked greedily, each taking its (2r+1)^2 region out of the pool: r = k is the
paper's region mode ("RA"), r = 0 its pixel mode ("PA").  Per batch, all on the device:

  ``acquire_head``  the network's label and ONE uncertainty per pixel (``--kind``) as a linear 16-bit q;
  ``ripu_score``    per pixel a 32-bit integer key from its window: ``uncertainty`` (sum q << 16) / cnt,
                    ``impurity`` (E << 16) / cnt, ``ripu`` (sum q * E) / cnt^2, ``oracle`` (needs labels)
                    (wrong << 32) / (cnt + 1), ``random`` a SplitMix64 hash; E = tlog[cnt] - sum_c tlog[h_c] with
                    tlog[h] = round(h ln h 2^14), so ripu's key is 65536 * 2^14 * U * I * ln nc in ``acquire``'s terms;
  ``ripu_select``   the greedy pick of every image: the largest key not yet taken (ties: the first in raster
                    order), until the next region would pass the image's budget, the best key is 0 or
                    ``--max-picks`` is reached.  Keys are not recomputed between picks (RIPU's rule);
  ``ripu_apply``    what an annotator of the picked regions hands back, on top of an earlier round's labels and
                    of fill labels, with the counters.

    python -m mdil_ss_amd.ripu --state CKPT --num-classes 20 20 --task 1 --dataset BDD --subset train \
        --budget 0.05 --radius 16 --kind entropy --by ripu --json FILE --out-root ROOT --layout BDD \
        [--select-radius R] [--previous SEL.json --previous-root ROOT0] [--fill-root PSEUDO_ROOT] [--max-picks P]
    python -m mdil_ss_amd.ripu --state CKPT ... --radius 1 --select-radius 0 --budget 0.0001 ...      (pixel mode)
    python -m mdil_ss_amd.ripu --state CKPT ... --images DIR --budget 0.05 --out DIR2 --json FILE

The budget is PER IMAGE (RIPU's protocol): each image may show ``--budget`` x its own pixels, unlike
``acquire``'s ranking over the whole split.  With labels the run simulates the annotator (``--out-root`` writes
a label tree the trainers open unchanged) and the report gives, for the chosen criterion and for each of the
others run through the same score and select, the pixels shown, the picks per image, how many images stopped
on the budget, on a zero key or on ``--max-picks``, and the error recall wrong_shown / wrong_all.  Without
labels ``--out`` writes ``<stem>_select.png`` and ``<stem>_score.png`` (key >> 24).  Both write
``selection.json`` with every pick as (y, x, key, fresh).

What is NOT measured.  The defaults (radius, kind, criterion, budget) are untuned.  Everything here was
measured on a randomly initialised network only: nothing says which criterion finds the errors of a trained
head on BDD or IDD.  No retraining on the selected labels is run."""
import json
import math
import os

import numpy as np
import torch

from . import _head_common as hc
from . import _report_common as rc
from . import _ripu_lib
from . import acquire as A

_PATH = "ripu"
KEY = torch.uint32
CRITERIA = ("uncertainty", "impurity", "ripu", "oracle", "random")      # the index is the library's `by`
STOPS = ("empty", "budget", "max_picks")                                # MDIL_RIPU_STOP_*
APPLY_COUNTERS = ("shown", "annotated", "kept", "filled", "bad_targets", "wrong_shown", "wrong_all")
MASK_SELECTED, MASK_KEPT, MASK_FILLED = 255, 128, 64
_M64 = (1 << 64) - 1
_tlog_cache = {}


def check_nc(fn, nc):
    return hc.check_nc(fn, _ripu_lib, nc)


def check_by(fn, by):
    if by not in CRITERIA:
        raise RuntimeError(f"mdil {fn}: criterion {by!r} (one of {list(CRITERIA)})")
    return CRITERIA.index(by)


def check_radius(fn, name, v, lo):
    try:
        ok = lo <= int(v) <= _ripu_lib.MAX_RADIUS and int(v) == v
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise RuntimeError(f"mdil {fn}: {name} {v!r} outside [{lo}, {_ripu_lib.MAX_RADIUS}]")
    return int(v)


def tlog_table(k):
    """What ``ripu_score`` reads the entropy from: int32 [(2k+1)^2 + 1] on the host, tlog[h] = round(h ln h 2^14)
    in fp64, tlog[0] = tlog[1] = 0."""
    k = check_radius("tlog_table", "k", k, _ripu_lib.MIN_RADIUS)
    h = torch.arange((2 * k + 1) ** 2 + 1, dtype=torch.float64)
    return torch.round(h * torch.log(h.clamp(min=1.0)) * float(1 << _ripu_lib.TLOG_SHIFT)).to(torch.int32)


def key_values(key):
    """A stored key map as int64 (uint32 tensors support few operations)."""
    return key.view(torch.int32).to(torch.int64) & 0xffffffff


def apply_counter_shapes(nc):
    return {"shown": (1,), "annotated": (nc,), "kept": (nc,), "filled": (nc,), "bad_targets": (1,), "wrong_shown": (1,),
            "wrong_all": (1,)}


def new_apply_counters(nc, dev, names=APPLY_COUNTERS):
    return hc.zero_counters(apply_counter_shapes(nc), dev, names)


def _maps(fn, first, name, dtype, others):
    """``first`` [N,Hl,Wl] of ``dtype`` on the device, and ``others`` ((tensor or None, name, dtype)) like it."""
    hc.chk(fn, _PATH, first, name, dtype)
    if first.dim() != 3 or first.numel() == 0:
        raise RuntimeError(f"mdil {fn}: {name} must be {str(dtype)[6:]} [N,Hl,Wl] (got {tuple(first.shape)})")
    N, Hl, Wl = first.shape
    if Hl * Wl > _ripu_lib.MAX_IMAGE_PIXELS:
        raise RuntimeError(f"mdil {fn}: maps of {Hl} x {Wl} (at most 2^24 pixels per image)")
    for t, other, dt in others:
        hc.check_tables(fn, _PATH, first.device, dt, ((t, other, (N, Hl, Wl)),))
    return N, Hl, Wl, first.device


# --------------------------------------------------------------------------------- entry points
def ripu_score(label, k, nc, by="ripu", qmap=None, target=None, ignore_index=-1, taken=None, tlog=None, seed=0,
               image0=0):
    """One 32-bit key per pixel from its clipped (2k+1)^2 window, on the current stream -> key uint32 [N,Hl,Wl].
    ``label``: u8 [N,Hl,Wl] on the device (``acquire_head``'s); ``qmap``: its u16 map, needed by "uncertainty" and
    "ripu"; ``target``: u8, needed by "oracle"; ``taken``: u8, non-zero pixels get key 0 (and still count in their
    neighbours' windows); ``tlog``: int32 [(2k+1)^2 + 1] on the device (default: ``tlog_table(k)``); ``seed`` and
    ``image0`` (the first image's place in the split) feed "random"."""
    fn = "ripu_score"
    lib = _ripu_lib.load()
    nc = check_nc(fn, nc)
    k = check_radius(fn, "k", k, _ripu_lib.MIN_RADIUS)
    b = check_by(fn, by)
    hc.check_ignore_index(fn, ignore_index)
    N, Hl, Wl, dev = _maps(fn, label, "label", torch.uint8, ((qmap, "qmap", torch.uint16), (target, "target", torch.uint8),
                                                            (taken, "taken", torch.uint8)))
    if qmap is None and by in ("uncertainty", "ripu"):
        raise RuntimeError(f"mdil {fn}: the criterion {by} needs a qmap (uint16 [N,Hl,Wl]) on the device")
    if target is None and by == "oracle":
        raise RuntimeError(f"mdil {fn}: the criterion oracle needs a target (uint8 [N,Hl,Wl]) on the device")
    if int(image0) < 0:
        raise RuntimeError(f"mdil {fn}: image0 {image0} is negative")
    if by in ("impurity", "ripu"):
        if tlog is None:
            if (k, dev) not in _tlog_cache:
                _tlog_cache[(k, dev)] = tlog_table(k).to(dev)
            tlog = _tlog_cache[(k, dev)]
        hc.check_tables(fn, _PATH, dev, torch.int32, ((tlog, "tlog", ((2 * k + 1) ** 2 + 1,)),))
    else:
        tlog = None
    seed = int(seed) & _M64
    with torch.no_grad(), torch.cuda.device(dev):
        key = torch.empty(N, Hl, Wl, dtype=KEY, device=dev)
        _ripu_lib.check(
            lib.mdil_ripu_score(label.data_ptr(), hc.ptr(qmap), hc.ptr(target), int(ignore_index), hc.ptr(taken), hc.ptr(tlog),
                                N, Hl, Wl, nc, k, b, seed - (1 << 64) if seed >> 63 else seed, int(image0), key.data_ptr(),
                                torch.cuda.current_stream(dev).cuda_stream),
            "mdil_ripu_score")
    return key


def ripu_select(key, taken, r, budget_pixels, max_picks, picks=None):
    """The greedy pick of every image, on the current stream.  ``key``: uint32 [N,Hl,Wl]; ``taken``: u8 [N,Hl,Wl],
    read AND written (the picked regions get 255; other non-zero marks stay); ``r``: 0 (pixels) to 32;
    ``budget_pixels``: what one image may show; ``picks``: int64 [N,max_picks,4] to write (y, x, key, fresh) into
    (default: a zeroed one; rows past the count are not touched).
    -> {"picks", "count" int64 [N], "shown" int64 [N], "stop" int64 [N] (index into ``STOPS``)}"""
    fn = "ripu_select"
    lib = _ripu_lib.load()
    r = check_radius(fn, "r", r, 0)
    N, Hl, Wl, dev = _maps(fn, key, "key", KEY, ((taken, "taken", torch.uint8),))
    if taken is None:
        raise RuntimeError(f"mdil {fn}: taken must be a uint8 [N,Hl,Wl] device tensor; it is written")
    if not 1 <= int(max_picks) <= _ripu_lib.MAX_PICKS:
        raise RuntimeError(f"mdil {fn}: max_picks {max_picks} outside [1, {_ripu_lib.MAX_PICKS}]")
    if int(budget_pixels) < 0:
        raise RuntimeError(f"mdil {fn}: budget_pixels {budget_pixels} is negative")
    P = int(max_picks)
    hc.check_tables(fn, _PATH, dev, torch.int64, ((picks, "picks", (N, P, 4)),))
    with torch.no_grad(), torch.cuda.device(dev):
        if picks is None:
            picks = torch.zeros(N, P, 4, dtype=torch.int64, device=dev)
        out = {"picks": picks}
        for name in ("count", "shown", "stop"):
            out[name] = torch.empty(N, dtype=torch.int64, device=dev)
        _ripu_lib.check(
            lib.mdil_ripu_select(key.data_ptr(), taken.data_ptr(), N, Hl, Wl, r, int(budget_pixels), P, picks.data_ptr(),
                                 out["count"].data_ptr(), out["shown"].data_ptr(), out["stop"].data_ptr(),
                                 torch.cuda.current_stream(dev).cuda_stream),
            "mdil_ripu_select")
    return out


def ripu_apply(selected, nc, target=None, previous=None, fill=None, label=None, ignore_index=-1, drop_id=255,
               counters=None, want_out=True, want_mask=False):
    """What an annotator of the picked regions hands back, on the current stream.  ``selected``: u8 [N,Hl,Wl] on
    the device, CHOSEN where it is 255 (``ripu_select``'s ``taken``); ``target``, ``previous``, ``fill``,
    ``label``: u8 [N,Hl,Wl] or None.  A chosen pixel is the target (``drop_id`` without one); elsewhere
    ``previous`` where that is not ``drop_id``, else ``fill`` where that is not ``drop_id``, else ``drop_id``.
    -> (out u8 or None, mask u8 or None: 255 newly selected, 128 kept, 64 filled, 0 none).  ``counters``: any of
    ``APPLY_COUNTERS`` as int64 device tensors (``apply_counter_shapes``), accumulated into; "annotated" and
    "bad_targets" need a target, "wrong_shown" and "wrong_all" a target and a label map."""
    fn = "ripu_apply"
    lib = _ripu_lib.load()
    nc = check_nc(fn, nc)
    hc.check_ignore_index(fn, ignore_index)
    drop_id = hc.check_id(fn, "drop_id", drop_id)
    N, Hl, Wl, dev = _maps(fn, selected, "selected", torch.uint8,
                           tuple((t, name, torch.uint8) for t, name in ((target, "target"), (previous, "previous"),
                                                                        (fill, "fill"), (label, "label"))))
    c = rc.check_counters(fn, counters, APPLY_COUNTERS)
    shapes = apply_counter_shapes(nc)
    hc.check_tables(fn, _PATH, dev, torch.int64, tuple((c[k], k, shapes[k]) for k in APPLY_COUNTERS))
    if target is None and (c["annotated"] is not None or c["bad_targets"] is not None):
        raise RuntimeError(f"mdil {fn}: the counters annotated and bad_targets need a target")
    if (target is None or label is None) and (c["wrong_shown"] is not None or c["wrong_all"] is not None):
        raise RuntimeError(f"mdil {fn}: the counters wrong_shown and wrong_all need a target and a label map")
    if not want_out and not want_mask and all(v is None for v in c.values()):
        raise RuntimeError(f"mdil {fn}: nothing to do (no out map, no mask, no counters)")
    with torch.no_grad(), torch.cuda.device(dev):
        out = torch.empty(N, Hl, Wl, dtype=torch.uint8, device=dev) if want_out else None
        mask = torch.empty(N, Hl, Wl, dtype=torch.uint8, device=dev) if want_mask else None
        _ripu_lib.check(
            lib.mdil_ripu_apply(selected.data_ptr(), hc.ptr(target), hc.ptr(previous), hc.ptr(fill), hc.ptr(label), N, Hl, Wl,
                                nc, int(ignore_index), drop_id, hc.ptr(out), hc.ptr(mask),
                                *(hc.ptr(c[k]) for k in APPLY_COUNTERS), torch.cuda.current_stream(dev).cuda_stream),
            "mdil_ripu_apply")
    return out, mask


# ------------------------------------------------------------------------------------------ CLI
def read_selection(path, size):
    """A ``selection.json`` of an earlier round -> ({stem: [(y, x), ...]}, its select radius)."""
    with open(path) as f:
        saved = json.load(f)
    if "picks" not in saved or "select_radius" not in saved:
        raise RuntimeError(f"--previous {path}: not a selection.json written by this command")
    if tuple(saved.get("size", size)) != tuple(size):
        raise RuntimeError(f"--previous {path}: selected on maps of {saved.get('size')}, this run has {list(size)}")
    return {stem: [(int(p[0]), int(p[1])) for p in picks] for stem, picks in saved["picks"].items()}, \
        int(saved["select_radius"])


def earlier_marks(stems, before, radius, size):
    """The regions an earlier round picked as a u8 map [n,Hl,Wl] of 128s (host): not chosen again, not shown."""
    marks = np.zeros((len(stems),) + tuple(size), dtype=np.uint8)
    for i, stem in enumerate(stems):
        for y, x in before.get(stem, ()):
            marks[i, max(0, y - radius):y + radius + 1, max(0, x - radius):x + radius + 1] = MASK_KEPT
    return torch.from_numpy(marks)


def main(args):
    _refusals(args)
    rc.refuse_task(args.task, args.num_classes)
    if args.previous and not os.path.isfile(args.previous):
        raise RuntimeError(f"--previous {args.previous}: no such file")
    for flag, path in (("--previous-root", args.previous_root), ("--fill-root", args.fill_root)):
        if path and not os.path.isdir(path):
            raise RuntimeError(f"{flag} {path}: no such folder")
    dev, nc, model = hc.load_model(args.state, args.num_classes, args.task)
    ignore = nc - 1                                    # the trainers' relabelled ignore class
    size = (args.height, args.width)
    labelled = not args.images
    k = args.radius
    r = k if args.select_radius is None else args.select_radius
    budget_pixels = int(math.floor(args.budget * size[0] * size[1]))
    w, b = (t.detach() for t in model.head_params(args.task))
    before, before_radius = read_selection(args.previous, size) if args.previous else ({}, 0)
    others = [by for by in CRITERIA if by != args.by] if labelled else []
    nonfinite = torch.zeros(1, dtype=torch.int64, device=dev)
    counters = new_apply_counters(nc, dev, APPLY_COUNTERS if labelled else ("shown", "kept", "filled"))
    side = {by: new_apply_counters(nc, dev, ("shown", "wrong_shown", "wrong_all")) for by in others}
    tallies = {by: {"picks": 0, "picks_max": 0, "stops": dict.fromkeys(STOPS, 0)} for by in [args.by] + others}
    given = torch.zeros(nc, dtype=torch.int64, device=dev)

    def tally(by, got):
        t = tallies[by]
        count, stop = got["count"].cpu(), got["stop"].cpu()
        t["picks"] += int(count.sum())
        t["picks_max"] = max(t["picks_max"], int(count.max()))
        for s in stop.tolist():
            t["stops"][STOPS[s]] += 1

    labels_dir = names = images_dir = None
    if args.out_root:
        labels_dir, names, images_dir = A.plan_label_tree(args)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    per_stem, written, stems_all, i0 = {}, [], [], 0
    with hc.png_pool() as pool:
        map_png, tree_png, image_png = hc.PngWriter(pool, args.out), hc.PngWriter(pool, labels_dir), \
            hc.PngWriter(pool, images_dir)
        for stems, images, target in rc.image_or_dataset_batches(args, nc, pool, dev, unique_stems=True):
            if tuple(images.shape[2:]) != size:
                raise RuntimeError(f"images of {tuple(images.shape[2:])}, expected {size}")
            n = len(stems)
            with torch.no_grad():
                feat = model.features(images, args.task).contiguous()
            label, qmap = A.acquire_head(feat, w, b, (2, 2), args.kind, counters={"nonfinite": nonfinite}, want_label=True,
                                         want_qmap=True)
            marks = earlier_marks(stems, before, before_radius, size).to(dev)
            ign = ignore if labelled else -1

            def run(by, taken):
                key = ripu_score(label, k, nc, by, qmap, target, ign, taken, seed=args.seed, image0=i0)
                return key, ripu_select(key, taken, r, budget_pixels, args.max_picks)

            for by in others:                              # the same score and select, counted and thrown away
                taken = marks.clone()
                tally(by, run(by, taken)[1])
                ripu_apply(taken, nc, target, label=label, ignore_index=ign, counters=side[by], want_out=False)
            taken = marks.clone()
            key, got = run(args.by, taken)
            tally(args.by, got)
            prev = fill = None
            if args.previous_root:
                prev = A._read_labels(args.previous_root, args.layout, args.subset, names[i0:i0 + n], size,
                                      "--previous-root").to(dev)
            if args.fill_root:
                fill = A._read_labels(args.fill_root, args.layout, args.subset, names[i0:i0 + n], size, "--fill-root").to(dev)
            out, mask = ripu_apply(taken, nc, target, prev, fill, label if labelled else None, ign, 255, counters,
                                   want_out=bool(args.out_root), want_mask=bool(args.out))
            count, picks = got["count"].cpu().tolist(), got["picks"].cpu()
            for j, stem in enumerate(stems):
                per_stem[stem] = picks[j, :count[j]].tolist()
            if target is not None:
                tl = target.reshape(-1).long()
                given += torch.bincount(tl[(tl < nc) & (tl != ignore)], minlength=nc)
            for png in (map_png, tree_png, image_png):
                png.wait()                                 # the batch before this one: bounds what is in flight
            if args.out:
                score = (key_values(key) >> 24).to(torch.uint8).cpu().numpy()
                host = mask.cpu().numpy()
                for j, stem in enumerate(stems):
                    map_png.submit(host[j], f"{stem}_select.png")
                    map_png.submit(score[j], f"{stem}_score.png")
            if args.out_root:
                out = torch.where(out == ignore, torch.full_like(out, 255), out)   # the label files' own ignore value
                host = out.cpu().numpy()
                for j in range(n):
                    tree_png.submit(host[j], names[i0 + j])
                if images_dir:
                    pics = (images.permute(0, 2, 3, 1) * 255.0).round().clamp(0, 255).to(torch.uint8).cpu().numpy()
                    for j, stem in enumerate(stems):
                        image_png.submit(pics[j], f"{stem}.png")
            stems_all.extend(stems)
            i0 += n
        for png in (map_png, tree_png, image_png):
            png.wait()
            written.extend(png.written)
    if args.out_root and len(names) != len(stems_all):
        raise RuntimeError(f"--out-root: {len(names)} label names for {len(stems_all)} images")

    M = len(stems_all)
    total = M * size[0] * size[1]
    c = {name: v.cpu() for name, v in counters.items()}
    selection = {"radius": k, "select_radius": r, "size": list(size), "kind": args.kind, "by": args.by,
                 "budget": args.budget, "budget_pixels_per_image": budget_pixels, "seed": args.seed, "picks": per_stem}

    def summary(by, shown):
        t = tallies[by]
        return {"shown": shown, "shown_share": shown / total if total else 0.0, "picks": t["picks"],
                "picks_per_image_mean": t["picks"] / max(1, M), "picks_per_image_max": t["picks_max"], "stops": t["stops"]}

    report = {"dataset": rc.source_name(args), "subset": args.subset, "task": args.task, "num_classes": nc,
              "kind": args.kind, "by": args.by, "radius": k, "select_radius": r, "size": list(size), "budget": args.budget,
              "budget_is": "per image: every image may show --budget x its own pixels (RIPU's protocol), unlike "
                           "acquire's ranking over the whole split",
              "budget_pixels_per_image": budget_pixels, "max_picks": args.max_picks, "seed": args.seed, "images": M,
              "total_pixels": total, "nonfinite": int(nonfinite.item()), "previous": args.previous,
              "kept": c["kept"].tolist(), "filled": c["filled"].tolist()}
    report.update(summary(args.by, int(c["shown"])))
    if labelled:
        if int(c["bad_targets"]):
            raise RuntimeError(f"ripu: {int(c['bad_targets'])} target pixels are outside [0, {nc})")
        wrong_all = int(c["wrong_all"])
        per = {args.by: dict(summary(args.by, int(c["shown"])), wrong_shown=int(c["wrong_shown"]))}
        for by in others:
            s = {name: int(v.item()) for name, v in side[by].items()}
            per[by] = dict(summary(by, s["shown"]), wrong_shown=s["wrong_shown"])
        for v in per.values():
            v["error_recall"] = v["wrong_shown"] / wrong_all if wrong_all else 0.0
        ann, giv = c["annotated"].tolist(), given.cpu().tolist()
        report.update(criteria=per, error_recall={by: v["error_recall"] for by, v in per.items()},
                      error_recall_chosen=per[args.by]["error_recall"], wrong_pixels=wrong_all, annotated=ann,
                      annotated_pixels=sum(ann), given=giv,
                      annotated_share_per_class=[a / g if g else 0.0 for a, g in zip(ann, giv)])
    for folder in (args.out_root, args.out):
        if folder:
            path = os.path.join(folder, "selection.json")
            hc.write_json(selection, path)
            written.append(path)
    report["written"] = written
    print(f"{report['dataset']} (task {args.task}): {M} images, {report['picks']} regions of radius {r} scored over radius {k} "
          f"by {args.by} ({args.kind}): {report['shown']} pixels shown ({report['shown_share'] * 100:.2f} % of the split; the "
          f"budget is {budget_pixels} pixels PER IMAGE); {report['nonfinite']} non-finite pixels")
    print("  images stopped: " + "  ".join(f"{name} {v}" for name, v in report["stops"].items()))
    if labelled:
        print("  error recall at the budget: " + "  ".join(f"{by} {v * 100:.2f} %" for by, v in report["error_recall"].items()))
    if written:
        print(f"{len(written)} files written")
    if args.json:
        hc.write_json(report, args.json)
    return report


def _refusals(args):
    """Raise a RuntimeError that names why this combination of flags is refused."""
    if sum(bool(v) for v in (args.images, args.dataset, args.synthetic)) != 1:
        raise RuntimeError("give one source of images: --images DIR, --dataset cityscapes|BDD|IDD or --synthetic N")
    if min(args.height, args.width, args.batch_size) < 1 or args.synthetic < 0:
        raise RuntimeError("sizes and --batch-size must be positive")
    if args.height % 2 or args.width % 2:
        raise RuntimeError("--height and --width must be even")
    if args.height * args.width > _ripu_lib.MAX_IMAGE_PIXELS:
        raise RuntimeError(f"--height {args.height} x --width {args.width}: at most 2^24 pixels per image")
    if not (args.json or args.out or args.out_root):
        raise RuntimeError("nothing to do: give --json FILE, --out DIR or --out-root ROOT")
    if not 0.0 < args.budget <= 1.0:
        raise RuntimeError(f"--budget {args.budget} outside (0, 1]: a share of every image's pixels")
    check_radius("--radius", "radius", args.radius, _ripu_lib.MIN_RADIUS)
    if args.select_radius is not None:
        check_radius("--select-radius", "radius", args.select_radius, 0)
    if not 1 <= args.max_picks <= _ripu_lib.MAX_PICKS:
        raise RuntimeError(f"--max-picks {args.max_picks} outside [1, {_ripu_lib.MAX_PICKS}]")
    if args.images and args.by == "oracle":
        raise RuntimeError("--by oracle needs labels: give --dataset or --synthetic")
    if args.out_root and args.images:
        raise RuntimeError("--out-root writes what an annotator would answer: it needs labels (--dataset or --synthetic); "
                           "with --images give --out DIR")
    if bool(args.out_root) != bool(args.layout):
        raise RuntimeError("--out-root and --layout cityscapes|BDD go together")
    if args.out_root and args.dataset == "IDD":
        raise RuntimeError("--out-root does not take --dataset IDD: its loaders remap level-3 ids, so the label "
                           "files would need the inverse map")
    if (args.previous_root or args.fill_root) and not args.out_root:
        raise RuntimeError("--previous-root and --fill-root are label trees laid out as --out-root lays its own: they need "
                           "--out-root and --layout")
    if args.previous_root and not args.previous:
        raise RuntimeError("--previous-root goes with --previous SEL.json, the selection that tree was written for")


def build_parser():
    p = hc.RefusingParser(_refusals, description="which regions of every image to label first, as RIPU does it: a key "
                                                 "per pixel from the (2k+1)^2 window centred on it, a greedy pick under "
                                                 "a per-image pixel budget, and the label tree an annotator of those "
                                                 "regions would hand back")
    p.add_argument("--state", required=True, help="checkpoint written by the trainers (or by the reference)")
    p.add_argument("--num-classes", type=int, nargs="+", required=True)
    p.add_argument("--task", type=int, required=True, help="which task's decoder predicts")
    p.add_argument("--images", help="folder of unlabelled .jpg / .png images (searched recursively)")
    rc.add_data_flags(p, dataset_help="a labelled dataset instead: the run simulates the annotator",
                      synthetic_help="N procedural images instead (labelled)")
    p.set_defaults(subset="train")
    p.add_argument("--budget", type=float, required=True, help="share of EVERY IMAGE's pixels that may be shown")
    p.add_argument("--radius", type=int, default=16, help="k of the (2k+1)^2 score window, 1 to 32 (default %(default)s)")
    p.add_argument("--select-radius", type=int, help="r of the (2r+1)^2 region a pick takes, 0 (pixel mode) to 32 "
                                                     "(default: --radius, region mode)")
    p.add_argument("--kind", choices=A.KINDS, default="entropy", help="the per-pixel uncertainty (default %(default)s)")
    p.add_argument("--by", choices=CRITERIA, default="ripu", help="the criterion (default %(default)s)")
    p.add_argument("--seed", type=int, default=0, help="of --by random (default %(default)s)")
    p.add_argument("--max-picks", type=int, default=4096, help="picks per image at most, 1 to 65536 (default %(default)s)")
    p.add_argument("--previous", help="an earlier round's selection.json: its regions are not picked or shown again")
    p.add_argument("--previous-root", help="the label tree of that round: its labelled pixels are kept")
    p.add_argument("--fill-root", help="a label tree (pseudo --out-root, say) for the pixels still empty")
    p.add_argument("--json", help="write the report here")
    p.add_argument("--out", help="write <stem>_select.png (255 selected, 128 kept, 64 filled) and <stem>_score.png "
                                 "(key >> 24) here")
    p.add_argument("--out-root", help="with labels: write a dataset tree the trainers open as --cs-datadir / --bdd-datadir")
    p.add_argument("--layout", choices=("cityscapes", "BDD"), help="the tree --out-root writes")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
