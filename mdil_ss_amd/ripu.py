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
from types import SimpleNamespace

import numpy as np
import torch

from . import _annotate_common as ac
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
    return dict(A.apply_counter_shapes(nc), wrong_shown=(1,), wrong_all=(1,))


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


def _batch(args, head, run, writer, stems, images, target):
    """One batch: ``acquire_head``'s maps, score and select by every criterion (the others counted and thrown
    away), ``ripu_apply`` for the chosen one, the maps of ``--out`` and the tree of ``--out-root``."""
    nc, size, dev, k, r = head.nc, head.size, head.dev, run.k, run.r
    label, qmap = A.acquire_head(ac.features(head, images), head.w, head.b, (2, 2), args.kind,
                                 counters={"nonfinite": run.nonfinite}, want_label=True, want_qmap=True)
    marks = earlier_marks(stems, run.before, run.before_radius, size).to(dev)

    def pick(by):
        taken = marks.clone()
        key = ripu_score(label, k, nc, by, qmap, target, head.ign, taken, seed=args.seed, image0=writer.seen)
        got = ripu_select(key, taken, r, run.budget_pixels, args.max_picks)
        t = run.tallies[by]
        count = got["count"].cpu()
        t["picks"] += int(count.sum())
        t["picks_max"] = max(t["picks_max"], int(count.max()))
        for s in got["stop"].cpu().tolist():
            t["stops"][STOPS[s]] += 1
        return key, taken, got

    for by in run.others:                              # the same score and select, counted and thrown away
        ripu_apply(pick(by)[1], nc, target, label=label, ignore_index=head.ign, counters=run.side[by], want_out=False)
    key, taken, got = pick(args.by)
    prev, fill = writer.earlier_labels(args, range(len(stems)), size, dev)
    out, mask = ripu_apply(taken, nc, target, prev, fill, label if head.labelled else None, head.ign, 255, run.counters,
                           want_out=bool(args.out_root), want_mask=bool(args.out))
    count, picks = got["count"].cpu().tolist(), got["picks"].cpu()
    for j, stem in enumerate(stems):
        run.per_stem[stem] = picks[j, :count[j]].tolist()
    ac.given_counts(run.given, target, nc, head.ignore)
    writer.wait()
    if args.out:
        writer.write_maps(stems, select=mask, score=(key_values(key) >> 24).to(torch.uint8))
    writer.write_batch(stems, images, out, head.ignore)


def _report(args, head, run, M):
    """The tallies and counters of the whole split -> (report, selection.json)"""
    nc, size, k, r = head.nc, head.size, run.k, run.r
    total = M * size[0] * size[1]
    c = {name: v.cpu() for name, v in run.counters.items()}
    selection = {"radius": k, "select_radius": r, "size": list(size), "kind": args.kind, "by": args.by,
                 "budget": args.budget, "budget_pixels_per_image": run.budget_pixels, "seed": args.seed, "picks": run.per_stem}

    def summary(by, shown):
        t = run.tallies[by]
        return {"shown": shown, "shown_share": shown / total if total else 0.0, "picks": t["picks"],
                "picks_per_image_mean": t["picks"] / max(1, M), "picks_per_image_max": t["picks_max"], "stops": t["stops"]}

    report = {"dataset": rc.source_name(args), "subset": args.subset, "task": args.task, "num_classes": nc,
              "kind": args.kind, "by": args.by, "radius": k, "select_radius": r, "size": list(size), "budget": args.budget,
              "budget_is": "per image: every image may show --budget x its own pixels (RIPU's protocol), unlike "
                           "acquire's ranking over the whole split",
              "budget_pixels_per_image": run.budget_pixels, "max_picks": args.max_picks, "seed": args.seed, "images": M,
              "total_pixels": total, "nonfinite": int(run.nonfinite.item()), "previous": args.previous,
              "kept": c["kept"].tolist(), "filled": c["filled"].tolist()}
    report.update(summary(args.by, int(c["shown"])))
    if head.labelled:
        annotated = ac.annotated_block("ripu", c, run.given, nc)
        wrong_all = int(c["wrong_all"])
        per = {args.by: dict(summary(args.by, int(c["shown"])), wrong_shown=int(c["wrong_shown"]))}
        for by in run.others:
            s = {name: int(v.item()) for name, v in run.side[by].items()}
            per[by] = dict(summary(by, s["shown"]), wrong_shown=s["wrong_shown"])
        for v in per.values():
            v["error_recall"] = v["wrong_shown"] / wrong_all if wrong_all else 0.0
        report.update(criteria=per, error_recall={by: v["error_recall"] for by, v in per.items()},
                      error_recall_chosen=per[args.by]["error_recall"], wrong_pixels=wrong_all, **annotated)
    return report, selection


def main(args):
    _refusals(args)
    head = ac.open_head(args)
    nc, size, dev, k = head.nc, head.size, head.dev, args.radius
    before, before_radius = read_selection(args.previous, size) if args.previous else ({}, 0)
    others = [by for by in CRITERIA if by != args.by] if head.labelled else []
    run = SimpleNamespace(
        k=k, r=k if args.select_radius is None else args.select_radius, before=before, before_radius=before_radius,
        budget_pixels=int(math.floor(args.budget * size[0] * size[1])), others=others,
        nonfinite=torch.zeros(1, dtype=torch.int64, device=dev), given=torch.zeros(nc, dtype=torch.int64, device=dev),
        counters=new_apply_counters(nc, dev, APPLY_COUNTERS if head.labelled else ("shown", "kept", "filled")),
        side={by: new_apply_counters(nc, dev, ("shown", "wrong_shown", "wrong_all")) for by in others},
        tallies={by: {"picks": 0, "picks_max": 0, "stops": dict.fromkeys(STOPS, 0)} for by in [args.by] + others},
        per_stem={})
    with hc.png_pool() as pool:
        writer = ac.LabelTreeWriter(pool, args, "--out-root", args.out_root, args.out)
        for stems, images, target in ac.batches(args, head, pool):
            _batch(args, head, run, writer, stems, images, target)
        written = writer.close()
    M, r = writer.seen, run.r
    report, selection = _report(args, head, run, M)
    print(f"{report['dataset']} (task {args.task}): {M} images, {report['picks']} regions of radius {r} scored over radius {k} "
          f"by {args.by} ({args.kind}): {report['shown']} pixels shown ({report['shown_share'] * 100:.2f} % of the split; the "
          f"budget is {run.budget_pixels} pixels PER IMAGE); {report['nonfinite']} non-finite pixels")
    print("  images stopped: " + "  ".join(f"{name} {v}" for name, v in report["stops"].items()))
    if head.labelled:
        print("  error recall at the budget: " + "  ".join(f"{by} {v * 100:.2f} %" for by, v in report["error_recall"].items()))
    return ac.finish(report, written, args, selection)


def _refusals(args):
    """Raise a RuntimeError that names why this combination of flags is refused."""
    ac.refuse_head(args, "every image's", _ripu_lib.MAX_IMAGE_PIXELS)
    check_radius("--radius", "radius", args.radius, _ripu_lib.MIN_RADIUS)
    if args.select_radius is not None:
        check_radius("--select-radius", "radius", args.select_radius, 0)
    if not 1 <= args.max_picks <= _ripu_lib.MAX_PICKS:
        raise RuntimeError(f"--max-picks {args.max_picks} outside [1, {_ripu_lib.MAX_PICKS}]")
    ac.refuse_rounds(args)


def build_parser():
    p = hc.RefusingParser(_refusals, description="which regions of every image to label first, as RIPU does it: a key "
                                                 "per pixel from the (2k+1)^2 window centred on it, a greedy pick under "
                                                 "a per-image pixel budget, and the label tree an annotator of those "
                                                 "regions would hand back")
    ac.add_source_flags(p, "share of EVERY IMAGE's pixels that may be shown")
    p.add_argument("--radius", type=int, default=16, help="k of the (2k+1)^2 score window, 1 to 32 (default %(default)s)")
    p.add_argument("--select-radius", type=int, help="r of the (2r+1)^2 region a pick takes, 0 (pixel mode) to 32 "
                                                     "(default: --radius, region mode)")
    ac.add_criterion_flags(p, A.KINDS, CRITERIA, "the criterion")
    p.add_argument("--max-picks", type=int, default=4096, help="picks per image at most, 1 to 65536 (default %(default)s)")
    ac.add_round_flags(p, "its regions are not picked or shown again", "<stem>_score.png (key >> 24)")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
