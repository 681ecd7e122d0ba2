"""Superpixel acquire on MI355X: regions that follow the image, answered with one click (Cai et al., "Revisiting
Superpixels for Active Learning in Semantic Segmentation with Realistic Annotation Costs", CVPR 2021; ViewAL).
``mdil_ss_amd.acquire`` ranks the tiles of a fixed grid and ``mdil_ss_amd.ripu`` sliding square windows; both
draw regions that ignore the image.  Here every image is over-segmented on the device by an integer SLIC
(include/mdil_spx.h spells the rule out), every superpixel gets ``acquire``'s table [pixels, sum q, wrong, valid,
label counts], the superpixels of the split are ranked by ``acquire``'s own criteria under a pixel budget, and the
annotator gives each chosen superpixel ONE label, its dominant one (``--answer dominant``; ``exact`` hands back
the target pixel by pixel).  The cost is counted in clicks, the price is label noise, and both are reported.

  ``acquire_head``  the network's label and ONE uncertainty per pixel (``--kind``) as a linear 16-bit q;
  ``spx_slic``      image -> id map, centres, sums: ``--step`` S, ``--compactness`` m, ``--iterations`` T;
  ``spx_table``     stored maps + id map -> the table and the valid-target counts per class;
  ``spx_apply``     what an annotator of the chosen superpixels hands back, with the counters.

    python -m mdil_ss_amd.superpixel --state CKPT --num-classes 20 20 --task 1 --dataset BDD --subset train \
        --budget 0.05 --step 16 --kind entropy --by ripu --json FILE --out-root ROOT --layout BDD \
        [--answer exact] [--max-per-image 0.5] [--previous SEL.json --previous-root ROOT0] [--fill-root PSEUDO_ROOT]
    python -m mdil_ss_amd.superpixel --state CKPT ... --images DIR --budget 0.05 --out DIR2 --json FILE
    python -m mdil_ss_amd.superpixel --state CKPT ... --dataset BDD --budget 1 --vote --out DIR --json FILE

The budget is a share of the SPLIT's pixels, as in ``acquire`` (``ripu``'s is per image); a superpixel's own pixel
count is its size, so the three acquisition commands stay comparable.  Two passes, as in ``acquire``: the table
of every image, then the ids again (they are deterministic, nothing is stored between the passes) and the apply.
``--vote`` writes ``<stem>_label.png`` with every superpixel's majority predicted label, a cheap regulariser of
pseudo-labels, and with labels the mIoU of the plain and of the voted maps; it uses no budget.

What is simplified and what is NOT measured.  The colour space is the RGB codes of the header, not CIELAB.
There is no connectivity enforcement, so a superpixel may be disconnected.  The defaults (step, compactness,
iterations, kind, criterion, budget) are untuned; ``achievable_accuracy`` is what ``--step`` should be tuned on.
Everything here was measured on a randomly initialised network only: nothing says which criterion finds the
errors of a trained head on BDD or IDD.  No retraining on the selected labels is run."""
import json
from types import SimpleNamespace

import numpy as np
import torch

from . import _annotate_common as ac
from . import _head_common as hc
from . import _report_common as rc
from . import _spx_lib
from . import acquire as A

_PATH = "superpixel"
FIELDS = _spx_lib.FIELDS
TABLE_COUNTERS = ("bad_targets", "bad_ids")
APPLY_COUNTERS = ("shown", "annotated", "kept", "filled", "bad_targets", "wrong_shown", "wrong_all", "noisy", "bad_ids")
ANSWERS = ("exact", "dominant")
MASK_SELECTED, MASK_KEPT, MASK_FILLED = 255, 128, 64


def check_nc(fn, nc):
    return hc.check_nc(fn, _spx_lib, nc)


def check_param(fn, name, v, lo, hi):
    try:
        ok = lo <= int(v) <= hi and int(v) == v
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise RuntimeError(f"mdil {fn}: {name} {v!r} outside [{lo}, {hi}]")
    return int(v)


def check_slic(fn, step, compactness, iterations):
    return (check_param(fn, "step", step, _spx_lib.MIN_STEP, _spx_lib.MAX_STEP),
            check_param(fn, "compactness", compactness, _spx_lib.MIN_COMPACTNESS, _spx_lib.MAX_COMPACTNESS),
            check_param(fn, "iterations", iterations, 0, _spx_lib.MAX_ITERATIONS))


def grid(size, step):
    """Cells of ``step`` over maps of ``size`` = (H, W) -> (Gy, Gx); K = Gy * Gx superpixels per image."""
    return -(-int(size[0]) // step), -(-int(size[1]) // step)


def apply_counter_shapes(nc):
    return {"shown": (1,), "annotated": (nc,), "kept": (nc,), "filled": (nc,), "bad_targets": (1,), "wrong_shown": (1,),
            "wrong_all": (1,), "noisy": (1,), "bad_ids": (1,)}


def new_apply_counters(nc, dev, names=APPLY_COUNTERS):
    return hc.zero_counters(apply_counter_shapes(nc), dev, names)


def _id_maps(fn, ids, others):
    """``ids`` int32 [N,H,W] on the device, and ``others`` ((tensor or None, name, dtype)) like it."""
    hc.chk(fn, _PATH, ids, "id", torch.int32)
    if ids.dim() != 3 or ids.numel() == 0:
        raise RuntimeError(f"mdil {fn}: id must be int32 [N,H,W] (got {tuple(ids.shape)})")
    N, H, W = ids.shape
    if max(H, W) > _spx_lib.MAX_SIDE:
        raise RuntimeError(f"mdil {fn}: maps of {H} x {W} (sides of at most {_spx_lib.MAX_SIDE})")
    for t, other, dt in others:
        hc.check_tables(fn, _PATH, ids.device, dt, ((t, other, (N, H, W)),))
    return N, H, W, ids.device


def _check_K(fn, K):
    if int(K) < 1:
        raise RuntimeError(f"mdil {fn}: K {K} (at least one superpixel per image)")
    return int(K)


# --------------------------------------------------------------------------------- entry points
def spx_slic(images, step=16, compactness=10, iterations=10):
    """The integer SLIC of include/mdil_spx.h on the current stream.  ``images``: f32 [N,3,H,W] on the device, the
    network's input in [0, 1].  -> (id int32 [N,H,W], centres int32 [N,K,5]: the state (Y, X, R, G, B) in 1/16 that
    the final assign read, sums int64 [N,K,6]: (n, sum y, sum x, sum r, sum g, sum b) of the final assignment)."""
    fn = "spx_slic"
    lib = _spx_lib.load()
    S, m, T = check_slic(fn, step, compactness, iterations)
    hc.chk(fn, _PATH, images, "image")
    if images.dim() != 4 or images.shape[1] != 3 or images.numel() == 0:
        raise RuntimeError(f"mdil {fn}: image must be float32 [N,3,H,W] (got {tuple(images.shape)})")
    N, _, H, W = images.shape
    if max(H, W) > _spx_lib.MAX_SIDE:
        raise RuntimeError(f"mdil {fn}: images of {H} x {W} (sides of at most {_spx_lib.MAX_SIDE})")
    Gy, Gx = grid((H, W), S)
    dev = images.device
    with torch.no_grad(), torch.cuda.device(dev):
        ids = torch.empty(N, H, W, dtype=torch.int32, device=dev)
        centres = torch.empty(N, Gy * Gx, 5, dtype=torch.int32, device=dev)
        sums = torch.empty(N, Gy * Gx, 6, dtype=torch.int64, device=dev)
        _spx_lib.check(lib.mdil_spx_slic(images.data_ptr(), N, H, W, S, m, T, ids.data_ptr(), centres.data_ptr(),
                                         sums.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "mdil_spx_slic")
    return ids, centres, sums


def spx_table(label, qmap, ids, K, nc, target=None, ignore_index=-1, table=None, tcount=None, counters=None):
    """The per-superpixel table over stored maps, on the current stream.  ``label`` u8 and ``qmap`` u16 [N,H,W]
    (``acquire_head``'s), ``ids`` int32 [N,H,W] (any values; those outside [0, K) count in "bad_ids" alone), ``target``
    u8 or None.  ``table`` int64 [N,K,4+nc] and ``tcount`` int64 [N,K,nc] are ACCUMULATED into (default: zeroed ones;
    ``tcount`` exists with a target alone).  ``counters``: any of ``TABLE_COUNTERS`` as int64 [1] device tensors.
    -> (table, tcount or None)"""
    fn = "spx_table"
    lib = _spx_lib.load()
    nc = check_nc(fn, nc)
    K = _check_K(fn, K)
    hc.check_ignore_index(fn, ignore_index)
    N, H, W, dev = _id_maps(fn, ids, ((label, "label", torch.uint8), (qmap, "qmap", A.QMAP), (target, "target", torch.uint8)))
    if label is None or qmap is None:
        raise RuntimeError(f"mdil {fn}: label (uint8) and qmap (uint16) [N,H,W] on the device are required")
    if N * K * (FIELDS + nc) > _spx_lib.MAX_CELLS:
        raise RuntimeError(f"mdil {fn}: a table of {N} x {K} x {FIELDS + nc} cells (at most 2^31)")
    c = rc.check_counters(fn, counters, TABLE_COUNTERS)
    hc.check_tables(fn, _PATH, dev, torch.int64, ((table, "table", (N, K, FIELDS + nc)), (tcount, "tcount", (N, K, nc))) +
                    tuple((c[name], name, (1,)) for name in TABLE_COUNTERS))
    if target is None and (tcount is not None or c["bad_targets"] is not None):
        raise RuntimeError(f"mdil {fn}: tcount and the counter bad_targets need a target (uint8 [N,H,W]) on the device")
    with torch.no_grad(), torch.cuda.device(dev):
        if table is None:
            table = torch.zeros(N, K, FIELDS + nc, dtype=torch.int64, device=dev)
        if tcount is None and target is not None:
            tcount = torch.zeros(N, K, nc, dtype=torch.int64, device=dev)
        _spx_lib.check(
            lib.mdil_spx_table(label.data_ptr(), qmap.data_ptr(), hc.ptr(target), int(ignore_index), ids.data_ptr(), N, H, W, K,
                               nc, table.data_ptr(), hc.ptr(tcount), *(hc.ptr(c[name]) for name in TABLE_COUNTERS),
                               torch.cuda.current_stream(dev).cuda_stream),
            "mdil_spx_table")
    return table, tcount


def spx_apply(ids, selected, nc, answer=None, target=None, previous=None, fill=None, label=None, ignore_index=-1,
              drop_id=255, counters=None, want_out=True, want_mask=False):
    """What an annotator of the chosen superpixels hands back, on the current stream.  ``ids``: int32 [N,H,W];
    ``selected``: u8 [N,K], CHOSEN where it is 255; ``answer``: u8 [N,K] or None, the one label of each superpixel;
    ``target``, ``previous``, ``fill``, ``label``: u8 [N,H,W] or None.  A chosen pixel is its superpixel's answer
    (without one the target, without either ``drop_id``); elsewhere ``previous`` where that is not ``drop_id``, else
    ``fill`` where that is not ``drop_id``, else ``drop_id``.  -> (out u8 or None, mask u8 or None: 255 newly selected,
    128 kept, 64 filled, 0 none).  ``counters``: any of ``APPLY_COUNTERS`` as int64 device tensors
    (``apply_counter_shapes``), accumulated into; "annotated" needs an answer or a target, "bad_targets" and "noisy"
    a target, "wrong_shown" and "wrong_all" a target and a label map."""
    fn = "spx_apply"
    lib = _spx_lib.load()
    nc = check_nc(fn, nc)
    hc.check_ignore_index(fn, ignore_index)
    drop_id = hc.check_id(fn, "drop_id", drop_id)
    N, H, W, dev = _id_maps(fn, ids, tuple((t, name, torch.uint8) for t, name in ((target, "target"), (previous, "previous"),
                                                                                 (fill, "fill"), (label, "label"))))
    hc.chk(fn, _PATH, selected, "selected", torch.uint8)
    if selected.dim() != 2 or selected.shape[0] != N or selected.shape[1] < 1:
        raise RuntimeError(f"mdil {fn}: selected must be uint8 [{N}, K] (got {tuple(selected.shape)})")
    K = selected.shape[1]
    hc.check_tables(fn, _PATH, dev, torch.uint8, ((answer, "answer", (N, K)),))
    c = rc.check_counters(fn, counters, APPLY_COUNTERS)
    shapes = apply_counter_shapes(nc)
    hc.check_tables(fn, _PATH, dev, torch.int64, tuple((c[k], k, shapes[k]) for k in APPLY_COUNTERS))
    if answer is None and target is None and c["annotated"] is not None:
        raise RuntimeError(f"mdil {fn}: the counter annotated needs an answer or a target")
    if target is None and (c["bad_targets"] is not None or c["noisy"] is not None):
        raise RuntimeError(f"mdil {fn}: the counters bad_targets and noisy need a target")
    if (target is None or label is None) and (c["wrong_shown"] is not None or c["wrong_all"] is not None):
        raise RuntimeError(f"mdil {fn}: the counters wrong_shown and wrong_all need a target and a label map")
    if not want_out and not want_mask and all(v is None for v in c.values()):
        raise RuntimeError(f"mdil {fn}: nothing to do (no out map, no mask, no counters)")
    with torch.no_grad(), torch.cuda.device(dev):
        out = torch.empty(N, H, W, dtype=torch.uint8, device=dev) if want_out else None
        mask = torch.empty(N, H, W, dtype=torch.uint8, device=dev) if want_mask else None
        _spx_lib.check(
            lib.mdil_spx_apply(ids.data_ptr(), selected.data_ptr(), hc.ptr(answer), hc.ptr(target), hc.ptr(previous),
                               hc.ptr(fill), hc.ptr(label), N, H, W, K, nc, int(ignore_index), drop_id, hc.ptr(out), hc.ptr(mask),
                               *(hc.ptr(c[k]) for k in APPLY_COUNTERS), torch.cuda.current_stream(dev).cuda_stream),
            "mdil_spx_apply")
    return out, mask


# ------------------------------------------------------------------------- the host arithmetic
def _dominant(counts, empty):
    """int64 [..., nc] -> u8 [...]: the largest count's class, ties to the lowest class, ``empty`` where all are 0."""
    counts = torch.as_tensor(counts)
    nc = counts.shape[-1]
    top = counts.max(-1, keepdim=True).values
    classes = torch.arange(nc, device=counts.device).expand(counts.shape)
    first = torch.where(counts == top, classes, torch.full_like(classes, nc)).min(-1).values
    return torch.where(top[..., 0] > 0, first, torch.full_like(first, int(empty))).to(torch.uint8)


def dominant_answers(tcount, drop_id=255):
    """The one-click answer of every superpixel: the class most of its valid target pixels have (``tcount``
    int64 [..., nc]), ties to the lowest class, ``drop_id`` where nothing is valid.  -> u8 [...]"""
    return _dominant(tcount, hc.check_id("dominant_answers", "drop_id", drop_id))


def majority_labels(table, drop_id=255):
    """The same over the label counts of a table int64 [..., 4 + nc]: every superpixel's majority PREDICTED label."""
    return _dominant(torch.as_tensor(table)[..., FIELDS:], hc.check_id("majority_labels", "drop_id", drop_id))


def achievable_accuracy(tcount):
    """sum_k max_c tcount[k][c] over sum tcount: the accuracy of one-click answers on every superpixel, the usual
    superpixel quality number and what ``--step`` should be tuned on.  0 where nothing is valid."""
    t = torch.as_tensor(tcount)
    total = int(t.sum())
    return int(t.max(-1).values.sum()) / total if total else 0.0


def superpixel_edges(ids):
    """u8 like ``ids`` [N,H,W]: 255 where the right or the lower neighbour belongs to another superpixel."""
    e = torch.zeros(ids.shape, dtype=torch.bool, device=ids.device)
    e[:, :, :-1] |= ids[:, :, :-1] != ids[:, :, 1:]
    e[:, :-1, :] |= ids[:, :-1, :] != ids[:, 1:, :]
    return e.to(torch.uint8) * 255


# ------------------------------------------------------------------------------------------ CLI
def slic_params(args):
    return {"step": args.step, "compactness": args.compactness, "iterations": args.iterations}


def read_selection(path, params, size):
    """A ``selection.json`` of an earlier round -> {stem: set of superpixel ids}; refused when it was made with other
    SLIC parameters or on another size: its ids would name other regions."""
    with open(path) as f:
        saved = json.load(f)
    if "superpixels" not in saved or "step" not in saved:
        raise RuntimeError(f"--previous {path}: not a selection.json written by this command")
    theirs = {k: saved.get(k) for k in params}
    if theirs != params or tuple(saved.get("size", ())) != tuple(size):
        raise RuntimeError(f"--previous {path}: selected with {theirs} on maps of {saved.get('size')}, this run has {params} "
                           f"on {list(size)}")
    return {stem: {int(r[0]) for r in rows} for stem, rows in saved["superpixels"].items()}


def _segment(args, head, images, target=None, want_table=True, counters=None):
    """One batch: ``acquire_head``'s maps, the ids, and the table -> (label, qmap, ids, centres, table, tcount)"""
    label, qmap = A.acquire_head(ac.features(head, images), head.w, head.b, (2, 2), args.kind,
                                 counters={"nonfinite": counters["nonfinite"]} if counters else None, want_label=True,
                                 want_qmap=True)
    ids, centres, _ = spx_slic(images.contiguous(), args.step, args.compactness, args.iterations)   # --images come in NHWC order
    table = tcount = None
    if want_table:
        K = centres.shape[1]
        c = {k: counters[k] for k in TABLE_COUNTERS if target is not None or k == "bad_ids"} if counters else None
        table, tcount = spx_table(label, qmap, ids, K, head.nc, target, head.ign, counters=c)
    return label, qmap, ids, centres, table, tcount


def _table_pass(args, head, pool):
    """Pass 1: every image's table, valid-target counts and centres, kept on the host."""
    nc, dev = head.nc, head.dev
    counters = hc.zero_counters(dict.fromkeys(("nonfinite",) + TABLE_COUNTERS, (1,)), dev)
    tables, tcounts, centres, stems, given = [], [], [], [], torch.zeros(nc, dtype=torch.int64, device=dev)
    for s, images, target in ac.batches(args, head, pool):
        _, _, _, cen, table, tcount = _segment(args, head, images, target, counters=counters)
        tables.append(table.cpu())
        centres.append(cen.cpu())
        if tcount is not None:
            tcounts.append(tcount.cpu())
        stems.extend(s)
        ac.given_counts(given, target, nc, head.ignore)
    if head.labelled:
        rc.refuse_bad_targets("superpixel", counters, nc, head.ignore)
    if int(counters["bad_ids"].item()):
        raise RuntimeError(f"superpixel: {int(counters['bad_ids'].item())} pixels carry an id outside the grid")
    return SimpleNamespace(table=torch.cat(tables).reshape(-1, FIELDS + nc), centres=torch.cat(centres).reshape(-1, 5),
                           tcount=torch.cat(tcounts).reshape(-1, nc) if tcounts else None, stems=stems, given=given,
                           nonfinite=int(counters["nonfinite"].item()))


def _split(args, p1, size, before):
    """Every superpixel of the split: its image, its id and home cell, its size, and whether it may be chosen."""
    Gy, Gx = grid(size, args.step)
    M, K = len(p1.stems), Gy * Gx
    kidx = np.tile(np.arange(K), M)
    usable = p1.table[:, 0].numpy() > 0
    for i, stem in enumerate(p1.stems):
        for k in before.get(stem, ()):
            if 0 <= k < K:
                usable[i * K + k] = False
    total = M * size[0] * size[1]
    return SimpleNamespace(M=M, K=K, grid=(Gy, Gx), image=np.repeat(np.arange(M), K), tidx=kidx, ty=kidx // Gx, tx=kidx % Gx,
                           pixels=p1.table[:, 0].numpy(), image_pixels=[size[0] * size[1]] * M, total=total,
                           budget_pixels=args.budget * total, usable=usable)


def _choose(args, table, sp, by, labelled):
    """Ranks the split's superpixels by ``by`` (``acquire``'s scores on ``acquire``'s fields) and takes them within
    the budget -> (scores, chosen in rank order, pixels shown)."""
    scores = A.tile_scores(table, by, sp.image, sp.tidx, args.seed, labelled).numpy()
    order = A.rank_tiles(scores, sp.image, sp.ty, sp.tx, sp.usable)
    return (scores,) + A.select_tiles(order, sp.pixels, sp.image, sp.image_pixels, sp.budget_pixels, args.max_per_image)


def _report(args, head, p1, sp, scores, chosen, spent, answers):
    """-> (the report without what pass 2 adds, selection.json, the images with a chosen superpixel)"""
    nc, size, table = head.nc, head.size, p1.table
    touched = sorted({int(sp.image[i]) for i in chosen})
    per_stem = {}
    for i in chosen:                                   # in rank order
        cy, cx = (int(v) >> _spx_lib.FRACTION_BITS for v in p1.centres[i, :2])
        per_stem.setdefault(p1.stems[int(sp.image[i])], []).append(
            [int(sp.tidx[i]), cy, cx, int(table[i, 0]), float(scores[i]), None if answers is None else int(answers[i])])
    selection = dict(slic_params(args), size=list(size), answer=args.answer, kind=args.kind, by=args.by, budget=args.budget,
                     seed=args.seed, superpixels=per_stem)
    area = table[:, 0]
    live = area[area > 0]
    report = {"dataset": rc.source_name(args), "subset": args.subset, "task": args.task, "num_classes": nc, "kind": args.kind,
              "by": args.by, "answer": args.answer, "size": list(size), "budget": args.budget,
              "budget_is": "a share of the split's pixels, as in acquire; a superpixel's own pixel count is its size",
              "max_per_image": args.max_per_image, "seed": args.seed, "images": sp.M, "total_pixels": sp.total,
              "pixels_asked": sp.budget_pixels, "shown": spent, "shown_share": spent / sp.total if sp.total else 0.0,
              "clicks": len(chosen), "images_touched": len(touched), "superpixels_per_image": sp.K,
              "superpixels": int(sp.M * sp.K), "empty_superpixels": int((area == 0).sum()),
              "area_min": int(live.min()) if live.numel() else 0, "area_median": float(live.double().median()) if live.numel() else 0.0,
              "area_max": int(live.max()) if live.numel() else 0, "nonfinite": p1.nonfinite, "previous": args.previous}
    report.update(slic_params(args))
    if head.labelled:
        sel_idx = torch.tensor(chosen, dtype=torch.long)
        recall = {by: A.error_recall(table, torch.tensor(_choose(args, table, sp, by, True)[1], dtype=torch.long))
                  for by in A.CRITERIA}
        valid = p1.tcount[sel_idx]
        noisy = int(valid.sum() - valid.max(-1).values.sum()) if args.answer == "dominant" and chosen else 0
        report.update(error_recall=recall, error_recall_chosen=A.error_recall(table, sel_idx),
                      wrong_pixels=int(table[:, 2].sum()), valid_pixels=int(table[:, 3].sum()),
                      achievable_accuracy=achievable_accuracy(p1.tcount), noisy=noisy,
                      noisy_share=noisy / spent if spent else 0.0)
    return report, selection, touched


def _write_pass(args, head, pool, sp, p1, chosen, answers):
    """Pass 2: the ids again, ``spx_apply``, the maps of ``--out`` and the tree of ``--out-root`` -> (what the report
    gains, the paths)"""
    nc, size, dev, K = head.nc, head.size, head.dev, sp.K
    selected = torch.zeros(sp.M, K, dtype=torch.uint8)
    selected.view(-1)[torch.tensor(chosen, dtype=torch.long)] = MASK_SELECTED
    names = APPLY_COUNTERS if head.labelled else ("shown", "kept", "filled", "bad_ids")
    counters = new_apply_counters(nc, dev, names)
    writer = ac.LabelTreeWriter(pool, args, "--out-root", args.out_root, args.out, sp.M)
    for s, images, target in ac.batches(args, head, pool):
        i0, n = writer.seen, len(s)
        label, qmap, ids, _, _, _ = _segment(args, head, images, want_table=False)
        answer = answers[i0 * K:(i0 + n) * K].reshape(n, K).contiguous().to(dev) if answers is not None else None
        prev, fill = writer.earlier_labels(args, range(n), size, dev)
        out, mask = spx_apply(ids, selected[i0:i0 + n].contiguous().to(dev), nc, answer, target, prev, fill,
                              label if head.labelled else None, head.ign, 255, counters, want_out=bool(args.out_root),
                              want_mask=bool(args.out))
        writer.wait()
        if args.out:
            writer.write_maps(s, select=mask, superpixels=superpixel_edges(ids), uncertainty=(A.q_values(qmap) >> 8).to(torch.uint8))
        writer.write_batch(s, images, out, head.ignore)
    written = writer.close()
    c = {k: v.cpu() for k, v in counters.items()}
    gained = dict(shown_applied=int(c["shown"]), kept=c["kept"].tolist(), filled=c["filled"].tolist())
    if head.labelled:
        gained.update(ac.annotated_block("superpixel", c, p1.given, nc), noisy_applied=int(c["noisy"]),
                      wrong_shown=int(c["wrong_shown"]))
    return gained, written


def _vote(args, head, pool):
    """``--vote``: every superpixel's majority predicted label as ``<stem>_label.png``; with labels the confusion
    matrices of the plain and of the voted maps -> (report, the paths)"""
    from . import fullres as FR
    nc, dev = head.nc, head.dev
    writer = ac.LabelTreeWriter(pool, args, "--out-root", None, args.out)
    conf = {k: torch.zeros(nc * nc, dtype=torch.int64, device=dev) for k in ("plain", "voted")}
    changed = 0
    for s, images, target in ac.batches(args, head, pool):
        label, _, ids, centres, table, _ = _segment(args, head, images)
        K = centres.shape[1]
        every = torch.full((len(s), K), MASK_SELECTED, dtype=torch.uint8, device=dev)
        voted, _ = spx_apply(ids, every, nc, majority_labels(table))
        changed += int((voted != label).sum())
        if target is not None:
            t = target.long()
            ok = (t < nc) & (t != head.ign)
            for name, pred in (("plain", label), ("voted", voted)):
                conf[name] += torch.bincount(t[ok] * nc + pred[ok].long().clamp(max=nc - 1), minlength=nc * nc)
        writer.wait()
        if args.out:
            writer.write_maps(s, label=voted)
        writer.seen += len(s)
    written = writer.close()
    report = {"dataset": rc.source_name(args), "subset": args.subset, "task": args.task, "num_classes": nc, "vote": True,
              "size": list(head.size), "images": writer.seen, "pixels_changed": changed}
    report.update(slic_params(args))
    if head.labelled:
        for name, m in conf.items():
            m = m.reshape(nc, nc).cpu().double()
            mean, per_class = FR.iou_rule(nc, head.ign, m.diagonal(), m.sum(0), m.sum(1))
            report[f"miou_{name}"], report[f"iou_{name}"] = float(mean), per_class.tolist()
    return report, written


def main(args):
    _refusals(args)
    head = ac.open_head(args)
    written = []
    with hc.png_pool() as pool:
        if args.vote:
            report, written = _vote(args, head, pool)
            print(f"{report['dataset']} (task {args.task}): {report['images']} images voted over superpixels of step {args.step}: "
                  f"{report['pixels_changed']} pixels changed" +
                  (f"; mIoU {report['miou_plain'] * 100:.2f} % plain, {report['miou_voted'] * 100:.2f} % voted" if head.labelled else ""))
            return ac.finish(report, written, args)
        before = read_selection(args.previous, slic_params(args), head.size) if args.previous else {}
        p1 = _table_pass(args, head, pool)
        sp = _split(args, p1, head.size, before)
        scores, chosen, spent = _choose(args, p1.table, sp, args.by, head.labelled)
        answers = dominant_answers(p1.tcount, 255) if head.labelled and args.answer == "dominant" else None
        report, selection, touched = _report(args, head, p1, sp, scores, chosen, spent, answers)
        if args.out or args.out_root:
            gained, written = _write_pass(args, head, pool, sp, p1, chosen, answers)
            report.update(gained)
    print(f"{report['dataset']} (task {args.task}): {sp.M} images, {len(chosen)} clicks on {sp.M * sp.K} superpixels of step "
          f"{args.step} in {len(touched)} images by {args.by} ({args.kind}): {spent} pixels of {sp.budget_pixels:.0f} asked "
          f"({report['shown_share'] * 100:.2f} % of the split); {report['nonfinite']} non-finite pixels")
    print(f"  areas {report['area_min']} / {report['area_median']:.0f} / {report['area_max']} (min / median / max), "
          f"{report['empty_superpixels']} empty")
    if head.labelled:
        print(f"  achievable accuracy {report['achievable_accuracy'] * 100:.2f} %; noisy share of the shown pixels "
              f"{report['noisy_share'] * 100:.2f} % ({args.answer} answers)")
        print("  error recall at the budget: " + "  ".join(f"{k} {v * 100:.2f} %" for k, v in report["error_recall"].items()))
    return ac.finish(report, written, args, selection)


def _refusals(args):
    """Raise a RuntimeError that names why this combination of flags is refused."""
    ac.refuse_head(args, "the split's")
    if max(args.height, args.width) > _spx_lib.MAX_SIDE:
        raise RuntimeError(f"--height {args.height} x --width {args.width}: sides of at most {_spx_lib.MAX_SIDE}")
    check_slic("--step / --compactness / --iterations", args.step, args.compactness, args.iterations)
    if args.max_per_image is not None and not 0.0 < args.max_per_image <= 1.0:
        raise RuntimeError(f"--max-per-image {args.max_per_image} outside (0, 1]: a share of one image's pixels")
    if args.vote and (args.out_root or args.previous or args.previous_root or args.fill_root):
        raise RuntimeError("--vote writes <stem>_label.png into --out and a report: it takes no --out-root, --previous, "
                           "--previous-root or --fill-root")
    ac.refuse_rounds(args)


def build_parser():
    p = hc.RefusingParser(_refusals, description="which superpixels of a split to label first: an integer SLIC on the "
                                                 "device, acquire's scores per superpixel, a ranking under a pixel budget, "
                                                 "and the label tree one-click answers would give")
    ac.add_source_flags(p, "share of the split's pixels that may be shown (read and not used by --vote)")
    p.add_argument("--step", type=int, default=16, help="S of the SLIC grid in pixels, 4 to 64 (default %(default)s)")
    p.add_argument("--compactness", type=int, default=10, help="m of the SLIC distance, 1 to 64 (default %(default)s)")
    p.add_argument("--iterations", type=int, default=10, help="assign + update rounds, 0 to 32 (default %(default)s)")
    p.add_argument("--answer", choices=ANSWERS, default="dominant",
                   help="what a chosen superpixel receives: its dominant label with one click, or the exact target "
                        "(default %(default)s)")
    ac.add_criterion_flags(p, A.KINDS, A.CRITERIA, "the superpixel criterion")
    p.add_argument("--max-per-image", type=float, help="skip a superpixel once its image has this share of its pixels selected")
    p.add_argument("--vote", action="store_true", help="write every superpixel's majority predicted label as "
                                                       "<stem>_label.png into --out instead; no budget is used")
    ac.add_round_flags(p, "its superpixels leave the ranking",
                       "<stem>_superpixels.png (255 on the borders), <stem>_uncertainty.png (q >> 8)")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
