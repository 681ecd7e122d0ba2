"""Acquire on MI355X: I can pay for labels on 5 % of these pixels -- which 5 %?  Region-based active
learning over fixed tiles of the label grid (Mackowiak et al., CEREALS, BMVC 2018) with the criteria of
Xie et al. (RIPU, CVPR 2022), two passes over a split:

  pass 1  the network and ``acquire_head``: per pixel the label and ONE uncertainty (``--kind`` msp, entropy
          or margin) as a linear 16-bit q, and per tile the integer table [pixels, sum q, wrong, with a
          valid target, label counts]; the host keeps the table alone;
  pass 2  only images with a selected tile: ``acquire_apply`` writes what an annotator of those tiles hands
          back, on top of an earlier round's labels and of fill labels.

    python -m mdil_ss_amd.acquire --state CKPT --num-classes 20 20 --task 1 --dataset BDD --subset train \
        --budget 0.05 --tile 32 32 --kind entropy --by ripu --json FILE --out-root ROOT --layout BDD \
        [--max-per-image 0.25] [--previous SEL.json --previous-root ROOT0] [--fill-root PSEUDO_ROOT] [--out DIR]
    python -m mdil_ss_amd.acquire --state CKPT ... --images DIR --budget 0.05 --out DIR --json FILE

Tile scores, fp64 from the integer table alone: ``uncertainty`` U = sum q / (65536 pixels); ``impurity``
I = the entropy of the tile's label histogram over ln nc; ``ripu`` U * I; ``random`` a SplitMix64 hash of
(seed, image, tile); ``oracle`` (needs labels) wrong / pixels.  Tiles are ranked by score, ties by (image,
ty, tx), and taken in that order while the pixels shown stay within ``--budget`` x the split's pixels.
With labels the run simulates the annotator: ``--out-root`` writes a label tree the trainers open unchanged
(targets inside the selected tiles, 255 or ``--fill-root``'s labels outside) and the report gives the
error recall at the budget for every criterion.  Without labels ``--out`` writes ``<stem>_select.png`` and
``<stem>_uncertainty.png``.  Both write ``selection.json``.

What is NOT measured.  Everything here was measured on a randomly initialised network only: nothing says
which criterion finds the errors of a trained head on BDD or IDD.  The fixed tile grid is a simplification
of RIPU's sliding (2k+1)^2 neighbourhood, which is not built.  No retraining on the selected labels is run."""
import json
import math
from types import SimpleNamespace

import numpy as np
import torch

from . import _acquire_lib
from . import _annotate_common as ac
from . import _head_common as hc
from . import _report_common as rc

_PATH = "acquisition"
Q_ONE = 65536                                   # q = min(65535, floor(max(u, 0) * Q_ONE))
QMAP = torch.uint16
FIELDS = _acquire_lib.TILE_FIELDS               # pixels, sum q, wrong, valid; then nc label counts
KINDS = ("msp", "entropy", "margin")
CRITERIA = ("uncertainty", "impurity", "ripu", "random", "oracle")
HEAD_COUNTERS = ("nonfinite", "bad_targets")
APPLY_COUNTERS = ("shown", "annotated", "kept", "filled", "bad_targets")
MASK_SELECTED, MASK_KEPT, MASK_FILLED = 255, 128, 64
_M64 = (1 << 64) - 1


q_values = hc.q_values                          # a stored q map as int64
check_id = hc.check_id
_read_labels = ac.read_labels


def check_nc(fn, nc):
    return hc.check_nc(fn, _acquire_lib, nc)


def check_tile(fn, tile):
    """-> (th, tw), each even and in [2, 256]."""
    try:
        th, tw = (int(v) for v in tile)
    except (TypeError, ValueError):
        raise RuntimeError(f"mdil {fn}: tile must be (height, width), got {tile!r}") from None
    lo, hi = _acquire_lib.MIN_TILE, _acquire_lib.MAX_TILE
    if not (lo <= th <= hi and lo <= tw <= hi) or th % 2 or tw % 2:
        raise RuntimeError(f"mdil {fn}: tile {th} x {tw} (each side even and in [{lo}, {hi}])")
    return th, tw


def check_kind(fn, kind):
    if kind not in KINDS:
        raise RuntimeError(f"mdil {fn}: kind {kind!r} (one of {list(KINDS)})")
    return KINDS.index(kind)


def tile_grid(size, tile):
    """Tiles of ``tile`` over a label grid of ``size`` = (Hl, Wl) -> (Ty, Tx); the last ones may be ragged."""
    return -(-int(size[0]) // tile[0]), -(-int(size[1]) // tile[1])


def inv_log_nc(nc):
    """What ``acquire_head`` multiplies the entropy by: float32(1 / ln nc)."""
    return float(np.float32(1.0 / math.log(nc)))


def apply_counter_shapes(nc):
    return {"shown": (1,), "annotated": (nc,), "kept": (nc,), "filled": (nc,), "bad_targets": (1,)}


def new_apply_counters(nc, dev, names=APPLY_COUNTERS):
    return hc.zero_counters(apply_counter_shapes(nc), dev, names)


def new_tiles(N, size, tile, nc, dev):
    """The zeroed table of ``acquire_head`` for N label maps of ``size``: int64 [N, Ty, Tx, 4 + nc]."""
    Ty, Tx = tile_grid(size, tile)
    return torch.zeros(N, Ty, Tx, FIELDS + nc, dtype=torch.int64, device=dev)


# --------------------------------------------------------------------------------- entry points
def acquire_head(features, weight, bias, tile, kind="entropy", target=None, ignore_index=-1, tiles=None,
                 counters=None, want_label=False, want_qmap=False):
    """``output_conv`` + argmax + one uncertainty as a linear 16-bit q on NHWC decoder features [N,H,W,16]
    and the ``ConvTranspose2d(16, nc, 2, 2)`` parameters, 2 <= nc <= 32, on the current stream.
    -> (label u8 [N,2H,2W] or None, qmap u16 [N,2H,2W] or None).  ``tile``: (th, tw), even, in [2, 256];
    ``kind``: "msp" (1 - p_top), "entropy" (over ln nc) or "margin" (1 - (p_top - p_second)); ``target``: u8
    [N,2H,2W] on the device; ``tiles``: int64 [N,Ty,Tx,4+nc] on the device (``new_tiles``), accumulated
    into, never cleared -- its fields 2 and 3 (wrong, with a valid target) are added to with a target alone;
    ``counters``: any of ``HEAD_COUNTERS`` as int64 [1] device tensors; "bad_targets" needs a target."""
    fn = "acquire_head"
    lib = _acquire_lib.load()
    for t, name in ((features, "features"), (weight, "weight"), (bias, "bias")):
        hc.chk(fn, _PATH, t, name)
    x, w, b = features, weight, bias
    nc = hc.check_params(fn, w, b, x)
    N, H, W = x.shape[0], x.shape[1], x.shape[2]
    hc.check_classes(fn, _acquire_lib, nc, x, w, b)
    th, tw = check_tile(fn, tile)
    k = check_kind(fn, kind)
    hc.check_ignore_index(fn, ignore_index)
    dev = x.device
    Ty, Tx = tile_grid((2 * H, 2 * W), (th, tw))
    hc.check_tables(fn, _PATH, dev, torch.uint8, ((target, "target", (N, 2 * H, 2 * W)),))
    c = rc.check_counters(fn, counters, HEAD_COUNTERS)
    hc.check_tables(fn, _PATH, dev, torch.int64, ((tiles, "tiles", (N, Ty, Tx, FIELDS + nc)),) +
                    tuple((c[name], name, (1,)) for name in HEAD_COUNTERS))
    if target is None and c["bad_targets"] is not None:
        raise RuntimeError(f"mdil {fn}: the counter bad_targets needs a target (uint8 [N,2H,2W]) on the device")
    if not want_label and not want_qmap and tiles is None and all(v is None for v in c.values()):
        raise RuntimeError(f"mdil {fn}: nothing to do (no label map, no q map, no tiles, no counters)")
    with torch.no_grad(), torch.cuda.device(dev):
        label = torch.empty(N, 2 * H, 2 * W, dtype=torch.uint8, device=dev) if want_label else None
        qmap = torch.empty(N, 2 * H, 2 * W, dtype=QMAP, device=dev) if want_qmap else None
        _acquire_lib.check(
            lib.mdil_acquire_head(x.data_ptr(), w.data_ptr(), b.data_ptr(), N, H, W, nc, th, tw, k, inv_log_nc(nc),
                                  hc.ptr(target), int(ignore_index), hc.ptr(label), hc.ptr(qmap), hc.ptr(tiles),
                                  *(hc.ptr(c[name]) for name in HEAD_COUNTERS),
                                  torch.cuda.current_stream(dev).cuda_stream),
            "mdil_acquire_head")
    return label, qmap


def acquire_apply(selected, size, tile, nc, target=None, previous=None, fill=None, ignore_index=-1, drop_id=255,
                  counters=None, want_out=True, want_mask=False):
    """What an annotator of the selected tiles hands back, on the current stream.  ``selected``: u8
    [N,Ty,Tx] on the device, non-zero where the tile is chosen, for maps of ``size`` = (Hl, Wl) and tiles
    of ``tile``; ``target``, ``previous``, ``fill``: u8 [N,Hl,Wl] or None.  In a chosen tile a pixel is the
    target (``drop_id`` without one); elsewhere ``previous`` where that is not ``drop_id``, else ``fill``
    where that is not ``drop_id``, else ``drop_id``.  -> (out u8 or None, mask u8 or None: 255 newly
    selected, 128 kept, 64 filled, 0 none).  ``counters``: any of ``APPLY_COUNTERS`` as int64 device tensors
    (``apply_counter_shapes``), accumulated into; "annotated" and "bad_targets" need a target."""
    fn = "acquire_apply"
    lib = _acquire_lib.load()
    nc = check_nc(fn, nc)
    th, tw = check_tile(fn, tile)
    hc.check_ignore_index(fn, ignore_index)
    drop_id = check_id(fn, "drop_id", drop_id)
    hc.chk(fn, _PATH, selected, "selected", torch.uint8)
    try:
        Hl, Wl = (int(v) for v in size)
    except (TypeError, ValueError):
        raise RuntimeError(f"mdil {fn}: size must be (height, width), got {size!r}") from None
    if Hl < 1 or Wl < 1 or selected.dim() != 3 or selected.numel() == 0 or \
            tuple(selected.shape[1:]) != tile_grid((Hl, Wl), (th, tw)):
        raise RuntimeError(f"mdil {fn}: selected must be uint8 [N, {-(-max(Hl, 1) // th)}, {-(-max(Wl, 1) // tw)}] for maps "
                           f"of {Hl} x {Wl} and tiles of {th} x {tw} (got {tuple(selected.shape)})")
    N, dev = selected.shape[0], selected.device
    hc.check_tables(fn, _PATH, dev, torch.uint8, tuple((t, name, (N, Hl, Wl)) for t, name in
                                                       ((target, "target"), (previous, "previous"), (fill, "fill"))))
    c = rc.check_counters(fn, counters, APPLY_COUNTERS)
    shapes = apply_counter_shapes(nc)
    hc.check_tables(fn, _PATH, dev, torch.int64, tuple((c[k], k, shapes[k]) for k in APPLY_COUNTERS))
    if target is None and (c["annotated"] is not None or c["bad_targets"] is not None):
        raise RuntimeError(f"mdil {fn}: the counters annotated and bad_targets need a target")
    if not want_out and not want_mask and all(v is None for v in c.values()):
        raise RuntimeError(f"mdil {fn}: nothing to do (no out map, no mask, no counters)")
    with torch.no_grad(), torch.cuda.device(dev):
        out = torch.empty(N, Hl, Wl, dtype=torch.uint8, device=dev) if want_out else None
        mask = torch.empty(N, Hl, Wl, dtype=torch.uint8, device=dev) if want_mask else None
        _acquire_lib.check(
            lib.mdil_acquire_apply(selected.data_ptr(), hc.ptr(target), hc.ptr(previous), hc.ptr(fill), N, Hl, Wl, th, tw,
                                   nc, int(ignore_index), drop_id, hc.ptr(out), hc.ptr(mask),
                                   *(hc.ptr(c[k]) for k in APPLY_COUNTERS), torch.cuda.current_stream(dev).cuda_stream),
            "mdil_acquire_apply")
    return out, mask


# ------------------------------------------------------------------------- the host arithmetic
def _table(table, who):
    t = torch.as_tensor(table)
    if t.is_cuda or t.dtype != torch.int64 or t.dim() != 2 or t.shape[1] < FIELDS + _acquire_lib.MIN_CLASSES:
        raise RuntimeError(f"mdil {who}: the tile table must be a host int64 tensor [tiles, 4 + nc] (got {t.dtype} "
                           f"{tuple(t.shape)} on {t.device})")
    return t


def mix64(seed, k):
    """signif.hip's generator: SplitMix64's finaliser of seed + golden * k, in 64-bit wrap-around arithmetic."""
    z = (seed + 0x9E3779B97F4A7C15 * k) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def random_score(seed, image, tile):
    """The ``random`` criterion of tile ``tile`` (= ty * Tx + tx) of image ``image`` (its place in the split):
    the upper 53 bits of mix64(mix64(seed, image + 1), tile + 1) as a number in [0, 1)."""
    return (mix64(mix64(int(seed) & _M64, int(image) + 1), int(tile) + 1) >> 11) / float(1 << 53)


def uncertainty_of(table):
    """U = sum q / (65536 pixels) per tile, fp64; 0 for a tile without a finite pixel."""
    t = _table(table, "acquire uncertainty_of")
    cnt = t[:, 0].double()
    return torch.where(cnt > 0, t[:, 1].double() / (Q_ONE * cnt.clamp(min=1.0)), torch.zeros_like(cnt))


def impurity_of(table):
    """I = -sum_c (h_c / pixels) ln(h_c / pixels) / ln nc per tile, fp64, over the classes with h_c > 0."""
    t = _table(table, "acquire impurity_of")
    nc = t.shape[1] - FIELDS
    cnt = t[:, 0].double().clamp(min=1.0)
    p = t[:, FIELDS:].double() / cnt[:, None]
    terms = torch.where(p > 0, -p * torch.log(p.clamp(min=1e-300)), torch.zeros_like(p))
    return terms.sum(1) / math.log(nc)


def tile_scores(table, by, image=None, tile=None, seed=0, labelled=True):
    """The criterion ``by`` of every tile of a host table [tiles, 4 + nc] -> float64 [tiles].  ``random``
    needs each tile's ``image`` and ``tile`` index; ``oracle`` needs a table filled with targets."""
    t = _table(table, "acquire tile_scores")
    if by not in CRITERIA:
        raise RuntimeError(f"mdil acquire tile_scores: criterion {by!r} (one of {list(CRITERIA)})")
    if by == "uncertainty":
        return uncertainty_of(t)
    if by == "impurity":
        return impurity_of(t)
    if by == "ripu":
        return uncertainty_of(t) * impurity_of(t)
    if by == "random":
        if image is None or tile is None:
            raise RuntimeError("mdil acquire tile_scores: the random criterion needs every tile's image and tile index")
        return torch.tensor([random_score(seed, i, j) for i, j in zip(image.tolist(), tile.tolist())],
                            dtype=torch.float64).reshape(-1)
    if not labelled:
        raise RuntimeError("mdil acquire tile_scores: the oracle criterion needs labels (fields 2 and 3 of the tile "
                           "table are filled with a target alone)")
    cnt = t[:, 0].double()
    return torch.where(cnt > 0, t[:, 2].double() / cnt.clamp(min=1.0), torch.zeros_like(cnt))


def rank_tiles(scores, image, ty, tx, usable=None):
    """The order tiles are offered in: score descending, ties by (image, ty, tx) ascending; ``usable`` (bool)
    leaves tiles out.  -> int64 indices (numpy)."""
    s = np.asarray(scores, dtype=np.float64)
    order = np.lexsort((np.asarray(tx), np.asarray(ty), np.asarray(image), -s))
    if usable is not None:
        order = order[np.asarray(usable, dtype=bool)[order]]
    return order


def select_tiles(order, pixels, image, image_pixels, budget_pixels, max_per_image=None):
    """Walks ``order``: a tile whose image would pass the share ``max_per_image`` of its ``image_pixels`` is
    skipped; the walk ends at the first other tile that would take the pixels shown past ``budget_pixels``.
    ``pixels``: every tile's own size.  -> (chosen indices in rank order, pixels shown)"""
    spent, chosen, per_image = 0, [], {}
    for i in order.tolist() if hasattr(order, "tolist") else order:
        n, im = int(pixels[i]), int(image[i])
        if max_per_image is not None and per_image.get(im, 0) + n > max_per_image * int(image_pixels[im]):
            continue
        if spent + n > budget_pixels:
            break
        spent += n
        per_image[im] = per_image.get(im, 0) + n
        chosen.append(i)
    return chosen, spent


def tile_boxes(size, tile):
    """(y0, x0, y1, x1) of every tile of one map, row-major, and its pixel count."""
    (Hl, Wl), (th, tw) = size, tile
    Ty, Tx = tile_grid(size, tile)
    boxes = [(y * th, x * tw, min(Hl, y * th + th), min(Wl, x * tw + tw)) for y in range(Ty) for x in range(Tx)]
    return boxes, [(b[2] - b[0]) * (b[3] - b[1]) for b in boxes]


# ------------------------------------------------------------------------------------------ CLI
def plan_label_tree(args):
    """The label tree of ``--out-root`` -> (labels' folder, label names, images' folder or None)."""
    return rc.plan_label_tree(args, args.out_root)


def read_selection(path, tile, size):
    """A ``selection.json`` of an earlier round -> {stem: set of (ty, tx)}."""
    with open(path) as f:
        saved = json.load(f)
    if "tiles" not in saved or "tile" not in saved:
        raise RuntimeError(f"--previous {path}: not a selection.json written by this command")
    if tuple(saved["tile"]) != tuple(tile) or tuple(saved.get("size", size)) != tuple(size):
        raise RuntimeError(f"--previous {path}: selected with tiles of {saved['tile']} on maps of {saved.get('size')}, this "
                           f"run has {list(tile)} on {list(size)}")
    return {stem: {(int(b[0]) // tile[0], int(b[1]) // tile[1]) for b in boxes} for stem, boxes in saved["tiles"].items()}


def error_recall(table, chosen):
    """Wrong pixels inside the chosen tiles over all wrong pixels (0 where nothing is wrong)."""
    wrong = int(table[:, 2].sum())
    return int(table[chosen, 2].sum()) / wrong if wrong else 0.0


def _table_pass(args, head, tile, pool):
    """Pass 1: the tile table of every image, kept on the host -> (table [tiles, 4 + nc], stems, given, nonfinite)."""
    nc, names = head.nc, HEAD_COUNTERS if head.labelled else ("nonfinite",)
    counters = hc.zero_counters(dict.fromkeys(HEAD_COUNTERS, (1,)), head.dev, names)
    tables, stems, given = [], [], torch.zeros(nc, dtype=torch.int64, device=head.dev)
    for s, images, target in ac.batches(args, head, pool):
        t = new_tiles(images.shape[0], head.size, tile, nc, head.dev)
        acquire_head(ac.features(head, images), head.w, head.b, tile, args.kind, target, head.ign, t, counters)
        tables.append(t.cpu())
        stems.extend(s)
        ac.given_counts(given, target, nc, head.ignore)
    if head.labelled:
        rc.refuse_bad_targets("acquire", counters, nc, head.ignore)
    return torch.cat(tables).reshape(-1, FIELDS + nc), stems, given, int(counters["nonfinite"].item())


def _split(args, table, stems, tile, size):
    """Every tile of the split: its image, its index and place in it, its size, and whether it may be chosen."""
    Ty, Tx = tile_grid(size, tile)
    boxes, box_pixels = tile_boxes(size, tile)
    M, T = len(stems), Ty * Tx
    tidx = np.tile(np.arange(T), M)
    usable = table[:, 0].numpy() > 0
    if args.previous:
        before = read_selection(args.previous, tile, size)
        for i, stem in enumerate(stems):
            for (y, x) in before.get(stem, ()):
                if y < Ty and x < Tx:
                    usable[i * T + y * Tx + x] = False
    total = M * size[0] * size[1]
    return SimpleNamespace(M=M, T=T, grid=(Ty, Tx), boxes=boxes, image=np.repeat(np.arange(M), T), tidx=tidx, ty=tidx // Tx,
                           tx=tidx % Tx, pixels=np.tile(np.asarray(box_pixels), M), image_pixels=[size[0] * size[1]] * M,
                           total=total, budget_pixels=args.budget * total, usable=usable)


def _choose(args, table, sp, by, labelled):
    """Ranks the split's tiles by ``by`` and takes them within the budget -> (scores, chosen in rank order, pixels)."""
    scores = tile_scores(table, by, sp.image, sp.tidx, args.seed, labelled).numpy()
    order = rank_tiles(scores, sp.image, sp.ty, sp.tx, sp.usable)
    return (scores,) + select_tiles(order, sp.pixels, sp.image, sp.image_pixels, sp.budget_pixels, args.max_per_image)


def _report(args, head, table, stems, sp, tile, scores, chosen, spent, nonfinite):
    """-> (the report without what pass 2 adds, selection.json, the images with a selected tile)"""
    nc, size, M, image = head.nc, head.size, sp.M, sp.image
    touched = sorted({int(image[i]) for i in chosen})
    per_stem = {}
    for i in chosen:                                   # in rank order
        per_stem.setdefault(stems[int(image[i])], []).append(list(sp.boxes[int(sp.tidx[i])]) + [float(scores[i])])
    selection = {"tile": list(tile), "size": list(size), "kind": args.kind, "by": args.by, "budget": args.budget,
                 "seed": args.seed, "tiles": per_stem}
    U, I = uncertainty_of(table), impurity_of(table)
    sel_idx = torch.tensor(chosen, dtype=torch.long)
    live = torch.from_numpy(table[:, 0].numpy() > 0)
    hist_all, hist_sel = table[:, FIELDS:].sum(0), table[sel_idx, FIELDS:].sum(0)
    per_image_tiles = np.bincount(image[chosen], minlength=M) if chosen else np.zeros(M, dtype=np.int64)
    report = {"dataset": rc.source_name(args), "subset": args.subset, "task": args.task, "num_classes": nc,
              "kind": args.kind, "by": args.by, "tile": list(tile), "size": list(size), "budget": args.budget,
              "max_per_image": args.max_per_image, "seed": args.seed, "images": M, "total_pixels": sp.total,
              "pixels_asked": sp.budget_pixels, "pixels_spent": spent, "spent_share": spent / sp.total,
              "tiles": int(M * sp.T), "tiles_selected": len(chosen), "images_touched": len(touched),
              "tiles_per_image_mean": len(chosen) / max(1, len(touched)), "tiles_per_image_max": int(per_image_tiles.max()),
              "mean_uncertainty_selected": float(U[sel_idx].mean()) if chosen else 0.0,
              "mean_uncertainty_all": float(U[live].mean()) if bool(live.any()) else 0.0,
              "mean_impurity_selected": float(I[sel_idx].mean()) if chosen else 0.0,
              "mean_impurity_all": float(I[live].mean()) if bool(live.any()) else 0.0,
              "predicted_selected": hist_sel.tolist(), "predicted_all": hist_all.tolist(),
              "nonfinite": nonfinite, "previous": args.previous}
    if head.labelled:
        recall = {by: error_recall(table, torch.tensor(_choose(args, table, sp, by, True)[1], dtype=torch.long))
                  for by in CRITERIA}
        report.update(error_recall=recall, error_recall_chosen=error_recall(table, sel_idx),
                      wrong_pixels=int(table[:, 2].sum()), valid_pixels=int(table[:, 3].sum()))
    return report, selection, touched


def _write_pass(args, head, tile, pool, sp, chosen, touched, given):
    """Pass 2, over the images with a selected tile (every image where an earlier round or fill labels come in):
    ``acquire_apply``, the maps of ``--out`` and the tree of ``--out-root`` -> (what the report gains, the paths)"""
    nc, size, dev = head.nc, head.size, head.dev
    selected = torch.zeros((sp.M,) + sp.grid, dtype=torch.uint8)
    selected.view(-1)[torch.tensor(chosen, dtype=torch.long)] = 1
    everywhere, touched = bool(args.previous_root or args.fill_root), set(touched)
    counters = new_apply_counters(nc, dev, APPLY_COUNTERS if head.labelled else ("shown", "kept", "filled"))
    writer = ac.LabelTreeWriter(pool, args, "--out-root", args.out_root, args.out, sp.M)
    for s, images, target in ac.batches(args, head, pool):
        i0 = writer.seen
        idx = [j for j in range(len(s)) if everywhere or (i0 + j) in touched]
        writer.wait()
        out = None
        if idx:
            pick = torch.tensor(idx, dtype=torch.long, device=dev)
            sel = selected[[i0 + j for j in idx]].contiguous().to(dev)
            prev, fill = writer.earlier_labels(args, idx, size, dev)
            tgt = target[pick].contiguous() if target is not None else None
            out, mask = acquire_apply(sel, size, tile, nc, tgt, prev, fill, head.ign, 255, counters,
                                      want_out=bool(args.out_root), want_mask=bool(args.out))
            if args.out:
                _, qmap = acquire_head(ac.features(head, images[pick].contiguous()), head.w, head.b, tile, args.kind,
                                       want_qmap=True)
                writer.write_maps([s[j] for j in idx], select=mask, uncertainty=(q_values(qmap) >> 8).to(torch.uint8))
        writer.write_batch(s, images, out, head.ignore, idx)
    written = writer.close()
    c = {k: v.cpu() for k, v in counters.items()}
    gained = dict(shown=int(c["shown"]), kept=c["kept"].tolist(), filled=c["filled"].tolist())
    if head.labelled:
        gained.update(ac.annotated_block("acquire", c, given, nc))
    return gained, written


def main(args):
    _refusals(args)
    head = ac.open_head(args)
    tile = check_tile("acquire", args.tile)
    written = []
    with hc.png_pool() as pool:
        table, stems, given, nonfinite = _table_pass(args, head, tile, pool)
        sp = _split(args, table, stems, tile, head.size)
        scores, chosen, spent = _choose(args, table, sp, args.by, head.labelled)
        report, selection, touched = _report(args, head, table, stems, sp, tile, scores, chosen, spent, nonfinite)
        if args.out or args.out_root:
            gained, written = _write_pass(args, head, tile, pool, sp, chosen, touched, given)
            report.update(gained)
    print(f"{report['dataset']} (task {args.task}): {sp.M} images, {len(chosen)} of {sp.M * sp.T} tiles of {tile[0]} x {tile[1]} in "
          f"{len(touched)} images by {args.by} ({args.kind}): {spent} pixels of {sp.budget_pixels:.0f} asked "
          f"({spent / sp.total * 100:.2f} % of the split); {report['nonfinite']} non-finite pixels")
    print(f"  mean uncertainty {report['mean_uncertainty_selected']:.4f} selected / {report['mean_uncertainty_all']:.4f} all; "
          f"mean impurity {report['mean_impurity_selected']:.4f} / {report['mean_impurity_all']:.4f}")
    if head.labelled:
        print("  error recall at the budget: " + "  ".join(f"{k} {v * 100:.2f} %" for k, v in report["error_recall"].items()))
    return ac.finish(report, written, args, selection)


def _refusals(args):
    """Raise a RuntimeError that names why this combination of flags is refused."""
    ac.refuse_head(args, "the split's")
    if args.max_per_image is not None and not 0.0 < args.max_per_image <= 1.0:
        raise RuntimeError(f"--max-per-image {args.max_per_image} outside (0, 1]: a share of one image's pixels")
    check_tile("--tile", args.tile)
    ac.refuse_rounds(args)


def build_parser():
    p = hc.RefusingParser(_refusals, description="which regions of a split to label first: tile scores from a fused "
                                                 "head kernel, a ranking under a pixel budget, and the label tree an "
                                                 "annotator of those tiles would hand back")
    ac.add_source_flags(p, "share of the split's pixels that may be shown")
    p.add_argument("--tile", type=int, nargs=2, default=[32, 32], metavar=("TH", "TW"),
                   help="tile size in label pixels, each even and in [2, 256] (default %(default)s)")
    ac.add_criterion_flags(p, KINDS, CRITERIA, "the tile criterion")
    p.add_argument("--max-per-image", type=float, help="skip a tile once its image has this share of its pixels selected")
    ac.add_round_flags(p, "its tiles leave the ranking", "<stem>_uncertainty.png (q >> 8)")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
