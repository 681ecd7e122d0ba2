"""CPU reference of the acquisition add-on (include/mdil_acquire.h, mdil_ss_amd/acquire.py): the three
uncertainties in torch fp64, their 16-bit code, and everything after it in integers and Python floats --
the tile table by bincount, the five tile criteria, the ranking, the budget walk and the apply rule.
Written from the header and the module's docstring, not from their code."""
import math

import torch

Q_ONE = 65536
FIELDS = 4
KINDS = ("msp", "entropy", "margin")
CRITERIA = ("uncertainty", "impurity", "ripu", "random", "oracle")
M64 = (1 << 64) - 1


def q_of(u):
    """fp64 uncertainties -> int64 codes: min(65535, floor(max(u, 0) * 65536))."""
    return (u.double().clamp(min=0.0) * Q_ONE).floor().clamp(max=Q_ONE - 1).to(torch.int64)


def scores(logits, kind):
    """[N,nc,Hl,Wl] logits (any float type; evaluated in that type) -> the uncertainty ``kind`` [N,Hl,Wl]."""
    nc = logits.shape[1]
    logp = torch.log_softmax(logits, 1)
    p = logp.exp()
    if kind == "msp":
        return 1.0 - p.max(1)[0]
    if kind == "entropy":
        return -(p * logp).sum(1) / math.log(nc)
    top = p.topk(2, dim=1)[0]
    return 1.0 - (top[:, 0] - top[:, 1])


def valid_of(target, nc, ignore):
    t = target.long()
    return (t < nc) & (t != ignore)


def grid(size, tile):
    return -(-size[0] // tile[0]), -(-size[1] // tile[1])


def tile_index(shape, tile):
    """The flat tile index (n * Ty + ty) * Tx + tx of every pixel of maps [N,Hl,Wl]."""
    N, Hl, Wl = shape
    Ty, Tx = grid((Hl, Wl), tile)
    ty = torch.arange(Hl) // tile[0]
    tx = torch.arange(Wl) // tile[1]
    n = torch.arange(N)
    return (n[:, None, None] * Ty + ty[None, :, None]) * Tx + tx[None, None, :]


def tile_table(label, q, target, nc, ignore, tile, finite=None):
    """-> int64 [N,Ty,Tx,4+nc] from a label map, a q map (int64) and a target or None."""
    N, Hl, Wl = label.shape
    Ty, Tx = grid((Hl, Wl), tile)
    T = N * Ty * Tx
    idx = tile_index(label.shape, tile).reshape(-1)
    keep = torch.ones(idx.numel(), dtype=torch.bool) if finite is None else finite.reshape(-1)
    lab, qq = label.reshape(-1).long(), q.reshape(-1).long()
    table = torch.zeros(T, FIELDS + nc, dtype=torch.int64)
    table[:, 0] = torch.bincount(idx[keep], minlength=T)
    table[:, 1] = torch.bincount(idx[keep], weights=qq[keep].double(), minlength=T).round().to(torch.int64)
    if target is not None:
        ok = valid_of(target, nc, ignore).reshape(-1) & keep
        wrong = ok & (lab != target.reshape(-1).long())
        table[:, 2] = torch.bincount(idx[wrong], minlength=T)
        table[:, 3] = torch.bincount(idx[ok], minlength=T)
    table[:, FIELDS:] = torch.bincount(idx[keep] * nc + lab[keep], minlength=T * nc).reshape(T, nc)
    return table.reshape(N, Ty, Tx, FIELDS + nc)


def mix(seed, k):
    z = (seed + 0x9E3779B97F4A7C15 * k) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def tile_score(row, by, nc, seed=0, image=0, tile=0):
    """One tile's criterion from its table row (a list of ints), in Python floats."""
    cnt = row[0]
    if by == "random":
        return (mix(mix(seed & M64, image + 1), tile + 1) >> 11) / float(1 << 53)
    if cnt == 0:
        return 0.0
    U = row[1] / (Q_ONE * cnt)
    I = -sum(h / cnt * math.log(h / cnt) for h in row[FIELDS:] if h > 0) / math.log(nc)
    return {"uncertainty": U, "impurity": I, "ripu": U * I, "oracle": row[2] / cnt}[by]


def all_scores(table, by, seed=0):
    """[M,Ty,Tx,4+nc] -> a list of (score, image, ty, tx) over every tile."""
    M, Ty, Tx, width = table.shape
    nc = width - FIELDS
    rows = table.reshape(-1, width).tolist()
    return [(tile_score(rows[(i * Ty + y) * Tx + x], by, nc, seed, i, y * Tx + x), i, y, x)
            for i in range(M) for y in range(Ty) for x in range(Tx)]


def rank(scored, removed=()):
    """Score descending, ties by (image, ty, tx) ascending; tiles in ``removed`` and tiles without pixels left out
    by the caller.  -> [(image, ty, tx)]"""
    return [(i, y, x) for s, i, y, x in sorted(scored, key=lambda t: (-t[0], t[1], t[2], t[3])) if (i, y, x) not in removed]


def tile_pixels(size, tile, y, x):
    return (min(size[0], (y + 1) * tile[0]) - y * tile[0]) * (min(size[1], (x + 1) * tile[1]) - x * tile[1])


def select(order, size, tile, images, budget, max_per_image=None):
    """The budget walk -> (chosen [(image, ty, tx)], pixels shown)."""
    limit = budget * images * size[0] * size[1]
    spent, chosen, per = 0, [], {}
    for i, y, x in order:
        n = tile_pixels(size, tile, y, x)
        if max_per_image is not None and per.get(i, 0) + n > max_per_image * size[0] * size[1]:
            continue
        if spent + n > limit:
            break
        spent += n
        per[i] = per.get(i, 0) + n
        chosen.append((i, y, x))
    return chosen, spent


def apply_ref(selected, size, tile, nc, target=None, previous=None, fill=None, ignore=-1, drop=255):
    """-> dict(out, mask u8 [N,Hl,Wl]; shown, bad_targets ints; annotated, kept, filled int64 [nc])."""
    N = selected.shape[0]
    idx = tile_index((N,) + tuple(size), tile)
    sel = selected.reshape(-1)[idx] != 0
    out = torch.full(idx.shape, drop, dtype=torch.uint8)
    mask = torch.zeros(idx.shape, dtype=torch.uint8)
    zero = torch.zeros(nc, dtype=torch.int64)
    res = dict(shown=int(sel.sum()), bad_targets=0, annotated=zero.clone(), kept=zero.clone(), filled=zero.clone())
    free = ~sel
    if previous is not None:
        keep = free & (previous != drop)
        out[keep], mask[keep] = previous[keep], 128
        res["kept"] = torch.bincount(previous[keep & (previous < nc)].long(), minlength=nc)
        free = free & ~keep
    if fill is not None:
        take = free & (fill != drop)
        out[take], mask[take] = fill[take], 64
        res["filled"] = torch.bincount(fill[take & (fill < nc)].long(), minlength=nc)
    mask[sel] = 255
    if target is not None:
        out[sel] = target[sel]
        ok = sel & valid_of(target, nc, ignore)
        res["annotated"] = torch.bincount(target[ok].long(), minlength=nc)
        res["bad_targets"] = int((sel & (target.long() >= nc) & (target.long() != ignore)).sum())
    res.update(out=out, mask=mask)
    return res
