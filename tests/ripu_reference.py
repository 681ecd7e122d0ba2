"""The reference of the sliding-region acquisition add-on, written from include/mdil_ripu.h and not from the
kernels: int64 box sums by 2-D cumsum with clipped corners, the five keys in Python integers, the greedy pick as a
plain loop, and the apply rule.  Everything is exact: the tests compare with ``torch.equal``."""
import math

import torch

CRITERIA = ("uncertainty", "impurity", "ripu", "oracle", "random")
STOP_EMPTY, STOP_BUDGET, STOP_PICKS = 0, 1, 2
M64 = (1 << 64) - 1
KEY_MAX = (1 << 32) - 1


def tlog(k):
    """round(h ln h * 2^14) for h = 0 .. (2k+1)^2, as Python ints; 0 for h = 0 and 1."""
    return [0, 0] + [int(round(h * math.log(h) * 16384.0)) for h in range(2, (2 * k + 1) ** 2 + 1)]


def mix(seed, j):
    z = (seed + 0x9E3779B97F4A7C15 * j) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def box_sums(v, k):
    """v int64 [N,H,W] -> the sum of v over the clipped (2k+1)^2 window of every pixel, by 2-D cumsum."""
    N, H, W = v.shape
    c = torch.zeros(N, H + 1, W + 1, dtype=torch.int64)
    c[:, 1:, 1:] = v.cumsum(1).cumsum(2)
    y, x = torch.arange(H), torch.arange(W)
    y0, y1 = (y - k).clamp(min=0), (y + k + 1).clamp(max=H)
    x0, x1 = (x - k).clamp(min=0), (x + k + 1).clamp(max=W)
    return c[:, y1][:, :, x1] - c[:, y0][:, :, x1] - c[:, y1][:, :, x0] + c[:, y0][:, :, x0]


def box_sums_brute(v, k):
    """The same by a loop over every pixel's window: for small maps."""
    N, H, W = v.shape
    out = torch.zeros_like(v)
    for y in range(H):
        for x in range(W):
            out[:, y, x] = v[:, max(0, y - k):y + k + 1, max(0, x - k):x + k + 1].sum((1, 2))
    return out


def window_counts(label, k, nc):
    """-> (cnt int64 [N,H,W], h int64 [nc,N,H,W])"""
    lab = label.long()
    cnt = box_sums(torch.ones_like(lab), k)
    return cnt, torch.stack([box_sums((lab == c).long(), k) for c in range(nc)])


def wrong_map(label, target, nc, ignore):
    t = target.long()
    return ((t < nc) & (t != ignore) & (label.long() != t)).long()


def keys(label, k, nc, by, q=None, target=None, ignore=-1, taken=None, table=None, seed=0, image0=0):
    """label u8 [N,H,W], q int64 [N,H,W] -> the keys as int64 [N,H,W], computed in Python integers."""
    N, H, W = label.shape
    cnt, h = window_counts(label, k, nc)
    table = tlog(k) if table is None else table
    sq = box_sums(q.long(), k) if q is not None else None
    wr = box_sums(wrong_map(label, target, nc, ignore), k) if target is not None else None
    out = torch.zeros(N, H, W, dtype=torch.int64)
    for n in range(N):
        s = mix(seed & M64, image0 + n + 1)
        for y in range(H):
            for x in range(W):
                if taken is not None and int(taken[n, y, x]):
                    continue
                c = int(cnt[n, y, x])
                if by in ("impurity", "ripu"):
                    E = max(0, table[c] - sum(table[int(h[j, n, y, x])] for j in range(nc)))
                if by == "uncertainty":
                    v = (int(sq[n, y, x]) << 16) // c
                elif by == "impurity":
                    v = (E << 16) // c
                elif by == "ripu":
                    v = (int(sq[n, y, x]) * E) // (c * c)
                elif by == "oracle":
                    v = (int(wr[n, y, x]) << 32) // (c + 1)
                else:
                    v = max(1, mix(s, y * W + x + 1) >> 32)
                out[n, y, x] = min(v, KEY_MAX)
    return out


def keys_fast(label, k, nc, by, q=None, target=None, ignore=-1, taken=None, seed=0, image0=0):
    """``keys`` in int64 tensor arithmetic for the larger test maps (every intermediate is below 2^63 for tlog(k));
    "random" goes through ``keys``."""
    if by == "random":
        return keys(label, k, nc, by, taken=taken, seed=seed, image0=image0)
    cnt, h = window_counts(label, k, nc)
    t = torch.tensor(tlog(k), dtype=torch.int64)
    E = (t[cnt] - t[h].sum(0)).clamp(min=0)
    if by == "uncertainty":
        v = (box_sums(q.long(), k) << 16) // cnt
    elif by == "impurity":
        v = (E << 16) // cnt
    elif by == "ripu":
        v = (box_sums(q.long(), k) * E) // (cnt * cnt)
    else:
        v = (box_sums(wrong_map(label, target, nc, ignore), k) << 32) // (cnt + 1)
    v = v.clamp(max=KEY_MAX)
    return torch.where(taken != 0, torch.zeros_like(v), v) if taken is not None else v


def select(key, taken, r, budget, max_picks):
    """key int64 [N,H,W], taken u8 [N,H,W] -> (taken after, picks: per image a list of (y, x, key, fresh), shown
    [N], stop [N]) by the header's loop."""
    N, H, W = key.shape
    taken = taken.clone()
    picks, shown, stop = [], [], []
    for n in range(N):
        mine, sh, why = [], 0, STOP_PICKS
        while len(mine) < max_picks:
            free = taken[n] == 0
            if not bool(free.any()):
                why = STOP_EMPTY
                break
            cand = torch.where(free, key[n], torch.full_like(key[n], -1)).reshape(-1)
            best = int(cand.max())
            if best <= 0:
                why = STOP_EMPTY
                break
            idx = int((cand == best).nonzero()[0])                    # the lowest y * W + x
            y, x = divmod(idx, W)
            region = taken[n, max(0, y - r):y + r + 1, max(0, x - r):x + r + 1]
            fresh = int((region == 0).sum())
            if sh + fresh > budget:
                why = STOP_BUDGET
                break
            region[region == 0] = 255
            sh += fresh
            mine.append((y, x, best, fresh))
        picks.append(mine)
        shown.append(sh)
        stop.append(why)
    return taken, picks, shown, stop


def apply_ref(selected, nc, target=None, previous=None, fill=None, label=None, ignore=-1, drop_id=255):
    """-> {"out", "mask" u8 [N,H,W], "shown", "annotated" [nc], "kept" [nc], "filled" [nc], "bad_targets",
    "wrong_shown", "wrong_all"}"""
    sel = selected == 255
    drop = torch.full_like(selected, drop_id)
    out, mask = drop.clone(), torch.zeros_like(selected)
    rest = ~sel
    out[sel] = target[sel] if target is not None else drop[sel]
    mask[sel] = 255
    kept = filled = torch.zeros_like(sel)
    if previous is not None:
        kept = rest & (previous != drop_id)
        out[kept], mask[kept] = previous[kept], 128
        rest = rest & ~kept
    if fill is not None:
        filled = rest & (fill != drop_id)
        out[filled], mask[filled] = fill[filled], 64

    def hist(v):
        v = v.long()
        return torch.bincount(v[v < nc], minlength=nc)

    res = {"out": out, "mask": mask, "shown": int(sel.sum()), "annotated": torch.zeros(nc, dtype=torch.int64),
           "kept": hist(previous[kept]) if previous is not None else torch.zeros(nc, dtype=torch.int64),
           "filled": hist(fill[filled]) if fill is not None else torch.zeros(nc, dtype=torch.int64),
           "bad_targets": 0, "wrong_shown": 0, "wrong_all": 0}
    if target is not None:
        t = target[sel].long()
        res["annotated"] = torch.bincount(t[(t < nc) & (t != ignore)], minlength=nc)
        res["bad_targets"] = int(((t >= nc) & (t != ignore)).sum())
        if label is not None:
            wrong = wrong_map(label, target, nc, ignore).bool()
            res["wrong_shown"], res["wrong_all"] = int((wrong & sel).sum()), int(wrong.sum())
    return res
