"""The rule of include/mdil_spx.h in int64 torch, for the CPU and GPU suites of the superpixel add-on: the
integer SLIC in two independent forms (``assign_loop``: a per-pixel loop in Python integers over the clipped
3 x 3 candidates; ``assign_fast``: nine shifted gathers whose winner is the minimum of D << 24 | k), the
per-superpixel table, the one-click annotator and the host helpers of mdil_ss_amd/superpixel.py."""
import numpy as np
import torch

FIELDS = 4
BIG = (1 << 62)


def emptied_image():
    """1 x 12, S = 4, m = 1: centre 1 starts on (100, 0, 0) at x = 6 and takes (0, 100, 0) at x = 5; after one update it
    sits on their mean (50, 50, 0) while centre 0 sits 1 away from the first and centre 2 54 away from the second: both
    leave, and centre 1 has no pixel."""
    img = torch.zeros(1, 3, 1, 12)
    img[0, 0, 0] = torch.tensor([101.0] * 5 + [0, 100, 0, 0, 0, 0, 0]) / 255.0
    img[0, 1, 0] = torch.tensor([0.0] * 5 + [100, 0, 130, 130, 130, 250, 130]) / 255.0
    return img


def quantise(image):
    """f32 [...] -> int64 colour codes.  The library's c8 = (uint32) fmaf(clamp(v), 255.0f, 0.5f) rounds v * 255 + 0.5
    ONCE to fp32.  Here the product and the sum are formed in fp64, where the product is exact (24 x 8 bits) and the
    sum is exact wherever it matters (it can round only where v * 255 < 2^-20 or so: there the sum lies within 2^-20
    of 0.5 and floors to 0 however it is rounded), so the single rounding to fp32 equals the fmaf."""
    v = image.to(torch.float32)
    v = torch.where(torch.isnan(v), torch.zeros_like(v), v).clamp(0.0, 1.0)
    return torch.floor((v.double() * 255.0 + 0.5).float()).long()


def grid(H, W, S):
    return -(-H // S), -(-W // S)


def init_centres(codes, S):
    """codes int64 [N,3,H,W] -> centres int64 [N,K,5]: 16 x (y, x, r, g, b) of each cell's start pixel."""
    N, _, H, W = codes.shape
    Gy, Gx = grid(H, W, S)
    ys = torch.clamp(torch.arange(Gy) * S + S // 2, max=H - 1)
    xs = torch.clamp(torch.arange(Gx) * S + S // 2, max=W - 1)
    yy, xx = ys[:, None].expand(Gy, Gx).reshape(-1), xs[None].expand(Gy, Gx).reshape(-1)
    col = codes[:, :, yy, xx].permute(0, 2, 1)                              # [N,K,3]
    pos = torch.stack([yy, xx], 1)[None].expand(N, -1, -1)
    return 16 * torch.cat([pos, col], 2)


def distance(S, m, y, x, r, g, b, c):
    """D of the header in Python integers; c = (Y, X, R, G, B)."""
    return S * S * ((16 * r - c[2]) ** 2 + (16 * g - c[3]) ** 2 + (16 * b - c[4]) ** 2) + \
        m * m * ((16 * y - c[0]) ** 2 + (16 * x - c[1]) ** 2)


def assign_loop(codes, centres, S, m):
    """Form 1: every pixel, its clipped 3 x 3 candidates in ascending k, a strict < (ties: the lowest k)."""
    N, _, H, W = codes.shape
    Gy, Gx = grid(H, W, S)
    cen, col = centres.tolist(), codes.tolist()
    out = torch.zeros(N, H, W, dtype=torch.int64)
    for n in range(N):
        for y in range(H):
            for x in range(W):
                best, bk = None, -1
                for gy in range(max(0, y // S - 1), min(Gy, y // S + 2)):
                    for gx in range(max(0, x // S - 1), min(Gx, x // S + 2)):
                        k = gy * Gx + gx
                        D = distance(S, m, y, x, col[n][0][y][x], col[n][1][y][x], col[n][2][y][x], cen[n][k])
                        if best is None or D < best:
                            best, bk = D, k
                out[n, y, x] = bk
    return out


def assign_fast(codes, centres, S, m):
    """Form 2: nine shifted gathers; the winner is the minimum of D << 24 | k (D < 2^39, k < 2^24)."""
    N, _, H, W = codes.shape
    Gy, Gx = grid(H, W, S)
    assert Gy * Gx < (1 << 24)
    y16 = (16 * torch.arange(H))[None, :, None].expand(N, H, W)
    x16 = (16 * torch.arange(W))[None, None, :].expand(N, H, W)
    hy, hx = (torch.arange(H) // S)[:, None].expand(H, W), (torch.arange(W) // S)[None].expand(H, W)
    best = torch.full((N, H, W), BIG, dtype=torch.int64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            gy, gx = hy + dy, hx + dx
            ok = (gy >= 0) & (gy < Gy) & (gx >= 0) & (gx < Gx)
            k = torch.where(ok, gy * Gx + gx, torch.zeros_like(gy))
            c = centres[:, k.reshape(-1)].reshape(N, H, W, 5)
            dc = sum((16 * codes[:, j] - c[..., 2 + j]) ** 2 for j in range(3))
            ds = (y16 - c[..., 0]) ** 2 + (x16 - c[..., 1]) ** 2
            D = S * S * dc + m * m * ds
            assert int(D.max()) < (1 << 39)
            best = torch.minimum(best, torch.where(ok[None], (D << 24) | k[None], torch.full_like(D, BIG)))
    return best & ((1 << 24) - 1)


def sums_of(codes, ids, K):
    """(n, sum y, sum x, sum r, sum g, sum b) per centre of an assignment: int64 [N,K,6]."""
    N, _, H, W = codes.shape
    yy = torch.arange(H)[None, :, None].expand(N, H, W)
    xx = torch.arange(W)[None, None, :].expand(N, H, W)
    vals = torch.stack([torch.ones_like(ids), yy, xx, codes[:, 0], codes[:, 1], codes[:, 2]], -1).reshape(-1, 6)
    flat = (torch.arange(N)[:, None, None] * K + ids).reshape(-1)
    return torch.zeros(N * K, 6, dtype=torch.int64).index_add_(0, flat, vals).reshape(N, K, 6)


def update(centres, sums):
    """(16 sum + n / 2) / n with floor divisions; a centre without pixels keeps its state."""
    n = sums[..., :1]
    new = (16 * sums[..., 1:] + n // 2) // n.clamp(min=1)
    return torch.where(n > 0, new, centres)


def slic(image, S, m, T, assign=assign_fast):
    """image f32 [N,3,H,W] -> (id [N,H,W], the centres the final assign read [N,K,5], its sums [N,K,6]), int64."""
    codes = quantise(image)
    Gy, Gx = grid(codes.shape[2], codes.shape[3], S)
    centres = init_centres(codes, S)
    for _ in range(T):
        centres = update(centres, sums_of(codes, assign(codes, centres, S, m), Gy * Gx))
    ids = assign(codes, centres, S, m)
    return ids, centres, sums_of(codes, ids, Gy * Gx)


def table_ref(label, q, ids, K, nc, target=None, ignore=-1):
    """-> {"table" [N,K,4+nc], "tcount" [N,K,nc], "bad_targets", "bad_ids"}; ``q`` int64, ``ids`` int64 (any values)."""
    N = label.shape[0]
    F = FIELDS + nc
    ok = (ids >= 0) & (ids < K)
    cell = (torch.arange(N)[:, None, None] * K + torch.where(ok, ids, torch.zeros_like(ids)))
    lab = label.long()
    table, tcount = torch.zeros(N * K * F, dtype=torch.int64), torch.zeros(N * K * nc, dtype=torch.int64)

    def add(dst, where, slot, value=None):
        idx = slot[where]
        dst.index_add_(0, idx, torch.ones_like(idx) if value is None else value[where])

    add(table, ok, cell * F)
    add(table, ok, cell * F + 1, q.long())
    inclass = ok & (lab < nc)
    add(table, inclass, cell * F + FIELDS + torch.where(inclass, lab, torch.zeros_like(lab)))
    res = {"bad_targets": 0, "bad_ids": int((~ok).sum())}
    if target is not None:
        t = target.long()
        valid = ok & (t < nc) & (t != ignore)
        add(table, valid, cell * F + 3)
        add(table, valid & (lab != t), cell * F + 2)
        add(tcount, valid, cell * nc + torch.where(valid, t, torch.zeros_like(t)))
        res["bad_targets"] = int((ok & (t >= nc) & (t != ignore)).sum())
    res.update(table=table.reshape(N, K, F), tcount=tcount.reshape(N, K, nc))
    return res


def apply_ref(ids, selected, nc, answer=None, target=None, previous=None, fill=None, label=None, ignore=-1, drop_id=255):
    """-> {"out", "mask" u8 [N,H,W], "shown", "annotated" [nc], "kept" [nc], "filled" [nc], "bad_targets",
    "wrong_shown", "wrong_all", "noisy", "bad_ids"}; ``selected`` / ``answer`` u8 [N,K], ``ids`` int64 (any values)."""
    N, K = selected.shape
    ok = (ids >= 0) & (ids < K)
    cell = (torch.arange(N)[:, None, None] * K + torch.where(ok, ids, torch.zeros_like(ids)))
    sel = ok & (selected.reshape(-1)[cell] == 255)
    out = torch.full(ids.shape, drop_id, dtype=torch.uint8)
    mask = torch.zeros(ids.shape, dtype=torch.uint8)
    if answer is not None:
        out[sel] = answer.reshape(-1)[cell][sel]
    elif target is not None:
        out[sel] = target[sel]
    mask[sel] = 255
    rest = ~sel
    kept = filled = torch.zeros_like(sel)
    if previous is not None:
        kept = rest & (previous != drop_id)
        out[kept], mask[kept] = previous[kept], 128
        rest = rest & ~kept
    if fill is not None:
        filled = rest & (fill != drop_id)
        out[filled], mask[filled] = fill[filled], 64

    def hist(v, but=-1):
        v = v.long()
        return torch.bincount(v[(v < nc) & (v != but)], minlength=nc)

    zero = torch.zeros(nc, dtype=torch.int64)
    res = {"out": out, "mask": mask, "shown": int(sel.sum()),
           "annotated": hist(out[sel], ignore) if answer is not None or target is not None else zero,
           "kept": hist(previous[kept]) if previous is not None else zero,
           "filled": hist(fill[filled]) if fill is not None else zero,
           "bad_targets": 0, "wrong_shown": 0, "wrong_all": 0, "noisy": 0, "bad_ids": int((~ok).sum())}
    if target is not None:
        t = target.long()
        valid = (t < nc) & (t != ignore)
        res["bad_targets"] = int((sel & (t >= nc) & (t != ignore)).sum())
        res["noisy"] = int((sel & valid & (out != target)).sum())
        if label is not None:
            wrong = valid & (label != target)
            res["wrong_shown"], res["wrong_all"] = int((wrong & sel).sum()), int(wrong.sum())
    return res


# ------------------------------------------------------------------------------- host helpers
def dominant(counts, empty):
    """Per row of int64 [rows, nc]: the class with the largest count, ties to the lowest class, ``empty`` where all are 0."""
    out = []
    for row in counts.tolist():
        best = max(row)
        out.append(row.index(best) if best > 0 else empty)
    return torch.tensor(out, dtype=torch.uint8)


def achievable_accuracy(tcount):
    rows = tcount.reshape(-1, tcount.shape[-1]).tolist()
    total = sum(sum(r) for r in rows)
    return sum(max(r) for r in rows) / total if total else 0.0


def edges(ids):
    """u8 [N,H,W]: 255 where the right or the lower neighbour belongs to another superpixel."""
    e = np.zeros(tuple(ids.shape), dtype=bool)
    a = ids.numpy()
    e[:, :, :-1] |= a[:, :, :-1] != a[:, :, 1:]
    e[:, :-1, :] |= a[:, :-1, :] != a[:, 1:, :]
    return torch.from_numpy(e.astype(np.uint8) * 255)
