"""Numpy reference of the boundary add-on (include/mdil_boundary.h): the distance of every pixel
of a label map to the contour of its own region, spelled twice and independently of the kernel's
separable form, and the six counters from a pair of distance maps.  Integers throughout."""
import numpy as np

COUNTERS = ("target_hist", "pred_hist", "both_hist", "confusion", "bad_targets", "bad_preds")


def distance_brute(label, cap):
    """The definition, pixel by pixel, for small maps: the smallest k whose (2k+1)^2 window around p
    leaves the image or holds another label.  u8 [H,W] -> u8 [H,W] of min(d, cap + 1)."""
    H, W = label.shape
    out = np.empty((H, W), dtype=np.uint8)
    for y in range(H):
        for x in range(W):
            d = cap + 1
            for k in range(1, cap + 1):
                if y - k < 0 or x - k < 0 or y + k >= H or x + k >= W or \
                        (label[y - k:y + k + 1, x - k:x + k + 1] != label[y, x]).any():
                    d = k
                    break
            out[y, x] = d
    return out


def distance_erode(label, cap):
    """The label-agnostic erosion: E_0 is everything; E_k[p] holds iff all 8 neighbours of p are
    inside the image, in E_{k-1} and carry p's label (E_k is a subset of E_{k-1}, so p itself need
    not be asked).  d = the first k with not E_k.  u8 [H,W] -> u8 [H,W] of min(d, cap + 1)."""
    H, W = label.shape
    lab = np.full((H + 2, W + 2), -1, dtype=np.int32)
    lab[1:-1, 1:-1] = label
    same = {(dy, dx): lab[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx] == label
            for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)}
    inside = np.ones((H, W), dtype=bool)
    d = np.full((H, W), cap + 1, dtype=np.int32)
    for k in range(1, cap + 1):
        padded = np.zeros((H + 2, W + 2), dtype=bool)
        padded[1:-1, 1:-1] = inside
        nxt = inside.copy()
        for (dy, dx), eq in same.items():
            nxt &= eq & padded[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]
        d[inside & ~nxt] = k
        inside = nxt
        if not inside.any():
            break
    return d.astype(np.uint8)


def distances(maps, cap, fn=distance_erode):
    """u8 [N,H,W] -> u8 [N,H,W]: every image on its own."""
    return np.stack([fn(m, cap) for m in maps])


def bins(d, widths):
    """bin k holds widths[k-1] < d <= widths[k]; the last one d > widths[-1]."""
    return np.searchsorted(np.asarray(widths), d.astype(np.int64), side="left")


def counters(pred, target, dist_pred, dist_target, nc, widths, ignore_index):
    """The six int64 counters of one call, from zero."""
    nb = len(widths) + 1
    g, q = target.reshape(-1).astype(np.int64), pred.reshape(-1).astype(np.int64)
    kt, kp = bins(dist_target.reshape(-1), widths), bins(dist_pred.reshape(-1), widths)
    kb = bins(np.maximum(dist_target, dist_pred).reshape(-1), widths)
    seen = g != ignore_index
    bad_t = seen & (g >= nc)
    bad_p = seen & ~bad_t & (q >= nc)
    ok = seen & ~bad_t & ~bad_p
    eq = ok & (g == q)

    def hist(idx, size):
        return np.bincount(idx, minlength=size).astype(np.int64)

    return {
        "target_hist": hist(g[ok] * nb + kt[ok], nc * nb).reshape(nc, nb),
        "pred_hist": hist(q[ok] * nb + kp[ok], nc * nb).reshape(nc, nb),
        "both_hist": hist(g[eq] * nb + kb[eq], nc * nb).reshape(nc, nb),
        "confusion": hist((kt[ok] * nc + g[ok]) * nc + q[ok], nb * nc * nc).reshape(nb, nc, nc),
        "bad_targets": np.array([bad_t.sum()], dtype=np.int64),
        "bad_preds": np.array([bad_p.sum()], dtype=np.int64),
    }


def blocky(shape, n_labels, seed, block=5):
    """u8 map of random labels in blocks of about ``block`` pixels, cropped to ``shape`` ([H,W] or [N,H,W])."""
    rng = np.random.default_rng(seed)
    *lead, H, W = shape
    small = rng.integers(0, n_labels, (*lead, H // block + 1, W // block + 1), dtype=np.uint8)
    return np.ascontiguousarray(small.repeat(block, axis=-2).repeat(block, axis=-1)[..., :H, :W])
