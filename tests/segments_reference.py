"""Numpy reference of the segments add-on (include/mdil_segments.h): the root of every pixel's
connected component spelled twice -- the definition by flood fill, and vectorised min-propagation
with pointer jumping --, the size-binned counters and the despeckle filter by ``bincount`` over the
roots, and the maps the GPU cases are built from.  Integers throughout."""
import numpy as np

from tests.boundary_reference import blocky  # noqa: F401  (the cases draw their block maps with it)

COUNTERS = ("segments", "pixels", "hit_pixels", "covered", "missed", "unjudged", "bad_labels")
HALF = {4: ((0, 1), (1, 0)), 8: ((0, 1), (1, 0), (1, 1), (1, -1))}      # each neighbour pair once


def roots_flood(label, connectivity):
    """The definition, for small maps: a flood fill from every pixel not yet reached, in raster
    order, so that the pixel a fill starts from is the smallest index of its segment.
    u8 [H,W] -> i32 [H,W] of y*W + x of that pixel."""
    H, W = label.shape
    steps = [(dy, dx) for dy, dx in HALF[connectivity]] + [(-dy, -dx) for dy, dx in HALF[connectivity]]
    root = np.full((H, W), -1, dtype=np.int32)
    for y0 in range(H):
        for x0 in range(W):
            if root[y0, x0] >= 0:
                continue
            root[y0, x0] = y0 * W + x0
            todo = [(y0, x0)]
            while todo:
                y, x = todo.pop()
                for dy, dx in steps:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and root[yy, xx] < 0 and label[yy, xx] == label[y0, x0]:
                        root[yy, xx] = y0 * W + x0
                        todo.append((yy, xx))
    return root


def roots_propagate(label, connectivity):
    """r starts as every pixel's own index; a sweep gives both pixels of every same-label neighbour
    pair the smaller of their two values, then r = r[r] until that changes nothing (every value is
    the index of a pixel of the same segment, so it is a pointer); repeated to a fixed point, where r
    is constant on a segment, at most the segment's smallest index and the index of one of its pixels."""
    H, W = label.shape
    r = np.arange(H * W, dtype=np.int32).reshape(H, W)
    pairs = []
    for dy, dx in HALF[connectivity]:
        a = (slice(0, H - dy), slice(max(0, -dx), W - max(0, dx)))
        b = (slice(dy, H), slice(max(0, dx), W + min(0, dx)))
        pairs.append((a, b, label[a] == label[b]))
    while True:
        before = r.copy()
        for a, b, same in pairs:
            low = np.minimum(r[a], r[b])
            r[a] = np.where(same, low, r[a])
            r[b] = np.where(same, np.minimum(low, r[b]), r[b])     # a pixel of both views keeps the smaller
        flat = r.reshape(-1)
        while True:
            nxt = flat[flat]
            if np.array_equal(nxt, flat):
                break
            flat[:] = nxt
        if np.array_equal(before, r):
            return r


def label(maps, connectivity, fn=roots_propagate):
    """u8 [N,H,W] -> (root, area) i32 [N,H,W]: every image on its own; the area at the root pixel."""
    N, H, W = maps.shape
    root = np.stack([fn(m, connectivity) for m in maps]).astype(np.int32)
    area = np.stack([np.bincount(r.reshape(-1), minlength=H * W).reshape(H, W) for r in root]).astype(np.int32)
    return root, area


def n_segments(area):
    return int((area > 0).sum())


def bins(a, edges):
    """bin k holds edges[k-1] < a <= edges[k]; the last one a > edges[-1]."""
    return np.searchsorted(np.asarray(edges), np.asarray(a, dtype=np.int64), side="left")


def counters(maps, other, root, area, nc, map_ignore, other_ignore, edges, cover_num, cover_den):
    """-> ({the six [nc,nb] counters and bad_labels [1], int64, from zero}, hit, void i32 [N,H,W])."""
    N, H, W = maps.shape
    nb = len(edges) + 1
    key = (np.arange(N, dtype=np.int64)[:, None, None] * (H * W) + root).reshape(-1)
    m, o = maps.reshape(-1).astype(np.int64), other.reshape(-1).astype(np.int64)
    hit = np.bincount(key[o == m], minlength=N * H * W)
    void = np.bincount(key[o == other_ignore], minlength=N * H * W)
    at = np.nonzero(area.reshape(-1) > 0)[0]
    a, c, h, v = area.reshape(-1)[at].astype(np.int64), m[at], hit[at], void[at]
    j, k = a - v, bins(a, edges)
    seen = c != map_ignore
    bad = seen & (c >= nc)
    ok = seen & ~bad
    judged = ok & (j > 0)

    def hist(mask, weights=None):
        w = None if weights is None else weights[mask].astype(np.float64)
        return np.bincount(c[mask] * nb + k[mask], weights=w, minlength=nc * nb).astype(np.int64).reshape(nc, nb)

    out = {
        "segments": hist(judged),
        "pixels": hist(judged, j),
        "hit_pixels": hist(judged, h),
        "covered": hist(judged & (h * cover_den >= cover_num * j)),
        "missed": hist(judged & (h == 0)),
        "unjudged": hist(ok & (j == 0)),
        "bad_labels": np.array([a[bad].sum()], dtype=np.int64),
    }
    shape = (N, H, W)
    return out, hit.astype(np.int32).reshape(shape), void.astype(np.int32).reshape(shape)


def filter(maps, root, area, min_area, keep_id, fill):  # noqa: A001  (the header's name)
    """-> (out u8 [N,H,W], removed_segments i64 [256], removed_pixels i64 [256])."""
    N, H, W = maps.shape
    least = np.asarray(min_area, dtype=np.int64)
    size = np.stack([area[n].reshape(-1)[root[n].reshape(-1)].reshape(H, W) for n in range(N)]).astype(np.int64)
    drop = (maps != keep_id) & (size < least[maps])
    out = np.where(drop, np.uint8(fill), maps).astype(np.uint8)
    own = np.arange(H * W, dtype=np.int64).reshape(1, H, W)
    return (out, np.bincount(maps[drop & (root == own)], minlength=256).astype(np.int64),
            np.bincount(maps[drop], minlength=256).astype(np.int64))


# ------------------------------------------------------------------------------------- the maps
def spiral(n, w=None):
    """n x n (or n x w), label 1 on a one-pixel path that winds inwards from the top left corner,
    label 0 on the one-pixel path between its windings: two segments at either connectivity."""
    h, w = n, n if w is None else w
    a = np.zeros((h, w), dtype=np.uint8)
    y = x = 0
    dy, dx = 0, 1
    a[0, 0] = 1

    def inside(yy, xx):
        return 0 <= yy < h and 0 <= xx < w

    while True:
        for _ in range(2):                                  # straight on, else one turn to the right
            y1, x1, y2, x2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if inside(y1, x1) and a[y1, x1] == 0 and not (inside(y2, x2) and a[y2, x2] == 1):
                y, x = y1, x1
                a[y, x] = 1
                break
            dy, dx = dx, -dy
        else:
            return a


def comb(h, teeth):
    """h x (2 * teeth - 1): teeth of label 1 in the even columns that join only in the last row,
    gaps of label 0 between them: 1 + (teeth - 1) segments at either connectivity."""
    a = np.zeros((h, 2 * teeth - 1), dtype=np.uint8)
    a[:, ::2] = 1
    a[h - 1, :] = 1
    return a


def checkerboard(h, w):
    """Two labels: h * w segments at 4-connectivity, 2 at 8-connectivity."""
    return ((np.arange(h)[:, None] + np.arange(w)[None, :]) % 2).astype(np.uint8)


def diagonal():
    """5 x 8 of label 0 with two pixels of label 1 that touch by a corner down-right and two of
    label 2 that touch by a corner down-left: 5 segments at 4-connectivity, 3 at 8-connectivity."""
    a = np.zeros((5, 8), dtype=np.uint8)
    a[1, 1] = a[2, 2] = 1
    a[1, 6] = a[2, 5] = 2
    return a


def noise(shape, seed, n_labels=2):
    return np.random.default_rng(seed).integers(0, n_labels, shape, dtype=np.uint8)
