"""numpy reference of the significance add-on (include/mdil_signif.h), the definition spelled twice:

  gather-and-add      the draws of all replicates hashed at once in uint64 arrays, the drawn rows
                      gathered and added in int64 (``resample``, ``replicate_gather``);
  multiplicities      the hash one counter at a time in Python integers, how often each image was
                      drawn (kept, left out, exchanged), and that many times its row, in Python
                      integers of any size (``replicate_multiplicity``).

``counts`` is the per-image table by bincount, ``score`` the iouEval rule with the mean added in class
order, ``report`` the report of ``mdil_ss_amd.significance`` from label maps: the replicates by this
file, the host arithmetic on them (``significance.build_report``: quantiles, BCa, p-values) by the
module's own float64 function, which tests/test_signif_cpu.py checks on its own."""
import numpy as np

MASK = (1 << 64) - 1
GOLDEN, MUL1, MUL2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
BOOTSTRAP, JACKKNIFE, SWAP = "bootstrap", "jackknife", "swap"


def splitmix(seed, b, j):
    """The hash of counter K = (b << 32) + j + 1 in Python integers."""
    z = (seed + GOLDEN * ((b << 32) + j + 1)) & MASK
    z ^= z >> 30
    z = (z * MUL1) & MASK
    z ^= z >> 27
    z = (z * MUL2) & MASK
    return z ^ (z >> 31)


def hashes(seed, first, B, M):
    """uint64 [B,M]: the same hash for b = first .. first + B - 1 and j < M (uint64 arrays wrap)."""
    b = np.arange(first, first + B, dtype=np.uint64)[:, None]
    j = np.arange(M, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.uint64(GOLDEN) * ((b << np.uint64(32)) + j + np.uint64(1))
        z ^= z >> np.uint64(30)
        z *= np.uint64(MUL1)
        z ^= z >> np.uint64(27)
        z *= np.uint64(MUL2)
        z ^= z >> np.uint64(31)
    return z


def draws(seed, first, B, M):
    """int64 [B,M]: the rows a bootstrap replicate adds."""
    return (((hashes(seed, first, B, M) >> np.uint64(32)) * np.uint64(M)) >> np.uint64(32)).astype(np.int64)


def bits(seed, first, B, M):
    """int64 [B,M]: 1 where a swap replicate exchanges the image's two predictors."""
    return (hashes(seed, first, B, M) >> np.uint64(63)).astype(np.int64)


def counts(pred, target, nc, ignore_index):
    """u8 [N,H,W] maps -> (int64 [N,3,nc]: tp, predicted, labelled; bad targets; unpredicted pixels)."""
    pred, target = np.asarray(pred), np.asarray(target)
    table = np.zeros((pred.shape[0], 3, nc), dtype=np.int64)
    bad = unpredicted = 0
    for n in range(pred.shape[0]):
        t, p = target[n].reshape(-1).astype(np.int64), pred[n].reshape(-1).astype(np.int64)
        seen = t != ignore_index
        bad += int((seen & (t >= nc)).sum())
        seen &= t < nc
        t, p = t[seen], p[seen]
        unpredicted += int((p >= nc).sum())
        table[n, 0] = np.bincount(t[p == t], minlength=nc)
        table[n, 1] = np.bincount(p[p < nc], minlength=nc)
        table[n, 2] = np.bincount(t, minlength=nc)
    return table, bad, unpredicted


def resample(table, mode, B, seed, first=0):
    """Gather-and-add: int64 [B,G,3,nc], the replicates first .. first + B - 1 of ``table`` [M,G,3,nc]."""
    table = np.asarray(table, dtype=np.int64)
    M, G = table.shape[:2]
    if mode == BOOTSTRAP:
        return table[draws(seed, first, B, M)].sum(1)
    if mode == JACKKNIFE:
        assert first + B <= M
        return table.sum(0)[None] - table[first:first + B]
    assert mode == SWAP and G == 2
    bit = bits(seed, first, B, M)                                       # [B,M]
    both = np.stack([table, table[:, ::-1]])                            # [2,M,G,3,nc]: as counted, exchanged
    return both[bit, np.arange(M)[None, :]].sum(1)


def replicate_gather(table, mode, b, seed):
    return resample(table, mode, 1, seed, first=b)[0]


def replicate_multiplicity(table, mode, b, seed):
    """The replicate ``b`` as nested lists [G][3][nc] of Python integers: how often every image
    enters, times its row."""
    table = np.asarray(table)
    M, G = table.shape[:2]
    rows = [[[[int(v) for v in plane] for plane in group] for group in image] for image in table.tolist()]
    weight = [[[0] * M for _ in range(G)] for _ in range(G)]            # weight[g][h][i]: of counts[i][h] in sums[g]
    for i in range(M):
        for g in range(G):
            if mode == BOOTSTRAP:
                weight[g][g][((splitmix(seed, b, i) >> 32) * M) >> 32] += 1
            elif mode == JACKKNIFE:
                weight[g][g][i] = 0 if i == b else 1
            else:
                weight[g][g ^ (splitmix(seed, b, i) >> 63)][i] += 1
    return [[[sum(weight[g][h][i] * rows[i][h][p][c] for h in range(G) for i in range(M))
              for c in range(len(rows[0][0][0]))] for p in range(3)] for g in range(G)]


def scored_classes(nc, ignore_index):
    assert ignore_index == nc - 1 or not 0 <= ignore_index < nc
    return nc - 1 if ignore_index == nc - 1 else nc


def score(sums, nc, ignore_index):
    """int [...,3,nc] -> (miou [...], iou [...,k], empty [...]) by the iouEval rule in float64: the
    denominator added left to right, the mean added in class order and divided by k."""
    k = scored_classes(nc, ignore_index)
    s = np.asarray(sums, dtype=np.int64)
    tp, pr, lb = s[..., 0, :].astype(np.float64), s[..., 1, :].astype(np.float64), s[..., 2, :].astype(np.float64)
    den = tp + (pr - tp)
    den = den + (lb - tp)
    den = den + 1e-15
    iou = (tp / den)[..., :k]
    total = iou[..., 0].copy()
    for c in range(1, k):
        total = total + iou[..., c]
    empty = np.zeros(s.shape[:-2], dtype=np.int64)
    for c in range(nc):
        empty |= ((s[..., 1, c] + s[..., 2, c]) == 0).astype(np.int64) << c
    return total / float(k), iou, empty


def replicates(table, nc, ignore_index, mode, B, seed, first=0):
    """-> {"sums", "miou", "iou", "empty"} of the replicates, as the library returns them."""
    sums = resample(table, mode, B, seed, first)
    miou, iou, empty = score(sums, nc, ignore_index)
    return {"sums": sums, "miou": miou, "iou": iou, "empty": empty}


def report(preds, target, nc, ignore_index, stems, replicates_n=10000, seed=0, level=0.95, influence=10):
    """The report of ``SignificanceMeter`` from u8 [M,H,W] label maps (``preds``: one or two of them)."""
    from mdil_ss_amd import significance as S
    table = np.stack([counts(p, target, nc, ignore_index)[0] for p in preds], axis=1)
    boot = replicates(table, nc, ignore_index, BOOTSTRAP, replicates_n, seed)
    jack = replicates(table, nc, ignore_index, JACKKNIFE, table.shape[0], seed)
    swap = replicates(table, nc, ignore_index, SWAP, replicates_n, seed) if len(preds) == 2 else None
    out = S.build_report(table.sum(0), boot, jack, swap, nc, ignore_index, list(stems), level=level,
                         influence=influence, seed=seed)
    out["unpredicted_pixels"] = sum(counts(p, target, nc, ignore_index)[2] for p in preds)
    return out


def synthetic_tables(rng, images, nc, pixels=400, concentration=1.5):
    """int64 [images,1,3,nc]: i.i.d. images.  An image draws its own class mix (Dirichlet) and its own
    accuracy (Beta(8, 3)); its pixels are labelled by the mix, predicted right with the accuracy and
    otherwise as one of the other classes, uniformly."""
    mix = rng.dirichlet(np.full(nc, concentration), size=images)
    labelled = rng.multinomial(pixels, mix)
    right = rng.binomial(labelled, rng.beta(8.0, 3.0, size=(images, 1)))
    astray = rng.multinomial(labelled - right, np.full(nc - 1, 1.0 / (nc - 1)))      # [images,nc,nc-1]
    predicted = right.copy()
    for t in range(nc):
        others = [c for c in range(nc) if c != t]
        predicted[:, others] += astray[:, t, :]
    return np.stack([right, predicted, labelled], axis=1)[:, None].astype(np.int64)
