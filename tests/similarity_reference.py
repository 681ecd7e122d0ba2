"""fp64 checker of the similarity add-on (include/mdil_similarity.h, mdil_ss_amd/similarity.py): the
moments by their definition, and every metric straight from the data rows -- centred matrices,
per-class means -- never from the moments."""
import numpy as np


def pivoted(x, pivot, dtype=np.float32):
    """w = fl32(x - pivot): the subtraction is part of the library's contract.  (``dtype`` float64:
    rows that are no fp32 data, for checks of the host algebra alone.)"""
    return (np.asarray(x, dtype=dtype) - np.asarray(pivot, dtype=dtype)[None, :]).astype(dtype)


def moments(x, y, labels, nc, pivot_x, pivot_y=None, dtype=np.float32):
    """The moments dict ``similarity.MomentMeter.moments`` returns, by definition, in fp64.  ``y``
    and ``pivot_y`` None: one population.  ``labels`` None: every row in class 0."""
    x = np.asarray(x, dtype=dtype)
    rows, cx = x.shape
    lab = np.zeros(rows, dtype=np.int64) if labels is None else np.asarray(labels).astype(np.int64)
    keep = lab < nc
    wx = pivoted(x, pivot_x, dtype).astype(np.float64)[keep]
    cy = 0 if y is None else np.asarray(y).shape[1]
    wy = pivoted(y, pivot_y, dtype).astype(np.float64)[keep] if cy else np.zeros((int(keep.sum()), 0))
    onehot = np.zeros((int(keep.sum()), nc))
    onehot[np.arange(int(keep.sum())), lab[keep]] = 1.0
    return {"cx": cx, "cy": cy, "nc": nc, "n": onehot.sum(0), "skipped": float((~keep).sum()),
            "sx": onehot.T @ wx, "sy": onehot.T @ wy, "gxx": wx.T @ wx, "gyy": wy.T @ wy, "gxy": wx.T @ wy,
            "pivot_x": np.asarray(pivot_x, dtype=dtype).astype(np.float64),
            "pivot_y": np.zeros(0) if not cy else np.asarray(pivot_y, dtype=dtype).astype(np.float64)}


def absolute_moments(x, y, labels, nc, pivot_x, pivot_y=None):
    """The same sums over |w| and |w_a| |w_b|: what a rounding bound is a multiple of."""
    x = np.asarray(x, dtype=np.float32)
    lab = np.zeros(len(x), dtype=np.int64) if labels is None else np.asarray(labels).astype(np.int64)
    keep = lab < nc
    wx = np.abs(pivoted(x, pivot_x).astype(np.float64))[keep]
    wy = np.abs(pivoted(y, pivot_y).astype(np.float64))[keep] if y is not None else np.zeros((int(keep.sum()), 0))
    onehot = np.zeros((int(keep.sum()), nc))
    onehot[np.arange(int(keep.sum())), lab[keep]] = 1.0
    return {"sx": onehot.T @ wx, "sy": onehot.T @ wy, "gxx": wx.T @ wx, "gyy": wy.T @ wy, "gxy": wx.T @ wy}


def pack(m):
    """The flat fp64 state in the header's order."""
    return np.concatenate([np.ravel(m["n"]), [m["skipped"]], np.ravel(m["sx"]), np.ravel(m["sy"]), np.ravel(m["gxx"]),
                           np.ravel(m["gyy"]), np.ravel(m["gxy"])]).astype(np.float64)


# --------------------------------------------------------------------- the metrics from the rows
def kept(x, labels, nc):
    """The rows that are counted, in fp64, and their labels."""
    x = np.asarray(x, dtype=np.float64)
    if labels is None:
        return x, np.zeros(len(x), dtype=np.int64)
    lab = np.asarray(labels).astype(np.int64)
    return x[lab < nc], lab[lab < nc]


def mean_cov(x):
    x = np.asarray(x, dtype=np.float64)
    mu = x.mean(0)
    d = x - mu
    return mu, d.T @ d / len(x)


def linear_cka(x, y):
    dx, dy = x - x.mean(0), y - y.mean(0)
    n = len(x)
    return float(np.linalg.norm(dx.T @ dy / n) ** 2 / (np.linalg.norm(dx.T @ dx / n) * np.linalg.norm(dy.T @ dy / n)))


def sqrtm_psd(S):
    w, V = np.linalg.eigh((S + S.T) / 2)
    return (V * np.sqrt(np.clip(w, 0, None))) @ V.T


def frechet(xa, xb):
    (ma, Sa), (mb, Sb) = mean_cov(xa), mean_cov(xb)
    ra = sqrtm_psd(Sa)
    w = np.linalg.eigvalsh(ra @ Sb @ ra)
    return float(((ma - mb) ** 2).sum() + np.trace(Sa) + np.trace(Sb) - 2 * np.sqrt(np.clip(w, 0, None)).sum())


def scatters(x, lab):
    """-> (tr S_b, tr S_w) with the per-class means taken from the rows."""
    mu = x.mean(0)
    tr_b = tr_w = 0.0
    for c in np.unique(lab):
        xc = x[lab == c]
        mc = xc.mean(0)
        tr_b += len(xc) * ((mc - mu) ** 2).sum()
        tr_w += ((xc - mc) ** 2).sum()
    return float(tr_b), float(tr_w)


def separability(x, lab):
    tr_b, tr_w = scatters(x, lab)
    return tr_b / tr_w


def class_shift(x, y, lab):
    """-> (classes, |mu_x,c - mu_y,c|, the same over sqrt(tr S_w(x) / N))."""
    classes = [int(c) for c in np.unique(lab)]
    shift = np.array([np.linalg.norm(x[lab == c].mean(0) - y[lab == c].mean(0)) for c in classes])
    sigma = np.sqrt(scatters(x, lab)[1] / len(x))
    return classes, shift, shift / sigma
