"""The density add-on said in plain numpy / torch fp64, for tests/test_density_cpu.py and
tests/test_density_gpu.py: the scores of include/mdil_density.h evaluated in fp64 from the fp32 model
buffer and fl32(x - pivot), the same in plain float32 torch, the first-order rounding bound per row,
the fit from rows directly, and a seeded clustered case.  Nothing here imports the package."""
import numpy as np
import torch

U = 2.0 ** -24
KINDS = ("maha", "rmaha")
NO_CLASS = 255


def gamma(k):
    return k * U / (1 - k * U)


def model_floats(C, K):
    return 2 * C + 2 * C * C + K * C


def parts(buffer, C, K):
    """The fp32 buffer pivot [C] | A [C][C] | A0 [C][C] | m0 [C] | m [K][C] -> float32 tensors."""
    b = torch.as_tensor(np.asarray(buffer, dtype=np.float32))
    assert b.numel() == model_floats(C, K)
    cuts = np.cumsum([C, C * C, C * C, C])
    pivot, A, A0, m0, m = b[:cuts[0]], b[cuts[0]:cuts[1]], b[cuts[1]:cuts[2]], b[cuts[2]:cuts[3]], b[cuts[3]:]
    return pivot, A.reshape(C, C).tril(), A0.reshape(C, C).tril(), m0, m.reshape(K, C)


def scores64(x, model):
    """x float32 [rows, C] -> dict of fp64 tensors: ``d`` [rows, K], ``d0``, ``maha``, ``rmaha`` [rows], the argmin
    ``k`` (ties to the lowest k), ``nearest`` = cls[k], the gap between the two smallest distances, and the
    rounding bounds ``tol_maha``, ``tol_rmaha`` [rows]:
        S_i = sum_j |A_ij| |w_j|,  b_k = gamma(C+2) d_k + 2 gamma(C+1) sum_i |z_i - m_k,i| S_i, b0 likewise
        tol_maha = 2 max_k b_k,  tol_rmaha = 2 (max_k b_k + b0) + 2^-23 |rmaha|"""
    C, cls = int(model["C"]), torch.as_tensor(np.asarray(model["cls"])).long()
    K = cls.numel()
    pivot, A, A0, m0, m = parts(model["buffer"], C, K)
    w = (x.reshape(-1, C).float() - pivot).double()                   # fl32(x - pivot), then exact
    A, A0, m0, m = A.double(), A0.double(), m0.double(), m.double()
    z, z0 = w @ A.T, w @ A0.T
    S, S0 = w.abs() @ A.abs().T, w.abs() @ A0.abs().T
    d = torch.empty(w.shape[0], K, dtype=torch.float64)
    b = torch.empty_like(d)
    for k in range(K):
        diff = z - m[k]
        d[:, k] = (diff * diff).sum(1)
        b[:, k] = gamma(C + 2) * d[:, k] + 2 * gamma(C + 1) * (diff.abs() * S).sum(1)
    diff0 = z0 - m0
    d0 = (diff0 * diff0).sum(1)
    b0 = gamma(C + 2) * d0 + 2 * gamma(C + 1) * (diff0.abs() * S0).sum(1)
    dmin, k = d.min(1)
    k = (d == dmin[:, None]).long().argmax(1)                       # the lowest k of a tie
    gap = torch.full_like(dmin, float("inf"))
    if K > 1:
        two = d.topk(2, dim=1, largest=False)[0]
        gap = two[:, 1] - two[:, 0]
    rmaha = dmin - d0
    bmax = b.max(1)[0]
    return {"d": d, "d0": d0, "maha": dmin, "rmaha": rmaha, "k": k, "nearest": cls[k], "gap": gap,
            "tol_maha": 2 * bmax, "tol_rmaha": 2 * (bmax + b0) + 2.0 ** -23 * rmaha.abs()}


def scores32(x, model):
    """The plain float32 torch evaluation: ``@``, broadcast difference, ``sum``, ``min`` -> (maha, rmaha)."""
    C, K = int(model["C"]), len(model["cls"])
    pivot, A, A0, m0, m = parts(model["buffer"], C, K)
    w = x.reshape(-1, C).float() - pivot
    z, z0 = w @ A.T, w @ A0.T
    d = torch.stack([((z - m[k]) ** 2).sum(1) for k in range(K)], 1)
    d0 = ((z0 - m0) ** 2).sum(1)
    dmin = d.min(1)[0]
    return dmin + 0.0, (dmin - d0) + 0.0


def fit(x, labels, classes, ridge=1e-4, min_rows=None, pivot=None):
    """The fit from rows directly, in fp64: x [rows, C], labels [rows]; rows with a label >= ``classes`` are
    left out.  -> the dict ``density.fit_model`` gives (means, covariances, cls, dropped, counts, the fp32 buffer)."""
    x = np.asarray(x, dtype=np.float64)
    lab = np.asarray(labels).reshape(-1)
    C = x.shape[1]
    min_rows = 2 * C if min_rows is None else min_rows
    used = lab < classes
    x, lab = x[used], lab[used]
    rows = len(x)
    counts = np.bincount(lab, minlength=classes)
    present = [k for k in range(classes) if counts[k] > 0]
    keep = [k for k in range(classes) if counts[k] >= min_rows]
    mu = {k: x[lab == k].mean(0) for k in present}
    S_w = np.zeros((C, C))
    for k in present:
        c = x[lab == k] - mu[k]
        S_w += c.T @ c
    within = S_w / (rows - len(present))
    within = within + ridge * np.trace(within) / C * np.eye(C)
    mt = x.mean(0)
    c = x - mt
    total = c.T @ c / (rows - 1)
    total = total + ridge * np.trace(total) / C * np.eye(C)
    pivot = np.zeros(C) if pivot is None else np.asarray(pivot, dtype=np.float32).astype(np.float64)
    A = np.tril(np.linalg.inv(np.linalg.cholesky(within)))
    A0 = np.tril(np.linalg.inv(np.linalg.cholesky(total)))
    means = np.stack([mu[k] for k in keep])
    m = (means - pivot) @ A.T
    m0 = A0 @ (mt - pivot)
    buffer = np.concatenate([pivot, A.reshape(-1), A0.reshape(-1), m0, m.reshape(-1)]).astype(np.float32)
    return {"C": C, "cls": np.asarray(keep, dtype=np.uint8), "dropped": np.asarray([k for k in range(classes) if k not in keep]),
            "counts": counts, "means": means, "mean_total": mt, "cov_within": within, "cov_total": total, "pivot": pivot,
            "buffer": buffer, "rows": rows}


def clustered(C, classes, rows, seed, far_share=0.05):
    """Seeded clustered rows: class means 2 N(0, I), one SPD covariance 0.25 (B B^T / C + 0.1 I), and
    ``far_share`` of the rows uniform in +-6 (their label is ``classes``, which a fit leaves out).
    -> (x float32 [rows, C], labels u8 [rows], far bool [rows])"""
    g = torch.Generator().manual_seed(seed)
    means = 2.0 * torch.randn(classes, C, generator=g, dtype=torch.float64)
    B = torch.randn(C, C, generator=g, dtype=torch.float64)
    cov = 0.25 * (B @ B.T / C + 0.1 * torch.eye(C, dtype=torch.float64))
    L = torch.linalg.cholesky(cov)
    labels = torch.randint(0, classes, (rows,), generator=g)
    x = means[labels] + torch.randn(rows, C, generator=g, dtype=torch.float64) @ L.T
    far = torch.rand(rows, generator=g) < far_share
    x[far] = torch.rand(int(far.sum()), C, generator=g, dtype=torch.float64) * 12.0 - 6.0
    labels[far] = classes
    return x.float(), labels.to(torch.uint8), far
