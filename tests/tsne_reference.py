"""The checker of the latent-space add-on: exact t-SNE in fp64 numpy, transcribed from the formulas
of include/mdil_tsne.h (which are sklearn.manifold._t_sne's exact method).  A plain module: it
imports nothing from the product."""
import numpy as np

EPS = np.finfo(np.float64).eps                 # sklearn's MACHINE_EPSILON, 2.22e-16
SEARCH_STEPS = 100
ENTROPY_TOL = 1e-5


def sqdist(X):
    """D[i][j] = sum_k (x_ik - x_jk)^2 from the differences, fp64."""
    X = np.asarray(X, dtype=np.float64)
    D = np.empty((X.shape[0], X.shape[0]))
    for s in range(0, X.shape[0], 64):
        D[s:s + 64] = ((X[s:s + 64, None, :] - X[None, :, :]) ** 2).sum(-1)
    return D


def _offdiag(N):
    return ~np.eye(N, dtype=bool)


def entropies(D, betas):
    """Per row: (H, S) with p_j = exp(-beta D_ij), j != i; S = sum p (0 -> 1e-8);
    H = log S + beta sum_j D_ij p_j / S."""
    D = np.asarray(D, dtype=np.float64)
    p = np.exp(-D * betas[:, None]) * _offdiag(D.shape[0])
    S = p.sum(1)
    S = np.where(S == 0.0, 1e-8, S)
    return np.log(S) + betas * (D * p).sum(1) / S, S


def conditional(D, betas):
    """The row-normalised conditional matrix at the given betas (zero diagonal)."""
    D = np.asarray(D, dtype=np.float64)
    p = np.exp(-D * betas[:, None]) * _offdiag(D.shape[0])
    S = p.sum(1)
    S = np.where(S == 0.0, 1e-8, S)
    return p / S[:, None]


def binary_search(D, perplexity):
    """sklearn's _binary_search_perplexity, all rows at once.  -> (betas the rows were last
    evaluated at, conditional matrix)."""
    D = np.asarray(D, dtype=np.float64)
    N = D.shape[0]
    target = np.log(perplexity)
    beta = np.ones(N)
    lo = np.full(N, -np.inf)
    hi = np.full(N, np.inf)
    used = beta.copy()
    active = np.ones(N, dtype=bool)
    for _ in range(SEARCH_STEPS):
        if not active.any():
            break
        idx = np.nonzero(active)[0]
        b = beta[idx]
        Dr = D[idx]
        p = np.exp(-Dr * b[:, None])
        p[np.arange(len(idx)), idx] = 0.0
        S = p.sum(1)
        S = np.where(S == 0.0, 1e-8, S)
        diff = np.log(S) + b * (Dr * p).sum(1) / S - target
        used[idx] = b
        done = np.abs(diff) <= ENTROPY_TOL
        up = (diff > 0.0) & ~done
        dn = (diff <= 0.0) & ~done
        iu, idn = idx[up], idx[dn]
        lo[iu] = beta[iu]
        beta[iu] = np.where(np.isinf(hi[iu]), beta[iu] * 2.0, (beta[iu] + hi[iu]) / 2.0)
        hi[idn] = beta[idn]
        beta[idn] = np.where(np.isinf(lo[idn]), beta[idn] / 2.0, (beta[idn] + lo[idn]) / 2.0)
        active[idx[done]] = False
    return used, conditional(D, used)


def joint(C):
    """P = max((C + C^T) / max(sum(C + C^T), eps), eps) off the diagonal, 0 on it; dense."""
    P = C + C.T
    P = np.maximum(P / max(P.sum(), EPS), EPS)
    np.fill_diagonal(P, 0.0)
    return P


def condensed(P):
    """The upper triangle, row by row (scipy's squareform order)."""
    return P[np.triu_indices(P.shape[0], 1)]


def kl_and_grad(P, Y, exaggeration=1.0, dtype=np.float64, want=("kl", "abs")):
    """-> (KL(eP || Q), grad [N,2], absterm [N,2]); absterm = per row and component
    sum_j |4 e p_ij n_ij (y_i - y_j)| + |4 n_ij^2 (y_i - y_j) / Z|, the scale of the error bounds.
    ``want``: leave "kl" or "abs" out to skip them (None is returned in their place)."""
    P = np.asarray(P, dtype=dtype) * dtype(exaggeration)
    Y = np.asarray(Y, dtype=dtype)
    N = Y.shape[0]
    dx = Y[:, None, 0] - Y[None, :, 0]
    dy = Y[:, None, 1] - Y[None, :, 1]
    n = dtype(1.0) / (dtype(1.0) + (dx * dx + dy * dy))
    np.fill_diagonal(n, 0.0)
    Z = n.sum(dtype=dtype)
    Q = np.maximum(n / Z, dtype(EPS))
    kl = absterm = None
    if "kl" in want:
        off = _offdiag(N)
        kl = float((P[off] * np.log(np.maximum(P[off], dtype(EPS)) / Q[off])).sum(dtype=np.float64))
    w = (P - Q) * n
    grad = dtype(4.0) * np.stack(((w * dx).sum(1, dtype=dtype), (w * dy).sum(1, dtype=dtype)), 1)
    if "abs" in want:
        m = np.abs(P * n) + np.abs(n * n / Z)
        absterm = 4.0 * np.stack(((m * np.abs(dx)).sum(1), (m * np.abs(dy)).sum(1)), 1)
    return kl, grad, absterm


def descend(P, Y0, iters, learning_rate=200.0, exaggeration=12.0, exaggeration_iters=250, first_iter=0,
            kl_every=50, dtype=np.float64, state=None):
    """sklearn's _gradient_descent on the exact KL, momentum 0.5 / 0.8 and the exaggeration switching
    at ``exaggeration_iters``, where ``update`` and ``gains`` restart from 0 and 1 (sklearn's TSNE runs the
    two phases as two _gradient_descent calls).
    -> (Y, [(KL, |grad|)] of the iterations with it % kl_every == kl_every - 1, (update, gains))."""
    Y = np.array(Y0, dtype=dtype)
    update, gains = (np.zeros_like(Y), np.ones_like(Y)) if state is None else \
        (np.array(state[0], dtype=dtype), np.array(state[1], dtype=dtype))
    log = []
    for it in range(iters):
        early = first_iter + it < exaggeration_iters
        if first_iter + it == exaggeration_iters:
            update, gains = np.zeros_like(Y), np.ones_like(Y)
        logged = kl_every > 0 and it % kl_every == kl_every - 1
        kl, grad, _ = kl_and_grad(P, Y, exaggeration if early else 1.0, dtype, ("kl",) if logged else ())
        if logged:
            log.append((kl, float(np.sqrt((grad.astype(np.float64) ** 2).sum()))))
        inc = update * grad < 0.0
        gains = np.maximum(np.where(inc, gains + dtype(0.2), gains * dtype(0.8)), dtype(0.01))
        update = dtype(0.5 if early else 0.8) * update - dtype(learning_rate) * (gains * grad)
        Y = Y + update
    return Y, log, (update, gains)


def purity(Y, labels):
    """Share of the points whose nearest neighbour in Y carries their label."""
    D = sqdist(Y)
    np.fill_diagonal(D, np.inf)
    labels = np.asarray(labels)
    return float((labels[D.argmin(1)] == labels).mean())


def clusters(n, seed=0, dim=16, k=3):
    """The fixtures' recipe: k Gaussian clusters, centres 6 * randn, unit noise.  -> (X f32, labels)."""
    rs = np.random.RandomState(seed)
    centres = 6.0 * rs.randn(k, dim)
    labels = np.arange(n) % k
    return (centres[labels] + rs.randn(n, dim)).astype(np.float32), labels


def random_init(n, seed):
    """What sklearn's init="random" draws."""
    return (1e-4 * np.random.RandomState(seed).standard_normal((n, 2))).astype(np.float32)
