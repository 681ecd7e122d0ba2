"""The fp64 reference of the calibration tests (tests/test_calib_cpu.py, tests/test_calib_gpu.py),
straight from logits and targets: softmax, equal-width confidence bins and the textbook ECE, MCE,
NLL, Brier score and entropy.  Also the tests' inputs: ``head_inputs`` of tests/head_cases.py and
targets sampled from the softmax of the fp64 logits at temperature 1.7, salted with ignored and
out-of-range pixels.  Nothing here touches a device."""
import functools

import torch
import torch.nn.functional as F

from tests.head_cases import CLASSES, SHAPES, U, head64, head_inputs  # noqa: F401  (the constants: for the suites)

Q_ONE = 1 << 24
T_TARGETS = 1.7                                   # the temperature the targets are sampled at
OUT_OF_RANGE = 200


def sample_targets(logits, nc, seed, ignore, t0=T_TARGETS, salt=True):
    """u8 targets [N,h,w] drawn per pixel from softmax(logits / t0); then about 2 % of the pixels are
    set to ``ignore`` and, when ``ignore`` is 255, about 1 % to an id outside [0, nc)."""
    g = torch.Generator().manual_seed(seed)
    p = F.softmax(logits / t0, 1).permute(0, 2, 3, 1).reshape(-1, nc)
    t = torch.multinomial(p, 1, generator=g).reshape(logits.shape[0], *logits.shape[2:]).to(torch.uint8)
    if salt:
        r = torch.rand(t.shape, generator=g)
        t[r < 0.02] = ignore
        if ignore == 255:
            t[(r >= 0.02) & (r < 0.03)] = OUT_OF_RANGE
    return t


@functools.lru_cache(maxsize=None)
def case(nc, shape, ignore_last):
    """-> dict of a test case, computed once and never modified: x, w, b, fp64 ``logits``,
    ``S`` = max_c (|b| + sum |x||w|) [N,2H,2W], ``target`` (u8), ``ignore``, ``counted`` mask, ``bad``
    (pixels out of range)."""
    x, w, b = head_inputs(nc, shape)
    logits, S = head64(x, w, b)
    S = S.max(1)[0]
    ignore = nc - 1 if ignore_last else 255
    target = sample_targets(logits, nc, 7 * nc + shape[2], ignore)
    tl = target.long()
    counted = (tl < nc) & (tl != ignore)
    return dict(x=x, w=w, b=b, logits=logits, S=S, target=target, ignore=ignore, counted=counted,
                bad=int(((tl >= nc) & (tl != ignore)).sum()))


def stats64(logits, target, counted, T):
    """Per pixel at temperature T, in the dtype of ``logits`` [N,nc,h,w]: (conf, label, nll, brier,
    ent); nll and brier are 0 where the pixel is not counted."""
    z = F.log_softmax(logits / T, 1)
    p = z.exp()
    conf, label = p.max(1)
    y = target.long().clamp(max=logits.shape[1] - 1).unsqueeze(1)
    nll = -z.gather(1, y)[:, 0]
    brier = (p * p).sum(1) - 2 * p.gather(1, y)[:, 0] + 1
    ent = -(p * z).sum(1)
    zero = torch.zeros_like(nll)
    return conf, label, torch.where(counted, nll, zero), torch.where(counted, brier, zero), ent


def pack(conf, correct, bins, dtype=torch.float64):
    """The histogram [bins][3] (pixels, correct, sum of q) of 1-D ``conf`` and ``correct``, by the
    library's rule evaluated in ``dtype``: bin = min(bins - 1, int(conf * bins)), q = int(conf * 2^24)."""
    conf = conf.to(dtype)
    b = (conf * torch.tensor(float(bins), dtype=dtype)).to(torch.int64).clamp(max=bins - 1)
    q = (conf * float(Q_ONE)).to(torch.int64)
    out = torch.zeros(bins, 3, dtype=torch.int64)
    out[:, 0] = torch.bincount(b, minlength=bins)
    out[:, 1] = torch.bincount(b, weights=correct.double(), minlength=bins).round().long()
    out[:, 2].index_add_(0, b, q)
    return out


def textbook(conf, correct, bins):
    """The textbook ECE and MCE of fp64 confidences: bins [i / bins, (i + 1) / bins), the last one closed."""
    conf = conf.double()
    n = conf.numel()
    b = (conf * bins).to(torch.int64).clamp(max=bins - 1)
    ece, mce = 0.0, 0.0
    for i in range(bins):
        sel = b == i
        if sel.any():
            gap = abs(correct[sel].double().mean().item() - conf[sel].mean().item())
            ece += gap * int(sel.sum()) / n
            mce = max(mce, gap)
    return ece, mce


def nll_curve(logits, target, counted, temps):
    """Sum of the NLL over the counted pixels at each temperature, fp64 -> list."""
    l2 = logits.permute(0, 2, 3, 1)[counted]
    y = target.long()[counted].unsqueeze(1)
    return [float(-F.log_softmax(l2 / float(T), 1).gather(1, y).sum()) for T in temps]


def dense_minimiser(logits, target, counted, lo=0.05, hi=40.0, iters=200):
    """The temperature of the smallest summed NLL, by golden-section search on log T in fp64 (the
    NLL is convex in 1/T, hence unimodal in log T)."""
    import math
    a, b = math.log(lo), math.log(hi)
    l2 = logits.permute(0, 2, 3, 1)[counted]
    y = target.long()[counted].unsqueeze(1)
    f = lambda u: float(-F.log_softmax(l2 / math.exp(u), 1).gather(1, y).sum())  # noqa: E731
    g = (math.sqrt(5) - 1) / 2
    c, d = b - g * (b - a), a + g * (b - a)
    fc, fd = f(c), f(d)
    for _ in range(iters):
        if fc < fd:
            b, d, fd = d, c, fc
            c = b - g * (b - a)
            fc = f(c)
        else:
            a, c, fc = c, d, fd
            d = a + g * (b - a)
            fd = f(d)
    return math.exp((a + b) / 2)
