"""Trained-regime inputs for the BatchNorm, loss and Adam kernels: the seeded draws, their fp64
references, the error bounds and fp32 emulations of tests/test_conditioning_cpu.py and
tests/test_conditioning_gpu.py.  Importing this needs CPU torch and numpy only.

Every other parity test draws N(0, ~1) tensors, where a naive fp32 E[x^2] - E[x]^2, a softmax without
its max subtraction and a sloppy bias correction give the same numbers as the right forms.  The draws
here are the ones that tell them apart:

* BatchNorm: channels with |mean| / std ~ 2^10 (bias +-64 on a conv part of std ~ 2^-4) and constant
  channels (a dead ReLU in front of a conv leaves ``bias`` everywhere);
* losses: logits of magnitude 30 .. 150 (exp overflows above 88.7 without the max subtraction),
  saturated teachers (exp(t - max) underflows to 0) and an image whose labels all carry weight 0;
* Adam: late steps, gradients whose square underflows, grad_scale != 1, given (m, v) states.

u = 2^-24 throughout.  The bounds are fixed here from rounding models and the CPU emulations, never
from what a kernel returned; tests/golden/conditioning_cases.json pins the bytes of every draw."""
import functools
import hashlib
import math
import types

import numpy as np
import torch
import torch.nn.functional as F

from tests import head_cases as HC

U = HC.U
BN_EPS = 1e-3
BN_MOMENTUM = 0.1
BN_T, BN_MAX_BLOCKS, BN_U = 512, 256, 8            # csrc/bn.hip: threads per block, partial rows, rows in flight
CONST_VALUES = (-3.7, 0.1, 64.0)                   # the three constant channels of every BatchNorm draw
F32 = np.float32


def const_channels(C):
    return (1, C // 2, C - 1)


def digest(t):
    t = t.contiguous()
    h = hashlib.sha256(f"{t.dtype} {tuple(t.shape)} ".encode())
    h.update(t.numpy().tobytes())
    return h.hexdigest()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=_gen(seed)) * scale


# ------------------------------------------------------------------------------------------------
# BatchNorm: draws
# ------------------------------------------------------------------------------------------------
def channel_draw(n, ratio, seed):
    """One channel of n values: mean 64, std 64 / ratio (fp32)."""
    return 64.0 + _randn(n, seed=seed) * (64.0 / ratio)


def ill_conditioned(N, H, W, C, seed, ratio=2.0 ** 10):
    """NHWC fp32: channel c ~ (+64, -64 alternating) + (64 / ratio) * randn; channels
    ``const_channels(C)`` hold ``CONST_VALUES``."""
    sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
    z = _randn(N, H, W, C, seed=seed, scale=64.0 / ratio) + 64.0 * sign
    for c, v in zip(const_channels(C), CONST_VALUES):
        z[..., c] = v
    return z


def affine(C, seed):
    """gamma = 1 + 0.1 randn, beta = randn: a trained BatchNorm's affine; on the constant channels gamma = 0.45, 0.40,
    0.35 and beta = 1.  (There invstd = 1 / sqrt(eps) = 31.6, so scale = gamma invstd lies in [8, 16), where a correctly
    rounded product is off by up to half an ulp = 8 u.  The coefficient bound 4 u (|beta| + |mean scale|) is
    4 u |beta| + 5.1 u on the channel that holds 0.1: with a small |beta| it would ask more than any fp32 multiply
    can promise.  beta = 1 puts it at 9.1 u.)"""
    gamma, beta = 1 + _randn(C, seed=seed, scale=0.1), _randn(C, seed=seed + 1)
    for c, g in zip(const_channels(C), (0.45, 0.40, 0.35)):
        gamma[c], beta[c] = g, 1.0
    return gamma, beta


# producer, (C, N, H, W, d, axis), adapter tap
CONV_CASES = (
    ("sconv", (64, 2, 9, 7, 1, "w"), False), ("sconv", (64, 2, 9, 7, 1, "w"), True),
    ("sconv", (128, 2, 9, 7, 1, "w"), False), ("sconv", (128, 2, 9, 7, 1, "w"), True),
    ("wconv", (128, 2, 9, 6, 1, "w"), False), ("wconv", (64, 2, 9, 8, 1, "w"), True),
    ("w4conv", (128, 2, 9, 12, 1, "w"), False), ("w4conv", (128, 2, 9, 12, 1, "w"), True),
    ("w4conv", (128, 2, 16, 9, 2, "h"), False),
    ("c16conv", (16, 2, 9, 7, 1, "w"), False),
)
CONV_IDS = tuple("%s-C%d-%dx%dx%d-d%d%s" % ((p,) + s) + ("-adapter" if a else "") for p, s, a in CONV_CASES)
# stand-alone csrc/bn.hip: (C, N, H, W); 9 rows per thread: one U = 8 batch, then the remainder loop
BN_CASES = ((128, 2, 129, 130), (64, 2, 130, 269), (16, 2, 260, 520))
BN_IDS = tuple("bn-C%d-%dx%dx%d" % s for s in BN_CASES)


def bn_plan(npix, C):
    """Mirror of csrc/bn.hip::bn_plan -> (blocks, pixels per block, rows per thread ``ipb``)."""
    ppi = BN_T // (C // 4)
    iters = -(-npix // ppi)
    nblk = max(1, min(iters, BN_MAX_BLOCKS))
    ipb = -(-iters // nblk)
    ppb = ipb * ppi
    return -(-npix // ppb), ppb, ipb


@functools.lru_cache(maxsize=2)
def conv_case(idx):
    """Seeded fp32 host tensors of CONV_CASES[idx].  Forward: x, x2 = relu(randn); 3-tap weights and the
    adapter randn * 2^-4 / sqrt(1.5 C) (conv part of std ~ 2^-4); bias +-64 alternating; the three constant
    channels have every weight row zero, bias CONST_VALUES and bias2 0.  Backward: gradient input gx, gx2,
    gate, and the BatchNorm input z = ``ill_conditioned``."""
    prod, (C, N, H, W, d, axis), adapter = CONV_CASES[idx]
    s = 1000 + 100 * idx
    c = types.SimpleNamespace(producer=prod, C=C, N=N, H=H, W=W, d=d, axis=axis, adapter=adapter, npix=N * H * W)
    kk = (3, 1) if axis == "h" else (1, 3)
    wscale = 2.0 ** -4 / math.sqrt(1.5 * C)
    c.x, c.x2 = F.relu(_randn(N, H, W, C, seed=s + 1)), F.relu(_randn(N, H, W, C, seed=s + 2))
    c.w, c.wa = _randn(C, C, *kk, seed=s + 3, scale=wscale), _randn(C, C, 1, 1, seed=s + 4, scale=wscale)
    c.b = torch.where(torch.arange(C) % 2 == 0, 64.0, -64.0)
    c.b2 = _randn(C, seed=s + 5, scale=0.1)
    for ch, v in zip(const_channels(C), CONST_VALUES):
        c.w[ch], c.wa[ch], c.b[ch], c.b2[ch] = 0.0, 0.0, v, 0.0
    c.gamma, c.beta = affine(C, s + 6)
    c.gx, c.gx2 = _randn(N, H, W, C, seed=s + 8), _randn(N, H, W, C, seed=s + 9)
    c.gate = _randn(N, H, W, C, seed=s + 10)
    c.z = ill_conditioned(N, H, W, C, s + 11)
    return c


@functools.lru_cache(maxsize=1)
def bn_case(idx):
    """Seeded fp32 host tensors of BN_CASES[idx]: z = ``ill_conditioned``; gy, relu_src = randn."""
    C, N, H, W = BN_CASES[idx]
    s = 5000 + 100 * idx
    c = types.SimpleNamespace(C=C, N=N, H=H, W=W, npix=N * H * W)
    c.z = ill_conditioned(N, H, W, C, s + 1)
    c.gamma, c.beta = affine(C, s + 2)
    c.gy, c.relu_src = _randn(N, H, W, C, seed=s + 4), _randn(N, H, W, C, seed=s + 5)
    return c


# ------------------------------------------------------------------------------------------------
# BatchNorm: fp64 reference and bounds
# ------------------------------------------------------------------------------------------------
def ref_stats(t):
    """fp64 (mean, biased variance, constant-channel mask) per channel of an fp32 [..., C] tensor.  A channel
    whose values are all equal has that value as its mean and variance 0, exactly."""
    f = t.detach().cpu().reshape(-1, t.shape[-1]).double()
    mean, var = f.mean(0), f.var(0, unbiased=False)
    const = f.max(0)[0] == f.min(0)[0]
    return torch.where(const, f[0], mean), torch.where(const, torch.zeros_like(var), var), const


def cond_ratio(mean, var):
    """r = |mean| / std; 0 for a constant channel."""
    return torch.where(var > 0, mean.abs() / var.clamp_min(1e-300).sqrt(), torch.zeros_like(var))


def mean_bound(mean, var):
    return 8 * U * mean.abs() + 8 * U * var.sqrt()


def var_bound(mean, var, eps=BN_EPS):
    """(4 r + 8) u var: the chunked two-pass + Chan-merge model at ten times its emulated worst case
    (0.4 r u); (16 u |mean|)^2: the floor of a constant channel (the chunk mean is off by a few ulp, the
    squared deviations from it are that small); 8 u (var + eps): the two roundings between the variance
    and the stored 1 / sqrt(var + eps)."""
    return (4 * cond_ratio(mean, var) + 8) * U * var + (16 * U * mean.abs()) ** 2 + 8 * U * (var + eps)


def var_from_invstd(invstd, eps=BN_EPS):
    return invstd.double() ** -2 - eps


def check_window(mean, var, const, lo=2.0 ** 9, hi=2.0 ** 11):
    """Precondition on the reference alone: the three constant channels are constant and every other
    channel has lo <= |mean| / std <= hi."""
    C = mean.numel()
    assert sorted(torch.nonzero(const).flatten().tolist()) == sorted(const_channels(C)), "constant channels"
    r = cond_ratio(mean, var)[~const]
    assert float(r.min()) >= lo and float(r.max()) <= hi, (float(r.min()), float(r.max()))
    return float(r.min()), float(r.max())


def bn_forward_ratios(coef, rm, rv, nbt, gamma, beta, mean, var, n):
    """|err| / bound per channel of a train-mode statistics launch that started from rm = rv = 0.
    coef: [4][C] save_mean, save_invstd, scale, shift.  -> {name: fp64 [C]}."""
    coef, rm, rv = coef.detach().cpu().double(), rm.detach().cpu().double(), rv.detach().cpu().double()
    gamma, beta = gamma.detach().cpu().double(), beta.detach().cpu().double()
    assert int(nbt) == 1
    mb, vb = mean_bound(mean, var), var_bound(mean, var)
    # ("var" holds every channel; the GPU suite prints constant and ill-conditioned channels apart)
    out = {"mean": (coef[0] - mean).abs() / mb,
           "var": (var_from_invstd(coef[1]) - var).abs() / vb,
           "rv": (rv * (n - 1) / (BN_MOMENTUM * n) - var).abs() / (vb + 4 * U * var),
           "rm": (rm / BN_MOMENTUM - mean).abs() / (mb + 4 * U * mean.abs())}
    cb = 4 * U * (beta.abs() + (mean * coef[2]).abs())
    out["scale"] = (coef[2] - gamma * coef[1]).abs() / cb
    out["shift"] = (coef[3] - (beta - coef[0] * coef[2])).abs() / cb
    return out


def bn_apply_ratio(y, z, coef, gamma, beta, mean, var):
    """|err| / bound (worst element) of y = z * scale + shift against fp64 (z - mean) invstd gamma + beta."""
    z64, coef = z.detach().cpu().double(), coef.detach().cpu().double()
    want = (z64 - mean) * (var + BN_EPS).rsqrt() * gamma.double() + beta.double()
    bound = 4 * U * ((z64 * coef[2]).abs() + coef[3].abs()) + 4 * U * want.abs()
    return float(((y.detach().cpu().double() - want).abs() / bound).max())


def bn_backward_ref(g64, z, gamma, mean32, invstd32):
    """fp64 BatchNorm backward of the (already gated) gradient g64 through z with the fp32 statistics the
    kernels are given -> (gz, dgamma, dbeta)."""
    C = z.shape[-1]
    n = z.numel() // C
    gf, z64 = g64.reshape(n, C), z.double().reshape(n, C)
    xhat = (z64 - mean32.double()) * invstd32.double()
    dbeta, dgamma = gf.sum(0), (gf * xhat).sum(0)
    gz = (gamma.double() * invstd32.double()) * (gf - dbeta / n - xhat * dgamma / n)
    return gz.reshape(z.shape), dgamma, dbeta


def coef_from_ref(z, gamma, beta):
    """[4][C] fp32 coefficient table from the fp64 statistics of z, rounded to fp32."""
    mean, var, _ = ref_stats(z)
    mean32, invstd32 = mean.float(), (var + BN_EPS).rsqrt().float()
    sc = gamma * invstd32
    return torch.stack([mean32, invstd32, sc, beta - mean32 * sc]).contiguous()


# ------------------------------------------------------------------------------------------------
# BatchNorm: fp32 emulations of the statistic forms (numpy, every operation rounded to fp32)
# ------------------------------------------------------------------------------------------------
def _chan32(n, mean, m2, nb, meanb, m2b):
    """csrc/common.h::welford_merge on fp32 arrays (nb > 0)."""
    nn = (n + nb).astype(F32)
    d = (meanb - mean).astype(F32)
    f = (nb / nn).astype(F32)
    return nn, (mean + d * f).astype(F32), (m2 + m2b + d * d * n * f).astype(F32)


def _two_pass32(c):
    """(mean, M2) along the last axis: fp32 sum in order, times 1 / m, then squared deviations from it."""
    m = c.shape[-1]
    s = c[..., 0].astype(F32)
    for j in range(1, m):
        s = (s + c[..., j]).astype(F32)
    bm = (s * F32(1.0 / m)).astype(F32)
    q = np.zeros_like(bm)
    for j in range(m):
        d = (c[..., j] - bm).astype(F32)
        q = (q + d * d).astype(F32)
    return bm, q


def emulate_chunked(x, k, groups=16):
    """The kernels' form: chunks of k values (the last one ragged) summarised by two passes, chunk j
    Chan-merged into the running summary of group j % groups (a thread / lane / wave), the groups merged
    up a binary tree.  -> (mean, biased variance) as Python floats of fp32 values."""
    x = np.asarray(x, dtype=F32)
    n = x.shape[0]
    rounds = (n // k) // groups
    gn, gm, gq = (np.zeros(groups, F32) for _ in range(3))
    body = x[:rounds * groups * k].reshape(rounds, groups, k)
    for r in range(rounds):
        bm, bq = _two_pass32(body[r])
        gn, gm, gq = _chan32(gn, gm, gq, F32(k), bm, bq)
    rest = x[rounds * groups * k:]
    for i, lo in enumerate(range(0, rest.shape[0], k)):
        c = rest[lo:lo + k]
        bm, bq = _two_pass32(c[None, :])
        j = slice(i % groups, i % groups + 1)
        gn[j], gm[j], gq[j] = _chan32(gn[j], gm[j], gq[j], F32(c.shape[0]), bm, bq)
    while gn.shape[0] > 1:
        a, b = slice(0, None, 2), slice(1, None, 2)
        keep = gn[b] > 0
        nn, mm, qq = _chan32(gn[a], gm[a], gq[a], np.where(keep, gn[b], F32(1)), gm[b], gq[b])
        gn, gm, gq = (np.where(keep, new, old[a]) for new, old in ((nn, gn), (mm, gm), (qq, gq)))
    assert float(gn[0]) == n
    return float(gm[0]), float(F32(gq[0] / F32(n)))


def emulate_naive_sequential(x):
    """fp32 E[x^2] - E[x]^2 with both sums taken in order."""
    x = np.asarray(x, dtype=F32)
    n = F32(x.shape[0])
    m = F32(np.cumsum(x, dtype=F32)[-1] / n)
    return float(m), float(F32(F32(np.cumsum((x * x).astype(F32), dtype=F32)[-1] / n) - F32(m * m)))


def _pairwise32(v):
    v = np.concatenate([v, np.zeros((1 << max(0, (v.shape[0] - 1).bit_length())) - v.shape[0], F32)])
    while v.shape[0] > 1:
        v = (v[0::2] + v[1::2]).astype(F32)
    return v[0]


def emulate_naive_pairwise(x):
    """fp32 E[x^2] - E[x]^2 with both sums taken up a binary tree (the best a naive form can do)."""
    x = np.asarray(x, dtype=F32)
    n = F32(x.shape[0])
    m = F32(_pairwise32(x) / n)
    return float(m), float(F32(F32(_pairwise32((x * x).astype(F32)) / n) - F32(m * m)))


def emulate_naive_grouped(x, groups=16):
    """fp32 E[x^2] - E[x]^2 laid out as a kernel would: value i goes to group i % groups (a thread), each group
    sums in order, the groups are summed up a binary tree."""
    x = np.asarray(x, dtype=F32)
    n = F32(x.shape[0])
    pad = np.concatenate([x, np.zeros(-x.shape[0] % groups, F32)]).reshape(-1, groups)
    s = _pairwise32(np.cumsum(pad, axis=0, dtype=F32)[-1])
    q = _pairwise32(np.cumsum((pad * pad).astype(F32), axis=0, dtype=F32)[-1])
    m = F32(s / n)
    return float(m), float(F32(F32(q / n) - F32(m * m)))


CHUNKINGS = (2, 4, 8, 32, 3)                       # pair, quad, U batch, direct-form tile, a ragged tile
EMULATION_DRAWS = tuple((n, r) for n in (1920, 7683) for r in (2.0 ** 6, 2.0 ** 10, 2.0 ** 12))


def emulation_channels():
    """[(name, fp32 values)]: the stand-alone draws at three ratios and two lengths, and the constant channels."""
    out = [(f"n{n}-r{int(r)}", channel_draw(n, r, seed=int(n + r))) for n, r in EMULATION_DRAWS]
    out += [(f"const{v}", torch.full((1920,), v)) for v in CONST_VALUES]
    return out


def stat_ratios(mean_got, var_got, x):
    """(|dmean| / bound, |dvar| / bound) of a statistic of the fp32 values x against their fp64 statistics."""
    mean, var, _ = ref_stats(x.reshape(-1, 1))
    return (float(abs(mean_got - mean[0]) / mean_bound(mean, var)[0]),
            float(abs(var_got - var[0]) / var_bound(mean, var, 0.0)[0]))


# ------------------------------------------------------------------------------------------------
# losses
# ------------------------------------------------------------------------------------------------
LOSS_SHAPE = (2, 24, 40)
LOGIT_DRAWS = {"confident": (30.0, 60.0), "moderate": (8.0, 25.0)}     # scale of randn, boost of the predicted class
LABEL_MAPS = ("a", "b", "c")
HEAD_SHAPES = ((1, 9, 7), (3, 16, 48))
HEAD_GAIN = 10.0


def class_weights(nc):
    """The class weights of tests/test_hip_parity.py::test_losses: class nc - 1 has weight 0."""
    from oracle import fixtures as fx
    return torch.tensor(fx.WEIGHT_BDD) if nc == 20 else torch.cat(
        [1.0 + 9.0 * torch.rand(nc - 1, generator=_gen(4)), torch.zeros(1)])


def _boosted(nc, shape, scale, boost, pred, seed):
    N, H, W = shape
    logits = _randn(N, nc, H, W, seed=seed, scale=scale)
    logits.scatter_add_(1, pred.unsqueeze(1), torch.full((N, 1, H, W), boost))
    return logits


@functools.lru_cache(maxsize=None)
def loss_logits(nc, draw):
    """-> (student logits [N,nc,H,W] fp32, teacher logits, student's predicted class [N,H,W]).  Student:
    randn * scale with ``boost`` added on a random predicted class per pixel; teacher: drawn the same way,
    with a predicted class of its own on 10 % of the pixels."""
    scale, boost = LOGIT_DRAWS[draw]
    seed = 7000 + 10 * nc + int(scale)
    g = _gen(seed)
    pred = torch.randint(0, nc, LOSS_SHAPE, generator=g)
    other = torch.randint(0, nc, LOSS_SHAPE, generator=g)
    tpred = torch.where(torch.rand(LOSS_SHAPE, generator=g) < 0.10, other, pred)
    return (_boosted(nc, LOSS_SHAPE, scale, boost, pred, seed + 1),
            _boosted(nc, LOSS_SHAPE, scale, boost, tpred, seed + 2), pred)


def label_map(kind, pred, nc, seed):
    """In-range int64 labels of pred's shape.  (a) the predicted class on 90 % of the pixels, the rest random,
    then 10 % set to the zero-weight class nc - 1; (b) as (a) with image 0 entirely nc - 1; (c) one class
    everywhere except 10 % nc - 1."""
    g = _gen(seed)
    rnd_cls = torch.randint(0, nc, pred.shape, generator=g)
    r1, r2 = torch.rand(pred.shape, generator=g), torch.rand(pred.shape, generator=g)
    lab = torch.where(r1 < 0.10, rnd_cls, pred) if kind in ("a", "b") else torch.full_like(pred, 3)
    lab = torch.where(r2 < 0.10, torch.full_like(lab, nc - 1), lab)
    if kind == "b":
        lab[0] = nc - 1
    return lab.contiguous()


def map_applies(kind, shape):
    """Map (b) on a single image would leave no pixel with a weight: torch returns NaN there too."""
    return not (kind == "b" and shape[0] == 1)


@functools.lru_cache(maxsize=None)
def head_case(nc, shape):
    """Fused-head inputs: ``head_cases.draw`` for student and teacher with the head weights and bias times
    HEAD_GAIN -> namespace of fp32 tensors x, w, b, xt, wt, bt and the fp64 logits / S of both."""
    seed = HC.case_seed(nc, shape)
    x, w, b = HC.draw(nc, shape, 9000 + seed)
    xt, wt, bt = HC.draw(nc, shape, 9500 + seed)
    c = types.SimpleNamespace(x=x, w=w * HEAD_GAIN, b=b * HEAD_GAIN, xt=xt, wt=wt * HEAD_GAIN, bt=bt * HEAD_GAIN)
    c.logits, c.S = HC.head64(c.x, c.w, c.b)
    c.tlogits, c.tS = HC.head64(c.xt, c.wt, c.bt)
    return c


def ce_ref(logits64, lab, weight):
    """fp64 weighted cross entropy (oracle/rap_oracle.py::ce2d)."""
    picked = F.log_softmax(logits64, dim=1).gather(1, lab.unsqueeze(1)).squeeze(1)
    w = weight.double()[lab]
    return -(w * picked).sum() / w.sum()


def kld_ref(s64, t64):
    """fp64 mean(t (log t - p_s)) (oracle/rap_oracle.py::kld_prob) with log t from log_softmax."""
    logt = F.log_softmax(t64, dim=1)
    return (logt.exp() * (logt - F.softmax(s64, dim=1))).mean()


def pixel_bound(logits64, S=None):
    """b_p = 2 E_p + 16 u (1 + max_k |l_pk|): twice the logit error E_p (0 for given logits, gamma(17) max_k S_pk
    for the fused head) plus the chain max / subtract / exp / sum / log at 16 u of the logit magnitude (3.5 u
    emulated with libm; the rest is room for the 1-ulp hardware exp / log / rcp)."""
    b = 16 * U * (1 + logits64.abs().amax(1))
    return b if S is None else b + 2 * HC.gamma(17) * S.amax(1)


def ce_bound(logits64, lab, weight, ce, S=None):
    w = weight.double()[lab]
    return float((w * pixel_bound(logits64, S)).sum() / w.sum() + 8 * U * abs(float(ce)))


def kld_bound(s64, t64, kld, Ss=None, St=None):
    nc = s64.shape[1]
    return float((pixel_bound(s64, Ss) + pixel_bound(t64, St)).mean() / nc + 8 * U * abs(float(kld)))


def emulate_ce_pixels(logits, lab, subtract_max=True):
    """csrc/loss.hip's per-pixel chain in fp32 (numpy): max, subtract, exp, sum in class order, log, minus
    the label's shifted logit.  logits [P, nc] fp32, lab [P] -> fp32 [P]."""
    x = np.asarray(logits, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        if subtract_max:
            x = (x - x.max(1, keepdims=True)).astype(F32)
        e = np.exp(x).astype(F32)
        se = e[:, 0].copy()
        for k in range(1, x.shape[1]):
            se = (se + e[:, k]).astype(F32)
        return (np.log(se).astype(F32) - x[np.arange(x.shape[0]), np.asarray(lab)]).astype(F32)


# ------------------------------------------------------------------------------------------------
# Adam
# ------------------------------------------------------------------------------------------------
ADAM_N = 100003
ADAM_STEPS = (1, 1000, 10 ** 6)
ADAM_SCALES = (1.0, 0.125)
ADAM = dict(lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-4)


@functools.lru_cache(maxsize=1)
def adam_state():
    """fp32 (p, g, m, v) of ADAM_N elements, regime = index % 4:
    0 ordinary: g, m ~ 1e-3 randn, v ~ 1e-6 (0.5 + rand), |p| >= 1e-2 (the parameter bound has no term for a
         cancelling m', so 2 u |p| has to carry it: step * 4u (|b1 m| + |(1-b1) g'|) / denom <= 0.02 u here);
    1 g = 0 (the weight decay alone moves m and v), p, m, v as in 0;
    2 |g| = 1e-20 with p = 0, so that g'^2 underflows; v in {0, 1e-30}, m ~ 1e-3 randn or 0;
    3 v = 1, m = -0.5 against g in (0.5, 2)."""
    g_ = _gen(11)
    n = ADAM_N
    rn = lambda: torch.randn(n, generator=g_)
    p = rn() * 0.1
    p = torch.where(p < 0, p - 0.01, p + 0.01)
    g, m = rn() * 1e-3, rn() * 1e-3
    v = (0.5 + torch.rand(n, generator=g_)) * 1e-6
    sign = torch.where(torch.rand(n, generator=g_) < 0.5, -1.0, 1.0)
    big = 0.5 + 1.5 * torch.rand(n, generator=g_)
    i = torch.arange(n)
    reg = i % 4
    g = torch.where(reg == 1, torch.zeros(n), g)
    g = torch.where(reg == 2, sign * 1e-20, g)
    p = torch.where(reg == 2, torch.zeros(n), p)
    v = torch.where(reg == 2, torch.where((i // 4) % 2 == 0, 0.0, 1e-30), v)
    m = torch.where((reg == 2) & ((i // 8) % 2 == 1), torch.zeros(n), m)
    g = torch.where(reg == 3, big, g)
    m = torch.where(reg == 3, torch.full((n,), -0.5), m)
    v = torch.where(reg == 3, torch.ones(n), v)
    return p.contiguous(), g.contiguous(), m.contiguous(), v.contiguous(), reg


def adam_ref(p, g, m, v, step, grad_scale, lr, beta1, beta2, eps, weight_decay):
    """One fp64 torch.optim.Adam (L2) step from the fp32 inputs with the host's double bias corrections.
    -> (p', m', v', update = lr / bc1 * m' / denom, (|b1 m|, |(1 - b1) g'|))."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    gp = g * grad_scale + weight_decay * p
    a, b = beta1 * m, (1.0 - beta1) * gp
    m1 = a + b
    v1 = beta2 * v + (1.0 - beta2) * gp * gp
    upd = (lr / bc1) * m1 / (v1.sqrt() / math.sqrt(bc2) + eps)
    return p - upd, m1, v1, upd, (a.abs(), b.abs())


def adam_ratios(got_p, got_m, got_v, p, ref):
    """Worst |err| / bound of (p, m, v):  |dp| <= 2u |p| + 16u |update|;  |dm| <= 4u (|b1 m| + |(1-b1) g'|);
    |dv| <= 4u v' + 2^-126 (a denormal v' may be flushed)."""
    p1, m1, v1, upd, (a, b) = ref
    rp = (got_p.double() - p1).abs() / (2 * U * p.double().abs() + 16 * U * upd.abs()).clamp_min(1e-300)
    rm = (got_m.double() - m1).abs() / (4 * U * (a + b)).clamp_min(1e-300)
    rv = (got_v.double() - v1).abs() / (4 * U * v1 + 2.0 ** -126)
    return rp, rm, rv


def adam_emulate32(p, g, m, v, step, grad_scale, lr, beta1, beta2, eps, weight_decay):
    """csrc/adam.hip in fp32 (numpy): scalars cast as the host casts them, every operation rounded."""
    p, g, m, v = (t.numpy().astype(F32) for t in (p, g, m, v))
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    stepf, b1, omb1, b2, omb2 = F32(lr / bc1), F32(beta1), F32(1.0 - beta1), F32(beta2), F32(1.0 - beta2)
    gi = (g * F32(grad_scale) + F32(weight_decay) * p).astype(F32)
    mi = (b1 * m + omb1 * gi).astype(F32)
    vi = (b2 * v + (omb2 * gi).astype(F32) * gi).astype(F32)
    denom = (np.sqrt(vi).astype(F32) / F32(math.sqrt(bc2)) + F32(eps)).astype(F32)
    return tuple(torch.from_numpy(t) for t in ((p - stepf * (mi / denom).astype(F32)).astype(F32), mi, vi))


# ------------------------------------------------------------------------------------------------
# the bytes of every draw (tests/golden/conditioning_cases.json)
# ------------------------------------------------------------------------------------------------
_CONV_FIELDS = ("x", "x2", "w", "wa", "b", "b2", "gamma", "beta", "gx", "gx2", "gate", "z")
_BN_FIELDS = ("z", "gamma", "beta", "gy", "relu_src")
_HEAD_FIELDS = ("x", "w", "b", "xt", "wt", "bt")


def _fields(ns, names):
    return {k: digest(getattr(ns, k)) for k in names}


def digests():
    """{section: {case: {tensor: sha256}}} of every seeded draw of this module."""
    out = {"conv": {CONV_IDS[i]: _fields(conv_case(i), _CONV_FIELDS) for i in range(len(CONV_CASES))},
           "bn": {BN_IDS[i]: _fields(bn_case(i), _BN_FIELDS) for i in range(len(BN_CASES))},
           "emulation": {name: digest(x) for name, x in emulation_channels()},
           "logits": {}, "labels": {}, "head": {}}
    for nc in (20, 27):
        for draw in LOGIT_DRAWS:
            s, t, pred = loss_logits(nc, draw)
            out["logits"][f"{nc} {draw}"] = {"student": digest(s), "teacher": digest(t), "pred": digest(pred)}
            for kind in LABEL_MAPS:
                out["labels"][f"{nc} {draw} {kind}"] = digest(label_map(kind, pred, nc, 40 + nc))
        for shape in HEAD_SHAPES:
            out["head"]["%d %dx%dx%d" % ((nc,) + shape)] = _fields(head_case(nc, shape), _HEAD_FIELDS)
    out["adam"] = dict(zip(("p", "g", "m", "v", "regime"), map(digest, adam_state())))
    return out
