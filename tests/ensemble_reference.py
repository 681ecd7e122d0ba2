"""The fp64 reference of the ensemble add-on (include/mdil_ensemble.h), shared by
tests/test_ensemble_cpu.py and tests/test_ensemble_gpu.py: the cases, their seeded inputs, the vote
in fp64 and, per pixel and class, a bound on what fp32 arithmetic of the kernel's kind may add.

Which pixels may differ.  The kernel's header counts ``k`` roundings on the longest path to a
resized logit, so ``|U - exact| <= gamma_k * Au`` (Au: the same two steps on absolute values,
gamma_k = k u / (1 - k u), u = 2^-24), and ``softmax: cs u`` for what the softmax arithmetic itself
adds to one probability.  A logit error of d moves a probability by at most 2 p (1 - p) d to first
order (every logit of the pixel may be off by d: |dp_c| <= p_c (1 - p_c) d + p_c sum_j!=c p_j d).
The sum over the views adds gamma_nviews * |S|.  A pixel whose fp64 top-2 margin is within the sum
of its two classes' bounds is excluded; every other pixel must equal the fp64 argmax, and at most
max(1, pixels // 1000) pixels of a case may be excluded -- none in a case of fewer than 100."""
import functools
import os
import re

import torch
import torch.nn.functional as F

from tests.head_cases import CLASSES, U, cap, gamma  # noqa: F401  (CLASSES and cap are for the two suites)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_MAX, CS_MAX = 96, 64
MODES = ("prob", "logit")
# view shapes (N, H, W), mirrored flags, output size
CASES = [
    ([(1, 1, 1)], [0], (5, 7)),
    ([(1, 1, 1)] * 2, [0, 1], (2, 2)),
    ([(1, 9, 7)] * 2, [0, 1], (25, 31)),
    ([(1, 9, 7), (1, 7, 5), (1, 11, 9)], [0, 0, 1], (18, 14)),
    ([(2, 12, 20)] * 2 + [(2, 9, 15)] * 2 + [(2, 15, 25)] * 2, [0, 1, 0, 1, 0, 1], (45, 77)),
    ([(2, 12, 20), (2, 9, 15), (2, 18, 30)], [1, 0, 0], (48, 80)),
    ([(3, 16, 48), (3, 16, 48), (3, 12, 36), (3, 24, 72)], [0, 1, 1, 0], (90, 135)),
    ([(1, 8, 12)] * 8, [0, 1] * 4, (33, 50)),
]
# goes round the kernel's bounded grid a second time (nc = 2 only)
BIG = ([(1, 200, 300), (1, 150, 225)], [0, 1], (1025, 2051))
BIG_NC, BIG_SEED = 2, 2099


def header_constants():
    """(k, cs) as the header comment of ensemble_head.hip states them."""
    src = open(os.path.join(REPO, "mdil_ss_amd", "ext", "ensemble_head.hip")).read()
    k = [int(v) for v in re.findall(r"k = (\d+) roundings", src)]
    cs = [int(v) for v in re.findall(r"softmax: (\d+) u\b", src)]
    assert len(k) == 1 and len(cs) == 1, (k, cs)
    return k[0], cs[0]


def inputs(nc, shapes, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(16, nc, 2, 2, generator=g)
    b = torch.randn(nc, generator=g) * 0.2
    xs = [F.relu(torch.randn(n, 16, h, w_, generator=g)) for n, h, w_ in shapes]
    return xs, w, b


def reference(xs, w, b, flips, size, mode, k, cs):
    """fp64 throughout -> (S [N,nc,Ho,Wo], label i64 [N,Ho,Wo], excluded bool [N,Ho,Wo], B like S)."""
    S = B = 0
    for x, f in zip(xs, flips):
        L = F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2)
        A = F.conv_transpose2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=2)
        if f:
            L, A = L.flip(3), A.flip(3)
        Lu = F.interpolate(L, size, mode="bilinear", align_corners=False)
        Au = F.interpolate(A, size, mode="bilinear", align_corners=False)
        if mode == "logit":
            S, B = S + Lu, B + gamma(k) * Au
        else:
            p = Lu.softmax(1)
            d = gamma(k) * Au.max(1, keepdim=True)[0]
            S, B = S + p, B + 2 * p * (1 - p) * d + cs * U      # first-order propagation + softmax's own error
    B = B + gamma(len(xs)) * S.abs()                            # the view sum
    top, idx = S.topk(2, dim=1)
    return S, S.max(1)[1], (top[:, 0] - top[:, 1]) <= B.gather(1, idx).sum(1), B


@functools.lru_cache(maxsize=None)
def case_inputs(nc, index):
    """Seeded inputs of case ``index`` (-1: the bounded-grid case); shared, never modified."""
    if index < 0:
        return inputs(nc, BIG[0], BIG_SEED)
    return inputs(nc, CASES[index][0], 1000 * nc + index)


@functools.lru_cache(maxsize=None)
def case(nc, index, mode):
    """-> (xs, w, b, flips, size, S, label, excluded, B) with the header's k and cs; computed once."""
    _, flips, size = BIG if index < 0 else CASES[index]
    xs, w, b = case_inputs(nc, index)
    k, cs = header_constants()
    return (xs, w, b, flips, size) + reference(xs, w, b, flips, size, mode, k, cs)
