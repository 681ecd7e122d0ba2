"""The open-set add-on said in plain numpy / torch fp64, for tests/test_openset_cpu.py and
tests/test_openset_gpu.py: the 16-bit key, the four scores from fp64 logits, the histograms by
``bincount``, the metrics as exact ``fractions.Fraction`` sums, and the apply rule pixel by pixel.
Nothing here imports the package."""
import math
from fractions import Fraction

import numpy as np
import torch

KINDS = ("msp", "maxlogit", "energy", "entropy")
CODES = 65536
NONFINITE = 65535


def key16(values):
    """float32 values (numpy or torch) -> int64 codes; -0 is taken as +0."""
    v = np.asarray(values, dtype=np.float32).copy()
    v[v == 0] = 0.0
    bits = v.view(np.uint32).astype(np.int64)
    key = np.where(bits & 0x80000000, ~bits & 0xffffffff, bits | 0x80000000)
    return torch.from_numpy(key >> 16)


def scores64(logits):
    """fp64 logits [N,nc,H,W] -> the four scores [4,N,H,W] in fp64, each from its definition."""
    m = logits.max(1)[0]
    lse = torch.logsumexp(logits, 1)
    logp = logits - lse.unsqueeze(1)
    p = logp.exp()
    msp = 1.0 - p.max(1)[0]
    ent = -(p * torch.where(p > 0, logp, torch.zeros_like(logp))).sum(1)
    return torch.stack([msp, -m, -lse, ent])


def scores32(x, w, b):
    """The plain float32 torch evaluation of the same formulas: conv_transpose2d, logsumexp, softmax."""
    import torch.nn.functional as F
    logits = F.conv_transpose2d(x, w, b, stride=2)
    lse = torch.logsumexp(logits, 1)
    p = F.softmax(logits, 1)
    ent = -(p * torch.where(p > 0, p.log(), torch.zeros_like(p))).sum(1)
    return torch.stack([1.0 - p.max(1)[0], -logits.max(1)[0], -lse, ent])


def hist_of(codes, groups):
    """codes, groups (int, one shape) -> int64 [2][65536]: bincount per group 0 / 1, code 65535 left
    out only where the caller masked it (pass groups = 2 there)."""
    c, g = codes.reshape(-1).long(), groups.reshape(-1).long()
    return torch.stack([torch.bincount(c[g == k], minlength=CODES) for k in (0, 1)])


def pairwise_auroc(neg, pos):
    """P(pos > neg) + P(pos == neg) / 2 over all pairs, as a Fraction (brute force)."""
    neg, pos = np.sort(np.asarray(neg)), np.asarray(pos)
    lower = np.searchsorted(neg, pos, side="left")
    upto = np.searchsorted(neg, pos, side="right")
    twice = int((lower + upto).sum())                              # 2 (lower) + (equal) = lower + upto
    return Fraction(twice, 2 * len(neg) * len(pos))


def metrics(hist_kind, tpr=0.95):
    """Exact Fractions from one [2][65536] table, each figure from its definition over thresholds."""
    known, unknown = (np.asarray(r, dtype=object) for r in torch.as_tensor(hist_kind).tolist())
    N, P = int(sum(known)), int(sum(unknown))
    occupied = [b for b in range(CODES) if known[b] or unknown[b]]
    n_below, auroc, ties = 0, Fraction(0), Fraction(0)
    for b in occupied:
        auroc += Fraction(int(unknown[b]) * (2 * n_below + int(known[b])), 2 * P * N)
        ties += Fraction(int(unknown[b]) * int(known[b]), P * N)
        n_below += int(known[b])
    need = math.ceil(Fraction(str(float(tpr))) * P)
    tp = fp = 0
    aupr, at = Fraction(0), None
    for b in reversed(occupied):
        tp += int(unknown[b])
        fp += int(known[b])
        if unknown[b]:
            aupr += Fraction(int(unknown[b]), P) * Fraction(tp, tp + fp)
        if at is None and tp >= need:
            at = (b, Fraction(fp, N))
    return {"auroc": auroc, "aupr": aupr, "fpr_at_tpr": at[1], "threshold_code": at[0], "tie_mass": ties, "P": P, "N": N}


def apply_rule(label, code, nc, thr, id_map=None, unknown_id=255, cdf=None, target=None, lut=None):
    """Pixel by pixel over flat maps -> dict of out, score and the counters (tensors / ints)."""
    n = label.numel()
    lab, cd = label.reshape(-1).tolist(), code.reshape(-1).tolist()
    tg = None if target is None else target.reshape(-1).tolist()
    groups = None if lut is None else lut.tolist()
    ids = list(range(nc)) if id_map is None else id_map.tolist()
    table = None if cdf is None else cdf.tolist()
    out, score = [0] * n, [0] * n
    seen, rejected = [0] * nc, [0] * nc
    detect = [[0, 0], [0, 0]]
    confusion = [[0] * nc for _ in range(nc)]
    bad_t = bad_l = 0
    for i in range(n):
        if table is not None:
            score[i] = table[cd[i]]
        if lab[i] >= nc:
            out[i] = unknown_id
            bad_l += 1
            continue
        rej = cd[i] >= thr
        out[i] = unknown_id if rej else ids[lab[i]]
        seen[lab[i]] += 1
        rejected[lab[i]] += rej
        if tg is not None:
            g = groups[tg[i]]
            if g < 2:
                detect[g][int(rej)] += 1
            if g == 0:
                if tg[i] >= nc:
                    bad_t += 1
                elif not rej:
                    confusion[tg[i]][lab[i]] += 1
    return {"out": torch.tensor(out, dtype=torch.uint8), "score": torch.tensor(score, dtype=torch.uint8),
            "seen": torch.tensor(seen), "rejected": torch.tensor(rejected), "detect": torch.tensor(detect),
            "confusion": torch.tensor(confusion), "bad_targets": bad_t, "bad_labels": bad_l}
