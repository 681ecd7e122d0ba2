"""The label-audit add-on said in plain torch fp64 / Python integers, for tests/test_audit_cpu.py and
tests/test_audit_gpu.py: the softmax, its 16-bit quantisation, the thresholds, the suggested class
from given q maps, the confident joint and the per-image counts by ``bincount``, the calibrated joint
as exact ``fractions.Fraction``s and the apply rule pixel by pixel.  Nothing here imports the package."""
from fractions import Fraction

import torch

Q_ONE = 65536


def probs64(logits):
    """fp64 logits [N,nc,H,W] -> the softmax over the classes, fp64."""
    return torch.softmax(logits.double(), 1)


def q_of(p):
    """min(65535, floor(p * 65536)) as int64; p >= 0."""
    return torch.clamp((p.double() * Q_ONE).floor(), max=Q_ONE - 1).to(torch.int64)


def valid_of(target, nc, ignore):
    t = target.long()
    return (t < nc) & (t != ignore)


def self_q(q, target, nc, ignore):
    """q [N,nc,H,W] -> the q of each pixel's given class [N,H,W], 0 where the pixel is not valid."""
    valid = valid_of(target, nc, ignore)
    idx = torch.where(valid, target.long(), torch.zeros_like(target.long()))
    return torch.where(valid, q.gather(1, idx.unsqueeze(1))[:, 0], torch.zeros_like(idx))


def count_qsum(selfq, target, nc, ignore, finite=None):
    """-> (count [nc], qsum [nc]) over the valid (and finite) pixels, by bincount."""
    keep = valid_of(target, nc, ignore) if finite is None else valid_of(target, nc, ignore) & finite
    t = target.long()[keep]
    count = torch.bincount(t, minlength=nc)
    qsum = torch.zeros(nc, dtype=torch.int64).index_add_(0, t, selfq[keep])
    return count, qsum


def thresholds(count, qsum):
    """ceil(qsum / count) in Python integers; 65536 where the class has no pixel."""
    out = []
    for n, s in zip(torch.as_tensor(count).tolist(), torch.as_tensor(qsum).tolist()):
        out.append(Q_ONE if n == 0 else (s + n - 1) // n)
    return out


def confident(q, thr):
    """q [N,nc,H,W] int64, thr nc ints -> bool [N,nc,H,W]: q_c >= thr[c]."""
    return q >= torch.tensor(thr, dtype=torch.int64).reshape(1, -1, 1, 1)


def suggest_from(q, thr, logits):
    """The confident class with the largest logit, ties to the lowest class; nc where none is confident."""
    nc = q.shape[1]
    inside = confident(q, thr)
    masked = torch.where(inside, logits.double(), torch.full_like(logits.double(), float("-inf")))
    best = masked.max(1, keepdim=True)[0]
    idx = torch.arange(nc).reshape(1, -1, 1, 1).expand_as(masked)
    first = torch.where(inside & (masked == best), idx, torch.full_like(idx, nc)).min(1)[0]
    return first


def near_tie_confident(logits, S, inside, gamma_k):
    """``head_cases.near_tie``'s rule on the confident classes: pixels whose two largest logits among
    them lie within 2 gamma_k S (the larger S of the two).  Fewer than two confident classes: no tie."""
    masked = torch.where(inside, logits, torch.full_like(logits, float("-inf")))
    top, idx = masked.topk(2, dim=1)
    bound = 2 * gamma_k * S.gather(1, idx).max(1)[0]
    two = inside.sum(1) >= 2
    gap = torch.where(two, top[:, 0] - top[:, 1], torch.full_like(top[:, 0], float("inf")))
    return gap <= bound


def joint_of(target, suggest, nc, ignore, finite=None):
    """suggest: int map with nc for "none" -> int64 [nc, nc + 1] over the valid (and finite) pixels."""
    keep = valid_of(target, nc, ignore) if finite is None else valid_of(target, nc, ignore) & finite
    t, s = target.long()[keep], suggest.long()[keep]
    return torch.bincount(t * (nc + 1) + s, minlength=nc * (nc + 1)).reshape(nc, nc + 1)


def issues_of(target, suggest, nc, ignore, finite=None):
    keep = valid_of(target, nc, ignore) if finite is None else valid_of(target, nc, ignore) & finite
    return keep & (suggest.long() != nc) & (suggest.long() != target.long())


def per_image_of(target, suggest, nc, ignore, finite=None):
    """-> int64 [N, nc, 2]: the valid pixels and the issues per image and given class."""
    keep = valid_of(target, nc, ignore) if finite is None else valid_of(target, nc, ignore) & finite
    issue = issues_of(target, suggest, nc, ignore, finite)
    out = torch.zeros(target.shape[0], nc, 2, dtype=torch.int64)
    for n in range(target.shape[0]):
        out[n, :, 0] = torch.bincount(target[n].long()[keep[n]], minlength=nc)
        out[n, :, 1] = torch.bincount(target[n].long()[issue[n]], minlength=nc)
    return out


def calibrated(joint, count):
    """Northcutt's eq. 2-3 as Fractions -> (Q [nc][nc], noise_given [nc], noise_missed [nc], issues)."""
    J = torch.as_tensor(joint).tolist()
    n = torch.as_tensor(count).tolist()
    nc = len(n)
    scaled = []
    for i in range(nc):
        row = sum(J[i][:nc])
        scaled.append([Fraction(J[i][j] * n[i], row) if row else Fraction(0) for j in range(nc)])
    total = sum(sum(r) for r in scaled)
    Q = [[v / total if total else Fraction(0) for v in r] for r in scaled]
    given = [sum(Q[i]) for i in range(nc)]
    true = [sum(Q[i][j] for i in range(nc)) for j in range(nc)]
    noise_given = [1 - Q[i][i] / given[i] if given[i] else Fraction(0) for i in range(nc)]
    noise_missed = [1 - Q[j][j] / true[j] if true[j] else Fraction(0) for j in range(nc)]
    issues = sum(Q[i][j] for i in range(nc) for j in range(nc) if i != j) * total
    return Q, noise_given, noise_missed, issues


def apply_ref(target, suggest, selfq, nc, ignore, none_id, mode, max_q, drop_id):
    """Pixel by pixel over flat maps -> dict of out, mask and the counters (tensors / ints).
    mode: "prune" or "relabel"; suggest holds none_id where nothing is suggested."""
    tg, sg, sq = target.reshape(-1).tolist(), suggest.reshape(-1).tolist(), selfq.reshape(-1).tolist()
    n = len(tg)
    out, mask = list(tg), [0] * n
    seen, acted, bad = [0] * nc, [[0] * nc for _ in range(nc)], 0
    for i in range(n):
        if tg[i] == ignore:
            continue
        if tg[i] >= nc:
            bad += 1
            continue
        seen[tg[i]] += 1
        if sg[i] == none_id or sg[i] >= nc or sg[i] == tg[i]:
            continue
        if sq[i] <= max_q[tg[i]]:
            mask[i] = 255
            out[i] = drop_id if mode == "prune" else sg[i]
            acted[tg[i]][sg[i]] += 1
        else:
            mask[i] = 128
    return {"out": torch.tensor(out, dtype=torch.uint8), "mask": torch.tensor(mask, dtype=torch.uint8),
            "seen": torch.tensor(seen), "acted": torch.tensor(acted), "bad_targets": bad}
