"""CPU reference of the pseudo-label add-on (include/mdil_pseudo.h), in plain torch: the
quantisation rule on a confidence tensor, the class-balanced threshold by a per-class ``torch.sort``
and the apply rule with its counters.  Nothing here shares code with mdil_ss_amd/pseudo.py."""
import math

import torch

Q_ONE = 65536


def quantise(conf):
    """q = min(65535, trunc(conf * 65536)) as int64; a NaN gives 0.  The scaling is exact in the
    tensor's own format (fp32 or fp64): a power of two."""
    v = conf * float(Q_ONE)
    return torch.where(torch.isnan(v), torch.zeros_like(v), v).floor().clamp(0, Q_ONE - 1).to(torch.int64)


def portions(portion, nc):
    return [float(portion)] * nc if isinstance(portion, (int, float)) else [float(p) for p in portion]


def sort_thresholds(label, q, nc, portion, floor=0.0):
    """thr_c = the k_c-th largest q among the pixels with label c, k_c = floor(p_c * n_c); k_c = 0
    gives 65536; then the floor.  -> (thr, k), two lists of nc ints."""
    label, q = label.reshape(-1).long(), q.reshape(-1).long()
    p = portions(portion, nc)
    fq = min(Q_ONE, math.ceil(floor * Q_ONE))
    thr, ks = [], []
    for c in range(nc):
        qs = torch.sort(q[label == c], descending=True)[0]
        k = math.floor(p[c] * qs.numel())
        ks.append(k)
        thr.append(max(Q_ONE if k == 0 else int(qs[k - 1]), fq))
    return thr, ks


def hist_level1(label, q, nc):
    label, q = label.reshape(-1).long(), q.reshape(-1).long()
    ok = label < nc
    return torch.bincount(label[ok] * 256 + (q[ok] >> 8), minlength=nc * 256).reshape(nc, 256)


def hist_level2(label, q, nc, sel):
    """-> (hist2 [nc,256], labels >= nc)."""
    label, q = label.reshape(-1).long(), q.reshape(-1).long()
    ok = label < nc
    s = torch.tensor(list(sel), dtype=torch.int64)
    hit = ok.clone()
    hit[ok] = (q[ok] >> 8) == s[label[ok]]
    return (torch.bincount(label[hit] * 256 + (q[hit] & 255), minlength=nc * 256).reshape(nc, 256),
            int((~ok).sum()))


def apply_rule(label, q, nc, thr, id_map=None, drop_id=255, target=None, ignore_index=-1):
    """-> dict: out u8 (label's shape), seen / kept i64 [nc], confusion i64 [nc,nc] over the kept
    pixels (row = target; zeros without a target), bad_targets over every pixel, bad_labels."""
    shape = label.shape
    label, q = label.reshape(-1).long(), q.reshape(-1).long()
    ok = label < nc
    safe = torch.where(ok, label, torch.zeros_like(label))
    keep = ok & (q >= torch.tensor(list(thr), dtype=torch.int64)[safe])
    ids = torch.arange(nc, dtype=torch.int64) if id_map is None else id_map.long()
    out = torch.where(keep, ids[safe], torch.full_like(label, int(drop_id))).to(torch.uint8).reshape(shape)
    res = {"out": out, "seen": torch.bincount(label[ok], minlength=nc), "kept": torch.bincount(label[keep], minlength=nc),
           "confusion": torch.zeros(nc, nc, dtype=torch.int64), "bad_targets": 0, "bad_labels": int((~ok).sum())}
    if target is not None:
        t = target.reshape(-1).long()
        counted = keep & (t < nc) & (t != ignore_index)
        res["confusion"] = torch.bincount(t[counted] * nc + label[counted], minlength=nc * nc).reshape(nc, nc)
        res["bad_targets"] = int(((t >= nc) & (t != ignore_index)).sum())
    return res
