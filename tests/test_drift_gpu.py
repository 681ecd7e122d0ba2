"""GPU: the fused twin-head kernel (mdil_ss_amd/ext/drift_head.hip) and the entry points over it
(mdil_ss_amd/drift.py), against an fp64 reference on the CPU: ``F.conv_transpose2d`` in double for
both models, ``log_softmax``, then ``kl = sum_c p^A_c (z^A_c - z^B_c)`` and
``kd = sum_c p^A_c (z^A_c - p^B_c)``.

Inputs.  A is ``head_inputs(nc, shape)`` of tests/head_cases.py, the case of the predict suite (seed
10 nc + H); the same draw with seed 10 nc + H + 1000 gives (x', w', b'); B = (x + 0.1 x', w + 0.05 w',
b).  No pixel of A or B is an fp32 near-tie (the 2 gamma_17 S rule of tests/head_cases.py) in the 16
cases, 8 of 2.1 M are at (1, 513, 1023) with two classes, and A and B disagree on 3 to 13 % of the
pixels.

Tolerance of kl and kd.  Per pixel ``K 2^-24 (1 + S^A + S^B) (1 + share)``, S^M the largest
``|b| + sum |x| |w|`` over the classes of the pixel, share = ``sum_c p^A_c |z^A_c - z^B_c|`` for kl
and ``sum_c p^A_c |z^A_c - p^B_c|`` for kd.  K is 4 x the worst constant of the DENSE FP32 TORCH
ROUTE on the same MI355X against the same fp64 values over the 16 cases (stored fp32 logits from
``F.conv_transpose2d`` on the device, ``log_softmax``, the formulas): the kernel's exp / log and
summation order differ from torch's by a few ulps per term, and the form already scales with the
terms.  Measured (K_KL_TORCH, K_KD_TORCH below; per case the tests print both routes' constants)."""
import functools
import glob
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import head_cases as HC
from tests.head_cases import CLASSES, SHAPES, U, as_bytes, host, make_target, nhwc, predict_labels

pytestmark = pytest.mark.gpu

MAX_EXCLUDED = 1e-3
LIMIT = HC.share(MAX_EXCLUDED)
# Worst constants of the dense fp32 torch route measured on an MI355X over the 16 cases: kl 3.034
# (nc 32, shape (2, 12, 20)), kd 1.703 (nc 27, shape (2, 12, 20)); per case 0.17 ... 3.03 and
# 0.11 ... 1.70.  The kernel's own kl constant over the same cases was 0.34 ... 5.03 (worst at nc 27,
# shape (2, 12, 20)); its kd is never stored per pixel: the sum over a case was off by at most 0.105 of
# the summed per-pixel tolerances (the torch route's sum: 0.100).  DESIGN.md, "Drift".
K_KL_TORCH = 3.034
K_KD_TORCH = 1.703
K_KL, K_KD = 4 * K_KL_TORCH, 4 * K_KD_TORCH


@pytest.fixture(scope="module")
def dev():
    return HC.device("drift")


@functools.lru_cache(maxsize=None)
def pair(nc, shape):
    """-> ((xa, wa, ba), (xb, wb, bb)), x as [N,16,H,W]; never modified."""
    xa, wa, ba = HC.head_inputs(nc, shape)
    xp, wp, _ = HC.draw(nc, shape, HC.case_seed(nc, shape) + 1000)
    return (xa, wa, ba), (xa + 0.1 * xp, wa + 0.05 * wp, ba.clone())


def reference_head(x, w, b):
    """-> (fp64 logits [N,nc,2H,2W], S [N,2H,2W], fp64 argmax, near-tie mask)."""
    logits, S = HC.head64(x, w, b)
    return logits, S.max(1)[0], logits.max(1)[1], HC.near_tie(logits, S, 17)


def divergences(la, lb):
    """(kl, kd, share of kl, share of kd) per pixel from two logit tensors [N,nc,h,w], in their dtype."""
    za, zb = F.log_softmax(la, 1), F.log_softmax(lb, 1)
    pa, pb = za.exp(), zb.exp()
    return ((pa * (za - zb)).sum(1), (pa * (za - pb)).sum(1), (pa * (za - zb).abs()).sum(1),
            (pa * (za - pb).abs()).sum(1))


def reference_of(a, b):
    la, Sa, label_a, near_a = reference_head(*a)
    lb, Sb, label_b, near_b = reference_head(*b)
    kl, kd, share_kl, share_kd = divergences(la, lb)
    scale = U * (1 + Sa + Sb)
    return dict(label_a=label_a, label_b=label_b, near_a=near_a, near_b=near_b, kl=kl, kd=kd,
                tol_kl=scale * (1 + share_kl), tol_kd=scale * (1 + share_kd))


@functools.lru_cache(maxsize=None)
def reference(nc, shape):
    """The fp64 reference of a case, computed once and shared (never modified)."""
    return reference_of(*pair(nc, shape))


def on(dev, a, b):
    return (nhwc(a[0]).to(dev), a[1].to(dev), a[2].to(dev), nhwc(b[0]).to(dev), b[1].to(dev), b[2].to(dev))


def new_counters(dev, nc, shape, scored, fill=0):
    from mdil_ss_amd.drift import workspace_bytes
    z = lambda *s: torch.full(s, fill, dtype=torch.int64, device=dev)  # noqa: E731
    c = {"transition": z(nc, nc), "bad_targets": z(1), "sums": torch.full((nc + 1,), float(fill), dtype=torch.float64,
                                                                         device=dev),
         "workspace": torch.empty(workspace_bytes(*shape, nc) // 8, dtype=torch.float64, device=dev)}
    if scored:
        c.update(confusion_a=z(nc, nc), confusion_b=z(nc, nc), outcome=z(nc, 4))
    return c


def run(dev, a, b, target=None, ignore=-1, counters=None, calls=1):
    """-> (maps, counters) on the host after ``calls`` calls into the same counters."""
    from mdil_ss_amd.drift import drift_head
    args = on(dev, a, b)
    tgt = None if target is None else target.to(dev)
    for _ in range(calls):
        out = drift_head(*args, target=tgt, ignore_index=ignore, labels=True, kl=True, change=True, counters=counters)
    torch.cuda.synchronize()
    return host(out), host(counters or {})


@functools.lru_cache(maxsize=None)
def plain(dev, nc, shape):
    """The kernel's outputs for a case without a target, computed once and shared (never modified)."""
    a, b = pair(nc, shape)
    return run(dev, a, b, counters=new_counters(dev, nc, shape, False))


# ------------------------------------------------------------------------------------ 1. labels
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nc", CLASSES)
def test_labels_are_predict_heads_and_match_fp64(dev, nc, shape):
    a, b = pair(nc, shape)
    ref = reference(nc, shape)
    out, _ = plain(dev, nc, shape)
    assert torch.equal(out["label_a"], predict_labels(dev, *a))
    assert torch.equal(out["label_b"], predict_labels(dev, *b))
    HC.check_labels(out["label_a"], ref["label_a"], ref["near_a"], f"nc {nc} shape {shape} A", LIMIT)
    HC.check_labels(out["label_b"], ref["label_b"], ref["near_b"], f"nc {nc} shape {shape} B", LIMIT)
    differ = (out["label_a"] != out["label_b"]).double().mean().item()
    print(f"nc {nc} shape {shape}: A and B disagree on {differ:.2%} of the pixels")


# ---------------------------------------------------------------------------- 2. ties and NaNs
def test_ties_go_to_the_lowest_class_in_b(dev):
    """Classes 3 and 11 of B with bit-identical weights and bias tie exactly at every pixel; with
    the largest bias they are also the winners almost everywhere.  11 must never be written."""
    a, (x, w, b) = pair(20, (2, 12, 20))
    w, b = w.clone(), b.clone()
    b[3] = b.max() + 1.0
    w[:, 11], b[11] = w[:, 3], b[3]
    out, _ = run(dev, a, (x, w, b))
    assert not (out["label_b"] == 11).any() and (out["label_b"] == 3).double().mean() > 0.5
    assert torch.equal(out["label_a"], plain(dev, 20, (2, 12, 20))[0]["label_a"])
    w[:, 11] = 0                      # without the twin class the same labels must come out
    b[11] = -1e30
    assert torch.equal(run(dev, a, (x, w, b))[0]["label_b"], out["label_b"])


def test_nan_logits_give_the_first_nan_class_in_b(dev):
    a, (x, w, b) = pair(20, (2, 12, 20))
    clean = plain(dev, 20, (2, 12, 20))[0]
    # one NaN feature: every logit of its four output pixels is NaN -> class 0, as torch.max says
    xn = x.clone()
    xn[1, 5, 7, 9] = float("nan")
    out, _ = run(dev, a, (xn, w, b))
    hit = torch.zeros_like(out["label_b"], dtype=torch.bool)
    hit[1, 14:16, 18:20] = True
    assert (out["label_b"][hit] == 0).all() and torch.equal(out["label_b"][~hit], clean["label_b"][~hit])
    assert torch.equal(out["label_a"], clean["label_a"])
    assert torch.isnan(out["kl"][hit]).all() and torch.equal(out["kl"][~hit], clean["kl"][~hit])
    # NaN logits at classes 7 and 12 only (their bias): the first of them wins everywhere
    bn = b.clone()
    bn[7] = bn[12] = float("nan")
    assert (run(dev, a, (x, w, bn))[0]["label_b"] == 7).all()


# ---------------------------------------------------------------------------------- 3. identity
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nc", CLASSES)
def test_a_model_does_not_drift_from_itself(dev, nc, shape):
    a, _ = pair(nc, shape)
    out, c = run(dev, a, a, counters=new_counters(dev, nc, shape, False))
    assert (out["kl"] == 0.0).all() and (out["change"] == 0).all()
    assert torch.equal(out["label_a"], out["label_b"])
    t = c["transition"]
    assert int(t.sum()) == out["kl"].numel() and torch.equal(t, torch.diag(t.diagonal()))
    assert (c["sums"][:nc] == 0.0).all() and int(c["bad_targets"]) == 0


# ------------------------------------------------------------------------------------ 4. KL map
def constant(got, want, tol):
    return ((got.double() - want).abs() / tol).max().item()


def torch_route(dev, a, b):
    """The dense fp32 route on the device: stored fp32 logits, log_softmax, the formulas -> (kl, kd) on the host."""
    la = F.conv_transpose2d(a[0].to(dev), a[1].to(dev), a[2].to(dev), stride=2)
    lb = F.conv_transpose2d(b[0].to(dev), b[1].to(dev), b[2].to(dev), stride=2)
    kl, kd, _, _ = divergences(la, lb)
    return kl.cpu(), kd.cpu()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nc", CLASSES)
def test_kl_map_matches_fp64(dev, nc, shape):
    ref = reference(nc, shape)
    out, _ = plain(dev, nc, shape)
    kl = out["kl"]
    assert kl.dtype == torch.float32 and tuple(kl.shape) == tuple(ref["kl"].shape) and torch.isfinite(kl).all()
    t_kl, t_kd = torch_route(dev, *pair(nc, shape))
    k = constant(kl, ref["kl"], ref["tol_kl"])
    print(f"nc {nc} shape {shape}: kl constant {k:.3f} (dense fp32 torch route {constant(t_kl, ref['kl'], ref['tol_kl']):.3f}; "
          f"kd of that route {constant(t_kd, ref['kd'], ref['tol_kd']):.3f}); mean kl {ref['kl'].mean().item():.4f}")
    assert k <= K_KL


# ------------------------------------------------------------------------------------ 5. counts
def expected(nc, label_a, label_b, target, ignore):
    """The counters and the change map from the kernel's own labels and the target, by bincount."""
    la, lb = label_a.reshape(-1).long(), label_b.reshape(-1).long()
    if target is None:
        change = (la != lb).to(torch.uint8)
        return {"transition": torch.bincount(la * nc + lb, minlength=nc * nc).reshape(nc, nc), "bad_targets": 0,
                "change": change.reshape(label_a.shape), "counted": torch.ones_like(la, dtype=torch.bool), "cls": la}
    t = target.reshape(-1).long()
    counted = (t < nc) & (t != ignore)
    ar, br = la == t, lb == t
    change = torch.full_like(t, 4)
    change[~ar & ~br & (la == lb)] = 3
    change[~ar & br] = 2
    change[ar & ~br] = 1
    change[ar & br] = 0
    change[~counted] = 255
    k = counted
    count = lambda i, j, n: torch.bincount(i[k] * n + j[k], minlength=nc * n).reshape(nc, n)  # noqa: E731
    return {"transition": count(la, lb, nc), "confusion_a": count(t, la, nc), "confusion_b": count(t, lb, nc),
            "outcome": count(t, change.clamp(max=3), 4), "bad_targets": int(((t >= nc) & (t != ignore)).sum()),
            "change": change.to(torch.uint8).reshape(label_a.shape), "counted": counted, "cls": t}


def check_counts(nc, out, c, want, times=1):
    assert torch.equal(out["change"], want["change"])
    for k in ("transition", "confusion_a", "confusion_b", "outcome"):
        if k in want:
            assert c[k].dtype == torch.int64 and torch.equal(c[k], times * want[k]), k
    assert int(c["bad_targets"]) == times * want["bad_targets"]
    assert int(c["transition"].sum()) == times * int(want["counted"].sum())


def check_class_sums(nc, out, c, want, times=1, exact=True):
    """sums[c] against the fp64 sum of the kernel's own kl map over the counted pixels of class c:
    an fp64 summation of n terms in any order is within n 2^-53 sum |kl| of the exact sum
    (``math.fsum``); with ``exact=False`` the reference is torch's own fp64 sum, which has the same
    bound, so twice that."""
    kl = out["kl"].reshape(-1).double()
    for cl in range(nc):
        v = kl[want["counted"] & (want["cls"] == cl)]
        n = v.numel()
        ref = math.fsum(v.tolist()) if exact else v.sum().item()
        bound = (1 if exact else 2) * n * 2.0 ** -53 * v.abs().sum().item()
        assert abs(c["sums"][cl].item() - times * ref) <= times * bound, (cl, n, c["sums"][cl].item(), ref, bound)


TARGETS = (None, "last", 255)


@functools.lru_cache(maxsize=None)
def scored(dev, nc, shape, ignore):
    """-> (target, ignore index, maps, counters after one call, counters after a second call)."""
    a, b = pair(nc, shape)
    ign = -1 if ignore is None else nc - 1 if ignore == "last" else 255
    N, H, W = shape
    target = None if ignore is None else make_target(nc, (N, 2 * H, 2 * W), ign, seed=nc + H)
    counters = new_counters(dev, nc, shape, target is not None)
    out, once = run(dev, a, b, target, ign, counters)
    out2, twice = run(dev, a, b, target, ign, counters)
    assert all(torch.equal(out[k], out2[k]) for k in out)
    return target, ign, out, once, twice


@pytest.mark.parametrize("ignore", TARGETS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nc", CLASSES)
def test_counts_are_bincounts_of_the_kernels_own_labels(dev, nc, shape, ignore):
    target, ign, out, once, twice = scored(dev, nc, shape, ignore)
    base = plain(dev, nc, shape)[0]
    assert torch.equal(out["label_a"], base["label_a"]) and torch.equal(out["label_b"], base["label_b"])
    assert torch.equal(out["kl"].view(torch.int32), base["kl"].view(torch.int32))   # at every pixel, counted or not
    want = expected(nc, out["label_a"], out["label_b"], target, ign)
    if target is not None:
        assert want["bad_targets"] > 0 or target.numel() < 50
    check_counts(nc, out, once, want)
    check_counts(nc, out, twice, want, times=2)           # a second add doubles every counter
    assert torch.equal(twice["sums"], 2 * once["sums"])   # ... and the sums: x + x is exact


# -------------------------------------------------------------------------------------- 6. sums
@pytest.mark.parametrize("ignore", TARGETS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nc", CLASSES)
def test_sums(dev, nc, shape, ignore):
    target, ign, out, once, _ = scored(dev, nc, shape, ignore)
    ref = reference(nc, shape)
    want = expected(nc, out["label_a"], out["label_b"], target, ign)
    assert once["sums"].dtype == torch.float64 and tuple(once["sums"].shape) == (nc + 1,)
    check_class_sums(nc, out, once, want)
    # kd over ALL pixels, against the fp64 reference: the per-pixel tolerance summed, plus the fp64 summation's own
    kd, tol = ref["kd"].reshape(-1), ref["tol_kd"].reshape(-1)
    got, exact = once["sums"][nc].item(), math.fsum(kd.tolist())
    slack = kd.numel() * 2.0 ** -53 * kd.abs().sum().item()
    print(f"nc {nc} shape {shape}: kd sum {got:.9g} (fp64 {exact:.9g}), |difference| / sum of tolerances "
          f"{abs(got - exact) / tol.sum().item():.3f}")
    assert abs(got - exact) <= K_KD * tol.sum().item() + slack


# ------------------------------------------------------------------------------- 7. determinism
@pytest.mark.parametrize("ignore", (None, "last"))
def test_two_calls_and_a_side_stream_give_the_same_bytes(dev, ignore):
    nc, shape = 27, (3, 16, 48)
    a, b = pair(nc, shape)
    target, ign, first_out, first_c, _ = scored(dev, nc, shape, ignore)
    second_out, second_c = run(dev, a, b, target, ign, new_counters(dev, nc, shape, target is not None))
    third_out, third_c = HC.side_stream(
        lambda: run(dev, a, b, target, ign, new_counters(dev, nc, shape, target is not None)))
    for out, c in ((second_out, second_c), (third_out, third_c)):
        for k in first_out:
            assert torch.equal(as_bytes(out[k]), as_bytes(first_out[k])), k
        for k in first_c:
            assert torch.equal(as_bytes(c[k]), as_bytes(first_c[k])), k


@pytest.mark.parametrize("shape", ((1, 1, 1), (1, 9, 7), (3, 16, 48)))
def test_null_outputs_and_guard_bands_stay_untouched(dev, shape):
    """One 0xA5-filled arena [guard | label_a | guard | label_b | guard | kl | guard | change | guard]
    and counters pre-filled with 7: maps that are not asked for keep their bytes, nothing lands
    outside the maps, counters that are not passed (or have no target to count) keep theirs."""
    from mdil_ss_amd import _drift_lib
    lib = _drift_lib.load()
    nc = 27
    a, b = pair(nc, shape)
    N, H, W = shape
    npx = N * 4 * H * W
    target, _, _, scored_c, _ = scored(dev, nc, shape, "last")
    base, plain_c = plain(dev, nc, shape)
    sizes = {"label_a": npx, "label_b": npx, "kl": 4 * npx, "change": npx}
    args = on(dev, a, b)
    tgt = target.to(dev)
    names = ("transition", "confusion_a", "confusion_b", "outcome", "bad_targets", "sums")
    for maps, with_target, passed in (((), False, ()), (("label_b",), False, ("bad_targets",)),
                                      (("kl", "change"), False, ("transition", "sums", "bad_targets")),
                                      (tuple(sizes), True, names)):
        arena = HC.Arena(dev, sizes)
        c = new_counters(dev, nc, shape, True, fill=7)
        p = lambda k: arena.ptr(k) if k in maps else None               # noqa: E731
        q = lambda k: c[k].data_ptr() if k in passed else None          # noqa: E731
        rc = lib.mdil_drift_head(*(t.data_ptr() for t in args), N, H, W, nc, tgt.data_ptr() if with_target else None,
                                 nc - 1, p("label_a"), p("label_b"), p("kl"), p("change"), *(q(k) for k in names),
                                 c["workspace"].data_ptr(), c["workspace"].numel() * 8,
                                 torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.mdil_drift_last_error()
        torch.cuda.synchronize()
        arena.read()
        c = host(c)
        arena.assert_untouched(maps, (maps, with_target))
        cut = arena.cut
        for k in ("label_a", "label_b"):
            if k in maps:
                assert torch.equal(cut(k), base[k].reshape(-1))
        if "kl" in maps:
            assert torch.equal(cut("kl"), as_bytes(base["kl"]).reshape(-1))
        want = expected(nc, base["label_a"], base["label_b"], target if with_target else None, nc - 1)
        if "change" in maps:
            assert torch.equal(cut("change"), want["change"].reshape(-1))
        for k in names[:4]:
            assert torch.equal(c[k], want[k] + 7 if k in passed else torch.full_like(c[k], 7)), k
        assert int(c["bad_targets"]) == 7 + (want["bad_targets"] if "bad_targets" in passed else 0)
        # sums[c] += the folded total, which is what a call into zeroed sums leaves there
        added = (scored_c if with_target else plain_c)["sums"] if "sums" in passed else torch.zeros(nc + 1).double()
        assert torch.equal(c["sums"], 7.0 + added)


# ------------------------------------------------------------------------------- 8. grid stride
def test_grid_stride_loop_past_the_grid_bound(dev):
    """The grid is bounded at 2048 work-groups of 256 feature pixels; 1 x 513 x 1023 = 524,799 of
    them is the smallest odd-sized grid that sends pixels (511) round the loop a second time.
    Two classes keep the fp64 reference cheap."""
    nc, shape = 2, (1, 513, 1023)
    assert shape[0] * shape[1] * shape[2] > 2048 * 256
    a, b = pair(nc, shape)
    target = make_target(nc, (1, 1026, 2046), 255, seed=3)
    out, c = run(dev, a, b, target, 255, new_counters(dev, nc, shape, True))
    assert torch.equal(out["label_a"], predict_labels(dev, *a)) and torch.equal(out["label_b"], predict_labels(dev, *b))
    for m, which in ((a, "a"), (b, "b")):
        _, _, label, near = reference_head(*m)
        HC.check_labels(out["label_" + which], label, near, f"nc {nc} shape {shape} {which.upper()}", LIMIT)
    want = expected(nc, out["label_a"], out["label_b"], target, 255)
    assert want["bad_targets"] > 0
    check_counts(nc, out, c, want)
    check_class_sums(nc, out, c, want, exact=False)


# --------------------------------------------------------------------- 9. the shipped forward
@pytest.fixture(scope="module")
def models(dev):
    return HC.teacher_student(dev)


def test_agrees_with_the_shipped_forward(dev, models):
    """``compare`` through a DriftMeter against the stored fp32 logits of both models: the KD loss is
    ``KLDivLoss()(softmax(student(x, 0)), softmax(teacher(x, 0)))`` within 1e-3 |v| + 1e-6, smoke()'s
    tolerance for this quantity; the labels are the stored logits' argmax outside the near-ties."""
    from mdil_ss_amd.drift import DriftMeter
    from oracle import fixtures as fx
    teacher, student = models
    images, _ = fx.make_batch(2, 64, 128, 20, seed=100)
    images = images.to(dev)
    with torch.no_grad():
        lt, ls = teacher(images, 0).float(), student(images, 0).float()
        want = torch.nn.KLDivLoss()(F.softmax(ls, 1), F.softmax(lt, 1)).item()
        ft, fs = teacher.features(images, 0), student.features(images, 0)
    meter = DriftMeter(20, -1)
    out = meter.add(teacher, student, images, 0, labels=True)
    torch.cuda.synchronize()
    report = meter.report()
    print(f"shipped path: kd_loss {report['kd_loss']:.9g} (KLDivLoss {want:.9g}), agreement {report['agreement']:.4f}")
    assert report["pixels"] == report["counted_pixels"] == 2 * 64 * 128
    assert abs(report["kd_loss"] - want) <= 1e-3 * abs(want) + 1e-6
    for model, feat, logits, key in ((teacher, ft, lt, "label_a"), (student, fs, ls, "label_b")):
        w, b = (t.detach().cpu() for t in model.head_params(0))
        _, S = HC.head64(feat.cpu().permute(0, 3, 1, 2), w, b)
        near = HC.near_tie(logits.cpu().double(), S, 17)
        HC.check_labels(out[key].cpu(), logits.max(1)[1].cpu(), near, f"shipped path {key}", LIMIT)
    assert 0 < report["agreement"] < 1


# ------------------------------------------------------------------------------------- 10. CLI
def test_cli_end_to_end(dev, models, tmp_path):
    """--synthetic 3 at 64 x 128 with --score --out --labels --json, in-process: twelve PNGs of the
    right size and mode that hold what ``compare`` returns, and a JSON file that holds what
    ``drift_report`` gives for the same counters."""
    from PIL import Image
    from mdil_ss_amd import drift as D
    from mdil_ss_amd.dataset import ProceduralSeg
    teacher, student = models
    out, report_file = tmp_path / "maps", tmp_path / "report.json"
    for model, name in ((teacher, "before.pth.tar"), (student, "after.pth.tar")):
        HC.save_checkpoint(model, tmp_path / name)
    report = D.main(D.build_parser().parse_args(
        ["--before", str(tmp_path / "before.pth.tar"), "--before-num-classes", "20", "--after",
         str(tmp_path / "after.pth.tar"), "--after-num-classes", "20", "20", "--task", "0", "--synthetic", "3",
         "--height", "64", "--width", "128", "--score", "--out", str(out), "--labels", "--json", str(report_file)]))
    files = sorted(glob.glob(str(out / "*.png")))
    assert len(files) == 12 and sorted(report["written"]) == files
    ds = ProceduralSeg(3, 64, 128, 20, seed=12, domain=0)
    images = torch.stack([ds[i][0] for i in range(3)]).to(dev)
    target = torch.stack([ds[i][1][0] for i in range(3)]).to(torch.uint8).to(dev)
    meter = D.DriftMeter(20, 19)
    maps = host(meter.add(teacher, student, images, 0, target=target, labels=True, kl=True, change=True))
    want = {"change": torch.from_numpy(D.change_colours(maps["change"].numpy())),
            "kl": D.kl_bytes(maps["kl"], 1.0), "before_label": maps["label_a"], "after_label": maps["label_b"]}
    assert torch.equal(maps["change"] == 255, target.cpu() == 19) and (maps["change"] <= 4).any()
    for i in range(3):
        for kind, mode in (("change", "RGB"), ("kl", "L"), ("before_label", "L"), ("after_label", "L")):
            with Image.open(os.path.join(out, f"synthetic_{i:04d}_{kind}.png")) as im:
                assert im.size == (128, 64) and im.mode == mode, (kind, im.size, im.mode)
                assert torch.equal(torch.from_numpy(np.array(im)), want[kind][i]), (i, kind)
    mine = D.drift_report(20, pixels=3 * 64 * 128, ignore_index=19, **meter.host())
    assert mine["pixels"] == 3 * 64 * 128 and mine["counted_pixels"] == int((target != 19).sum())
    saved = json.load(open(report_file))
    for k, v in json.loads(json.dumps(mine)).items():
        assert saved[k] == v and json.loads(json.dumps(report[k])) == v, k
    assert (saved["dataset"], saved["task"], saved["images"]) == ("synthetic", 0, 3)
    assert len(saved["iou_before"]) == 19 and len(saved["forgotten"]) == 20
