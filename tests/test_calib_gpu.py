"""GPU: the fused calibration kernel (mdil_ss_amd/ext/calib_head.hip) and the entry points over it
(mdil_ss_amd/calibrate.py), against the fp64 reference of tests/calib_reference.py:
``F.conv_transpose2d`` in double, ``log_softmax(l / T)``, then confidence, NLL, Brier score and entropy.

Inputs.  ``case(nc, shape, ignore_last)`` of tests/calib_reference.py: ``head_inputs`` of
tests/head_cases.py, the case of the predict suite (seed 10 nc + H), targets sampled per pixel from
softmax(l64 / 1.7) (seed 7 nc + W), about 2 % of them set to the ignore index (nc - 1 or 255) and,
with 255, about 1 % to an id out of range.  16 temperatures, geometric on [0.25, 4].
tests/test_calib_cpu.py checks on the CPU that the NLL of every case is unimodal in T and where its
minimum lies.

Tolerances, with S = max_c (|b| + sum |x| |w|) of the pixel and U = 2^-24:
    conf   K_CONF  U (1 + S / T)
    nll    K_NLL   U (1 + S / T) (1 + |nll64|)
    brier  K_BRIER U (1 + S / T) 2           (summed over the counted pixels for the sum)
    ent    K_ENT   U (1 + S / T) (1 + ent64) (summed likewise)
Each K is 4 x the worst per-pixel constant of the DENSE FP32 TORCH ROUTE on the same MI355X against
the same fp64 values over the 32 cases and 16 temperatures (stored fp32 logits from
``F.conv_transpose2d`` on the device, divided by T, ``log_softmax``, the formulas): the kernel's exp,
log and summation order differ from torch's by a few ulps per term, and the forms already scale with
the terms.  Measured (K_*_TORCH below; per case the tests print both routes' constants)."""
import functools
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

from tests import calib_reference as R
from tests import head_cases as HC
from tests.head_cases import CLASSES, SHAPES, U, as_bytes, host, nhwc, predict_labels

pytestmark = pytest.mark.gpu

MAX_EXCLUDED = 1e-3
TEMPS = tuple(0.25 * 16 ** (i / 15) for i in range(16))
# Worst per-pixel constants of the dense fp32 torch route measured on an MI355X over the 32 cases
# and 16 temperatures: conf 2.767 and nll 3.232 (nc 2, shape (3, 16, 48)), brier 2.920 (the same
# case, ignore 255), ent 4.754; per case 0.20 ... 2.77, 0.61 ... 3.23, 0.17 ... 2.92 and 0.22 ... 4.75.
# The kernel's own constants over the same cases: conf 0.17 ... 0.94, nll 0.47 ... 2.15; its Brier
# score and entropy are never stored per pixel: test_sums prints how far their sums are from fp64 as
# a share of the summed per-pixel tolerances.  DESIGN.md, "Calibration".
K_CONF_TORCH = 2.767
K_NLL_TORCH = 3.232
K_BRIER_TORCH = 2.920
K_ENT_TORCH = 4.754
K_CONF, K_NLL, K_BRIER, K_ENT = 4 * K_CONF_TORCH, 4 * K_NLL_TORCH, 4 * K_BRIER_TORCH, 4 * K_ENT_TORCH
IGNORES = (True, False)                              # the ignore index is nc - 1, or 255


@pytest.fixture(scope="module")
def dev():
    return HC.device("calibration")


@functools.lru_cache(maxsize=None)
def reference(nc, shape, ignore_last):
    """The fp64 reference of a case at the 16 temperatures, computed once and shared (never
    modified): conf, nll, brier, ent [16,N,2H,2W] (nll and brier 0 where not counted), label, near."""
    c = R.case(nc, shape, ignore_last)
    per_t = [R.stats64(c["logits"], c["target"], c["counted"], T) for T in TEMPS]
    near = HC.near_tie(*HC.head64(c["x"], c["w"], c["b"]), 17)
    scale = torch.stack([U * (1 + c["S"] / T) for T in TEMPS])
    out = {k: torch.stack([s[i] for s in per_t]) for i, k in ((0, "conf"), (2, "nll"), (3, "brier"), (4, "ent"))}
    out.update(label=c["logits"].max(1)[1], near=near, tol_conf=scale, tol_nll=scale * (1 + out["nll"].abs()),
               tol_brier=scale * 2, tol_ent=scale * (1 + out["ent"]))
    return out


def on(dev, c):
    return nhwc(c["x"]).to(dev), c["w"].to(dev), c["b"].to(dev), c["target"].to(dev)


def new_counters(dev, nc, shape, K, bins=15, class_hist=True, fill=0):
    from mdil_ss_amd.calibrate import workspace_bytes
    z = lambda *s: torch.full(s, fill, dtype=torch.int64, device=dev)  # noqa: E731
    c = {"hist": z(K, bins, 3), "nonfinite": z(K), "bad_targets": z(1),
         "sums": torch.full((K, 3), float(fill), dtype=torch.float64, device=dev),
         "workspace": torch.empty(workspace_bytes(*shape, nc, K) // 8, dtype=torch.float64, device=dev)}
    if class_hist:
        c["class_hist"] = z(nc, bins, 3)
    return c


def run(dev, c, temps=TEMPS, bins=15, class_temp=None, counters=None, calls=1, **over):
    """-> (maps, counters) on the host after ``calls`` calls into the same counters."""
    from mdil_ss_amd.calibrate import calib_head
    x, w, b, t = on(dev, c)
    x, w, b = over.get("x", x), over.get("w", w), over.get("b", b)
    for _ in range(calls):
        out = calib_head(x, w, b, t, temps, bins=bins, ignore_index=c["ignore"], class_temp=class_temp, label=True,
                         maps=True, counters=counters)
    torch.cuda.synchronize()
    return host(out), host(counters or {})


@functools.lru_cache(maxsize=None)
def full(dev, nc, shape, ignore_last):
    """The kernel's outputs for a case at the 16 temperatures, 15 bins, class_hist at temperature 0:
    (maps, counters after one call, counters after a second call); computed once, never modified."""
    c = R.case(nc, shape, ignore_last)
    counters = new_counters(dev, nc, shape, 16)
    out, once = run(dev, c, class_temp=0, counters=counters)
    out2, twice = run(dev, c, class_temp=0, counters=counters)
    assert all(torch.equal(as_bytes(out[k]), as_bytes(out2[k])) for k in out)
    return out, once, twice


def expected_hist(c, conf, label, bins, rows=None):
    """The histogram the library's rule gives for the kernel's own fp32 confidences [N,h,w] and labels:
    [bins,3], or with ``rows`` = nc one per predicted class [nc,bins,3]."""
    k = c["counted"]
    correct = (label.long() == c["target"].long())[k]
    if rows is None:
        return R.pack(conf[k], correct, bins, dtype=torch.float32)
    lab = label.long()[k]
    return torch.stack([R.pack(conf[k][lab == cl], correct[lab == cl], bins, dtype=torch.float32) for cl in range(rows)])


# ------------------------------------------------------------------------------------ 1. labels
@pytest.mark.parametrize("ignore_last", IGNORES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nc", CLASSES)
def test_labels_are_predict_heads_and_match_fp64(dev, nc, shape, ignore_last):
    c = R.case(nc, shape, ignore_last)
    ref = reference(nc, shape, ignore_last)
    out, _, _ = full(dev, nc, shape, ignore_last)
    assert torch.equal(out["label"], predict_labels(dev, c["x"], c["w"], c["b"]))
    HC.check_labels(out["label"], ref["label"], ref["near"], f"nc {nc} shape {shape}", HC.share(MAX_EXCLUDED))


# -------------------------------------------------------------------------------------- 2. maps
def constant(got, want, tol, mask=None):
    r = (got.double() - want).abs() / tol
    return (r if mask is None else r[mask.expand_as(r)]).max().item() if r.numel() else 0.0


def torch_route(dev, c):
    """The dense fp32 route on the device: stored fp32 logits, divided by T, log_softmax, the formulas
    -> dict of [16,N,2H,2W] maps on the host."""
    logits = F.conv_transpose2d(c["x"].to(dev), c["w"].to(dev), c["b"].to(dev), stride=2)
    t, k = c["target"].to(dev), c["counted"].to(dev)
    per_t = [R.stats64(logits, t, k, T) for T in TEMPS]
    return {name: torch.stack([s[i] for s in per_t]).cpu() for i, name in ((0, "conf"), (2, "nll"), (3, "brier"), (4, "ent"))}


@pytest.mark.parametrize("ignore_last", IGNORES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nc", CLASSES)
def test_maps_match_fp64(dev, nc, shape, ignore_last):
    c = R.case(nc, shape, ignore_last)
    ref = reference(nc, shape, ignore_last)
    out, _, _ = full(dev, nc, shape, ignore_last)
    conf, nll = out["conf"], out["nll"]
    assert conf.dtype == nll.dtype == torch.float32 and tuple(conf.shape) == tuple(nll.shape) == tuple(ref["conf"].shape)
    assert torch.isfinite(conf).all() and torch.isfinite(nll).all()
    assert (nll[:, ~c["counted"]] == 0).all() and (conf > 0).all() and (conf <= 1).all()
    t = torch_route(dev, c)
    k = c["counted"][None]
    mine = {"conf": constant(conf, ref["conf"], ref["tol_conf"]), "nll": constant(nll, ref["nll"], ref["tol_nll"], k)}
    theirs = {"conf": constant(t["conf"], ref["conf"], ref["tol_conf"]),
              "nll": constant(t["nll"], ref["nll"], ref["tol_nll"], k),
              "brier": constant(t["brier"], ref["brier"], ref["tol_brier"], k),
              "ent": constant(t["ent"], ref["ent"], ref["tol_ent"], k)}
    print(f"nc {nc} shape {shape} ignore {c['ignore']}: kernel conf {mine['conf']:.3f} nll {mine['nll']:.3f}; dense fp32 "
          f"torch route conf {theirs['conf']:.3f} nll {theirs['nll']:.3f} brier {theirs['brier']:.3f} ent {theirs['ent']:.3f}")
    assert mine["conf"] <= K_CONF and mine["nll"] <= K_NLL


# -------------------------------------------------------------------------------- 3. histograms
def check_counters(c, out, counters, bins, temps, class_temp, times=1):
    nc = c["w"].shape[1]
    hist = counters["hist"]
    assert hist.dtype == torch.int64 and tuple(hist.shape) == (len(temps), bins, 3)
    for k in range(len(temps)):
        assert torch.equal(hist[k], times * expected_hist(c, out["conf"][k], out["label"], bins)), k
    assert int(hist[:, :, 0].sum()) == times * len(temps) * int(c["counted"].sum())
    if class_temp is not None:
        want = expected_hist(c, out["conf"][class_temp], out["label"], bins, rows=nc)
        assert torch.equal(counters["class_hist"], times * want)
        assert torch.equal(counters["class_hist"].sum(0), hist[class_temp])
    assert (counters["nonfinite"] == 0).all()
    assert int(counters["bad_targets"]) == times * c["bad"]


@pytest.mark.parametrize("ignore_last", IGNORES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nc", CLASSES)
def test_histograms_are_the_binning_of_the_kernels_own_maps(dev, nc, shape, ignore_last):
    c = R.case(nc, shape, ignore_last)
    out, once, twice = full(dev, nc, shape, ignore_last)
    if not ignore_last:
        assert c["bad"] > 0 or c["target"].numel() < 50
    check_counters(c, out, once, 15, TEMPS, 0)
    check_counters(c, out, twice, 15, TEMPS, 0, times=2)      # a second add doubles every counter
    assert torch.equal(twice["sums"], 2 * once["sums"])       # ... and the sums: x + x is exact


@pytest.mark.parametrize("bins, temps, class_temp", [(1, TEMPS, 15), (32, TEMPS, 15), (15, (1.3,), 0), (15, TEMPS[:5], None)])
def test_histograms_at_other_bin_and_temperature_counts(dev, bins, temps, class_temp):
    nc, shape = 27, (3, 16, 48)
    c = R.case(nc, shape, False)
    out, counters = run(dev, c, temps, bins, class_temp, new_counters(dev, nc, shape, len(temps), bins, class_temp is not None))
    check_counters(c, out, counters, bins, temps, class_temp)
    base = full(dev, nc, shape, False)[0]
    assert torch.equal(out["label"], base["label"])
    if temps is TEMPS:
        assert torch.equal(as_bytes(out["conf"]), as_bytes(base["conf"]))


# -------------------------------------------------------------------------------------- 4. sums
def check_nll_sums(c, out, counters, K, times=1, exact=True):
    """sums[k][0] against the fp64 sum of the kernel's own nll map over the counted pixels: an fp64
    summation of n terms in any order is within n 2^-53 sum |v| of the exact sum (``math.fsum``);
    with ``exact=False`` the reference is torch's own fp64 sum, which has the same bound, so twice that."""
    for k in range(K):
        v = out["nll"][k][c["counted"]].double()
        n = v.numel()
        ref = math.fsum(v.tolist()) if exact else v.sum().item()
        bound = (1 if exact else 2) * n * 2.0 ** -53 * v.abs().sum().item()
        got = counters["sums"][k, 0].item()
        assert abs(got - times * ref) <= times * bound, (k, n, got, ref, bound)


@pytest.mark.parametrize("ignore_last", IGNORES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nc", CLASSES)
def test_sums(dev, nc, shape, ignore_last):
    c = R.case(nc, shape, ignore_last)
    ref = reference(nc, shape, ignore_last)
    out, once, _ = full(dev, nc, shape, ignore_last)
    sums = once["sums"]
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (16, 3)
    check_nll_sums(c, out, once, 16)
    k = c["counted"]
    worst = {}
    for j, name, K_ in ((1, "brier", K_BRIER), (2, "ent", K_ENT)):
        for i in range(16):
            v, tol = ref[name][i][k], ref["tol_" + name][i][k]
            exact = math.fsum(v.tolist())
            slack = v.numel() * 2.0 ** -53 * v.abs().sum().item()
            share = abs(sums[i, j].item() - exact) / tol.sum().item()
            worst[name] = max(worst.get(name, 0.0), share)
            assert abs(sums[i, j].item() - exact) <= K_ * tol.sum().item() + slack, (name, i, sums[i, j].item(), exact)
    print(f"nc {nc} shape {shape} ignore {c['ignore']}: |sum - fp64| / sum of tolerances at the worst temperature: "
          f"brier {worst['brier']:.3f} ent {worst['ent']:.3f}")


# ------------------------------------------------------------------------------- 5. determinism
def test_two_calls_and_a_side_stream_give_the_same_bytes(dev):
    nc, shape = 27, (3, 16, 48)
    c = R.case(nc, shape, True)
    first_out, first_c, _ = full(dev, nc, shape, True)
    second_out, second_c = run(dev, c, class_temp=0, counters=new_counters(dev, nc, shape, 16))
    third_out, third_c = HC.side_stream(lambda: run(dev, c, class_temp=0, counters=new_counters(dev, nc, shape, 16)))
    for out, cn in ((second_out, second_c), (third_out, third_c)):
        for k in first_out:
            assert torch.equal(as_bytes(out[k]), as_bytes(first_out[k])), k
        for k in first_c:
            assert torch.equal(as_bytes(cn[k]), as_bytes(first_c[k])), k


# ------------------------------------------------------------- 6. NULL outputs and guard bands
@pytest.mark.parametrize("shape", ((1, 1, 1), (1, 9, 7), (3, 16, 48)))
def test_null_outputs_and_guard_bands_stay_untouched(dev, shape):
    """One 0xA5-filled arena [guard | label | guard | conf | guard | nll | guard] and counters
    pre-filled with 7: maps that are not asked for keep their bytes, nothing lands outside the maps,
    counters that are not passed keep theirs and the others gain exactly what a call adds."""
    import ctypes as C
    from mdil_ss_amd import _calib_lib
    lib = _calib_lib.load()
    nc, K = 27, 16
    c = R.case(nc, shape, True)
    N, H, W = shape
    npx = N * 4 * H * W
    base, added, _ = full(dev, nc, shape, True)
    sizes = {"label": npx, "conf": 4 * K * npx, "nll": 4 * K * npx}
    x, w, b, tgt = on(dev, c)
    temps = (C.c_float * K)(*TEMPS)
    names = ("hist", "class_hist", "sums", "nonfinite", "bad_targets")
    for maps, passed in (((), ()), (("label",), ("bad_targets",)), (("conf",), ("hist", "nonfinite")),
                         (("nll",), ("class_hist", "sums")), (tuple(sizes), names)):
        arena = HC.Arena(dev, sizes)
        cn = new_counters(dev, nc, shape, K, fill=7)
        p = lambda k: arena.ptr(k) if k in maps else None               # noqa: E731
        q = lambda k: cn[k].data_ptr() if k in passed else None         # noqa: E731
        rc = lib.mdil_calib_head(x.data_ptr(), w.data_ptr(), b.data_ptr(), N, H, W, nc, tgt.data_ptr(), c["ignore"], temps,
                                 K, 15, 0 if "class_hist" in passed else -1, p("label"), p("conf"), p("nll"),
                                 *(q(k) for k in names), cn["workspace"].data_ptr(), cn["workspace"].numel() * 8,
                                 torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.mdil_calib_last_error()
        torch.cuda.synchronize()
        arena.read()
        cn = host(cn)
        arena.assert_untouched(maps, (maps, passed))
        for k in maps:
            assert torch.equal(arena.cut(k), as_bytes(base[k]).reshape(-1)), k
        for k in names:
            want = 7 + added[k] if k in passed else torch.full_like(cn[k], 7)
            assert torch.equal(cn[k], want.to(cn[k].dtype)), (k, maps, passed)


# ------------------------------------------------------------------------------- 7. grid stride
def test_grid_stride_loop_past_the_grid_bound(dev):
    """The grid is bounded at 512 work-groups of 256 feature pixels; 1 x 257 x 511 = 131,327 of them
    is the smallest odd-sized grid that sends pixels (255) round the loop a second time.  Two
    classes and three temperatures keep the fp64 reference cheap."""
    nc, shape, temps = 2, (1, 257, 511), (0.5, 1.0, 2.0)
    assert shape[1] * shape[2] > 512 * 256 and (shape[1] - 2) * shape[2] < 512 * 256
    c = R.case(nc, shape, False)
    out, counters = run(dev, c, temps, 15, 1, new_counters(dev, nc, shape, 3))
    assert torch.equal(out["label"], predict_labels(dev, c["x"], c["w"], c["b"]))
    assert c["bad"] > 0
    check_counters(c, out, counters, 15, temps, 1)
    check_nll_sums(c, out, counters, 3, exact=False)
    for i, T in enumerate(temps):
        conf64, _, nll64, _, _ = R.stats64(c["logits"], c["target"], c["counted"], T)
        scale = U * (1 + c["S"] / T)
        assert constant(out["conf"][i], conf64, scale) <= K_CONF
        assert constant(out["nll"][i], nll64, scale * (1 + nll64.abs()), c["counted"]) <= K_NLL


# -------------------------------------------------------------------------- 8. NaN and inf logits
def test_nan_and_inf_logits_are_counted_and_not_binned(dev):
    from mdil_ss_amd.calibrate import CalibrationMeter
    nc, shape = 20, (2, 12, 20)
    c = R.case(nc, shape, False)
    clean, clean_c, _ = full(dev, nc, shape, False)
    # one NaN feature: every logit of its four output pixels is NaN -> class 0, as torch.max says
    xn = c["x"].clone()
    xn[1, 5, 7, 9] = float("nan")
    out, cn = run(dev, c, class_temp=0, counters=new_counters(dev, nc, shape, 16), x=nhwc(xn).to(dev))
    hit = torch.zeros_like(c["counted"])
    hit[1, 14:16, 18:20] = True
    lost = int((hit & c["counted"]).sum())
    assert lost > 0
    assert (out["label"][hit] == 0).all() and torch.equal(out["label"][~hit], clean["label"][~hit])
    assert torch.isnan(out["conf"][:, hit]).all()
    assert torch.equal(as_bytes(out["conf"][:, ~hit]), as_bytes(clean["conf"][:, ~hit]))
    assert (cn["nonfinite"] == lost).all()
    assert (cn["hist"][:, :, 0].sum(1) == int(c["counted"].sum()) - lost).all()
    assert int(cn["class_hist"][:, :, 0].sum()) == int(c["counted"].sum()) - lost
    for k in range(16):
        keep = c["counted"] & ~hit
        conf = out["conf"][k]
        correct = (out["label"].long() == c["target"].long())[keep]
        assert torch.equal(cn["hist"][k], R.pack(conf[keep], correct, 15, dtype=torch.float32))
    # an infinite logit of class 7 (its bias) at every pixel: the label is 7, nothing can be binned
    bi = c["b"].clone()
    bi[7] = float("inf")
    out, cn = run(dev, c, counters=new_counters(dev, nc, shape, 16, class_hist=False), b=bi.to(dev))
    assert (out["label"] == 7).all() and (cn["nonfinite"] == int(c["counted"].sum())).all() and (cn["hist"] == 0).all()
    # NaN logits at classes 7 and 12 only: the first of them wins everywhere
    bn = c["b"].clone()
    bn[7] = bn[12] = float("nan")
    assert (run(dev, c, b=bn.to(dev))[0]["label"] == 7).all()
    x, w, b, t = on(dev, c)
    meter = CalibrationMeter(nc, TEMPS, 15, c["ignore"])
    salted = t.clone()
    salted[t == R.OUT_OF_RANGE] = c["ignore"]
    meter.add(nhwc(xn).to(dev), w, b, target=salted)
    with pytest.raises(RuntimeError, match="non-finite NLL"):
        meter.host()
    meter = CalibrationMeter(nc, TEMPS, 15, c["ignore"])
    meter.add(x, w, b, target=t)
    with pytest.raises(RuntimeError, match=f"{c['bad']} target pixels are outside"):
        meter.host()


# ----------------------------------------------------------------------- 9. the fit on the device
def test_fit_on_the_device(dev):
    """Three rounds of 16 temperatures through a CalibrationMeter: T* within two cells of the last
    grid (a factor 1.0033^2) of the dense fp64 minimiser on the same logits -- the NLL difference of
    neighbouring cells there is of the order of the fp32 rounding per pixel, so one cell of slack on
    each side is a condition, not a measurement -- and (3 w, 3 b) gives 3 T* within the same slack."""
    from mdil_ss_amd.calibrate import CalibrationMeter, fit_temperature
    nc, shape = 20, (3, 16, 48)
    c = R.case(nc, shape, True)
    x, w, b, t = on(dev, c)
    best = R.dense_minimiser(c["logits"], c["target"], c["counted"])

    def fit(scale, lo, hi):
        def nll_of(temps):
            meter = CalibrationMeter(nc, temps, 15, c["ignore"])
            meter.add(x, w * scale, b * scale, target=t)
            return meter.host()["sums"][:, 0].tolist()
        return fit_temperature(nll_of, lo=lo, hi=hi, rounds=3)

    one, three = fit(1.0, 0.25, 4.0), fit(3.0, 0.75, 12.0)
    cell = 16 ** ((2 / 15) ** 2 / 15)
    print(f"fit on the device: T* {one['temperature']:.6f} (fp64 {best:.6f}), with 3 w, 3 b {three['temperature']:.6f}; "
          f"cell {one['cell']:.6f}")
    assert one["cell"] == pytest.approx(cell, rel=1e-9) and 1.0032 < cell < 1.0034
    assert abs(math.log(one["temperature"] / best)) <= 2 * math.log(cell)
    assert abs(math.log(three["temperature"] / (3 * best))) <= 2 * math.log(cell)
    assert len(one["trace"]) == 48


# -------------------------------------------------------------------- 10. the shipped forward
@pytest.fixture(scope="module")
def models(dev):
    return HC.teacher_student(dev)


@pytest.mark.parametrize("which", (0, 1))
def test_agrees_with_the_shipped_forward(dev, models, which):
    """``CalibrationMeter.add(model, images, task, target)`` is ``calib_head`` on ``model.features``,
    and its NLL sum at T = 1 is ``F.cross_entropy`` of the model's stored logits, in double, within
    the summed tolerance of the NLL map."""
    from mdil_ss_amd.calibrate import CalibrationMeter, calib_head
    from oracle import fixtures as fx
    model = models[which]
    images, _ = fx.make_batch(2, 64, 128, 20, seed=100)
    images = images.to(dev)
    target = torch.randint(0, 20, (2, 64, 128), generator=torch.Generator().manual_seed(3), dtype=torch.uint8).to(dev)
    with torch.no_grad():
        logits = model(images, 0).double()
        feat = model.features(images, 0).contiguous()
        w, b = (t.detach() for t in model.head_params(0))
    a, bm = CalibrationMeter(20, [1.0, 2.0], 15, 19, 0), CalibrationMeter(20, [1.0, 2.0], 15, 19, 0)
    out_a = a.add(model, images, 0, target=target, label=True, maps=True)
    out_b = bm.add(feat, w, b, target=target, label=True, maps=True)
    direct = calib_head(feat, w, b, target, [1.0, 2.0], ignore_index=19, label=True, maps=True)
    torch.cuda.synchronize()
    for k in out_a:
        assert torch.equal(as_bytes(out_a[k]), as_bytes(out_b[k])) and torch.equal(as_bytes(out_a[k]), as_bytes(direct[k])), k
    ha, hb = a.host(), bm.host()
    assert all(torch.equal(as_bytes(ha[k]), as_bytes(hb[k])) for k in ha)
    counted = target != 19
    per_pixel = F.cross_entropy(logits, target.long(), reduction="none")[counted]
    S = F.conv_transpose2d(feat.double().permute(0, 3, 1, 2).abs(), w.double().abs(), b.double().abs(), stride=2).max(1)[0]
    bound = (K_NLL * U * (1 + S[counted]) * (1 + per_pixel.abs())).sum().item()
    want = per_pixel.sum().item()
    got = ha["sums"][0, 0].item()
    report = a.report()
    print(f"shipped path: NLL sum {got:.9g} (cross_entropy {want:.9g}), |difference| / bound {abs(got - want) / bound:.3f}")
    assert abs(got - want) <= bound
    assert report["temperatures"][0]["pixels"] == int(counted.sum()) and len(report["class_ece"]) == 20
    assert report["temperatures"][0]["nll"] == pytest.approx(want / int(counted.sum()), rel=1e-5)


# ------------------------------------------------------------------------------------- 11. CLI
def test_cli_end_to_end(dev, models, tmp_path):
    """--synthetic 2 at 64 x 128 with --fit --out --json, in-process: every field of the report, an
    NLL at the fitted temperature that is not above the one at T = 1, a reliability diagram that
    opens, and the same numbers bit for bit when no feature is kept on the device."""
    from PIL import Image
    from mdil_ss_amd import calibrate as K
    _, student = models
    ckpt = tmp_path / "model.pth.tar"
    HC.save_checkpoint(student, ckpt)
    base = ["--state", str(ckpt), "--num-classes", "20", "20", "--task", "0", "--synthetic", "2", "--height", "64",
            "--width", "128", "--fit"]
    first = K.main(K.build_parser().parse_args(base + ["--out", str(tmp_path / "o"), "--json", str(tmp_path / "a.json")]))
    second = K.main(K.build_parser().parse_args(base + ["--feature-cache-gb", "0", "--json", str(tmp_path / "b.json")]))
    a, b = json.load(open(tmp_path / "a.json")), json.load(open(tmp_path / "b.json"))
    assert json.loads(json.dumps(first)) == a and json.loads(json.dumps(second)) == b
    assert (a["dataset"], a["task"], a["images"], a["classes"], a["bins"]) == ("synthetic", 0, 2, 20, 15)
    t1, fitted = a["report_t1"]["temperatures"][0], a["report_scaled"]["temperatures"][0]
    assert t1["temperature"] == 1.0 and fitted["temperature"] == a["fit"]["temperature"]
    lo, hi = a["fit"]["bracket"]
    assert lo < a["fit"]["temperature"] < hi and len(a["fit"]["trace"]) == 64
    for row in (t1, fitted):
        assert row["pixels"] == t1["pixels"] > 0 and len(row["reliability"]) == 15
        assert all(row[k] is not None and math.isfinite(row[k]) for k in ("accuracy", "ece", "mce", "nll", "brier", "entropy"))
    assert fitted["nll"] <= t1["nll"]
    for rep in (a["report_t1"], a["report_scaled"]):
        assert len(rep["class_ece"]) == 20 and rep["classwise_ece"] is not None
    assert (a["cache"]["mode"], b["cache"]["mode"]) == ("features", "recompute")
    assert a["cache"]["bytes"] == 2 * (32 * 64 * 16 * 4 + 64 * 128) and b["cache"]["bytes"] == 0
    with Image.open(os.path.join(tmp_path, "o", "reliability.png")) as im:
        assert im.mode == "RGB" and im.size == (640, 360)
    assert a["written"] == [os.path.join(str(tmp_path / "o"), "reliability.png")]
    for k in ("report_t1", "fit", "report_scaled", "images", "classes", "bins"):
        assert a[k] == b[k], k
