"""CPU: the bounds of tests/conditioning_cases.py have teeth.  fp32 emulations of the forms the kernels
document (chunked two-pass + Chan merge; softmax with its max subtracted; Adam with host-side double bias
corrections) pass them; the forms a kernel could slide into without any N(0, 1) test noticing (fp32
E[x^2] - E[x]^2, exp without the max) fail them on the very same draws.  Every precondition that the GPU
cases make on their reference alone is checked here for the committed seeds, and the bytes of every draw
are pinned by tests/golden/conditioning_cases.json."""
import json
import os

import numpy as np
import pytest
import torch

from tests import conditioning_cases as CC
from tests import head_cases as HC
from tests import streaming_tiles as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conditioning_cases.json")
CHANNELS = CC.emulation_channels()


# ------------------------------------------------------------------------------------------------
# BatchNorm statistics
# ------------------------------------------------------------------------------------------------
def test_emulation_draws_have_the_stated_ratios():
    for (name, x), (n, r) in zip(CHANNELS, CC.EMULATION_DRAWS):
        mean, var, const = CC.ref_stats(x.reshape(-1, 1))
        assert x.numel() == n and not bool(const[0])
        assert 0.9 * r <= float(CC.cond_ratio(mean, var)[0]) <= 1.1 * r, name
    for (name, x), v in zip(CHANNELS[len(CC.EMULATION_DRAWS):], CC.CONST_VALUES):
        mean, var, const = CC.ref_stats(x.reshape(-1, 1))
        assert bool(const[0]) and float(var[0]) == 0.0 and float(mean[0]) == float(torch.tensor(v)), name


@pytest.mark.parametrize("k", CC.CHUNKINGS)
def test_chunked_two_pass_with_chan_merges_meets_the_bounds(k):
    worst = [0.0, 0.0, 0.0]
    for name, x in CHANNELS:
        mean, var = CC.emulate_chunked(x.numpy(), k)
        rm, rv = CC.stat_ratios(mean, var, x)
        assert rm <= 1.0 and rv <= 1.0, (name, k, rm, rv)
        m64, v64, _ = CC.ref_stats(x.reshape(-1, 1))
        r = float(CC.cond_ratio(m64, v64)[0])
        if r > 0:       # the model the bound scales: |dvar| / (r u var); the issue's emulation gave <= 0.4
            worst[2] = max(worst[2], abs(var - float(v64[0])) / (r * CC.U * float(v64[0])))
        else:
            assert 0.0 <= var <= 30 * (CC.U * float(m64[0])) ** 2, (name, k, var)
        worst[0], worst[1] = max(worst[0], rm), max(worst[1], rv)
    print(f"CONDITIONING emulation chunk {k}: worst |err|/bound mean {worst[0]:.3f} var {worst[1]:.3f}; "
          f"|dvar| / (r u var) {worst[2]:.3f}")
    assert worst[2] <= 0.4 * 2      # twice the recorded worst case; the bound itself leaves ten times


@pytest.mark.parametrize("naive", [CC.emulate_naive_sequential, CC.emulate_naive_pairwise, CC.emulate_naive_grouped],
                         ids=["sequential", "pairwise", "grouped"])
def test_naive_sum_of_squares_fails_the_variance_bound_on_every_draw(naive):
    """Exact by arithmetic, whatever the form, and therefore no failure to assert: the constant 64 = 2^6 (every
    partial sum of 64 and of 4096 is an fp32 number), and any constant under the full binary tree (equal
    addends double exactly at every level, and the zero padding adds nothing)."""
    lowest = float("inf")
    for name, x in CHANNELS:
        _, var = naive(x.numpy())
        _, rv = CC.stat_ratios(0.0, var, x)
        if name == "const64.0" or (name.startswith("const") and naive is CC.emulate_naive_pairwise):
            assert var == 0.0, (name, var)
            continue
        lowest = min(lowest, rv)
        assert rv > 1.0, f"{name}: the naive form is within the variance bound ({rv:.3f}): the bound has no teeth"
    print(f"CONDITIONING naive {naive.__name__}: lowest |dvar|/bound {lowest:.1f}")


def test_naive_variance_of_a_constant_channel_is_negative():
    _, var = CC.emulate_naive_sequential(np.full(1920, -3.7, np.float32))
    assert var < 0 and abs(var) > 0.1 * CC.BN_EPS, var          # a visible part of eps, below zero


def test_bn_plan_mirror_enters_the_batched_loop_once():
    for C, N, H, W in CC.BN_CASES:
        nblk, _, ipb = CC.bn_plan(N * H * W, C)
        assert ipb >= 9 and ipb % CC.BN_U != 0, (C, ipb)
        assert nblk > 200 and N * H * W * C * 4 <= 18 * 2 ** 20
        # the threshold of the batched loop: U rows per thread need more than (U - 1) * 256 block iterations
        ppi = CC.BN_T // (C // 4)
        assert CC.bn_plan(1792 * ppi, C)[2] == 7 and CC.bn_plan(1792 * ppi + 1, C)[2] == 8
    for _, (C, N, H, W, _, _), _ in CC.CONV_CASES:
        if C == 16:
            assert CC.bn_plan(N * H * W, C)[2] < CC.BN_U        # remainder loop only


def test_conv_cases_select_their_producer_and_end_in_a_ragged_tile():
    seen = set()
    for prod, (C, N, H, W, d, axis), adapter in CC.CONV_CASES:
        seen.add(prod)
        assert N == 2
        if C == 16:
            assert prod == "c16conv" and not adapter
            continue
        fam = T.expected_family(C, 4 if adapter else 3, W if axis == "w" else H, d)
        assert fam == prod, (prod, fam)
        assert (N * H * W) % T.PX_PER_TILE[fam] != 0
    assert seen == {"sconv", "wconv", "w4conv", "c16conv"}


def test_ill_conditioned_draws_are_inside_the_ratio_window():
    for idx in range(len(CC.BN_CASES)):
        c = CC.bn_case(idx)
        lo, hi = CC.check_window(*CC.ref_stats(c.z))
        assert 0.9 * 2 ** 10 <= lo <= hi <= 1.1 * 2 ** 10
    for idx in range(len(CC.CONV_CASES)):
        CC.check_window(*CC.ref_stats(CC.conv_case(idx).z))


def test_conv_outputs_are_inside_the_ratio_window():
    """fp64 conv of the forward draws: the stored tensor of the GPU case is this one up to the conv's own
    rounding, so the window the GPU test asserts on the stored tensor holds with room."""
    for idx, (_, (C, _, _, _, d, axis), adapter) in enumerate(CC.CONV_CASES):
        c = CC.conv_case(idx)
        y = T.ref_conv3(c.x.double(), c.w, d, axis) + c.b.double()
        if adapter:
            y = y + T.ref_1x1(c.x2.double(), c.wa) + c.b2.double()
        mean, var, const = CC.ref_stats(y.float())
        lo, hi = CC.check_window(mean, var, const)
        assert 1.1 * 2 ** 9 <= lo and hi <= 0.9 * 2 ** 11, (CC.CONV_IDS[idx], lo, hi)
        for ch, v in zip(CC.const_channels(C), CC.CONST_VALUES):
            assert float(mean[ch]) == float(torch.tensor(v))


def test_the_forward_check_rejects_a_naive_statistic():
    """``bn_forward_ratios`` on coefficients built from the fp64 statistics passes; with the naive variance
    of one channel it fails."""
    c = CC.bn_case(0)
    z = c.z[:, :8, :15].contiguous()                                  # 240 pixels are enough here
    n = z.numel() // c.C
    mean, var, _ = CC.ref_stats(z)
    coef = CC.coef_from_ref(z, c.gamma, c.beta)
    rm, rv = CC.BN_MOMENTUM * mean, CC.BN_MOMENTUM * var * n / (n - 1)
    good = CC.bn_forward_ratios(coef, rm.float(), rv.float(), 1, c.gamma, c.beta, mean, var, n)
    assert all(float(v.max()) <= 1.0 for v in good.values()), {k: float(v.max()) for k, v in good.items()}
    _, nv = CC.emulate_naive_pairwise(z[..., 0].reshape(-1).numpy())
    bad = coef.clone()
    bad[1, 0] = (nv + CC.BN_EPS) ** -0.5
    assert float(CC.bn_forward_ratios(bad, rm.float(), rv.float(), 1, c.gamma, c.beta, mean, var, n)["var"][0]) > 1.0


# ------------------------------------------------------------------------------------------------
# losses
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [20, 27])
def test_logit_draws_overflow_and_saturate(nc):
    s, t, pred = CC.loss_logits(nc, "confident")
    assert float(s.max()) > 88.7 and float(t.max()) > 88.7
    shifted = (t - t.amax(1, keepdim=True)).numpy()
    assert bool((np.exp(shifted.astype(np.float32)) == 0).any()), "no teacher class underflows"
    assert bool((torch.softmax(t.double(), 1) > 0).all()), "the fp64 reference must not underflow"
    sm = CC.loss_logits(nc, "moderate")[0]
    assert 25 < float(sm.max()) < 88.7
    weight = CC.class_weights(nc)
    assert float(weight[nc - 1]) == 0.0 and bool((weight[:-1] > 0).all())
    for kind in CC.LABEL_MAPS:
        lab = CC.label_map(kind, pred, nc, 40 + nc)
        assert lab.dtype == torch.int64 and 0 <= int(lab.min()) and int(lab.max()) < nc
        assert bool((lab == nc - 1).any()) and float(weight[lab][1].sum()) > 0
        assert bool((lab[0] == nc - 1).all()) == (kind == "b")
    for shape in CC.HEAD_SHAPES:
        c = CC.head_case(nc, shape)
        assert float(c.logits.abs().max()) > 25 and tuple(c.logits.shape) == (shape[0], nc, 2 * shape[1], 2 * shape[2])
    assert not CC.map_applies("b", (1, 9, 7)) and CC.map_applies("b", (3, 16, 48)) and CC.map_applies("a", (1, 9, 7))


@pytest.mark.parametrize("draw", list(CC.LOGIT_DRAWS))
@pytest.mark.parametrize("nc", [20, 27])
def test_cross_entropy_chain_in_fp32_meets_the_pixel_bound(nc, draw):
    s, _, pred = CC.loss_logits(nc, draw)
    rows = s.permute(0, 2, 3, 1).reshape(-1, nc)
    lab = CC.label_map("a", pred, nc, 40 + nc).reshape(-1)
    want = -torch.log_softmax(rows.double(), 1).gather(1, lab[:, None])[:, 0]
    got = torch.from_numpy(CC.emulate_ce_pixels(rows.numpy(), lab.numpy())).double()
    b = CC.pixel_bound(rows.double())
    ratio = float(((got - want).abs() / b).max())
    model = float(((got - want).abs() / (CC.U * (1 + rows.double().abs().amax(1)))).max())
    print(f"CONDITIONING emulation ce nc{nc} {draw}: worst |err|/b_p {ratio:.3f} ({model:.2f} u (1 + max|l|))")
    assert bool(torch.isfinite(got).all()) and ratio <= 1.0
    assert model <= 3.5 * 2          # twice the recorded worst case of the libm chain
    naive = CC.emulate_ce_pixels(rows.numpy(), lab.numpy(), subtract_max=False)
    assert bool(np.isfinite(naive).all()) == (draw == "moderate")    # scale 30: exp overflows without the max


def test_loss_bounds_reject_a_small_relative_error():
    """The value bounds scale with u times the logit magnitude, not with the loss: a kernel that is off by
    1e-4 (CE) / 1e-3 (KLD) of the loss itself fails them."""
    s, t, pred = CC.loss_logits(20, "confident")
    lab, w = CC.label_map("a", pred, 20, 60), CC.class_weights(20)
    ce, kld = CC.ce_ref(s.double(), lab, w), CC.kld_ref(s.double(), t.double())
    assert float(ce) > 1 and abs(float(kld)) > 1e-3
    assert CC.ce_bound(s.double(), lab, w, ce) < 1e-4 * float(ce)
    assert CC.kld_bound(s.double(), t.double(), kld) < 1e-3 * abs(float(kld))


# ------------------------------------------------------------------------------------------------
# Adam
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gs", CC.ADAM_SCALES)
@pytest.mark.parametrize("step", CC.ADAM_STEPS)
def test_adam_in_fp32_meets_the_bounds_and_a_float_bias_correction_does_not(step, gs):
    p, g, m, v, reg = CC.adam_state()
    assert [int((reg == r).sum()) for r in range(4)] == [25001, 25001, 25001, 25000]
    assert bool((p[reg != 2].abs() >= 0.01).all()) and bool((p[reg == 2] == 0).all())
    g32 = (g * gs).numpy().astype(np.float32)
    assert bool(((g32 * g32)[reg == 2] < 2.0 ** -126).all())          # g^2 underflows: zero or a denormal
    ref = CC.adam_ref(p, g, m, v, step, gs, **CC.ADAM)
    assert all(bool(torch.isfinite(t).all()) for t in ref[:4])
    rp, rm, rv = CC.adam_ratios(*CC.adam_emulate32(p, g, m, v, step, gs, **CC.ADAM), p, ref)
    worst = [[float(r[reg == k].max()) for k in range(4)] for r in (rp, rm, rv)]
    print(f"CONDITIONING emulation adam step {step} grad_scale {gs}: worst |err|/bound by regime p {worst[0]} "
          f"m {worst[1]} v {worst[2]}")
    assert max(map(max, worst)) <= 1.0, worst
    if step == 1000:
        # bias corrections formed in float: 0.999f^1000 is off by ~5e-5 relative, the update by ~1e-5 of itself --
        # ten times the 16 u it is allowed where |p| does not carry the bound (regime 2: p = 0)
        b1f, b2f = np.float32(CC.ADAM["beta1"]), np.float32(CC.ADAM["beta2"])
        bc1f = float(np.float32(1) - np.float32(b1f ** np.float32(step)))
        bc2f = float(np.float32(1) - np.float32(b2f ** np.float32(step)))
        upd = ref[3]
        upd_bad = upd * ((1 - 0.9 ** step) / bc1f) * np.sqrt(bc2f / (1 - 0.999 ** step))
        bound = (2 * CC.U * p.double().abs() + 16 * CC.U * upd.abs()).clamp_min(1e-300)
        assert float(((upd_bad - upd).abs() / bound)[reg == 2].min()) > 1.0


# ------------------------------------------------------------------------------------------------
# the bytes
# ------------------------------------------------------------------------------------------------
def test_draws_are_the_recorded_bytes():
    """A changed seed, shape or scale must not silently change what is tested."""
    want = json.load(open(GOLDEN))
    got = CC.digests()
    assert sorted(got) == sorted(k for k in want if k != "recorded_from")
    for section in got:
        assert got[section] == want[section], section
    assert HC.draw(20, (1, 9, 7), 9000 + HC.case_seed(20, (1, 9, 7)))[0].equal(CC.head_case(20, (1, 9, 7)).x)
