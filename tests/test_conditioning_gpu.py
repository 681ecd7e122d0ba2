"""GPU: the BatchNorm, loss and Adam kernels at trained-regime inputs (tests/conditioning_cases.py) against
fp64 references, with bounds that an fp32 E[x^2] - E[x]^2, a softmax without its max subtraction or a float
bias correction cannot meet (tests/test_conditioning_cpu.py shows that they cannot).

Every BatchNorm case asserts that the producer it names took the launch (ops.profile_begin / profile_end),
takes its reference from the fp32 tensor the launch itself stored, asserts the |mean| / std window on that
reference alone, and prints one ``CONDITIONING`` line of worst |err| / bound figures before it asserts."""
import pytest
import torch
import torch.nn.functional as F

from tests import conditioning_cases as CC
from tests import head_cases as HC
from tests import streaming_tiles as T
from tests.test_hip_parity import ATOL, RTOL, close, nchw, nhwc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return HC.device("conditioning")


def _worst(ratios):
    return {k: float(v.max()) for k, v in ratios.items()}


def _line(what, worst):
    print(f"CONDITIONING {what}: worst |err|/bound " + " ".join(f"{k} {v:.2g}" for k, v in worst.items()))


def _assert_within(what, worst):
    over = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not over, f"{what}: |err| / bound above 1: {over}"


# ------------------------------------------------------------------------------------------------
# 1. BatchNorm statistics, every producer
# ------------------------------------------------------------------------------------------------
def _geometry(ops, c, flip=False):
    taps = (ops._taps_1x3 if c.axis == "w" else ops._taps_3x1)(c.d, flip) + ([(0, 0, 1)] if c.adapter else [])
    return ops.make_geom(c.N, c.H, c.W, c.H, c.W, taps, c.C, c.H, c.W, c.C)


def _check_statistics(what, stored, run, gamma, beta):
    """``run(fin)`` -> (coef, rm, rv, nbt) of a launch from rm = rv = 0 with ops.BN_FIN = fin; ``stored``:
    the fp32 tensor whose statistics it took."""
    from mdil_ss_amd import ops
    n = stored.numel() // stored.shape[-1]
    mean, var, const = CC.ref_stats(stored)
    lo, hi = CC.check_window(mean, var, const)
    coef, rm, rv, nbt = run(True)
    ratios = CC.bn_forward_ratios(coef, rm, rv, int(nbt), gamma, beta, mean, var, n)
    ratios["var"], ratios["var_const"] = ratios["var"][~const], ratios["var"][const]
    ratios["rv"], ratios["rv_const"] = ratios["rv"][~const], ratios["rv"][const]
    worst = _worst(ratios)
    y = ops.bn_apply(stored, coef[2], coef[3], relu=False)
    worst["apply"] = CC.bn_apply_ratio(y, stored, coef, gamma, beta, mean, var)
    _line(f"{what} (|mean|/std {lo:.0f}..{hi:.0f})", worst)
    _assert_within(what, worst)
    assert ops.BN_FIN is True
    try:        # the stand-alone finalize launch: same device code, bit-identical
        ops.BN_FIN = False
        coef2, rm2, rv2, nbt2 = run(False)
    finally:
        ops.BN_FIN = True
    assert torch.equal(coef, coef2) and torch.equal(rm, rm2) and torch.equal(rv, rv2) and int(nbt2) == 1


@pytest.mark.parametrize("idx", range(len(CC.CONV_CASES)), ids=CC.CONV_IDS)
def test_fused_producer_statistics(dev, idx):
    """conv + bias -> train-mode statistics in the producing launch (sconv / wconv / w4conv epilogues; C = 16:
    c16conv, then csrc/bn.hip's remainder loop) on channels with |mean| / std ~ 2^10 and constant channels."""
    from mdil_ss_amd import ops
    c = CC.conv_case(idx)
    C = c.C
    if C != 16:
        fam = T.expected_family(C, 4 if c.adapter else 3, c.W if c.axis == "w" else c.H, c.d)
        assert fam == c.producer and c.npix % T.PX_PER_TILE[fam] != 0, "the case is about a ragged last tile"
    ops.invalidate_packs()
    try:
        t = {k: getattr(c, k).to(dev) for k in ("x", "x2", "w", "wa", "b", "b2", "gamma", "beta")}
        g = _geometry(ops, c)
        wp = ops.pack_pair(t["w"], t["wa"] if c.adapter else None, "fwd")
        out = torch.empty_like(t["x"])

        def run(fin):
            rm, rv = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
            nbt = torch.zeros((), dtype=torch.int64, device=dev)
            ret = []
            kinds = T.paths(lambda: ret.append(ops.tapconv_bn(
                g, C, C, t["x"], t["x2"] if c.adapter else None, wp, out, t["gamma"], t["beta"], rm, rv, nbt,
                bias=t["b"], bias2=t["b2"] if c.adapter else None)), 16)
            assert kinds == [c.producer], f"expected one {c.producer} launch, the library made {kinds}"
            return ret[0], rm, rv, nbt

        run(True)
        stored = out.clone()
        for ch, v in zip(CC.const_channels(C), CC.CONST_VALUES):
            assert bool((stored[..., ch] == v).all()), f"channel {ch} is not the constant {v}"
        _check_statistics(f"{c.producer} {CC.CONV_IDS[idx]}", stored, run, c.gamma, c.beta)
        assert torch.equal(out, stored)
    finally:
        ops.invalidate_packs()


@pytest.mark.parametrize("idx", range(len(CC.BN_CASES)), ids=CC.BN_IDS)
def test_standalone_statistics(dev, idx):
    """csrc/bn.hip::bn_stats_kernel with 9 rows per thread: the U = 8 batched main loop once, then the
    remainder loop once, at every channel count."""
    from mdil_ss_amd import ops
    c = CC.bn_case(idx)
    ipb = CC.bn_plan(c.npix, c.C)[2]
    assert ipb >= 9 and ipb % CC.BN_U != 0, ipb
    z, gamma, beta = c.z.to(dev), c.gamma.to(dev), c.beta.to(dev)

    def run(fin):
        rm, rv = torch.zeros(c.C, device=dev), torch.zeros(c.C, device=dev)
        nbt = torch.zeros((), dtype=torch.int64, device=dev)
        return ops.bn_train_stats(z, gamma, beta, rm, rv, nbt), rm, rv, nbt

    _check_statistics(f"bn.hip {CC.BN_IDS[idx]}", z, run, c.gamma, c.beta)


def _bnred_ids():
    return [i for i, (p, _, _) in enumerate(CC.CONV_CASES) if p != "c16conv"]


@pytest.mark.parametrize("idx", _bnred_ids(), ids=[CC.CONV_IDS[i] for i in _bnred_ids()])
def test_fused_backward_reductions(dev, idx):
    """The BNRED epilogues: dgrad launch that stores g = conv^T(..) * (gate > 0) and emits sum(g), sum(g xhat)
    through an ill-conditioned z; finalize + apply.  Set up as _bnred_form of test_streaming_multitile_gpu.py,
    with its tolerances."""
    from mdil_ss_amd import ops
    c = CC.conv_case(idx)
    C = c.C
    ops.invalidate_packs()
    try:
        coef_h = CC.coef_from_ref(c.z, c.gamma, c.beta)
        g64 = T.ref_conv3(c.gx.double(), c.w, c.d, c.axis, True)
        if c.adapter:
            g64 = g64 + T.ref_1x1(c.gx2.double(), c.wa, True)
        g64 = g64 * (c.gate > 0)
        gz64, dgamma, dbeta = CC.bn_backward_ref(g64, c.z, c.gamma, coef_h[0], coef_h[1])
        t = {k: getattr(c, k).to(dev) for k in ("gx", "gx2", "w", "wa", "gate", "z", "gamma", "beta")}
        coef = coef_h.to(dev)
        geom = _geometry(ops, c, flip=True)
        wp = ops._pack_pair_dgrad(t["w"], t["wa"] if c.adapter else None)
        out = torch.empty_like(t["gx"])
        ret = []
        kinds = T.paths(lambda: ret.append(ops.tapconv_bnred(geom, C, C, t["gx"], t["gx2"] if c.adapter else None,
                                                             wp, out, t["gate"], t["z"], coef)), 16)
        assert kinds == [c.producer], f"expected one {c.producer} launch, the library made {kinds}"
        assert ret[0] is not None
        g1, partial, nblk = ret[0]
        gz1, dg1, db1 = ops.bn_backward_partials(g1, t["z"], t["gamma"], t["beta"], coef, True, partial, nblk)
        what = f"{c.producer} {CC.CONV_IDS[idx]}"
        _print_backward(what, gz1, gz64, dg1, dgamma, db1, dbeta)
        close(g1, g64, rtol=RTOL, atol=ATOL, what=what + " g")
        close(gz1, gz64, rtol=1e-3, atol=1e-4, what=what + " gz")
        close(dg1, dgamma, rtol=1e-3, atol=1e-4, what=what + " dgamma")
        close(db1, dbeta, rtol=1e-3, atol=1e-4, what=what + " dbeta")
        # the route whose launch finalizes too
        sg, sb = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        out2 = torch.empty_like(out)
        g2, coef3, zero = ops.tapconv_bnred(geom, C, C, t["gx"], t["gx2"] if c.adapter else None, wp, out2, t["gate"],
                                            t["z"], coef, fin=(t["gamma"], sg, sb))
        gz2 = ops.bn_backward_apply(g2, t["z"], coef, coef3)
        assert zero == 0 and torch.equal(g1, g2) and torch.equal(gz1, gz2)
        close(sg, dgamma, rtol=1e-3, atol=1e-4, what=what + " dgamma (finalized by the launch)")
        close(sb, dbeta, rtol=1e-3, atol=1e-4, what=what + " dbeta (finalized by the launch)")
    finally:
        ops.invalidate_packs()


def _print_backward(what, gz, gz64, dg, dgamma, db, dbeta):
    def rel(a, b, rtol=1e-3, atol=1e-4):
        b = b.double()
        bound = atol * max(1e-30, float(b.abs().max())) + rtol * b.abs()
        return float(((a.detach().cpu().double() - b).abs() / bound).max())
    print(f"CONDITIONING backward {what}: worst |err|/bound gz {rel(gz, gz64):.3f} dgamma {rel(dg, dgamma):.3f} "
          f"dbeta {rel(db, dbeta):.3f}")


@pytest.mark.parametrize("idx", range(len(CC.BN_CASES)), ids=CC.BN_IDS)
def test_standalone_backward(dev, idx):
    """csrc/bn.hip::bn_bwd_reduce_kernel with 9 rows per thread (two U = 4 batches and one remainder row)
    through an ill-conditioned z."""
    from mdil_ss_amd import ops
    c = CC.bn_case(idx)
    assert CC.bn_plan(c.npix, c.C)[2] == 9
    coef_h = CC.coef_from_ref(c.z, c.gamma, c.beta)
    g64 = c.gy.double() * (c.relu_src > 0)
    gz64, dgamma, dbeta = CC.bn_backward_ref(g64, c.z, c.gamma, coef_h[0], coef_h[1])
    gz, dg, db = ops.bn_backward(c.gy.to(dev), c.relu_src.to(dev), None, c.z.to(dev), c.gamma.to(dev), c.beta.to(dev),
                                 coef_h.to(dev), True)
    what = f"bn.hip {CC.BN_IDS[idx]}"
    _print_backward(what, gz, gz64, dg, dgamma, db, dbeta)
    close(gz, gz64, rtol=1e-3, atol=1e-4, what=what + " gz")
    close(dg, dgamma, rtol=1e-3, atol=1e-4, what=what + " dgamma")
    close(db, dbeta, rtol=1e-3, atol=1e-4, what=what + " dbeta")


# ------------------------------------------------------------------------------------------------
# 2. losses in the confident regime
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", CC.LABEL_MAPS)
@pytest.mark.parametrize("draw", list(CC.LOGIT_DRAWS))
@pytest.mark.parametrize("nc", [20, 27])
def test_unfused_losses(dev, nc, draw, kind):
    """ops.cross_entropy2d / ops.kld_prob (csrc/loss.hip) on logits up to ~150 in magnitude, saturated teachers
    and (map b) an image of zero-weight labels only."""
    from mdil_ss_amd import ops
    s, t, pred = CC.loss_logits(nc, draw)
    lab, weight = CC.label_map(kind, pred, nc, 40 + nc), CC.class_weights(nc)
    if draw == "confident":
        assert float(s.max()) > 88.7
    s64 = s.double().requires_grad_(True)
    ce = CC.ce_ref(s64, lab, weight)
    gce, = torch.autograd.grad(ce, s64)
    kld = CC.kld_ref(s64, t.double())
    gkld, = torch.autograd.grad(kld, s64)

    sd = s.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    td = t.to(dev).contiguous(memory_format=torch.channels_last)
    ce_d = ops.cross_entropy2d(sd, lab.to(dev), weight.to(dev))
    dce, = torch.autograd.grad(ce_d, sd)
    kld_d = ops.kld_prob(sd, td)
    dkld, = torch.autograd.grad(kld_d, sd)
    ops.check_labels()
    ce, kld = ce.detach(), kld.detach()
    worst = {"ce": abs(float(ce_d.detach()) - float(ce)) / CC.ce_bound(s64.detach(), lab, weight, ce),
             "kld": abs(float(kld_d.detach()) - float(kld)) / CC.kld_bound(s64.detach(), t.double(), kld)}
    _line(f"loss.hip nc{nc} {draw} map {kind}", worst)
    assert bool(torch.isfinite(dce).all()) and bool(torch.isfinite(dkld).all())
    _assert_within(f"loss.hip nc{nc} {draw} map {kind}", worst)
    close(dce, gce, rtol=1e-4, atol=1e-5, what="d ce / d logits")
    close(dkld, gkld, rtol=1e-4, atol=1e-5, what="d kld / d logits")
    if kind == "b":
        assert bool((dce[0] == 0).all()), "image 0 carries no weight: its CE gradient rows must be exactly zero"


# (map b on the single-image shape would leave no pixel with a weight: torch returns NaN there too)
_HEAD = [(nc, shape, kind) for nc in (20, 27) for shape in CC.HEAD_SHAPES for kind in CC.LABEL_MAPS
         if CC.map_applies(kind, shape)]


@pytest.mark.parametrize("nc,shape,kind", _HEAD, ids=["nc%d-%dx%dx%d-%s" % ((nc,) + s + (k,)) for nc, s, k in _HEAD])
def test_fused_head_losses(dev, nc, shape, kind):
    """ops.head_ce / ops.head_kld (csrc/head.hip, 1-ulp hardware exp / log / rcp) with head weights and bias of
    student and teacher times 10."""
    from mdil_ss_amd import ops
    c = CC.head_case(nc, shape)
    pred = c.logits.argmax(1)
    lab, weight = CC.label_map(kind, pred, nc, 50 + nc + shape[1]), CC.class_weights(nc)
    x64, w64, b64 = (v.double().requires_grad_(True) for v in (c.x, c.w, c.b))
    logits = F.conv_transpose2d(x64, w64, b64, stride=2)
    ce = CC.ce_ref(logits, lab, weight)
    gce = torch.autograd.grad(ce, (x64, w64, b64), retain_graph=True)
    kld = CC.kld_ref(logits, c.tlogits)
    gkld = torch.autograd.grad(kld, (x64, w64, b64))

    def leaf(v, perm=False):
        return (nhwc(v) if perm else v.clone()).to(dev).requires_grad_(True)
    xd, wd, bd = leaf(c.x, True), leaf(c.w), leaf(c.b)
    ce_d = ops.head_ce(xd, wd, bd, lab.to(dev), weight.to(dev))
    dce = torch.autograd.grad(ce_d, (xd, wd, bd))
    xd2, wd2, bd2 = leaf(c.x, True), leaf(c.w), leaf(c.b)
    kld_d = ops.head_kld(xd2, wd2, bd2, nhwc(c.xt).to(dev), c.wt.to(dev), c.bt.to(dev))
    dkld = torch.autograd.grad(kld_d, (xd2, wd2, bd2))
    ops.check_labels()
    what = "head.hip nc%d %dx%dx%d map %s" % ((nc,) + shape + (kind,))
    ce, kld = ce.detach(), kld.detach()
    worst = {"ce": abs(float(ce_d.detach()) - float(ce)) / CC.ce_bound(logits.detach(), lab, weight, ce, c.S),
             "kld": abs(float(kld_d.detach()) - float(kld)) / CC.kld_bound(logits.detach(), c.tlogits, kld, c.S, c.tS)}
    _line(what, worst)
    for got in dce + dkld:
        assert bool(torch.isfinite(got).all())
    _assert_within(what, worst)
    for name, got, want, perm in (("gx", dce[0], gce[0], True), ("dw", dce[1], gce[1], False),
                                  ("db", dce[2], gce[2], False)):
        close(nchw(got) if perm else got, want, rtol=1e-3, atol=1e-4, what=f"{what} CE {name}")
    for name, got, want, perm, atol in (("gx", dkld[0], gkld[0], True, 1e-4), ("dw", dkld[1], gkld[1], False, 1e-4),
                                        ("db", dkld[2], gkld[2], False, 2e-4)):
        close(nchw(got) if perm else got, want, rtol=1e-3, atol=atol, what=f"{what} KLD {name}")
    if kind == "b":
        assert bool((dce[0][0] == 0).all()), "image 0 carries no weight: its feature gradient must be exactly zero"


# ------------------------------------------------------------------------------------------------
# 3. Adam, single steps from given states
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gs", CC.ADAM_SCALES)
@pytest.mark.parametrize("step", CC.ADAM_STEPS)
def test_adam_single_step(dev, step, gs):
    from mdil_ss_amd import ops
    p, g, m, v, reg = CC.adam_state()
    ref = CC.adam_ref(p, g, m, v, step, gs, **CC.ADAM)
    pd, md, vd = p.to(dev), m.to(dev), v.to(dev)
    ops.adam_step(pd, g.to(dev), md, vd, step, CC.ADAM["lr"], CC.ADAM["beta1"], CC.ADAM["beta2"], CC.ADAM["eps"],
                  weight_decay=CC.ADAM["weight_decay"], grad_scale=gs)
    got = pd.cpu(), md.cpu(), vd.cpu()
    assert all(bool(torch.isfinite(t).all()) for t in got)
    rp, rm, rv = CC.adam_ratios(*got, p, ref)
    worst = {f"{name}{k}": float(r[reg == k].max()) for name, r in (("p", rp), ("m", rm), ("v", rv)) for k in range(4)}
    _line(f"adam.hip step {step} grad_scale {gs} (by regime 0..3)", worst)
    _assert_within(f"adam step {step} grad_scale {gs}", worst)
