"""GPU: the streaming C -> C convs (csrc/sconv.hip direct form, wconv.hip F(2,3), w4conv.hip F(4,3)) where
ONE WAVE RUNS SEVERAL TILES, against an fp64 reference.

The kernels are persistent (tests/streaming_tiles.py): on a 256-CU device a wave gets a second tile only
above 16,384 .. 131,072 pixels, depending on the form -- more than any shape of the other per-kernel parity
tests.  What runs only then: the operand ring refilled from the wave's NEXT tile under the current tile's
MFMAs and the A/B hand-over; the per-lane Welford summary (statistics form) and the reduction registers
(BatchNorm-backward and tail forms) carried across tiles; a ragged last tile that falls into a later round;
the per-image Dropout2d factor of the tail form on the division (non-power-of-two) index path.

Every case asserts its preconditions before it compares anything -- the expected kernel family took the
launch (ops.profile_begin / profile_end), max tiles per wave >= 2, uneven queues, a ragged last tile where
the case is about one -- and FAILS (never skips) when one does not hold."""
import ctypes
import functools
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import rap_oracle as O
from tests import helpers as Hh
from tests import streaming_tiles as T
from tests.test_hip_parity import ATOL, RTOL, _grad_check, close, nb_block_case, nchw, nhwc

gpu = pytest.mark.gpu
SENTINEL = 12345.5
EPS = 1e-3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _lib
    _lib.load()
    torch.set_num_threads(Hh.host_threads())
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------
# CPU: the helpers themselves
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis,d", [("w", 1), ("w", 2), ("h", 1), ("h", 2)])
def test_reference_conv_equals_conv2d(axis, d):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 8, 12, 5, generator=g, dtype=torch.float64)
    w = torch.randn(5, 5, *((3, 1) if axis == "h" else (1, 3)), generator=g, dtype=torch.float64)
    wa = torch.randn(5, 5, 1, 1, generator=g, dtype=torch.float64)
    pad, dil = ((d, 0), (d, 1)) if axis == "h" else ((0, d), (1, d))
    xr = nchw(x).requires_grad_(True)
    y = F.conv2d(xr, w, None, padding=pad, dilation=dil) + F.conv2d(xr, wa)
    torch.testing.assert_close(T.ref_conv3(x, w, d, axis) + T.ref_1x1(x, wa), nhwc(y.detach()), rtol=1e-13, atol=1e-13)
    go = torch.randn(2, 8, 12, 5, generator=g, dtype=torch.float64)
    y.backward(nchw(go))
    torch.testing.assert_close(T.ref_conv3(go, w, d, axis, True) + T.ref_1x1(go, wa, True), nhwc(xr.grad),
                               rtol=1e-13, atol=1e-13)


def test_tile_mirror_on_a_256_cu_device():
    """The thresholds of DESIGN.md's table and the tiles per wave of this module's cases, for 256 CUs; every
    tile of the pair / quad numbering holds exactly its 32 / 64 pixels (the last one the rest)."""
    tpw = lambda *a: T.tiles_per_wave(*a, cus=256)
    for kind, C, nt, plain, limit in [("sconv", 128, 3, True, 32768), ("sconv", 64, 3, True, 65536),
                                      ("wconv", 128, 3, True, 32768), ("wconv", 128, 4, True, 16384),
                                      ("wconv", 64, 3, True, 65536), ("w4conv", 128, 3, True, 32768),
                                      ("w4conv", 128, 4, False, 32768), ("w4conv", 64, 3, False, 65536),
                                      ("w4conv", 64, 3, True, 131072)]:
        assert tpw(kind, C, nt, limit, plain) == (1, 1) and tpw(kind, C, nt, limit + 4, plain) == (1, 2)
    assert tpw("w4conv", 128, 3, 73200, False) == tpw("w4conv", 128, 4, 73200, False) == (2, 3)
    assert tpw("wconv", 128, 3, 81000, True) == (2, 3) and tpw("wconv", 128, 4, 81000, True) == (4, 5)
    assert tpw("w4conv", 64, 3, 204000, False) == (3, 4) and tpw("w4conv", 64, 3, 204000, True) == (1, 2)
    assert tpw("sconv", 64, 4, 146340, True) == (2, 3)
    for kind, (N, H, W, d, axis) in [("w4conv", (2, 8, 24, 2, "w")), ("w4conv", (3, 16, 5, 2, "h")),
                                     ("wconv", (3, 6, 20, 1, "w")), ("wconv", (2, 12, 7, 3, "h")),
                                     ("sconv", (1, 7, 9, 1, "w"))]:
        tm = T.tile_map(kind, N, H, W, d, axis)
        cnt = torch.bincount(tm)
        px = T.PX_PER_TILE[kind]
        assert cnt.numel() == -(-N * H * W // px) and bool((cnt[:-1] == px).all()) and int(cnt.sum()) == N * H * W


# ------------------------------------------------------------------------------------------------
# per-launch forms against fp64
# ------------------------------------------------------------------------------------------------
# family, (C, N, H, W, d, axis), ragged last tile
CASES = [
    ("w4conv", (128, 3, 50, 488, 2, "w"), True),      # 73,200 px: division path, ragged
    ("w4conv", (128, 5, 64, 128, 4, "w"), False),     # 40,960 px: shift path, N not a power of two
    ("w4conv", (128, 3, 96, 136, 8, "h"), False),     # 39,168 px: division path along H
    ("w4conv", (64, 3, 136, 500, 1, "w"), False),     # 204,000 px: C=64 (the adapter launch goes to F(2,3))
    ("wconv", (128, 3, 100, 270, 2, "h"), True),      # 81,000 px
    ("wconv", (128, 6, 80, 160, 16, "w"), False),     # 76,800 px: the ensemble's 1.25 scale
    ("wconv", (64, 3, 150, 322, 1, "w"), True),       # 144,900 px
    ("sconv", (128, 3, 81, 300, 4, "w"), True),       # 72,900 px
    ("sconv", (128, 2, 135, 240, 1, "h"), False),     # 64,800 px: IDD-sized eval
    ("sconv", (64, 2, 271, 270, 1, "h"), True),       # 146,340 px
]
_IDS = ["%s-C%d-%dx%dx%d-d%d%s" % ((f,) + c) for f, c, _ in CASES]


def _rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@functools.lru_cache(maxsize=1)
def _case(idx):
    """Seeded inputs of a case (fp32, host) and, lazily, the fp64 convolutions every form shares."""
    fam, (C, N, H, W, d, axis), ragged = CASES[idx]
    c = types.SimpleNamespace(fam=fam, C=C, N=N, H=H, W=W, d=d, axis=axis, ragged=ragged, npix=N * H * W, memo={})
    kk = (3, 1) if axis == "h" else (1, 3)
    c.x, c.x2 = _rnd(N, H, W, C, seed=1), _rnd(N, H, W, C, seed=2)
    c.w, c.wa = _rnd(C, C, *kk, seed=3, scale=(1.0 / (3 * C)) ** 0.5), _rnd(C, C, 1, 1, seed=4, scale=(1.0 / C) ** 0.5)
    c.b, c.b2 = _rnd(C, seed=5, scale=0.1), _rnd(C, seed=6, scale=0.1)
    c.scale, c.shift = 1 + _rnd(C, seed=7, scale=0.1), _rnd(C, seed=8, scale=0.1)
    c.gamma, c.beta = 1 + _rnd(C, seed=9, scale=0.1), _rnd(C, seed=10, scale=0.1)
    c.res, c.gate = _rnd(N, H, W, C, seed=11), _rnd(N, H, W, C, seed=12)
    c.z = _rnd(N, H, W, C, seed=13) * 1.7 + 0.3
    return c


def _ref(c, what, adapter):
    """fp64: 'fwd' = conv(x) + b [+ adapter(x2) + b2]; 'dgrad' = conv^T(x) [+ adapter^T(x2)]."""
    key = (what, adapter)
    if key not in c.memo:
        tr = what == "dgrad"
        if (what, False) not in c.memo:
            y = T.ref_conv3(c.x.double(), c.w, c.d, c.axis, tr)
            c.memo[(what, False)] = y if tr else y + c.b.double()
        if adapter:
            y = c.memo[(what, False)] + T.ref_1x1(c.x2.double(), c.wa, tr)
            c.memo[key] = y if tr else y + c.b2.double()
    return c.memo[key]


class _Launcher:
    """One (case, adapter) on the device: geometry, packed weights, guarded outputs, the precondition
    checks of every launch and the comparison split by tile round."""

    def __init__(self, c, adapter, dev):
        from mdil_ss_amd import ops
        self.ops, self.c, self.adapter, self.dev = ops, c, adapter, dev
        self.ntaps = 4 if adapter else 3
        L = c.W if c.axis == "w" else c.H
        self.fam = T.expected_family(c.C, self.ntaps, L, c.d)
        want_fam = "wconv" if (c.fam == "w4conv" and c.C == 64 and adapter) else c.fam
        assert self.fam == want_fam, (self.fam, want_fam)       # C = 64 + adapter: mdil_w4conv_covers -> F(2,3)
        self.px = T.PX_PER_TILE[self.fam]
        if c.ragged:
            assert c.npix % self.px != 0, "the case is about a ragged last tile"
        taps = (ops._taps_1x3 if c.axis == "w" else ops._taps_3x1)
        ad = [(0, 0, 1)] if adapter else []
        mk = lambda t: ops.make_geom(c.N, c.H, c.W, c.H, c.W, t + ad, c.C, c.H, c.W, c.C)
        self.g_fwd, self.g_bwd = mk(taps(c.d)), mk(taps(c.d, True))
        self.t = {k: getattr(c, k).to(dev) for k in ("x", "x2", "w", "wa", "b", "b2", "scale", "shift", "gamma",
                                                      "beta", "res", "gate", "z")}
        t = self.t
        self.in1 = t["x2"] if adapter else None
        self.bias2 = t["b2"] if adapter else None
        self.wp_fwd = ops.pack_pair(t["w"], t["wa"] if adapter else None, "fwd")
        self.wp_bwd = ops._pack_pair_dgrad(t["w"], t["wa"] if adapter else None)
        self.tmap = T.tile_map(self.fam, c.N, c.H, c.W, c.d, c.axis)

    def tiles(self, plain):
        """(queues, tiles, (min, max) per wave) of a launch of this geometry; asserts several tiles per wave."""
        c = self.c
        nq, ntiles = T.tiling(self.fam, c.C, self.ntaps, c.npix, plain)
        lo, hi = T.tiles_per_wave(self.fam, c.C, self.ntaps, c.npix, plain)
        assert hi >= 2, f"{self.fam} C{c.C} {c.npix} px: one tile per wave only ({nq} queues, {ntiles} tiles)"
        assert lo < hi, f"{self.fam} C{c.C} {c.npix} px: even queues ({lo} tiles per wave everywhere)"
        return nq, ntiles, (lo, hi)

    def launch(self, fn):
        """fn(out) -> whatever the op returns.  ``out`` sits between two guard bands of one tile each."""
        c = self.c
        band = self.px * c.C
        buf = torch.full(((c.npix + 2 * self.px) * c.C,), SENTINEL, device=self.dev)
        out = buf[band:band + c.npix * c.C].view(c.N, c.H, c.W, c.C)
        ret = []
        kinds = T.paths(lambda: ret.append(fn(out)), 16)
        assert kinds == [self.fam], f"expected one {self.fam} launch, the library made {kinds}"
        assert bool((buf[:band] == SENTINEL).all()), "the launch wrote in front of its output"
        assert bool((buf[band + c.npix * c.C:] == SENTINEL).all()), "the launch wrote beyond its last valid pixel"
        return out, ret[0]

    def compare(self, got, want, form, plain, rtol=RTOL, atol=ATOL):
        """``close`` on the whole tensor; the same error measure split by tile round k = tile // (8 nq) and
        for the last (ragged) tile, so a failure names the round."""
        c = self.c
        nq, ntiles, tpw = self.tiles(plain)
        what = f"{form} [{self.fam} C{c.C} {c.N}x{c.H}x{c.W} d{c.d}{c.axis} adapter={self.adapter}] tiles/wave {tpw}"
        g64 = got.detach().cpu().double()
        bound = atol * max(1e-30, float(want.abs().max())) + rtol * want.abs()
        ratio = ((g64 - want).abs() / bound).reshape(c.npix, c.C).amax(1)
        rounds = self.tmap // (T.WAVES * nq)
        nr = int(rounds.max()) + 1
        assert nr == tpw[1]
        per_round = torch.zeros(nr, dtype=torch.float64).scatter_reduce(0, rounds, ratio, "amax", include_self=False)
        last = float(ratio[self.tmap == ntiles - 1].max())
        report = "  ".join(f"round {k}: {float(v):.3f}" for k, v in enumerate(per_round)) + f"  last tile: {last:.3f}"
        print(f"MULTITILE {what}: worst |err|/bound by {report}")
        try:
            close(got, want, rtol=rtol, atol=atol, what=what)
        except AssertionError as e:
            raise AssertionError(f"{e}\n  |err|/bound by tile round: {report}") from None
        assert float(per_round.max()) <= 1.0 and last <= 1.0, report


def _plain_forms(L):
    """Plain and epilogue-operand forms: bias; bias + ReLU; folded BN + residual + ReLU (the eval block's last
    launch); the two dgrad forms (mirrored taps): residual gated by a second operand, and the gate alone."""
    ops, c, t = L.ops, L.c, L.t
    C = c.C
    fwd, dg = _ref(c, "fwd", L.adapter), _ref(c, "dgrad", L.adapter)
    out, _ = L.launch(lambda o: ops.tapconv(L.g_fwd, C, C, t["x"], L.in1, L.wp_fwd, o, bias=t["b"], bias2=L.bias2))
    L.compare(out, fwd, "bias", True)
    out, _ = L.launch(lambda o: ops.tapconv(L.g_fwd, C, C, t["x"], L.in1, L.wp_fwd, o, bias=t["b"], bias2=L.bias2,
                                            relu=True))
    L.compare(out, fwd.relu(), "bias+relu", True)
    out, _ = L.launch(lambda o: ops.tapconv(L.g_fwd, C, C, t["x"], L.in1, L.wp_fwd, o, bias=t["b"], bias2=L.bias2,
                                            scale=t["scale"], shift=t["shift"], res=t["res"], relu=True))
    L.compare(out, (fwd * c.scale.double() + c.shift.double() + c.res.double()).relu(), "scale/shift+res+relu", False)
    out, _ = L.launch(lambda o: ops.tapconv(L.g_bwd, C, C, t["x"], L.in1, L.wp_bwd, o, res=t["res"],
                                            res_gate=t["gate"]))
    L.compare(out, dg + c.res.double() * (c.gate > 0), "dgrad+res*res_gate", False)
    out, _ = L.launch(lambda o: ops.tapconv(L.g_bwd, C, C, t["x"], L.in1, L.wp_bwd, o, gate=t["gate"]))
    L.compare(out, dg * (c.gate > 0), "dgrad*gate", False)


def _statistics_form(L):
    """conv + bias -> train-mode BatchNorm statistics in the same launch.  A wave that drops or double-counts
    one of its later tiles shifts the mean by a relative 1 / ntiles -- far above the 1e-5 asked here."""
    from mdil_ss_amd import _lib
    ops, c, t = L.ops, L.c, L.t
    C, n = c.C, c.npix
    nq, _, _ = L.tiles(False)
    assert _lib.load().mdil_tapconv_stat_blocks(ctypes.byref(L.g_fwd), C, C) == nq, "the tile mirror has drifted"
    fwd = _ref(c, "fwd", L.adapter)

    def run():
        rm, rv = torch.zeros(C, device=L.dev), torch.ones(C, device=L.dev)
        nbt = torch.zeros((), dtype=torch.int64, device=L.dev)
        out, coef = L.launch(lambda o: ops.tapconv_bn(L.g_fwd, C, C, t["x"], L.in1, L.wp_fwd, o, t["gamma"], t["beta"],
                                                      rm, rv, nbt, bias=t["b"], bias2=L.bias2))
        return out, coef, rm, rv, nbt

    out, coef, rm, rv, nbt = run()
    L.compare(out, fwd, "statistics: output", False)
    flat = fwd.reshape(n, C)
    mean, var = flat.mean(0), flat.var(0, unbiased=False)
    got = coef.cpu().double()
    print(f"MULTITILE statistics [{L.fam} C{C} {n} px adapter={L.adapter}]: mean err "
          f"{float((got[0] - mean).abs().max()):.2e}, invstd rel err "
          f"{float(((got[1] - (var + EPS).rsqrt()) / (var + EPS).rsqrt()).abs().max()):.2e}")
    torch.testing.assert_close(got[0], mean, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(got[1], (var + EPS).rsqrt(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(rv.cpu().double(), 0.9 + 0.1 * var * n / (n - 1), rtol=1e-5, atol=0.0)
    torch.testing.assert_close(rm.cpu().double(), 0.1 * mean, rtol=1e-5, atol=1e-6)
    assert int(nbt) == 1
    assert ops.BN_FIN is True
    try:        # the finalize inside the launch (last-arriving work-group) against the stand-alone one
        ops.BN_FIN = False
        out2, coef2, rm2, rv2, nbt2 = run()
    finally:
        ops.BN_FIN = True
    assert torch.equal(out, out2) and torch.equal(coef, coef2) and torch.equal(rm, rm2) and torch.equal(rv, rv2)
    assert int(nbt2) == 1


def _bnred_form(L):
    """dgrad launch that stores g = conv^T(..) * (gate > 0) and emits sum(g), sum(g xhat) of the BatchNorm backward
    through ``z``; finalize + apply (bn_backward_partials), and the route whose launch finalizes too."""
    ops, c, t = L.ops, L.c, L.t
    C, n = c.C, c.npix
    z64 = c.z.double().reshape(n, C)
    mean, invstd = z64.mean(0).float(), (z64.var(0, unbiased=False) + EPS).rsqrt().float()
    sc = c.gamma * invstd
    coef = torch.stack([mean, invstd, sc, c.beta - mean * sc]).contiguous().to(L.dev)
    g64 = _ref(c, "dgrad", L.adapter) * (c.gate > 0)
    gf = g64.reshape(n, C)
    xhat = (z64 - mean.double()) * invstd.double()
    dbeta, dgamma = gf.sum(0), (gf * xhat).sum(0)
    gz64 = ((c.gamma.double() * invstd.double()) * (gf - dbeta / n - xhat * dgamma / n)).reshape(g64.shape)

    g1, (_, partial, nblk) = L.launch(lambda o: ops.tapconv_bnred(L.g_bwd, C, C, t["x"], L.in1, L.wp_bwd, o, t["gate"],
                                                                   t["z"], coef))
    assert nblk == L.tiles(False)[0]
    gz1, dg1, db1 = ops.bn_backward_partials(g1, t["z"], t["gamma"], t["beta"], coef, True, partial, nblk)
    L.compare(g1, g64, "bn-backward reductions: g", False)
    L.compare(gz1, gz64, "bn-backward reductions: gz", False, rtol=1e-3, atol=1e-4)
    close(dg1, dgamma, rtol=1e-3, atol=1e-4, what=f"{L.fam} dgamma")
    close(db1, dbeta, rtol=1e-3, atol=1e-4, what=f"{L.fam} dbeta")
    sg, sb = torch.zeros(C, device=L.dev), torch.zeros(C, device=L.dev)
    g2, (_, coef3, zero) = L.launch(lambda o: ops.tapconv_bnred(L.g_bwd, C, C, t["x"], L.in1, L.wp_bwd, o, t["gate"],
                                                                 t["z"], coef, fin=(t["gamma"], sg, sb)))
    gz2 = ops.bn_backward_apply(g2, t["z"], coef, coef3)
    assert zero == 0 and torch.equal(g1, g2)
    assert torch.equal(gz1, gz2), float((gz1 - gz2).abs().max())
    close(sg, dgamma, rtol=1e-3, atol=1e-4, what=f"{L.fam} dgamma (finalized by the launch)")
    close(sb, dbeta, rtol=1e-3, atol=1e-4, what=f"{L.fam} dbeta (finalized by the launch)")


_FORMS = {"plain": _plain_forms, "statistics": _statistics_form, "bnred": _bnred_form}


@gpu
@pytest.mark.parametrize("form", list(_FORMS))
@pytest.mark.parametrize("adapter", [False, True], ids=["3taps", "adapter"])
@pytest.mark.parametrize("idx", range(len(CASES)), ids=_IDS)
def test_streaming_launch_with_several_tiles_per_wave(dev, idx, adapter, form):
    from mdil_ss_amd import ops
    ops.invalidate_packs()
    try:
        _FORMS[form](_Launcher(_case(idx), adapter, dev))
    finally:
        ops.invalidate_packs()


# ------------------------------------------------------------------------------------------------
# block level
# ------------------------------------------------------------------------------------------------
def _streaming_tiles_of(recs):
    """[(family, C, ntaps, npix, (min, max) ...)] of the streaming launches among profile records; F(4,3) at
    C = 64 without the adapter is listed with both of its work-group widths (the record does not say which)."""
    out = []
    for kind, ci, co, nt, npix in recs:
        if kind in T.STREAMING and ci == co and ci in (64, 128):
            tp = {T.tiles_per_wave(kind, ci, nt, npix, plain) for plain in (True, False)}
            out.append((kind, ci, nt, npix, sorted(tp)))
    return out


def _assert_multitile(recs, what, expect_families):
    st = _streaming_tiles_of(recs)
    fams = {s[0] for s in st}
    summary = sorted({(s[0], s[1], s[2], s[3], tuple(s[4])) for s in st})
    print(f"MULTITILE {what}: launches (family, C, taps, px, tiles/wave) {summary}")
    assert fams == set(expect_families), (what, fams, expect_families)
    for s in st:
        assert all(hi >= 2 for _, hi in s[4]), (what, s)


@gpu
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("C,N,H,W,d", [(128, 3, 80, 160, 2), (128, 3, 80, 160, 16), (128, 3, 81, 300, 4),
                                       (64, 3, 136, 500, 1)])
def test_nb_block_with_several_tiles_per_wave(dev, C, N, H, W, d, train):
    """tests/test_hip_parity.py::test_nb_block's body (same oracle with replayed gates, same tolerances) where
    every streaming launch of the block runs several tiles per wave."""
    recs = []
    nb_block_case(dev, C, H, W, d, True, train, N=N, run=lambda fn: recs.extend(T.launches(fn)))
    fams = {T.expected_family(C, nt, L, dd) for nt, L, dd in ((3, H, 1), (4, W, 1), (3, H, d), (4, W, d))}
    if train:       # the data gradients: 3 taps along W, 3 taps + the adapter along H
        fams |= {T.expected_family(C, nt, L, dd) for nt, L, dd in ((3, W, 1), (4, H, 1), (3, W, d), (4, H, d))}
    _assert_multitile(recs, f"nb block C{C} {N}x{H}x{W} d{d} train={train}", fams)


def _chain(dev, first_layer, shape, profile_backward=False, oracle=False):
    """Two chained encoder blocks, train mode, per-image Dropout2d factors: every gradient with the
    block-boundary fusion (the consumer's last dgrad launch takes the tail form) and without it.
    -> (TAIL_COUNT of the fused run, its backward's launches)."""
    from mdil_ss_amd import ops
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    N, H, W, C = shape
    torch.manual_seed(3)
    net = Net([20], 1, 0)
    b1, b2 = net.encoder.layers[first_layer], net.encoder.layers[first_layer + 1]
    assert b1.chann == b2.chann == C
    S = {f"b{i + 1}.{k}": v.detach().clone() for i, b in enumerate((b1, b2)) for k, v in b.state_dict().items()}
    b1.to(dev).train(), b2.to(dev).train()
    gen = torch.Generator().manual_seed(17)
    x0 = F.relu(torch.randn(N, C, H, W, generator=gen))
    go = torch.randn(N, C, H, W, generator=gen)
    assert b1.dropout.p != 0 and b2.dropout.p != 0
    masks = [torch.empty(N, C, 1, 1).bernoulli_(0.7, generator=gen).div_(0.7) for _ in (b1, b2)]
    for m in masks:
        assert all(not torch.equal(m[0], m[n]) for n in range(1, N)), "the Dropout2d factors must differ per image"
    drops = [m.reshape(N, C).to(dev) for m in masks]
    xd0, god = nhwc(x0).to(dev), nhwc(go).to(dev)
    named = [(f"b{i + 1}.{n}", p) for i, b in enumerate((b1, b2)) for n, p in b.named_parameters()]
    res, counts, recs, gates, y_fused = {}, None, [], None, None
    was = ops.BN_TAIL
    try:
        for fused in (True, False):
            ops.BN_TAIL = fused
            ops.invalidate_packs()
            ops.TAIL_COUNT["tail"] = ops.TAIL_COUNT["head"] = 0
            for b in (b1, b2):
                for p in b.parameters():
                    p.grad = None
            x = xd0.clone().requires_grad_(True)
            B = ops.boundaries(2)
            ops.GATE_LOG = [] if fused else None
            y1 = b1.run(x, 0, True, drops[0], links=(B[0], B[1]))
            y2 = b2.run(y1, 0, True, drops[1], links=(B[1], B[2]))
            if fused:
                gates, ops.GATE_LOG, y_fused = [g.cpu() for g in ops.GATE_LOG], None, y2.detach()
            if fused and profile_backward:
                recs = T.launches(lambda: y2.backward(god))
            else:
                y2.backward(god)
            torch.cuda.synchronize()
            if fused:
                counts = dict(ops.TAIL_COUNT)
            else:
                assert ops.TAIL_COUNT == {"tail": 0, "head": 0}
            res[fused] = {"x": x.grad.clone(), **{n: p.grad.clone() for n, p in named if p.grad is not None}}
    finally:
        ops.BN_TAIL = was
        ops.GATE_LOG = None
        ops.invalidate_packs()
    assert res[True].keys() == res[False].keys() and len(res[True]) > 20
    worst = 0.0
    for n in res[True]:
        if Hh.zero_grad_bias(n):
            continue
        a, b = res[True][n].double(), res[False][n].double()
        rel = float((a - b).norm() / (b.norm() + 1e-30))
        worst = max(worst, rel)
        assert rel < 2e-5, (n, rel)
    print(f"MULTITILE chain {shape}: tail fusion vs unfused, worst per-tensor rel-L2 {worst:.2e}; TAIL_COUNT {counts}")
    if oracle:
        assert len(gates) == 8
        names = [n for n, _ in named]
        for n in names:
            S[n].requires_grad_(True)
        xc = x0.clone().requires_grad_(True)
        o1 = O._rap(S, "b1", xc, 0, True, b1.dilated, masks[0], gates)
        o2 = O._rap(S, "b2", o1, 0, True, b2.dilated, masks[1], gates)
        assert not gates
        what = f"chain {shape}"
        close(nchw(y_fused), o2, what=what + " fwd")
        o2.backward(go)
        close(nchw(res[True]["x"]), xc.grad, rtol=1e-3, atol=1e-4, what=what + " gx")
        Sd = {n: types.SimpleNamespace(grad=res[True].get(n)) for n in names}
        _grad_check(S, Sd, names, what)
    return counts, recs


@gpu
@pytest.mark.parametrize("first_layer,shape", [(7, (3, 80, 160, 128)), (7, (5, 64, 128, 128)), (1, (3, 136, 500, 64))])
def test_tail_form_with_several_tiles_per_wave(dev, first_layer, shape):
    """The tail form (the consumer block's last dgrad launch gates its input gradient by the producer's output
    and emits the reductions of the producer's OUTER BatchNorm backward, taken of g * Dropout2d factor of the
    pixel's image): fused against unfused (proves the fusion), both against the oracle chain with replayed
    gates (proves either is right at all)."""
    N, H, W, C = shape
    counts, recs = _chain(dev, first_layer, shape, profile_backward=True, oracle=True)
    assert counts == {"tail": 1, "head": 1}, counts
    tail_family = T.expected_family(C, 4, H, 1)          # 3x1 data gradient of dilation 1 + the adapter^T
    assert tail_family in ("wconv", "w4conv")
    st = _streaming_tiles_of(recs)
    print(f"MULTITILE tail chain {shape}: backward launches {sorted({(s[0], s[1], s[2], s[3], tuple(s[4])) for s in st})}")
    tail = [s for s in st if s[0] == tail_family and s[2] == 4]
    assert tail, (tail_family, st)
    for s in st:
        assert all(hi >= 2 for _, hi in s[4]), s


@gpu
@pytest.mark.parametrize("N,tail", [(16, 1), (17, 0)])
def test_tail_staging_bound(dev, N, tail):
    """The tail form stages the Dropout2d factors of the whole batch in LDS: 16 images fill the table exactly
    (WC_TAIL_MAXN / W4_TAIL_MAXN), 17 must take the unfused route."""
    counts, _ = _chain(dev, 1, (N, 8, 16, 64))
    assert counts == {"tail": tail, "head": tail}, counts


# ------------------------------------------------------------------------------------------------
# whole network, eval
# ------------------------------------------------------------------------------------------------
@gpu
def test_eval_forward_batch_equals_single_images_at_640x1280(dev):
    """tests/test_fullsize_properties.py::test_eval_forward_batch_equals_single_images at the ensemble's 1.25
    scale: the N = 6 launches run several tiles per wave (division index path, all three kernel families at
    C = 128), the N = 1 launches exactly one -- so bit-equality of the rows is a test of the tile loop."""
    from mdil_ss_amd import ops
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    from oracle import fixtures as fx
    ops.invalidate_packs()
    torch.manual_seed(0)
    model = Net([20, 20], 2, 1)
    sd = model.state_dict()
    fx.perturb_bn(sd, seed=3)
    model.load_state_dict(sd)
    model.to(dev).eval()
    N = 6
    x = torch.rand(N, 3, 640, 1280, generator=torch.Generator().manual_seed(1234)).to(dev)
    out = {}
    try:
        with torch.no_grad():
            full = model(x, 1)                                  # (packs the weights, fills the caches)
            rec6 = T.launches(lambda: out.__setitem__("full", model(x, 1)), 1024)
            assert tuple(full.shape) == (N, 20, 640, 1280) and bool(torch.isfinite(full).all())
            assert torch.equal(full, out["full"])
            rec1 = None
            for n in (0, 3, 5):
                if rec1 is None:
                    rec1 = T.launches(lambda: out.__setitem__("one", model(x[n:n + 1], 1)), 1024)
                else:
                    out["one"] = model(x[n:n + 1], 1)
                assert torch.equal(out["one"][0], full[n]), f"image {n}: batch row differs from the single-image forward"
    finally:
        ops.invalidate_packs()
    s6, s1 = _streaming_tiles_of(rec6), _streaming_tiles_of(rec1)
    assert len(s6) == len(s1) > 40
    assert {s[0] for s in s6 if s[1] == 128} == {"sconv", "wconv", "w4conv"}
    print(f"MULTITILE eval 6x3x640x1280: (family, C, taps, px, tiles/wave) "
          f"{sorted({(s[0], s[1], s[2], s[3], tuple(s[4])) for s in s6})}")
    for a, b in zip(s6, s1):
        assert a[:3] == b[:3] and a[3] == N * b[3], (a, b)
        assert all(hi >= 2 for _, hi in a[4]), a
        assert all(hi == 1 for _, hi in b[4]), b
