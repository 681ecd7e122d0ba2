"""CPU: the host mirror of the capped grids (tests/grid_rounds.py), the case table of
tests/test_grid_rounds_gpu.py and the float64 references it compares with.

The plans depend on nothing but the sizes, so what the GPU cases presuppose -- several rounds, uneven rounds,
a ragged last tile in a later round, the reduce kernel's clamped tail -- is decided here; the constants are
pinned against the text of the sources, so a change of a grid bound fails here instead of silently moving the
GPU cases back to one round.  The conditions on the drawn inputs that make the comparisons sharp (every class
drawn, one live tile moves dW by far more than the tolerance, tied pool windows in both rounds, no tied
maximum among the logits) are conditions on the references alone and are asserted here as well."""
import functools
import os
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import fixtures as fx
from oracle import rap_oracle as O
from tests import grid_rounds as G
from tests import head_cases as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = [(name, nc) for name in G.HEAD_CASES for nc in G.NCS]
HEAD_IDS = [f"{name}-nc{nc}" for name, nc in HEAD]


@functools.lru_cache(None)
def source(name):
    text = open(os.path.join(ROOT, "mdil_ss_amd", "csrc", name)).read()
    return re.sub(r"\s+", " ", re.sub(r"//[^\n]*", "", text))


# ------------------------------------------------------------------------------------------------
# pins against the source text
# ------------------------------------------------------------------------------------------------
def test_constants_are_the_sources():
    assert re.findall(r"#define MDIL_WG (\d+)", source("common.h")) == [str(G.MDIL_WG)]
    s = source("head.hip")
    assert re.findall(r"constexpr int HD_T = (\d+);", s) == [str(G.HD_T)]
    assert "constexpr int HD_WAVES = HD_T / 64;" in s and G.HD_WAVES == G.HD_T // 64
    assert re.findall(r"constexpr int HD_MAX_BLOCKS = (\d+);", s) == [str(G.HD_MAX_BLOCKS)]
    assert G.HD_TILE == 16
    assert "long long b = ((npix + 15) / 16 + HD_WAVES - 1) / HD_WAVES;" in s
    assert "return (int)(b > HD_MAX_BLOCKS ? HD_MAX_BLOCKS : (b < 1 ? 1 : b));" in s
    walk = ("for (long long tile = (long long)blockIdx.x * HD_WAVES + wave; tile < ntiles; "
            "tile += (long long)gridDim.x * HD_WAVES)")
    assert s.count(walk) == 4 and s.count("const long long ntiles = (npix + 15) / 16;") == 4     # CE / KLD, fwd / bwd
    assert "const long long q = tile * 16 + (lane & 15);" in s and "const long long q0 = tile * 16 + j;" in s
    assert "for (int k0 = sl; k0 < nblk; k0 += 4 * 16)" in s and "const int k = k0 + 4 * u;" in s
    assert G.HD_REDUCE_STRIDE == 4 * 16
    s = source("loss.hip")
    assert re.findall(r"constexpr int LOSS_MAX_BLOCKS = (\d+);", s) == [str(G.LOSS_MAX_BLOCKS)]
    assert "long long b = (npix + MDIL_WG - 1) / MDIL_WG;" in s
    assert "return (int)(b > LOSS_MAX_BLOCKS ? LOSS_MAX_BLOCKS : (b < 1 ? 1 : b));" in s
    assert s.count("dim3(grid), dim3(MDIL_WG)") == 7          # every per-pixel launch takes loss_grid's grid
    s = source("pool.hip")
    assert re.findall(r"return \(int\)\(b > (\d+) \? (\d+) : \(b < 1 \? 1 : b\)\);", s) == [(str(G.POOL_MAX_BLOCKS),) * 2]
    assert s.count("dim3(grid_for(total)), dim3(MDIL_WG)") == 2
    s = source("adam.hip")
    assert re.findall(r"if \(b > (\d+)\) b = (\d+);", s) == [(str(G.ADAM_MAX_BLOCKS),) * 2]
    assert "long long b = (n + MDIL_WG - 1) / MDIL_WG;" in s and "dim3((int)b), dim3(MDIL_WG)" in s
    assert (G.HEAD_BOUND, G.LOSS_BOUND, G.POOL_BOUND, G.ADAM_BOUND) == (65536, 524288, 1048576, 524288)


# ------------------------------------------------------------------------------------------------
# the plans
# ------------------------------------------------------------------------------------------------
def test_bounds_are_where_a_second_round_starts():
    at, over = G.head_plan(G.HEAD_BOUND), G.head_plan(G.HEAD_BOUND + 1)
    assert (at.blocks, at.rounds, at.per_wave) == (1024, 1, (1, 1)) and at.last_px == 16
    assert (over.rounds, over.per_wave, over.last_px, over.last_round, over.last_slot) == (2, (1, 2), 1, 1, 0)
    for cap, bound in ((G.LOSS_MAX_BLOCKS, G.LOSS_BOUND), (G.POOL_MAX_BLOCKS, G.POOL_BOUND)):
        assert G.flat_plan(bound, G.MDIL_WG, cap).per_thread == (1, 1)
        assert G.flat_plan(bound + 1, G.MDIL_WG, cap).per_thread == (1, 2)
    assert G.flat_round(G.LOSS_BOUND - 1, 721200) == 0 and G.flat_round(G.LOSS_BOUND, 721200) == 1


def test_older_parity_shapes_run_one_round():
    """What the module rests on: the largest shapes of the per-kernel parity tests."""
    assert G.head_plan(3 * 16 * 48).rounds == 1 and G.head_plan(2 * 128 * 256).per_wave == (1, 1)      # covering size
    assert G.flat_plan(2 * 24 * 40).rounds == 1 and G.flat_plan(3 * 16 * 24).rounds == 1          # test_losses, confusion
    assert G.flat_plan(2 * 6 * 20 * 16, G.MDIL_WG, G.POOL_MAX_BLOCKS).rounds == 1                 # test_down_block
    assert G.flat_plan(100003, G.MDIL_WG, G.ADAM_MAX_BLOCKS).rounds == 1                          # test_adam


def test_the_head_plans_of_the_table():
    p = G.head_plan(2 * 130 * 257)
    assert (p.npix, p.tiles, p.blocks, p.per_wave, p.last_px, p.last_round) == (66820, 4177, 1024, (1, 2), 4, 1)
    assert G.live_tiles(p.npix) == [5, 4101, 80, 4176]
    p = G.head_plan(2 * 260 * 257)
    assert (p.npix, p.tiles, p.blocks, p.per_wave, p.last_px, p.last_round) == (133640, 8353, 1024, (2, 3), 8, 2)
    assert G.live_tiles(p.npix) == [5, 4101, 8197, 160, 4256, 8352]
    p = G.head_plan(1 * 100 * 131)
    assert (p.npix, p.tiles, p.blocks, p.rounds, p.last_px) == (13100, 819, 205, 1, 12)
    assert (p.reduce_passes, p.reduce_clamped) == (4, True)
    assert G.live_tiles(p.npix) == [5, 818]
    for name, (N, H, W) in G.HEAD_CASES.items():
        p = G.head_plan(N * H * W)
        assert p.last_px < G.HD_TILE and W % 2 == 1, name                  # ragged last tile; W no power of two
        assert p.reduce_passes >= 4, name


def test_round_and_slot_of_a_pixel():
    npix = 66820
    assert (G.head_round(0, npix), G.head_slot(0, npix)) == (0, 0)
    assert (G.head_round(65535, npix), G.head_slot(65535, npix)) == (0, 4095)
    assert (G.head_round(65536, npix), G.head_slot(65536, npix)) == (1, 0)
    assert (G.head_round(npix - 1, npix), G.head_slot(npix - 1, npix)) == (1, 80)
    c = G.head_inputs("H1", 20)
    r = G.round_map(c).reshape(-1)
    assert torch.equal(torch.bincount(r), torch.tensor([65536, 1284]))
    assert int(G.last_tile_map(c).sum()) == 4 and bool(r[G.last_tile_map(c).reshape(-1)].eq(1).all())
    assert int(G.live_mask(c).sum()) == 3 * 16 + 4
    u = G.up2(G.round_map(c))
    assert tuple(u.shape) == (2, 260, 514) and int(u[0, 7, 9]) == int(G.round_map(c)[0, 3, 4])


def test_the_flat_plans_of_the_table():
    for nc in G.NCS:
        c = G.loss_inputs("L1", nc)
        assert (c.npix, c.plan.blocks, c.plan.per_thread) == (721200, 2048, (1, 2))
        assert G.sparse_loss_pixels(c) == [7, 7 + 524288, 721199]
        assert [G.flat_round(p, c.npix) for p in G.sparse_loss_pixels(c)] == [0, 1, 1]
    want = {"P1": 1087200, "P2": 1053360, "P3": 1059840}
    for name, ((N, H, W, C), pitch, coff) in G.POOL_CASES.items():
        p = G.flat_plan(N * (H // 2) * (W // 2) * C, G.MDIL_WG, G.POOL_MAX_BLOCKS)
        assert (p.n, p.blocks, p.per_thread) == (want[name], 4096, (1, 2)), name
        assert coff + C == pitch and H % 2 == 0 and W % 2 == 0
    p = G.flat_plan(G.ADAM_CASES["A1"], G.MDIL_WG, G.ADAM_MAX_BLOCKS)
    assert (p.n, p.blocks, p.per_thread) == (1060921, 2048, (2, 3))


# ------------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", G.NCS)
def test_references_are_the_oracle_with_autograd(nc):
    """head_ce_ref / head_kld_ref against conv_transpose2d + O.ce2d / O.kld_prob + autograd, float64, at a shape
    where tests/test_hip_parity.py::test_fused_head_and_loss stands."""
    shape = HC.SHAPES[2]
    N, H, W = shape
    x, w, b = HC.head_inputs(nc, shape)
    xt, wt, bt = HC.draw(nc, shape, 99)
    lab = fx.make_batch(N, 2 * H, 2 * W, nc, seed=3)[1][:, 0]
    cw = G.class_weights(nc)
    assert float(cw[-1]) == 0.0 and bool((cw[:-1] > 0).all())
    for kind in ("ce", "kld"):
        xo, wo, bo = (t.double().requires_grad_(True) for t in (x, w, b))
        logits = F.conv_transpose2d(xo, wo, bo, stride=2)
        if kind == "ce":
            loss = O.ce2d(logits, lab, cw.double())
            (G.CE_SCALE * loss).backward()
            r = G.head_ce_ref(x, w, b, lab, cw)
            torch.testing.assert_close(r.logits, G.nhwc(logits.detach()), rtol=0, atol=0)
            assert r.wsum == pytest.approx(float(cw.double()[lab].sum()), rel=1e-14)
        else:
            loss = O.kld_prob(logits, F.conv_transpose2d(xt.double(), wt.double(), bt.double(), stride=2))
            (G.KLD_SCALE * loss).backward()
            r = G.head_kld_ref(x, w, b, xt, wt, bt)
        assert r.loss == pytest.approx(float(loss.detach()), rel=1e-13)
        for got, want in ((r.gx, G.nhwc(xo.grad)), (r.dw, wo.grad), (r.db, bo.grad)):
            torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-15)
    # the unfused references: the same two functions on drawn logits
    s, t = torch.randn(2, nc, 5, 7, dtype=torch.float64), torch.randn(2, nc, 5, 7, dtype=torch.float64)
    y = torch.randint(0, nc, (2, 5, 7))
    assert float(G.ce64(s, y, cw.double())[0]) == pytest.approx(float(O.ce2d(s, y, cw.double())), rel=1e-13)
    assert float(G.kld64(s, t)) == pytest.approx(float(O.kld_prob(s, t)), rel=1e-13)


@pytest.mark.parametrize("name,nc", HEAD, ids=HEAD_IDS)
def test_dense_references_are_finite_and_every_class_is_drawn(name, nc):
    c = G.head_inputs(name, nc)
    assert torch.equal(c.lab.unique(), torch.arange(nc)), "a class is missing from the labels"
    assert tuple(c.lab.shape) == (c.N, 2 * c.H, 2 * c.W) and c.x.dtype == torch.float32
    assert float(c.x.min()) == 0.0 and 0.4 < float((c.x > 0).float().mean()) < 0.6          # after ReLU
    for r in (G.dense_ce_ref(c), G.dense_kld_ref(c)):
        for k, v in vars(r).items():
            v = torch.as_tensor(v)
            assert bool(torch.isfinite(v).all()), (name, nc, k)
            assert v.numel() == 1 or float(v.abs().max()) > 0, (name, nc, k)
        assert tuple(r.gx.shape) == (c.N, c.H, c.W, 16)


@pytest.mark.parametrize("name,nc", HEAD, ids=HEAD_IDS)
def test_one_live_tile_moves_the_sparse_reference(name, nc):
    """What makes the sparse forms sharp: with any ONE live tile removed, some element of the reference's dW (and
    of the CE's db) moves by more than 100 x the bound the GPU test allows (rtol 1e-3, atol 1e-4 of the largest
    element); the CE loss and the sum of weights move by more than 100 x theirs (rel 2e-5)."""
    c = G.head_inputs(name, nc)
    tiles = G.live_tiles(c.npix)
    assert len(tiles) == 2 * c.plan.rounds and len(set(tiles)) == len(tiles)
    assert {t // c.plan.waves for t in tiles} == set(range(c.plan.rounds)) and c.plan.tiles - 1 in tiles
    ce, q = G.sparse_ce_ref(c)
    kld, _ = G.sparse_kld_ref(c)
    assert q.numel() == int(G.live_mask(c).sum()) and ce.wsum > 0
    for k, t in enumerate(tiles):
        rest = tiles[:k] + tiles[k + 1:]
        ce1, _ = G.sparse_ce_ref(c, rest)
        kld1, _ = G.sparse_kld_ref(c, rest)
        assert float(G.ratio(ce1.dw, ce.dw, 1e-3, 1e-4).max()) > 100, (name, nc, t, "CE dW")
        assert float(G.ratio(ce1.db, ce.db, 1e-3, 1e-4).max()) > 100, (name, nc, t, "CE db")
        assert float(G.ratio(kld1.dw, kld.dw, 1e-3, 1e-4).max()) > 100, (name, nc, t, "KLD dW")
        assert abs(ce1.wsum - ce.wsum) > 100 * 2e-5 * ce.wsum, (name, nc, t, "wsum")


@pytest.mark.parametrize("nc", G.NCS)
def test_sparse_references_are_those_of_the_whole_tensor(nc):
    """The one-row image of the live pixels against the reference of the whole tensor, at H3."""
    c = G.head_inputs("H3", nc)
    m = G.live_mask(c)
    ce, q = G.sparse_ce_ref(c)
    full = G.head_ce_ref(c.x, c.w, c.b, G.sparse_target(c), c.cw)
    assert ce.loss == pytest.approx(full.loss, rel=1e-12) and ce.wsum == pytest.approx(full.wsum, rel=1e-14)
    assert torch.equal(torch.nonzero(m.reshape(-1))[:, 0].sort()[0], q.sort()[0])
    assert int(torch.count_nonzero(full.gx[~m])) == 0
    rows = full.gx.reshape(-1, 16)
    for got, want in ((ce.gx, rows[q]), (ce.dw, full.dw), (ce.db, full.db)):
        torch.testing.assert_close(got, want, rtol=1e-11, atol=1e-16)
    kld, _ = G.sparse_kld_ref(c)
    xs, xt = G.sparse_features(c)
    assert int(torch.count_nonzero(xs[:, :, ~m[0]])) == 0 and torch.equal(xs[:, :, m[0]], c.x[:, :, m[0]])
    full = G.head_kld_ref(xs, c.w, c.b, xt, c.wt, c.bt)
    rows = full.gx.reshape(-1, 16)
    torch.testing.assert_close(kld.dw, full.dw, rtol=1e-11, atol=1e-18)
    torch.testing.assert_close(kld.gx, rows[q], rtol=1e-11, atol=1e-18)
    outside = rows[~m.reshape(-1)]
    torch.testing.assert_close(outside, kld.gx_zero.expand_as(outside), rtol=1e-11, atol=1e-18)
    assert float(kld.gx_zero.abs().max()) > 0          # every other pixel adds its constant to db and to the loss:
    assert float(G.ratio(kld.db, full.db, 1e-3, 2e-4).max()) > 1       # those two stay dense-only


# ------------------------------------------------------------------------------------------------
# unfused losses, pool, Adam: conditions on the drawn inputs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", G.NCS)
def test_loss_case_inputs(nc):
    c = G.loss_inputs("L1", nc)
    assert torch.equal(c.lab.unique(), torch.arange(nc))          # the ignore class nc - 1 included
    top = c.s.topk(2, dim=1)[0]
    assert float((top[:, 0] - top[:, 1]).min()) > 0, "a pixel has two equal largest logits: 'first maximum' would matter"
    cnt = G.confusion_ref(c.s, c.lab, nc, nc - 1)
    assert int(cnt[0].sum() + cnt[2].sum()) == int((c.lab != nc - 1).sum())     # every kept pixel is a hit or a miss
    assert int(cnt[:, nc - 1].sum()) == 0 and bool((cnt[:, :nc - 1] > 0).all())
    sp = G.sparse_loss_target(c).reshape(-1)
    w = c.cw[sp]
    assert torch.equal(torch.nonzero(w)[:, 0], torch.tensor(G.sparse_loss_pixels(c)))


@pytest.mark.parametrize("name", list(G.POOL_CASES))
def test_pool_case_inputs(name):
    c = G.pool_inputs(name)
    assert c.plan.per_thread == (1, 2) and c.total == c.plan.n
    assert bool((c.x * 4 == (c.x * 4).round()).all()) and float(c.x.min()) == 0.0 and float(c.x.max()) == 2.0
    tied = G.pool_tied_windows(c)
    rounds = torch.arange(c.total) // G.POOL_BOUND
    for k in (0, 1):
        sel = tied[rounds == k]
        assert sel.numel() > 0 and 0.1 < float(sel.float().mean()) < 0.9, (name, k)      # "common": one window in ten
    # tied windows whose maximum is not 0 (a tie at 0 hands a gradient to a dead input all the same)
    x = c.x.reshape(c.N, c.H // 2, 2, c.W // 2, 2, c.C)
    assert int((tied & (x.amax((2, 4)).reshape(-1) > 0) & (rounds == 1)).sum()) > 100
    assert float(c.gz[..., :c.coff].abs().min()) > 0
    y, gx = G.pool_refs(c)
    assert tuple(y.shape) == (c.N, c.H // 2, c.W // 2, c.C) and tuple(gx.shape) == tuple(c.x.shape)
    # one input per window takes the gradient, the FIRST maximum in scan order (0,0), (0,1), (1,0), (1,1)
    g6 = gx.reshape(c.N, c.H // 2, 2, c.W // 2, 2, c.C).permute(0, 1, 3, 5, 2, 4).reshape(-1, 4)
    x6 = x.permute(0, 1, 3, 5, 2, 4).reshape(-1, 4)
    first = (x6 == x6.amax(1, keepdim=True)).float().argmax(1)
    assert torch.equal(torch.count_nonzero(g6, 1), torch.ones(c.total, dtype=torch.int64))
    assert torch.equal(g6.abs().argmax(1), first)
    assert torch.equal(g6.gather(1, first[:, None])[:, 0], c.gz[..., c.coff:].reshape(-1))


def test_adam_case_inputs():
    c = G.adam_inputs("A1")
    assert c.plan.per_thread == (2, 3) and c.p.numel() == c.n == 1060921
    assert G.flat_round(c.n - 1, c.n, G.MDIL_WG, G.ADAM_MAX_BLOCKS) == 2
