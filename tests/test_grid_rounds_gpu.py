"""GPU: the kernels of the training path whose grid is capped -- the fused head (csrc/head.hip), the unfused
losses and the confusion counts (loss.hip), the max-pool half of the down block (pool.hip), Adam (adam.hip) --
where a thread (a wave) runs SEVERAL ROUNDS of its grid-stride loop, against float64 references on the host.

The per-kernel parity tests (tests/test_hip_parity.py) stay one to two orders of magnitude below the grid
bounds; tests/test_fullsize_properties.py reaches the loops but compares HIP with HIP.  What runs only from the
second round on: the head's per-wave LDS staging of x and dl reused under a compiler-only fence, its dW / db
accumulators and loss sums carried across tiles, the clamped lanes of a ragged last tile that falls into a
later round, the LDS histogram of the confusion kernel filled over several passes, and the reduce kernel's
strided walk over more than 64 partial rows.

tests/grid_rounds.py holds the mirror of the grid plans, the cases and the references (pinned and proven by
tests/test_grid_rounds_cpu.py).  Every case first asserts its plan -- several rounds, uneven rounds, a ragged
last tile where it has one -- and FAILS (never skips) when that does not hold.  Per-pixel outputs are compared
element by element, nothing sampled or left out, and the error measure |err| / bound is reported per round
and for the last tile (``ROUNDS ...`` lines)."""
import functools

import pytest
import torch

from oracle import rap_oracle as O
from tests import grid_rounds as G
from tests import helpers as Hh
from tests.test_hip_parity import ATOL, RTOL, close

pytestmark = pytest.mark.gpu
SENTINEL = G.SENTINEL
HEAD = [(name, nc) for name in G.HEAD_CASES for nc in G.NCS]
HEAD_IDS = [f"{name}-nc{nc}" for name, nc in HEAD]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _lib
    _lib.load()
    torch.set_num_threads(Hh.host_threads(16))
    return torch.device("cuda:0")


def by_round(form, got, want, rounds, last, rtol, atol):
    """``got`` / ``want`` [rows, k] and the round of every row: ``close`` on the whole tensor, its error measure
    split by round and for the rows of the last tile, so that a failure names the round.  -> the report."""
    ratio = G.ratio(got, want, rtol, atol).reshape(rounds.numel(), -1).amax(1)
    nr = int(rounds.max()) + 1
    per = torch.zeros(nr, dtype=torch.float64).scatter_reduce(0, rounds.reshape(-1), ratio, "amax", include_self=False)
    report = "  ".join(f"round {k}: {float(v):.3f}" for k, v in enumerate(per))
    worst_last = None
    if last is not None:
        worst_last = float(ratio[last.reshape(-1)].max())
        report += f"  last tile: {worst_last:.3f}"
    print(f"ROUNDS {form}: worst |err|/bound by {report}")
    try:
        close(got, want, rtol=rtol, atol=atol, what=form)
    except AssertionError as e:
        raise AssertionError(f"{e}\n  |err|/bound by round: {report}") from None
    assert float(per.max()) <= 1.0 and (worst_last is None or worst_last <= 1.0), report
    return per


def whole(form, got, want, rtol, atol):
    """``close`` on a tensor that has no rounds of its own (dw, db: sums over every round), worst ratio reported."""
    print(f"ROUNDS {form}: worst |err|/bound {float(G.ratio(got, want, rtol, atol).max()):.3f}")
    close(got, want, rtol=rtol, atol=atol, what=form)


def assert_plan(p, rounds, uneven=True):
    lo, hi = p.per_wave if hasattr(p, "per_wave") else p.per_thread
    assert hi == rounds, f"the case no longer runs {rounds} rounds: {vars(p)}"
    assert (lo < hi) or not uneven, f"even rounds: {vars(p)}"


# ------------------------------------------------------------------------------------------------
# fused head through the C ABI, as ops.HeadCEFn / HeadKLDFn build the calls
# ------------------------------------------------------------------------------------------------
class Head:
    """One head case on the device.  ``gx`` and ``logits_out`` sit between two sentinel bands of one tile of rows
    (16 feature rows, 64 logit rows); every call checks both bands afterwards: the clamped lanes of the ragged
    last tile are what would write there."""

    def __init__(self, c, dev):
        from mdil_ss_amd import _lib, ops
        self.c, self.dev, self.ops, self.lib = c, dev, ops, _lib.load()
        self.check = _lib.check
        p = c.plan
        assert (p.blocks, p.tiles) == (min(1024, -(-p.tiles // 4)), -(-c.npix // 16))
        if c.name == "H3":          # one round; the case is the reduce kernel's walk over 205 partial rows
            assert p.rounds == 1 and p.reduce_passes == 4 and p.reduce_clamped, vars(p)
        else:
            assert_plan(p, {"H1": 2, "H2": 3}[c.name])
            assert p.last_round == p.rounds - 1, "the ragged tile must fall into the last round"
        assert 0 < p.last_px < 16, "the case is about a ragged last tile"
        self.P = (c.nc + 3) // 4 * 4
        self.rounds, self.last = G.round_map(c).reshape(-1), G.last_tile_map(c).reshape(-1)
        self.rounds_out, self.last_out = G.up2(G.round_map(c)).reshape(-1), G.up2(G.last_tile_map(c)).reshape(-1)
        d = lambda t: t.to(dev).contiguous()
        self.w, self.b, self.wt, self.bt, self.cw = d(c.w), d(c.b), d(c.wt), d(c.bt), d(c.cw)
        self.x, self.xt, self.lab = d(G.nhwc(c.x)), d(G.nhwc(c.xt)), d(c.lab)
        self.out = torch.empty(2, device=dev)                       # loss, wsum
        self.ws = ops._head_ws(self.lib, dev)

    def _guarded(self, rows, width):
        band = (16 if width == 16 else 64) * width
        buf = torch.full((rows * width + 2 * band,), SENTINEL, device=self.dev)
        return buf, buf[band:band + rows * width].view(rows, width), band

    def _bands_untouched(self, buf, band, what):
        assert bool((buf[:band] == SENTINEL).all()), f"{what}: the launch wrote in front of its output"
        assert bool((buf[-band:] == SENTINEL).all()), f"{what}: the launch wrote beyond its last valid pixel"

    def _wgrad_args(self, wgrad, prior):
        if not wgrad:
            return None, None, 0
        if prior is None:
            return (torch.full((16, self.c.nc, 2, 2), SENTINEL, device=self.dev),
                    torch.full((self.c.nc,), SENTINEL, device=self.dev), 0)
        return prior[0].clone(), prior[1].clone(), 1

    def ce_fwd(self, lab, x=None, want_logits=False):
        """-> (loss, wsum, logits [4 npix, P] or None) of the forward call."""
        c, ops = self.c, self.ops
        x = self.x if x is None else x
        buf = lg = None
        if want_logits:
            buf, lg, band = self._guarded(4 * c.npix, self.P)
        self.out.fill_(SENTINEL)
        self.check(self.lib.mdil_head_ce(ops._p(x), ops._p(self.w), ops._p(self.b), c.N, c.H, c.W, c.nc, ops._p(lab),
                                         ops._p(self.cw), None, self.out.data_ptr(), self.out.data_ptr() + 4, None, None,
                                         None, 0, ops._p(lg), ops._p(ops._label_counter(self.dev)), self.ws.data_ptr(),
                                         self.ws.numel(), ops._stream()), "mdil_head_ce")
        loss, wsum = self.out.tolist()
        ops.check_labels()
        if want_logits:
            self._bands_untouched(buf, band, f"head_ce forward {c.name} nc{c.nc}, logits")
        return loss, wsum, lg

    def ce_bwd(self, lab, x=None, wgrad=True, prior=None, scale=G.CE_SCALE):
        """(after ``ce_fwd`` on the same labels: it left wsum) -> gx [npix,16], dw, db."""
        c, ops = self.c, self.ops
        x = self.x if x is None else x
        buf, gx, band = self._guarded(c.npix, 16)
        dw, db, acc = self._wgrad_args(wgrad, prior)
        g = torch.tensor([scale], device=self.dev)
        self.check(self.lib.mdil_head_ce(ops._p(x), ops._p(self.w), ops._p(self.b), c.N, c.H, c.W, c.nc, ops._p(lab),
                                         ops._p(self.cw), ops._p(g), None, self.out.data_ptr() + 4, ops._p(gx), ops._p(dw),
                                         ops._p(db), acc, None, None, self.ws.data_ptr(), self.ws.numel(),
                                         ops._stream()), "mdil_head_ce")
        self._bands_untouched(buf, band, f"head_ce backward {c.name} nc{c.nc} wgrad={wgrad}")
        return gx, dw, db

    def kld(self, xs=None, xt=None, backward=False, wgrad=True, prior=None, scale=G.KLD_SCALE):
        """-> loss (forward) or (gx [npix,16], dw, db)."""
        c, ops = self.c, self.ops
        xs, xt = self.x if xs is None else xs, self.xt if xt is None else xt
        head = (ops._p(xs), ops._p(self.w), ops._p(self.b), ops._p(xt), ops._p(self.wt), ops._p(self.bt), c.N, c.H, c.W, c.nc)
        if not backward:
            self.out.fill_(SENTINEL)
            self.check(self.lib.mdil_head_kld(*head, None, self.out.data_ptr(), None, None, None, 0, self.ws.data_ptr(),
                                              self.ws.numel(), ops._stream()), "mdil_head_kld")
            return self.out.tolist()[0]
        buf, gx, band = self._guarded(c.npix, 16)
        dw, db, acc = self._wgrad_args(wgrad, prior)
        g = torch.tensor([scale], device=self.dev)
        self.check(self.lib.mdil_head_kld(*head, ops._p(g), None, ops._p(gx), ops._p(dw), ops._p(db), acc,
                                          self.ws.data_ptr(), self.ws.numel(), ops._stream()), "mdil_head_kld")
        self._bands_untouched(buf, band, f"head_kld backward {c.name} nc{c.nc} wgrad={wgrad}")
        return gx, dw, db

    def prior(self):
        g = torch.Generator().manual_seed(5)
        return (torch.randn(16, self.c.nc, 2, 2, generator=g).to(self.dev), torch.randn(self.c.nc, generator=g).to(self.dev))


@functools.lru_cache(maxsize=1)
def _head(name, nc, dev):
    return Head(G.head_inputs(name, nc), dev)


@pytest.mark.parametrize("name,nc", HEAD, ids=HEAD_IDS)
def test_head_ce_dense(dev, name, nc):
    """mdil_head_ce, every pixel weighted: loss with and without the logits store (the same float), the stored
    logits and their zero pad entry, the backward with dw / db, with both null (frozen head) and accumulating."""
    h = _head(name, nc, dev)
    c, what = h.c, f"head CE {name} nc{nc}"
    ref = G.dense_ce_ref(c)
    loss, wsum, lg = h.ce_fwd(h.lab, want_logits=True)
    loss2, wsum2, _ = h.ce_fwd(h.lab)
    print(f"ROUNDS {what}: loss {loss:.7f} (float64 {ref.loss:.7f}), rel err {abs(loss - ref.loss) / ref.loss:.2e}")
    assert loss == loss2 and wsum == wsum2, "the logits store changed the loss"
    assert loss == pytest.approx(ref.loss, rel=2e-5) and wsum == pytest.approx(ref.wsum, rel=2e-5)
    by_round(f"{what} logits", lg[:, :nc], ref.logits.reshape(-1, nc), h.rounds_out, h.last_out, RTOL, ATOL)
    if h.P > nc:
        assert int(torch.count_nonzero(lg[:, nc:])) == 0, "the pad entry of the 28-float rows must be exactly 0"
    gx, dw, db = h.ce_bwd(h.lab)
    by_round(f"{what} gx", gx, ref.gx.reshape(-1, 16), h.rounds, h.last, 1e-3, 1e-4)
    whole(what + " dw", dw, ref.dw, 1e-3, 1e-4)
    whole(what + " db", db, ref.db, 1e-3, 1e-4)
    gx0, none_w, none_b = h.ce_bwd(h.lab, wgrad=False)
    assert none_w is None and none_b is None
    by_round(f"{what} gx, dw = db = null", gx0, ref.gx.reshape(-1, 16), h.rounds, h.last, 1e-3, 1e-4)
    pw, pb = h.prior()
    _, dwa, dba = h.ce_bwd(h.lab, prior=(pw, pb))
    assert torch.equal(dwa, pw + dw) and torch.equal(dba, pb + db), "accumulate = 1 is not prior + gradient"
    whole(what + " dw, accumulated", dwa, pw.cpu().double() + ref.dw, 1e-3, 1e-4)
    whole(what + " db, accumulated", dba, pb.cpu().double() + ref.db, 1e-3, 1e-4)


@pytest.mark.parametrize("name,nc", HEAD, ids=HEAD_IDS)
def test_head_kld_dense(dev, name, nc):
    """mdil_head_kld alone (not summed with the CE term, which is two orders of magnitude larger): forward,
    backward with dw / db, with both null (the frozen old-domain head of step 2), and accumulating."""
    h = _head(name, nc, dev)
    c, what = h.c, f"head KLD {name} nc{nc}"
    ref = G.dense_kld_ref(c)
    loss = h.kld()
    print(f"ROUNDS {what}: loss {loss:.4e} (float64 {ref.loss:.4e}), rel err {abs(loss - ref.loss) / abs(ref.loss):.2e}")
    assert loss == pytest.approx(ref.loss, rel=1e-4, abs=1e-7)
    gx, dw, db = h.kld(backward=True)
    by_round(f"{what} gx", gx, ref.gx.reshape(-1, 16), h.rounds, h.last, 1e-3, 1e-4)
    whole(what + " dw", dw, ref.dw, 1e-3, 1e-4)
    whole(what + " db", db, ref.db, 1e-3, 2e-4)
    gx0, none_w, none_b = h.kld(backward=True, wgrad=False)
    assert none_w is None and none_b is None
    by_round(f"{what} gx, frozen head", gx0, ref.gx.reshape(-1, 16), h.rounds, h.last, 1e-3, 1e-4)
    pw, pb = h.prior()
    _, dwa, dba = h.kld(backward=True, prior=(pw, pb))
    assert torch.equal(dwa, pw + dw) and torch.equal(dba, pb + db), "accumulate = 1 is not prior + gradient"


@pytest.mark.parametrize("name,nc", HEAD, ids=HEAD_IDS)
def test_head_ce_sparse(dev, name, nc):
    """A dense comparison resolves one lost tile only to 1 / ntiles (2.4e-4 at H1, 1.2e-4 at H2: below every
    tolerance).  Here every output pixel carries the zero-weight class except those under the live tiles
    (wave slot 5 and the last tile's slot, in every round), so the loss, the sum of weights, dw and db come from
    2 to 6 tiles: a tile lost, doubled or read from another round moves them by far more than 100 x the tolerance
    (tests/test_grid_rounds_cpu.py).  Outside the live tiles gx is exactly zero."""
    h = _head(name, nc, dev)
    c, what = h.c, f"head CE sparse {name} nc{nc}"
    ref, q = G.sparse_ce_ref(c)
    lab = G.sparse_target(c).to(dev)
    loss, wsum, _ = h.ce_fwd(lab)
    print(f"ROUNDS {what}: tiles {G.live_tiles(c.npix)}, loss {loss:.7f} (float64 {ref.loss:.7f}), wsum {wsum:.5f} "
          f"({ref.wsum:.5f})")
    assert loss == pytest.approx(ref.loss, rel=2e-5) and wsum == pytest.approx(ref.wsum, rel=2e-5)
    live = G.live_mask(c).reshape(-1)
    for wgrad in (True, False):
        gx, dw, db = h.ce_bwd(lab, wgrad=wgrad)
        assert int(torch.count_nonzero(gx[~live.to(dev)])) == 0, "gx outside the live tiles"
        by_round(f"{what} gx of the live pixels, wgrad={wgrad}", gx[q.to(dev)], ref.gx, h.rounds[q], h.last[q], 1e-3, 1e-4)
        if wgrad:
            whole(what + " dw", dw, ref.dw, 1e-3, 1e-4)
            whole(what + " db", db, ref.db, 1e-3, 1e-4)


@pytest.mark.parametrize("name,nc", HEAD, ids=HEAD_IDS)
def test_head_kld_sparse(dev, name, nc):
    """Both feature tensors zero outside the live tiles: staged zeros contribute exact zeros, so dw comes from 2
    to 6 tiles and is as sharp as in the CE form; gx is compared per pixel (outside the live tiles every pixel
    has the row of a zero feature vector).  The KLD db and loss stay DENSE-ONLY: every pixel outside the live
    tiles adds a non-zero constant to them whatever its features, so there a whole lost round (at least 1/3 of
    the sum) is caught by test_head_kld_dense, one lost tile is not."""
    h = _head(name, nc, dev)
    c, what = h.c, f"head KLD sparse {name} nc{nc}"
    ref, q = G.sparse_kld_ref(c)
    xs, xt = (G.nhwc(t).to(dev) for t in G.sparse_features(c))
    live = G.live_mask(c).reshape(-1)
    want = ref.gx_zero.expand(c.npix, 16).clone()
    want[q] = ref.gx
    for wgrad in (True, False):
        gx, dw, db = h.kld(xs, xt, backward=True, wgrad=wgrad)
        by_round(f"{what} gx, wgrad={wgrad}", gx, want, h.rounds, h.last, 1e-3, 1e-4)
        by_round(f"{what} gx of the live pixels, wgrad={wgrad}", gx[q.to(dev)], ref.gx, h.rounds[q], h.last[q], 1e-3, 1e-4)
        if wgrad:
            whole(what + " dw", dw, ref.dw, 1e-3, 1e-4)
    assert int(live.sum()) == q.numel()


# ------------------------------------------------------------------------------------------------
# unfused losses and the metric
# ------------------------------------------------------------------------------------------------
def _layouts(c, t, dev):
    """The device layouts of [N,nc,H,W] logits: channels-last rows of nc floats (nc = 20); for nc = 27 the
    pitch-28 rows the model returns (pad entry set to a large value: it must be ignored) and a plain tensor."""
    if c.nc == 20:
        return {"rows20": t.to(dev).contiguous(memory_format=torch.channels_last)}
    rows = torch.full((c.N, c.H, c.W, 28), 1e9, device=dev)
    rows[..., :27] = t.to(dev).permute(0, 2, 3, 1)
    return {"rows28": rows[..., :27].permute(0, 3, 1, 2), "plain": t.to(dev)}


@pytest.mark.parametrize("nc", G.NCS)
def test_unfused_losses(dev, nc):
    from mdil_ss_amd import ops
    c = G.loss_inputs("L1", nc)
    assert_plan(c.plan, 2)
    rounds = torch.arange(c.npix) // G.LOSS_BOUND
    ref = G.loss_refs(c, c.lab)
    sparse_lab = G.sparse_loss_target(c)
    sref = G.loss_refs(c, sparse_lab)
    px = G.sparse_loss_pixels(c)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(c.npix, nc)
    keep = torch.ones(c.npix, dtype=torch.bool)
    keep[px] = False
    assert int(torch.count_nonzero(rows(sref.dce)[keep])) == 0 and bool((rows(sref.dce)[px].abs().amax(1) > 0).all())
    lab_d, sparse_d, cw_d = c.lab.to(dev), sparse_lab.to(dev), c.cw.to(dev)
    t_lay = _layouts(c, c.t, dev)
    for lay, s in _layouts(c, c.s, dev).items():
        what = f"losses L1 nc{nc} {lay}"
        s = s.detach().requires_grad_(True)
        relaid = ops._nhwc_logits(s)[0].data_ptr() != s.data_ptr()
        assert relaid == (lay == "plain"), f"{lay}: unexpected (re-)layout"
        ce = ops.cross_entropy2d(s, lab_d, cw_d)
        ops.check_labels()
        print(f"ROUNDS {what}: CE {float(ce):.7f} (float64 {ref.ce:.7f})")
        assert float(ce) == pytest.approx(ref.ce, rel=1e-5)
        ce.backward()
        by_round(f"{what} dCE", rows(s.grad), rows(ref.dce), rounds, None, 1e-4, 1e-5)
        s.grad = None
        kld = ops.kld_prob(s, t_lay[lay])
        print(f"ROUNDS {what}: KLD {float(kld):.5e} (float64 {ref.kld:.5e})")
        assert float(kld) == pytest.approx(ref.kld, rel=1e-4, abs=1e-7)
        kld.backward()
        by_round(f"{what} dKLD", rows(s.grad), rows(ref.dkld), rounds, None, 1e-4, 1e-5)
        s.grad = None
        # sparse CE: weight at pixels 7, 7 + 524,288 and the last one only
        ce = ops.cross_entropy2d(s, sparse_d, cw_d)
        assert float(ce) == pytest.approx(sref.ce, rel=1e-5)
        ce.backward()
        got = rows(s.grad)
        assert int(torch.count_nonzero(got[keep.to(dev)])) == 0, "sparse CE: gradient outside the weighted pixels"
        close(got[px], rows(sref.dce)[px], rtol=1e-4, atol=1e-5, what=what + " dCE, sparse")


@pytest.mark.parametrize("nc", G.NCS)
def test_argmax_confusion_counts(dev, nc):
    """Exact: the counts of two calls into the same tensor are twice the bincount of the argmax of the same fp32
    logits (no pixel has a tied maximum, tests/test_grid_rounds_cpu.py); labels include the ignore class."""
    from mdil_ss_amd import ops
    c = G.loss_inputs("L1", nc)
    assert_plan(c.plan, 2)
    want = G.confusion_ref(c.s, c.lab, nc, nc - 1)
    assert int((c.lab == nc - 1).sum()) > 0
    lab_d = c.lab.to(dev)
    for lay, s in _layouts(c, c.s, dev).items():
        counts = torch.zeros(3, nc, dtype=torch.int64, device=dev)
        for k in (1, 2):
            ops.argmax_confusion(s, lab_d, nc - 1, counts)
            assert torch.equal(counts.cpu(), k * want), f"{lay}, call {k}"
        ops.check_labels()


# ------------------------------------------------------------------------------------------------
# max-pool half of the down block, through the C ABI as ops.DownFn calls it
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.POOL_CASES))
def test_maxpool_concat(dev, name):
    """Exact.  Forward into the channel slice [coff, coff + C) of a sentinel-filled z: the pooled slice equals
    F.max_pool2d, the conv slice keeps the sentinel.  Backward: the first maximum in scan order takes the
    gradient (ATen's rule, csrc/pool.hip) -- tied windows are common in both rounds -- and equals the float64
    autograd of max_pool2d; the conv slice of gz is non-zero, so a wrong offset shows."""
    from mdil_ss_amd import _lib, ops
    lib = _lib.load()
    c = G.pool_inputs(name)
    assert_plan(c.plan, 2)
    y_ref, gx_ref = G.pool_refs(c)
    HO, WO = c.H // 2, c.W // 2
    x, gz = c.x.to(dev), c.gz.to(dev)
    band = WO * c.pitch
    zbuf = torch.full((2 * band + c.N * HO * WO * c.pitch,), SENTINEL, device=dev)
    z = zbuf[band:-band].view(c.N, HO, WO, c.pitch)
    _lib.check(lib.mdil_maxpool_concat_fwd(ops._p(x), c.N, c.H, c.W, c.C, ops._p(z), c.pitch, c.coff, ops._stream()),
               "mdil_maxpool_concat_fwd")
    pooled = z[..., c.coff:c.coff + c.C].cpu()
    rounds = (torch.arange(c.total) // G.POOL_BOUND).reshape(pooled.shape)
    wrong = pooled != y_ref
    assert not wrong.any(), f"{name} forward: {int(wrong.sum())} wrong, by round {torch.bincount(rounds[wrong], minlength=2).tolist()}"
    assert bool((z[..., :c.coff] == SENTINEL).all()) and bool((z[..., c.coff + c.C:] == SENTINEL).all())
    assert bool((zbuf[:band] == SENTINEL).all()) and bool((zbuf[-band:] == SENTINEL).all())
    band = c.W * c.C
    gbuf = torch.full((2 * band + x.numel(),), SENTINEL, device=dev)
    gx = gbuf[band:-band].view_as(x)
    _lib.check(lib.mdil_maxpool_concat_bwd(ops._p(x), ops._p(gz), c.N, c.H, c.W, c.C, c.pitch, c.coff, ops._p(gx),
                                           ops._stream()), "mdil_maxpool_concat_bwd")
    wrong = (gx.cpu() != gx_ref).reshape(c.N, HO, 2, WO, 2, c.C).any(4).any(2)
    assert not wrong.any(), f"{name} backward: {int(wrong.sum())} wrong windows, by round {torch.bincount(rounds[wrong], minlength=2).tolist()}"
    assert torch.equal(gx.cpu(), gx_ref)
    assert bool((gbuf[:band] == SENTINEL).all()) and bool((gbuf[-band:] == SENTINEL).all())
    print(f"ROUNDS maxpool {name}: {c.total} items, {c.plan.blocks} blocks, forward and backward exact in both rounds; "
          f"tied windows {int(G.pool_tied_windows(c).sum())}")


# ------------------------------------------------------------------------------------------------
# Adam
# ------------------------------------------------------------------------------------------------
def test_adam_rounds(dev):
    """tests/test_hip_parity.py::test_adam's three steps at its tolerances, 2 to 3 elements per thread, and a
    fourth step with grad_scale = 0.5 against the oracle fed the scaled gradient; the oracle runs in float64."""
    from mdil_ss_amd import ops
    c = G.adam_inputs("A1")
    assert_plan(c.plan, 3)
    p = c.p.double()
    m, v = torch.zeros(c.n, dtype=torch.float64), torch.zeros(c.n, dtype=torch.float64)
    pd, md, vd = c.p.to(dev), torch.zeros(c.n, device=dev), torch.zeros(c.n, device=dev)
    rounds = torch.arange(c.n) // G.ADAM_BOUND
    for step in (1, 2, 3, 4):
        gi = c.g * step                                  # fp32, what the kernel reads
        scale = 0.5 if step == 4 else 1.0
        O.adam_l2_step(p, gi.double() * scale, m, v, step, 5e-4)
        ops.adam_step(pd, gi.to(dev), md, vd, step, 5e-4, weight_decay=1e-4, grad_scale=scale)
        if step >= 3:
            by_round(f"adam step {step} param", pd[:, None], p[:, None], rounds, None, 1e-6, 1e-7)
            by_round(f"adam step {step} v", vd[:, None], v[:, None], rounds, None, 1e-5, 1e-12)
