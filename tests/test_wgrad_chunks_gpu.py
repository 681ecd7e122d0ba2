"""GPU: the weight-gradient kernels (csrc/wgrad.hip) where ONE CHUNK RUNS SEVERAL STAGES, bit for bit
against the float64 reference of the layer.

At the shapes of the other per-kernel parity tests almost every chunk of a weight-gradient launch holds
one stage (tests/wgrad_chunks.py says where the second one starts), so the register-prefetch hand-over,
the double-buffered coordinate table, the accumulators and bias sums carried across stages, the row and
image wrap of the streaming kernels' scalar descriptors, a ragged last stage in a later round and chunks
without work were compared with a reference only through whole networks.  Here every case runs at least
two stages / quads / tiles per chunk, on integer operands: every partial sum is exact in fp32 in any
order, so the result must EQUAL the reference (torch.equal) -- one dropped, doubled or mispaired pixel
out of 10^5 fails.  A second pass on N(0, 1) operands uses the weight-gradient tolerances of
test_tapconv_factorised.

The sampler, stem and head launches are the product's: ops.DownFn / UpFn / OutFn run once with
ops.tapconv / ops.wgrad wrapped, and exactly the recorded calls (geometry, channel counts, ktap, strides,
epilogue operands) are replayed on the test's tensors; the forward and dgrad launches the capture records
are compared the same way.  Every case asserts its preconditions first -- the kernel family the launch
profiler reports, the chunk count the library's workspace size implies, >= 2 units per chunk -- and
FAILS (never skips) when one does not hold."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from tests import helpers as Hh
from tests import wgrad_chunks as WC
from tests.test_hip_parity import ATOL, RTOL, close, nhwc, rnd

pytestmark = pytest.mark.gpu
SENTINEL = -7777.0       # output channels / pixels a launch does not own
FOREIGN = 1000.0         # gout channels a launch must not use


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _lib
    _lib.load()
    torch.set_num_threads(Hh.host_threads())
    return torch.device("cuda:0")


def cases(*kinds):
    sel = [c for c in WC.CASES if c.kind in kinds]
    return pytest.mark.parametrize("c", sel, ids=[c.name.replace(" ", "_") for c in sel])


# ------------------------------------------------------------------------------------------------
# capture and replay of the product's launches
# ------------------------------------------------------------------------------------------------
class Capture:
    """Wraps ops.tapconv / ops.wgrad (and the weight packers, to know what a packed image holds) while
    ``fn`` runs; tensors are recorded by name: those of ``named``, else t0, t1, ... in order of appearance."""

    def __init__(self, ops, monkeypatch, named):
        self.ops, self.calls, self.packs, self.keep = ops, [], {}, []
        self.names = {t.data_ptr(): n for n, t in named.items() if t is not None}
        real = SimpleNamespace(tapconv=ops.tapconv, wgrad=ops.wgrad, pack_conv=ops.pack_conv, pack_into=ops.pack_into)

        def pack_into(dst, w, ktap, M, K, s_m, s_k, stem=False, register=True):
            out = real.pack_into(dst, w, ktap, M, K, s_m, s_k, stem=stem, register=register)
            self.keep.append(dst)
            self.packs.setdefault(dst.data_ptr(), ("into", tuple(dst.shape), self.name(w), tuple(ktap), M, K, s_m, s_k, stem))
            return out

        def pack_conv(w, mode, ktap=None, k_pad=None):
            out = real.pack_conv(w, mode, ktap, k_pad)
            self.keep.append(out)
            self.packs[out.data_ptr()] = ("conv", self.name(w), mode, None if ktap is None else tuple(ktap), k_pad)
            return out

        def tapconv(g, cin, cout, in0, in1, wpk, out, bias=None, scale=None, shift=None, res=None, res_gate=None,
                    gate=None, relu=False, bias2=None):
            self.calls.append(dict(op="tapconv", g=g, cin=cin, cout=cout, in0=self.name(in0), in1=self.name(in1),
                                   wpk=self.packs.get(wpk.data_ptr()), out=self.name(out), bias=self.name(bias),
                                   scale=self.name(scale), shift=self.name(shift), res=self.name(res),
                                   res_gate=self.name(res_gate), gate=self.name(gate), relu=bool(relu),
                                   bias2=self.name(bias2)))
            return real.tapconv(g, cin, cout, in0, in1, wpk, out, bias=bias, scale=scale, shift=shift, res=res,
                                res_gate=res_gate, gate=gate, relu=relu, bias2=bias2)

        def wgrad(g, cin, cout, in0, in1, gout, ktap, s_co, s_ci, w, b, dw=None, db=None, second=None):
            sec = None if second is None else (second[0], second[1], second[2], self.name(second[3]), self.name(second[4]))
            self.calls.append(dict(op="wgrad", g=g, cin=cin, cout=cout, in0=self.name(in0), in1=self.name(in1),
                                   gout=self.name(gout), ktap=None if ktap is None else tuple(ktap), s_co=s_co,
                                   s_ci=s_ci, w=self.name(w), b=self.name(b), second=sec))
            return real.wgrad(g, cin, cout, in0, in1, gout, ktap, s_co, s_ci, w, b, dw, db, second)

        for k, v in (("tapconv", tapconv), ("wgrad", wgrad), ("pack_conv", pack_conv), ("pack_into", pack_into)):
            monkeypatch.setattr(ops, k, v)
        self._undo = lambda: [monkeypatch.setattr(ops, k, getattr(real, k)) for k in vars(real)]

    def name(self, t):
        if t is None:
            return None
        n = self.names.get(t.data_ptr())
        if n is None:
            n = self.names[t.data_ptr()] = f"t{len(self.names)}"
            self.keep.append(t)             # alive: the allocator must not hand its address to another tensor
        return n

    def done(self):
        self._undo()
        return self.calls


def replay_tapconv(ops, rec, env):
    """One recorded ops.tapconv call on the tensors of ``env``."""
    pk = rec["wpk"]
    assert pk is not None, "the packed image of a recorded launch was not built by ops.pack_conv / pack_into"
    for k in ("scale", "shift", "res_gate", "gate", "bias2", "in1"):
        assert rec[k] is None, (k, "the replay has no reference for this epilogue operand")
    assert not rec["relu"]
    if pk[0] == "conv":
        wpk = ops.pack_conv(env[pk[1]], pk[2], pk[3], pk[4])
    else:
        _, shape, wn, ktap, M, K, s_m, s_k, stem = pk
        wpk = ops.pack_into(torch.empty(shape, dtype=torch.float32, device=env[wn].device), env[wn], ktap, M, K,
                            s_m, s_k, stem=stem, register=False)
    ops.tapconv(rec["g"], rec["cin"], rec["cout"], env[rec["in0"]], None, wpk, env[rec["out"]],
                bias=None if rec["bias"] is None else env[rec["bias"]],
                res=None if rec["res"] is None else env[rec["res"]])


def replay_wgrads(ops, recs, env):
    """The recorded ops.wgrad calls of ONE layer: all accumulate into one dw / db (+ dw2 / db2)."""
    dw = db = None
    extra = ()
    for r in recs:
        sec = None
        if r["second"] is not None:
            n2, sc2, si2, w2, b2 = r["second"]
            sec = (n2, sc2, si2, env[w2], env[b2])
        out = ops.wgrad(r["g"], r["cin"], r["cout"], env[r["in0"]], None if r["in1"] is None else env[r["in1"]],
                        env[r["gout"]], r["ktap"], r["s_co"], r["s_ci"], env[r["w"]], env[r["b"]], dw, db, sec)
        dw, db, extra = out[0], out[1], out[2:]
    return (dw, db) + tuple(extra)


def wgrad_families(ops, fn, capacity=64):
    """Kernel families ("wgrad", "wgrad2", "wgradw") of the weight-gradient launches of ``fn``, in order."""
    ops.profile_begin(capacity)
    try:
        fn()
    finally:
        recs = ops.profile_end(capacity)
    return [r[0] for r in recs if r[0] in ops._PROF_WGRAD]


def check_plans(ops, c, launches):
    """The preconditions of a case on its real launches [(geometry, cin, cout)] -> their plans."""
    from mdil_ss_amd import _lib
    lib = _lib.load()
    host = [WC.plan_for(*l) for l in WC.host_launches(c)]
    plans = [WC.plan_for(g, ci, co) for g, ci, co in launches]
    key = lambda p: (p.sub, p.total, p.per_chunk, p.chunks, p.empty)
    assert [key(p) for p in plans] == [key(p) for p in host], "the product's launches are not the case table's"
    for (g, ci, co), p in zip(launches, plans):
        print(WC.plan_line(c.name, p))
        assert p.family == c.family and (c.sub is None or p.sub == c.sub), (c.name, p.family, p.sub)
        assert p.per_chunk >= 2, (c.name, p.per_chunk)
        assert WC.exact_budget(g.N * g.HO * g.WO) < 2 ** 23
        if p.family == "wgrad":
            nbytes = lib.mdil_wgrad_workspace(ctypes.byref(g), ci, co)
            assert WC.lds_chunks_from_workspace(nbytes, g.ntaps, co, ci) == p.chunks, (c.name, nbytes, p.chunks)
    if c.cross is not None:
        assert bool(plans[0].row_cross) == ("r" in c.cross) and bool(plans[0].image_cross) == ("i" in c.cross)
    return plans


def compare(what, got, want, exact, rtol, atol):
    if exact:
        msg = WC.mismatch_report(what, got, want)
        assert not msg, msg
    else:
        close(got, want, rtol=rtol, atol=atol, what=what)


def compare_grads(c, got, ref, exact):
    names = ("dw", "db", "dw2", "db2")[:len(got)]
    for n, g in zip(names, got):
        assert g.dtype == torch.float32
        compare(f"{c.name} {n}", g, ref[n], exact, 5e-4, 5e-5)


# ------------------------------------------------------------------------------------------------
# sampler, stem and head: the launches of ops.DownFn / UpFn / OutFn
# ------------------------------------------------------------------------------------------------
def capture_layer(ops, monkeypatch, dev, c):
    """Run the case's autograd Function once (train mode, N(0, 1) operands) -> its recorded launches."""
    N, H, W = c.N, c.H, c.W
    (ws, nb) = WC.weight_shapes(c)[0]
    fan = ws[1] * ws[2] * ws[3]
    x = nhwc(rnd(N, c.cin, H, W, seed=4)).to(dev).requires_grad_(c.kind != "stem")
    w = rnd(*ws, seed=1, scale=(1.0 / fan) ** 0.5).to(dev).requires_grad_(True)
    b = rnd(nb, seed=2, scale=0.1).to(dev).requires_grad_(True)
    cap = Capture(ops, monkeypatch, {"x": x, "w": w, "b": b})
    try:
        if c.kind == "out":
            y = ops.OutFn.apply(x, w, b)
        else:
            bn = [(1 + rnd(c.cout, seed=5, scale=0.1)).to(dev).requires_grad_(True),
                  rnd(c.cout, seed=6, scale=0.1).to(dev).requires_grad_(True), rnd(c.cout, seed=7, scale=0.1).to(dev),
                  (1 + rnd(c.cout, seed=8, scale=0.1).abs()).to(dev), torch.zeros((), dtype=torch.int64, device=dev)]
            y = (ops.UpFn if c.kind == "up" else ops.DownFn).apply(x, w, b, *bn, True, None)
        (gs, owned) = WC.gout_shape(c)
        assert tuple(y.shape) == gs[:3] + (c.cout,)
        gy = torch.randn(gs, device=dev)
        y.backward(gy[..., :c.cout] if c.kind == "out" else gy)       # the head's rows are padded to 4 floats
        torch.cuda.synchronize()
    finally:
        calls = cap.done()
    return calls


@cases("stem", "down", "up", "out")
def test_sampler_weight_gradients_with_several_stages_per_chunk(dev, monkeypatch, c):
    from mdil_ss_amd import ops
    ops.invalidate_packs()
    calls = capture_layer(ops, monkeypatch, dev, c)
    wg = [r for r in calls if r["op"] == "wgrad"]
    assert len(wg) == len(WC.host_launches(c)) and len({r["gout"] for r in wg}) == 1
    gname = wg[0]["gout"]
    fwd = [r for r in calls if r["op"] == "tapconv" and r["in0"] == "x"]
    dgr = [r for r in calls if r["op"] == "tapconv" and r["in0"] == gname]
    assert len(fwd) + len(dgr) == len(calls) - len(wg)
    assert len(fwd) == {"stem": 1, "down": 1, "up": 4, "out": 0}[c.kind]          # (the head's forward is outconv.hip)
    assert len(dgr) == {"stem": 0, "down": 4, "up": 1, "out": 1}[c.kind]
    assert all(r["in0"] == "x" and r["w"] == "w" and r["b"] == "b" and r["second"] is None for r in wg)
    check_plans(ops, c, [(r["g"], r["cin"], r["cout"]) for r in wg])
    (gs, owned) = WC.gout_shape(c)

    for draw, exact in ((WC.draw_int, True), (WC.draw_normal, False)):
        ops.invalidate_packs()
        t = WC.draw_case(c, draw)
        ref = WC.reference(c, t, with_input=True)
        env = {k: t[k].to(dev) for k in ("x", "w", "b")}
        gout = torch.full(gs, FOREIGN)
        gout[..., :owned] = t["gout"]
        env[gname] = gout.to(dev)
        for r in fwd:
            env.setdefault(r["out"], torch.full(gs[:3] + (c.cout,), SENTINEL, device=dev))
        for r in dgr:
            env.setdefault(r["out"], t["r"].to(dev) if "r" in t else torch.full(t["x"].shape, SENTINEL, device=dev))
        fams = wgrad_families(ops, lambda: env.update(grads=replay_wgrads(ops, wg, env)))
        assert fams == [c.family] * len(wg), (c.name, fams)
        compare_grads(c, env["grads"], ref, exact)
        for r in fwd + dgr:
            replay_tapconv(ops, r, env)
        if fwd:
            z = env[fwd[0]["out"]].cpu()
            compare(f"{c.name} forward", z[..., :owned], ref["out"], exact, RTOL, ATOL)
            assert bool((z[..., owned:] == SENTINEL).all()), "the forward launch wrote channels it does not own"
        if dgr:
            want = ref["gx"] + (t["r"].double() if "r" in t else 0)
            compare(f"{c.name} dgrad", env[dgr[0]["out"]].cpu(), want, exact, RTOL, ATOL)
        assert torch.equal(env[gname].cpu(), gout) and torch.equal(env["x"].cpu(), t["x"])
    ops.invalidate_packs()


# ------------------------------------------------------------------------------------------------
# 3-tap C -> C and C = 16 convs: the geometry of test_tapconv_factorised
# ------------------------------------------------------------------------------------------------
@cases("conv3")
def test_three_tap_weight_gradients_with_several_quads_per_chunk(dev, c):
    from mdil_ss_amd import ops
    C = c.cin
    taps = ops._taps_3x1(c.d) if c.axis == "h" else ops._taps_1x3(c.d)
    g = ops.make_geom(c.N, c.H, c.W, c.H, c.W, taps, C, c.H, c.W, C)
    check_plans(ops, c, [(g, C, C)])
    for draw, exact in ((WC.draw_int, True), (WC.draw_normal, False)):
        t = WC.draw_case(c, draw)
        ref = WC.reference(c, t)
        d = {k: v.to(dev) for k, v in t.items()}
        res = {}
        fams = wgrad_families(ops, lambda: res.update(grads=ops.wgrad(g, C, C, d["x"], None, d["gout"], (0, 1, 2),
                                                                        C * 3, 3, d["w"], d["b"])))
        assert fams == [c.family], (c.name, fams)
        compare_grads(c, res["grads"], ref, exact)
        assert torch.equal(d["gout"].cpu(), t["gout"]) and torch.equal(d["x"].cpu(), t["x"])


# ------------------------------------------------------------------------------------------------
# 1x3 conv + 1x1 adapter as 4th tap: the launch of ops.NbFn's backward (per-launch path, which
# test_nb_block_abi_is_the_per_launch_path holds bit-identical to the block ABI)
# ------------------------------------------------------------------------------------------------
def capture_adapter_block(ops, monkeypatch, dev, c):
    C, N, H, W = c.cin, c.N, c.H, c.W
    monkeypatch.setattr(ops, "BLOCK_ABI", False)
    P = {}
    for i, (kk, nm) in enumerate([((3, 1), "w31_1"), ((1, 3), "w13_1"), ((3, 1), "w31_2"), ((1, 3), "w13_2")]):
        P[nm] = rnd(C, C, *kk, seed=10 + i, scale=(1.0 / (3 * C)) ** 0.5)
        P["b" + nm[1:]] = rnd(C, seed=20 + i, scale=0.1)
    for j in (1, 2):
        P[f"pw{j}"], P[f"pb{j}"] = rnd(C, C, 1, 1, seed=30 + j, scale=(1.0 / C) ** 0.5), rnd(C, seed=40 + j, scale=0.1)
        P[f"g{j}"], P[f"be{j}"] = 1 + rnd(C, seed=50 + j, scale=0.1), rnd(C, seed=60 + j, scale=0.1)
    P = {k: v.to(dev).requires_grad_(True) for k, v in P.items()}
    bufs = tuple(t for j in (1, 2) for t in (rnd(C, seed=70 + j, scale=0.1).to(dev),
                                             (1 + rnd(C, seed=80 + j, scale=0.1).abs()).to(dev),
                                             torch.zeros((), dtype=torch.int64, device=dev)))
    x = nhwc(torch.relu(rnd(N, C, H, W, seed=5))).to(dev).requires_grad_(True)
    cap = Capture(ops, monkeypatch, dict(P, x=x))
    try:
        out = ops.NbFn.apply(x, P["w31_1"], P["b31_1"], P["w13_1"], P["b13_1"], P["pw1"], P["pb1"], P["g1"], P["be1"],
                             P["w31_2"], P["b31_2"], P["w13_2"], P["b13_2"], P["pw2"], P["pb2"], P["g2"], P["be2"],
                             bufs, None, c.d, True, None, None)
        out.backward(torch.randn(N, H, W, C, device=dev))
        torch.cuda.synchronize()
    finally:
        calls = cap.done()
    return calls


@cases("adapter")
def test_adapter_weight_gradients_with_several_quads_per_chunk(dev, monkeypatch, c):
    from mdil_ss_amd import ops
    ops.invalidate_packs()
    calls = capture_adapter_block(ops, monkeypatch, dev, c)
    wg = [r for r in calls if r["op"] == "wgrad" and r["second"] is not None]
    assert len(wg) == 2, "one 1x3 + adapter launch per half of the block"
    seen = set()
    for r in wg:
        g = r["g"]
        assert g.ntaps == 4 and r["in1"] is not None and r["ktap"] == (0, 1, 2, 0)
        dd = max(abs(g.dw[k]) for k in range(3))
        seen.add(dd)
        cd = SimpleNamespace(**dict(vars(c), d=dd))             # the block's first half runs at dilation 1
        check_plans(ops, cd, [(g, r["cin"], r["cout"])])
        for draw, exact in ((WC.draw_int, True), (WC.draw_normal, False)):
            t = WC.draw_case(cd, draw)
            ref = WC.reference(cd, t)
            env = {r["in0"]: t["x"].to(dev), r["in1"]: t["x2"].to(dev), r["gout"]: t["gout"].to(dev),
                   r["w"]: t["w"].to(dev), r["b"]: t["b"].to(dev), r["second"][3]: t["w2"].to(dev),
                   r["second"][4]: t["b2"].to(dev)}
            assert len(env) == 7
            fams = wgrad_families(ops, lambda: env.update(grads=replay_wgrads(ops, [r], env)))
            assert fams == [c.family], (c.name, fams)
            assert len(env["grads"]) == 4
            compare_grads(cd, env["grads"], ref, exact)
    assert seen == {1, c.d}
    ops.invalidate_packs()
