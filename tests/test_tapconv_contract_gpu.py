"""GPU: the contract of ``mdil_tapconv`` (include/mdil_hip.h) on every route behind it, against the float64
reference of tests/tapconv_contract.py.

Part A runs the 14 LDS-tiled ``tapconv_kernel`` instantiations in the geometries ops.DownFn / UpFn / OutFn build
(297 pixels: three tiles at BM = 128 that straddle the image ends, a ragged last one), part B the stride-1 C -> C
routes (c16conv, direct sconv, F(2,3) wconv, F(4,3) w4conv and the router's fall-backs) -- each with the
epilogue forms E0 .. E10 of the table.  Every case asserts FIRST that the kernel family the launch profiler
reports is the one the host mirror of the router names, and fails (never skips) when it is not.

route x form, integer draw: ``tapconv``, ``c16conv``, ``sconv`` and ``wconv`` (F(2,3): its transform constants
are 1 and 1/2, all dyadic) must EQUAL the reference over the whole output buffer, sentinel-filled elements the
launch does not own included; ``w4conv`` (1/6, 1/24) is held to RTOL / ATOL of tests/test_hip_parity.py.  The
N(0, 1) draw holds every route to that tolerance on the owned elements and to bit equality elsewhere.  Part C
runs one conv through its own route and through the LDS-tiled kernel and asks for the same bits, as
csrc/c16conv.hip and csrc/tapconv.hip claim."""
import pytest
import torch

from tests import helpers as Hh
from tests import streaming_tiles as T
from tests import tapconv_contract as TC
from tests import wgrad_chunks as WC
from tests.test_hip_parity import ATOL, RTOL, close

pytestmark = pytest.mark.gpu
EXACT_ROUTES = ("tapconv", "c16conv", "sconv", "wconv")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _lib
    _lib.load()
    torch.set_num_threads(Hh.host_threads())
    return torch.device("cuda:0")


def _pack(ops, c, w):
    """The packed image of the dense draw w [cout][cin][ntaps] (the stem: [13][3][9], im2col order)."""
    if c.stem:
        dst = torch.empty(1, 16, 32, dtype=torch.float32, device=w.device)
        return ops.pack_into(dst, w, (0,), c.cout, 27, 27, 1, stem=True, register=False)
    nt = c.g.ntaps
    dst = torch.empty(nt, TC._r16(c.cout), TC._r16(c.cin), dtype=torch.float32, device=w.device)
    return ops.pack_into(dst, w, tuple(range(nt)), c.cout, c.cin, c.cin * nt, nt, register=False)


class _Device:
    """The operands of one (case, form, draw) on the device, and the launch."""

    def __init__(self, ops, dev, c, t, e, before):
        self.ops, self.c, self.t, self.e = ops, c, t, e
        self.g = ops.make_geom(*c.gargs, **c.gkw)
        for k in vars(c.g):                                    # one set of fields feeds mirror and struct
            got = getattr(self.g, k)
            assert (list(got) if isinstance(getattr(c.g, k), list) else got) == getattr(c.g, k), k
        self.in0 = t.in0.to(dev)
        self.in1_base = None if t.in1_base is None else t.in1_base.to(dev)
        self.in1 = self.in1_base
        if c.in1 == "wide":
            self.in1 = self.in1_base[..., c.g.in_pitch[1] - c.cin:]
            assert self.in1.data_ptr() % 16 == 0
        self.w = t.w.to(dev)
        self.wpk = _pack(ops, c, self.w)
        self.out = before.to(dev)
        self.epi = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in vars(e).items()}
        if e.res is before:
            self.epi["res"] = self.out                         # in place

    def launch(self):
        c = self.c
        return T.paths(lambda: self.ops.tapconv(self.g, c.cin, c.cout, self.in0, self.in1, self.wpk, self.out,
                                                **self.epi), 16)

    def inputs_unchanged(self, before):
        t, e = self.t, self.e
        assert torch.equal(self.in0.cpu(), t.in0) and torch.equal(self.w.cpu(), t.w), "the launch wrote its inputs"
        if self.in1_base is not None:
            assert torch.equal(self.in1_base.cpu(), t.in1_base), "the launch wrote its second source"
        for k, v in vars(e).items():
            if torch.is_tensor(v) and v is not before:
                assert torch.equal(self.epi[k].cpu(), v), f"the launch wrote its {k} operand"


def _check(c, form, draw, r, got, want, before, mask):
    what = f"{c.name} {form} [{r}, {TC.epilogue_path(c.cout) if r == 'tapconv' else 'streaming'}] {draw} draw"
    if draw == "int" and r in EXACT_ROUTES:
        msg = WC.mismatch_report(what, got, want)
        assert not msg, msg
        return
    close(got[mask], want[mask], rtol=RTOL, atol=ATOL, what=what)
    assert torch.equal(got[~mask], before[~mask]), what + ": the launch wrote elements it does not own"


@pytest.mark.parametrize("name,form", TC.PARAMS, ids=[f"{n}-{f}" for n, f in TC.PARAMS])
def test_tapconv_contract(dev, name, form):
    from mdil_ss_amd import ops
    c = TC.BY_NAME[name]
    want_route = TC.expected_route(c, form)
    mask = TC.owned_mask(c.g, c.cout)
    ops.invalidate_packs()
    try:
        for draw in ("int", "normal"):
            t, e, before, want = TC.expected(c, form, draw)
            d = _Device(ops, dev, c, t, e, before)
            routes = d.launch()
            assert routes == [want_route], f"{name} {form}: expected one {want_route} launch, the library made {routes}"
            _check(c, form, draw, want_route, d.out.cpu(), want, before, mask)
            d.inputs_unchanged(before)
    finally:
        ops.invalidate_packs()


def _widen(t, C, fill):
    """[N, H, W, C] -> the first C floats of a 2C-float row."""
    out = torch.full(tuple(t.shape[:3]) + (2 * C,), fill)
    out[..., :C] = t
    return out


@pytest.mark.parametrize("name,form", TC.IDENTITY_PARAMS, ids=[f"{n}-{f}" for n, f in TC.IDENTITY_PARAMS])
def test_own_route_and_the_tiled_kernel_give_the_same_bits(dev, name, form):
    """csrc/c16conv.hip:16 and csrc/tapconv.hip:681-683: the same conv through its own route and through the
    LDS-tiled kernel (a 2C-float output row forces it; res and the gates are laid out the same way)."""
    from mdil_ss_amd import ops
    c = TC.BY_NAME[name]
    C = c.cout
    ops.invalidate_packs()
    try:
        t, e, before, want = TC.expected(c, form, "normal")
        own = _Device(ops, dev, c, t, e, before)
        assert own.launch() == [c.expect]
        wide_before = _widen(before, C, TC.SENTINEL)
        we = TC.epilogue(**{k: (_widen(v, C, TC.FOREIGN) if torch.is_tensor(v) and v.dim() == 4 else v)
                            for k, v in vars(e).items()})
        if e.res is before:
            we.res = wide_before
        forced = _Device(ops, dev, c.forced, t, we, wide_before)
        assert forced.launch() == ["tapconv"]
        a, b = own.out.cpu(), forced.out.cpu()
        what = f"{name} {form}"
        close(a, want, rtol=RTOL, atol=ATOL, what=what + f" [{c.expect}]")
        close(b[..., :C], want, rtol=RTOL, atol=ATOL, what=what + " [tapconv]")
        assert torch.equal(b[..., C:], wide_before[..., C:]), what + ": the forced launch wrote past its channels"
        msg = WC.mismatch_report(what + f": {c.expect} against the LDS-tiled kernel", a, b[..., :C].contiguous())
        assert not msg, msg
        own.inputs_unchanged(before)
        forced.inputs_unchanged(wide_before)
    finally:
        ops.invalidate_packs()
