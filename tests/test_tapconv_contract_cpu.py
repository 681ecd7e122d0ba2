"""CPU: the float64 reference, the draws, the case table and the router mirror of tests/tapconv_contract.py.

What tests/test_tapconv_contract_gpu.py presupposes is decided here, on the host: the general reference is
F.conv2d / F.conv_transpose2d for every geometry of the table; it writes exactly the owned elements; the
integer draw stays below 2^23 at every stage and every gate tensor holds both zeros; the tile arithmetic the
table was sized for (297 -> 128 / 128 / 41, the c16conv grids of 189 and 2,442 pixels) follows from constants
pinned against the text of csrc/tapconv.hip and csrc/c16conv.hip; every TC(...) line, every route and every
epilogue code path has its cases."""
import functools
import os
import re

import pytest
import torch

from tests import tapconv_contract as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = TC.CASES + TC.IDENTITY + [c.forced for c in TC.IDENTITY]
ALL_IDS = [c.name for c in ALL]


@functools.lru_cache(None)
def source(name):
    text = open(os.path.join(ROOT, "mdil_ss_amd", "csrc", name)).read()
    return re.sub(r"\s+", " ", re.sub(r"//[^\n]*", "", text))


# ------------------------------------------------------------------------------------------------
# pins against the source text
# ------------------------------------------------------------------------------------------------
def test_constants_are_the_sources():
    assert re.findall(r"#define MDIL_WG (\d+)", source("common.h")) == [str(TC.MDIL_WG)]
    s = source("tapconv.hip")
    lines = re.findall(r"TC\((\d+), (\d+), (\d+), (true|false)\);", s)
    assert [(int(a), int(b), int(m), st == "true") for a, b, m, st in lines] == list(TC.TC_LINES)
    assert "const int grid = cdiv(npix, BM);" in s
    # the three epilogue code paths and what selects them
    assert "if constexpr (COUT % 4 == 0) {" in s
    assert "constexpr bool QINV = (MDIL_WG % (COUT / 4)) == 0;" in s
    assert "if constexpr (QINV) { v = v * vscale + vbias;" in s
    # the router: streaming kernels first, then c16conv, then the TC lines
    assert s.index("mdil_sconv(g, cin, cout, in0, in1, wpk, epi, out, nullptr") < s.index("mdil_c16conv_covers(g, cin, cout, epi)") \
        < s.index("TC(64, 64, 128, false);")
    c = source("c16conv.hip")
    assert re.findall(r"#define C16_TN_ (\d+)", c) == [str(TC.C16_TN)]
    assert re.findall(r"constexpr int C16_WAVES = (\d+);", c) == [str(TC.C16_WAVES)]
    assert "constexpr int C16_PXT = 16 * C16_TN;" in c
    assert "const int grid = (a.nwg + 7) / 8 * 8;" in c
    assert "const int per = gridDim.x >> 3;" in c and "const int g = (blockIdx.x & 7) * per + (blockIdx.x >> 3);" in c
    assert "if (e->res && e->gate) return false;" in c
    assert "static bool sconv_epilogue_ok(const mdil_epilogue* e) { return !(e->res && e->gate); }" in source("sconv.hip")
    assert "if (cin == 64 && g->ntaps == 4) return false;" in source("w4conv.hip")
    # F(2,3)'s only transform constant is 1/2: the integer draw stays exact there
    assert re.findall(r"\* (\d*\.\d+)f", source("wconv.hip").split("wconv_queues")[0]) == ["0.5"] * 4


def test_tile_arithmetic_of_the_table():
    N, HO, WO = TC.GRID
    npix = N * HO * WO
    assert npix == 297 and TC.IMAGE_ENDS == (HO * WO, 2 * HO * WO)
    assert TC.lds_tiles(npix, 128) == [128, 128, 41]
    assert TC.lds_tiles(npix, 64) == [64, 64, 64, 64, 41]
    for t, end in enumerate(TC.IMAGE_ENDS):                 # every tile but the last straddles an image end
        assert t * 128 < end < (t + 1) * 128
    assert all(end % 64 for end in TC.IMAGE_ENDS)
    assert {bm for _, _, bm, _ in TC.TC_LINES} == {64, 128}
    p = TC.c16_plan(3 * 9 * 7)
    assert (p.tiles, p.nwg, p.grid, p.empty, p.last_groups) == (6, 2, 8, 6, [16, 13])
    assert p.walk == list(range(8))
    p = TC.c16_plan(2 * 33 * 37)
    assert (p.tiles, p.nwg, p.grid, p.empty, p.last_groups) == (77, 20, 24, 4, [10, 0])
    assert sorted(p.walk) == list(range(24)) and p.walk != list(range(24))
    names = {c.name for c in TC.CASES}
    assert {"c16conv-3x9x7-d2h", "c16conv-2x33x37-d1w", "c16conv-3x9x7-d16h"} <= names
    d16 = TC.BY_NAME["c16conv-3x9x7-d16h"].g
    assert all(abs(d16.dh[t]) >= d16.HI for t in (0, 2)), "both side taps are out of range everywhere"


# ------------------------------------------------------------------------------------------------
# coverage of the table
# ------------------------------------------------------------------------------------------------
def test_every_instantiation_route_and_epilogue_path_has_its_cases():
    routes = {(c.name, f): TC.expected_route(c, f) for c in TC.CASES for f in c.forms}
    assert set(routes.values()) == set(TC.ROUTES)
    tiled = {}
    for (name, f), r in routes.items():
        c = TC.BY_NAME[name]
        if r == "tapconv":
            tiled.setdefault((c.cin, c.cout), set()).add(f)
    assert set(tiled) == {(ci, co) for ci, co, _, _ in TC.TC_LINES}
    paths = {}
    for (ci, co), forms in tiled.items():
        paths.setdefault(TC.epilogue_path(co), set()).update(forms)
    assert set(paths) == {"hoisted", "per-iteration", "scalar"}
    for forms in paths.values():
        assert {"E3", "E5", "E7", "E9"} <= forms
    assert {TC.epilogue_path(co) for co in (16, 64, 128)} == {"hoisted"}
    assert {TC.epilogue_path(co) for co in (48, 20)} == {"per-iteration"}
    assert {TC.epilogue_path(co) for co in (13, 27)} == {"scalar"}
    # the product's own forms on the product's geometries, in place where DownFn.backward is
    for c in TC.CASES:
        if c.part == "A" and not c.name.startswith("s1-"):
            assert set(TC.BASE_FORMS) <= set(c.forms), c.name
            assert ("E10" in c.forms) == c.parity, c.name
        if c.part == "B":
            assert c.forms == TC.ALL_FORMS, c.name
    # one out_coff = 4 case per epilogue path, inside a row 8 floats wider
    coff = [c for c in TC.CASES if c.g.out_coff]
    assert sorted(TC.epilogue_path(c.cout) for c in coff) == ["hoisted", "per-iteration", "scalar"]
    for c in coff:
        plain = TC.BY_NAME[c.name.replace("-coff4", "")]
        assert c.g.out_coff == 4 and c.g.out_pitch == plain.g.out_pitch + 8
    for r in ("c16conv", "sconv", "wconv", "w4conv"):       # each streaming route runs the whole matrix
        forms = {f for (n, f), rr in routes.items() if rr == r}
        assert forms == set(TC.ALL_FORMS) - {"E8"}, (r, forms)


@pytest.mark.parametrize("c", ALL, ids=ALL_IDS)
def test_expected_routes(c):
    for f in c.forms:
        r = TC.expected_route(c, f)
        assert r in TC.ROUTES
        both = "res" in TC.FORMS[f] and "gate" in TC.FORMS[f]
        assert both == (f == "E8")
        if c.expect is not None:            # the producer named by the table the shape came from; E8 falls back
            assert r == ("tapconv" if both else c.expect), (c.name, f, r)
        if c.part == "A":
            assert r == "tapconv", (c.name, f, r)
    g = c.g
    assert g.out_pitch % 4 == 0 and g.out_coff % 4 == 0 and g.out_coff + c.cout <= g.out_pitch
    assert c.stem or all(p % 4 == 0 for p in g.in_pitch)
    assert TC.exact_budget(c) < 2 ** 23


def test_identity_cases_force_the_tiled_kernel():
    for c in TC.IDENTITY:
        for f in c.forms:
            assert TC.expected_route(c, f) == c.expect and TC.expected_route(c.forced, f) == "tapconv"
        assert c.forced.g.out_pitch == 2 * c.cout and c.forced.gargs[:9] == c.gargs[:9]
    assert {c.expect for c in TC.IDENTITY} == {"c16conv", "sconv"}


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", TC.CASES, ids=[c.name for c in TC.CASES])
def test_reference_is_the_torch_convolution(c):
    t = TC.inputs(c.name, "normal")
    want = TC.layer_acc(c, t.in0, t.in1, t.w)
    torch.testing.assert_close(t.acc, want, rtol=1e-13, atol=1e-13)
    # through the public entry point, E0: the owned elements are the convolution, the rest is untouched
    g = c.ref_g
    before = torch.full((g.N, g.OH, g.OW, g.out_pitch), TC.SENTINEL)
    after = TC.reference(g, c.ref_cin, c.cout, t.in0, t.in1, t.W, TC.epilogue(), before)
    mask = TC.owned_mask(c.g, c.cout)
    assert torch.equal(after != TC.SENTINEL, mask), "write footprint"
    assert int(mask.sum()) == g.N * g.HO * g.WO * c.cout
    torch.testing.assert_close(after[mask], want.reshape(-1), rtol=1e-13, atol=1e-13)
    if c.in1 == "wide":
        assert t.in1.stride(2) == 128 and bool((t.in1_base[..., :64] == TC.FOREIGN).all())
    if c.g.in_pitch[0] > c.ref_cin:
        assert bool((t.in0[..., c.ref_cin:] == TC.FOREIGN).all())


def test_reference_feels_every_tap_and_the_foreign_channels_do_not_show():
    c = TC.BY_NAME["dhead27-16"]
    t = TC.inputs(c.name, "int")
    assert c.g.in_pitch[0] == 28 and bool((t.in0[..., 27] == TC.FOREIGN).all())
    assert float(t.acc.abs().max()) <= 9 * c.ref_ntaps * c.ref_cin
    for k in range(c.ref_ntaps):
        W = t.W.clone()
        W[k] = 0
        assert not torch.equal(TC.conv_acc(c.ref_g, c.ref_cin, c.cout, t.in0, t.in1, W), t.acc)


@pytest.mark.parametrize("form", TC.ALL_FORMS)
def test_epilogue_stages(form):
    """Every form on one parity-class case against the stages written out by hand, strict gates included."""
    c = TC.BY_NAME["up64-16-class11-coff4"]
    f = TC.FORMS[form]
    t, e, before, after = TC.expected(c, form, "int")
    mask = TC.owned_mask(c.g, c.cout)
    assert torch.equal(after[~mask], before.double()[~mask])
    v = t.acc.reshape(-1, c.cout).clone()
    pick = lambda x: x.double()[mask].reshape(-1, c.cout)
    if "bias" in f:
        v += e.bias.double()
    if "bias2" in f:
        v += e.bias2.double()
    if "scale" in f:
        v = v * e.scale.double() + e.shift.double()
    if "res" in f:
        r = pick(e.res)
        assert ("inplace" in f) == (e.res is before)
        v += r * (pick(e.res_gate) > 0) if "res_gate" in f else r
    if "relu" in f:
        v = v.relu()
    if "gate" in f:
        v = v * (pick(e.gate) > 0)
    assert torch.equal(after[mask].reshape(-1, c.cout), v)
    assert float(after[mask].abs().max()) <= TC.exact_budget(c)
    assert bool((after[mask] == after[mask].round()).all())
    for name in ("res_gate", "gate"):
        gt = getattr(e, name)
        assert (gt is not None) == (name in f)
        if gt is not None:
            assert TC.has_both_zeros(gt[mask].reshape(-1)) and float(gt.max()) > 0 > float(gt.min())
    if "scale" in f:
        assert set(e.scale.tolist()) <= set(TC.SCALE_VALUES) and bool((e.shift == e.shift.round()).all())


@pytest.mark.parametrize("c", TC.CASES + TC.IDENTITY, ids=[c.name for c in TC.CASES + TC.IDENTITY])
def test_gate_draws_hold_both_zeros_where_the_launch_reads_them(c):
    mask = TC.owned_mask(c.g, c.cout)
    for form in c.forms:
        _, e, _ = TC.operands(c, form, "int")
        for gt in (e.res_gate, e.gate):
            if gt is not None:
                assert TC.has_both_zeros(gt[mask])
