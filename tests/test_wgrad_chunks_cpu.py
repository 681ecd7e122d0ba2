"""CPU: the host mirror of the weight-gradient chunk plans (tests/wgrad_chunks.py) and the case table of
tests/test_wgrad_chunks_gpu.py.

The plans do not depend on the CU count, so everything the GPU cases presuppose -- which kernel takes
the launch, at least two stages / quads / tiles per chunk, chunks that cross a row end and an image end,
empty chunks, the exactness budget -- is decided here; the constants the mirror copies are pinned against
the text of csrc/wgrad.hip, so a change of plan fails here instead of silently moving the GPU cases back
to one stage per chunk."""
import functools
import os
import re

import pytest
import torch

from tests import wgrad_chunks as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(None)
def source():
    text = open(os.path.join(ROOT, "mdil_ss_amd", "csrc", "wgrad.hip")).read()
    return re.sub(r"\s+", " ", re.sub(r"//[^\n]*", "", text))


# ------------------------------------------------------------------------------------------------
# pins against the source text
# ------------------------------------------------------------------------------------------------
def test_constants_are_the_sources():
    s = source()
    assert re.findall(r"const int target = (\d+);", s) == [str(WC.TARGET)]
    assert re.findall(r"constexpr int WG16_CHUNKS = (\d+);", s) == [str(WC.WG16_CHUNKS)]
    assert re.findall(r'atoi\(getenv\("MDIL_WGRAD2_CUS"\)\) : (\d+);', s) == [str(WC.STREAM_GROUPS)]
    assert re.findall(r"int ngroups = (\d+) / NZ;", s) == [str(WC.STREAM_GROUPS)]              # launch_wgradw
    got = {(int(c), int(t)): int(w) for c, t, w in re.findall(r"launch_wgrad2<(\d+), (\d+), (\d+)>\(c, bt\)", s)}
    assert got == WC.CPW
    assert re.findall(r"constexpr int CPW = (\d+), NPOS = 4;", s) == [str(WC.CPW_W)] * 2       # wgradw, wgradx
    assert re.findall(r"constexpr int NB = C / 64, NZ = NB \* NB, CPW = (\d+);", s) == [str(WC.CPW_W)]
    assert "static constexpr int PS = (CO_P * CI_P <= 256) ? 256 : ((CO_P * CI_P <= 1024) ? 128 : 64);" in s
    assert "static constexpr int CI_P = STEM ? 32 : (CI + 15) / 16 * 16;" in s
    assert "int nch = target / (ntaps * nz);" in s
    assert "int nchunks = (int)((tiles + 3) / 4);" in s
    cfgs = {(int(a), int(b)): (int(c), int(d), e == "true")
            for a, b, c, d, e in re.findall(r"X\((\d+), (\d+), (\d+), (\d+), (true|false)\)", s)}
    assert cfgs == WC.WG_CONFIGS


def test_tile_configurations():
    """PS = 128 for the stem, the 16 <-> 48 / 64 sampler ends and the heads, 64 for the 64 x 64 tiles; only
    those split the tile over the waves; only the stem stages without the register prefetch."""
    ps = {k: WC.wg_cfg(*k).PS for k in WC.WG_CONFIGS}
    assert ps == {(64, 64): 64, (128, 128): 64, (64, 128): 64, (16, 16): 256, (48, 16): 128, (16, 64): 128,
                  (20, 16): 128, (27, 16): 128, (13, 27): 128}
    assert [k for k in WC.WG_CONFIGS if WC.wg_cfg(*k).TILE_SPLIT] == [(64, 64), (128, 128), (64, 128)]
    assert [k for k in WC.WG_CONFIGS if not WC.wg_cfg(*k).PIPE] == [(13, 27)]


# ------------------------------------------------------------------------------------------------
# thresholds: one stage / quad / tile per chunk at the limit, two just beyond
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntaps,cout,cin,limit", [
    (9, 48, 16, 10880), (9, 64, 64, 5440),           # down-sampler convs
    (1, 64, 128, 24576),                             # 1-tap class of the 128 -> 64 up-sampler
    (1, 16, 64, 98304), (1, 20, 16, 98304), (1, 27, 16, 98304), (1, 13, 27, 98304),
])
def test_lds_second_stage_threshold(ntaps, cout, cin, limit):
    c = WC.wg_cfg(cout, cin)
    assert limit == WC.TARGET // (ntaps * c.nz_co * c.nz_ci) * c.PS
    at, over = WC.lds_plan(limit, ntaps, cout, cin), WC.lds_plan(limit + 1, ntaps, cout, cin)
    assert at.per_chunk == 1 and at.chunks == limit // c.PS
    assert over.per_chunk == 2 and over.last_chunk == 2 - over.total % 2 and over.last_px == 1
    assert WC.lds_chunks_from_workspace(over.ws_bytes, ntaps, cout, cin) == over.chunks


@pytest.mark.parametrize("sub,C,ntaps,W,rows_at", [
    ("wgrad2", 64, 3, 16, 512), ("wgrad2", 64, 4, 16, 512), ("wgradx", 64, 3, 32, 512), ("wgradw", 64, 3, 16, 1024),
    ("wgrad2", 128, 3, 16, 256), ("wgrad2", 128, 4, 16, 128), ("wgradw", 128, 3, 16, 256), ("wgradx", 128, 3, 32, 128),
])
def test_streaming_second_quad_threshold(sub, C, ntaps, W, rows_at):
    """One work item per image row (pair of rows for wgradw): ``rows_at`` rows fill every chunk slot once."""
    at = WC.stream_plan(sub, C, ntaps, 1, rows_at, W)
    assert at.per_chunk == 1 and at.total == at.chunks and at.empty == 0
    step = 2 if sub == "wgradw" else 1
    over = WC.stream_plan(sub, C, ntaps, 1, rows_at + step, W)
    assert over.per_chunk == 2 and over.total == at.total + 1 and over.empty == at.chunks - cdiv2(over.total)
    if C == 64:
        assert at.total == 512          # the issue's figure: more than 512 quads at C = 64


def cdiv2(n):
    return (n + 1) // 2


def test_wgrad16_second_tile_threshold():
    at, over = WC.wg16_plan(65536), WC.wg16_plan(65537)
    assert at.per_chunk == 1 and at.empty == 0 and at.chunks == 4096
    assert over.per_chunk == 2 and over.empty == 4096 - 2049 and over.last_px == 1
    assert WC.wg16_plan(8580).per_chunk == 1        # the largest case of test_tapconv_factorised


def test_existing_parity_shapes_run_one_stage_per_chunk():
    """What the issue rests on: test_down_block / test_up_block / test_output_conv and the W = 64 cases."""
    for kind, cin, cout, H, W in [("stem", 3, 16, 16, 24), ("down", 16, 64, 12, 40), ("down", 64, 128, 8, 12),
                                  ("up", 128, 64, 6, 10), ("up", 64, 16, 10, 12), ("out", 16, 20, 10, 12),
                                  ("out", 16, 27, 10, 12)]:
        c = WC._case("x", kind, cin, cout, H, W)
        for g, ci, co in WC.host_launches(c):
            assert WC.plan_for(g, ci, co).per_chunk == 1, (kind, cin, cout)
    for H, d in ((33, 4), (40, 4)):       # C = 128, W = 64: two quads per chunk, four per row: no crossing
        p = WC.plan_for(WC.geom(2, H, 64, H, 64, WC.taps3(d, "h"), 128, H, 64, 128), 128, 128)
        assert p.per_chunk == 2 and not p.row_cross and not p.image_cross, (H, p)


# ------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------
def plans(c):
    return [WC.plan_for(g, ci, co) for g, ci, co in WC.host_launches(c)]


@pytest.mark.parametrize("c", WC.CASES, ids=WC.CASE_IDS)
def test_case_meets_its_preconditions(c):
    ps = plans(c)
    for (g, ci, co), p in zip(WC.host_launches(c), ps):
        print(WC.plan_line(c.name, p))
        assert p.family == c.family, (c.name, p.family)
        assert c.sub is None or p.sub == c.sub, (c.name, p.sub)
        assert p.per_chunk >= 2, (c.name, p.per_chunk)
        assert WC.exact_budget(g.N * g.HO * g.WO) < 2 ** 23, c.name
    if c.cross is not None:
        p = ps[0]
        assert bool(p.row_cross) == ("r" in c.cross) and bool(p.image_cross) == ("i" in c.cross), (c.name, p)


def test_every_streaming_kernel_crosses_a_row_end_and_an_image_end():
    seen = {}
    for c in WC.CASES:
        if c.cross is not None:
            seen.setdefault(c.sub, set()).update(c.cross)
    assert seen == {k: {"r", "i"} for k in (
        "wgrad2_kernel<64,3,2>", "wgrad2_kernel<64,4,2>", "wgrad2_kernel<128,3,4>", "wgrad2_kernel<128,4,2>",
        "wgradw_kernel<64>", "wgradw_kernel<128>", "wgradx_kernel<64>", "wgradx_kernel<128>")}


def test_the_quoted_plans():
    """The figures of DESIGN.md's case table."""
    P = {c.name: plans(c) for c in WC.CASES}
    p = P["stem"][0]
    assert (p.total, p.per_chunk, p.chunks, p.last_chunk, p.last_px, p.cfg.PS) == (781, 2, 391, 1, 60, 128)
    p = P["down16-64"][0]
    assert (p.total, p.per_chunk, p.last_chunk, p.last_px, p.cfg.PS) == (93, 2, 1, 50, 128)
    p = P["down64-128"][0]
    assert (p.total, p.per_chunk, p.last_px, p.cfg.PS) == (93, 2, 48, 64)
    assert [(p.total, p.ntaps, p.per_chunk) for p in P["up128-64"]] == [(389, 1, 2), (389, 2, 3), (389, 2, 3), (389, 4, 5)]
    for name in ("up64-16", "head20", "head27"):
        assert all((p.total, p.last_px, p.cfg.PS) == (771, 8, 128) for p in P[name]), name
    assert [p.per_chunk for p in P["up64-16"]] == [2, 3, 3, 5]
    assert [p.per_chunk for p in P["head20"]] == [2] * 4 and [p.per_chunk for p in P["head27"]] == [2] * 4
    for name in ("wgrad2<64,3> 3x1 d1", "wgrad2<64,3> 1x3 d2", "wgrad2<64,4> 1x3 d2 + adapter", "wgradw<64> 3x1 d1"):
        p = P[name][0]
        assert (p.total, p.per_chunk, p.empty, p.per_row, p.per_image) == (670, 2, 177, 5, 335), name
    p = P["wgradx<64> 1x3 d1"][0]
    assert (p.total, p.per_chunk, p.per_row, p.per_image) == (546, 2, 3, 273)
    p = P["wgrad2<128,3> 3x1 d2"][0]
    assert (p.total, p.per_chunk, p.groups, p.per_row, p.per_image) == (270, 2, 64, 3, 135)
    p = P["wgrad16 3x1"][0]
    assert (p.total, p.per_chunk, p.last_px, p.chunks, p.empty) == (4112, 2, 14, 4096, 2040)


# ------------------------------------------------------------------------------------------------
# draws and reference
# ------------------------------------------------------------------------------------------------
def test_draws():
    a = WC.draw_int((4, 5, 6, 7), 3)
    assert a.dtype == torch.float32 and set(a.unique().tolist()) == set(WC.INT_VALUES)
    assert torch.equal(a, WC.draw_int((4, 5, 6, 7), 3)) and not torch.equal(a, WC.draw_int((4, 5, 6, 7), 4))
    assert WC.draw_normal((3, 4), 1).dtype == torch.float32


def test_mismatch_report_counts_per_tap():
    w = torch.zeros(4, 5, 3, 3)
    g = w.clone()
    g[1, 2, 0, 1] = 2
    g[3, 0, 2, 2] = -1
    msg = WC.mismatch_report("dW", g, w)
    assert "2/180" in msg and "[0, 1, 0, 0, 0, 0, 0, 0, 1]" in msg and "2.0" in msg
    assert WC.mismatch_report("dW", w, w) == ""


@pytest.mark.parametrize("c", WC.CASES, ids=WC.CASE_IDS)
def test_reference_feels_every_pixel(c):
    """The reference with ONE pixel of gout zeroed -- the first pixel of chunk 0's second stage, the last
    valid pixel, the first pixel of the second image -- differs from the full one in every (co, ci) of
    every tap that is inside the image there (and in no other tap), in every bias element, and the
    integer results fit fp32 exactly."""
    t = WC.draw_case(c, WC.draw_int)
    g, ci, co = WC.host_launches(c)[0]
    full = WC.reference(c, t)
    for k, v in full.items():
        assert torch.equal(v, v.round()) and float(v.abs().max()) < 2 ** 24, (c.name, k)
        assert torch.equal(v.float().double(), v)
    (gs, _) = WC.gout_shape(c)
    for n, h, w in (WC.second_unit_pixel(WC.plan_for(g, ci, co), g), (c.N - 1, gs[1] - 1, gs[2] - 1), (1, 0, 0)):
        gz = t["gout"].clone()
        gz[n, h, w] = 0
        part = WC.reference(c, t, gout=gz)
        inside = WC.taps_inside(c, n, h, w)
        assert inside.any()
        moved = full["dw"] != part["dw"]
        assert torch.equal(moved, inside[None, None].expand_as(moved)), (c.name, (n, h, w))
        assert bool((full["db"] != part["db"]).all())
        if "dw2" in full:
            assert bool((full["dw2"] != part["dw2"]).all()) and bool((full["db2"] != part["db2"]).all())
