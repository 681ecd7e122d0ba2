"""GPU: the segments kernels (mdil_ss_amd/ext/segments.hip) and the entry points over them
(mdil_ss_amd/segments.py) against the numpy reference of tests/segments_reference.py.  The kernels
are integer only, so every comparison is exact equality: roots, areas, the per-segment sums, every
counter and the filtered map.  The cases sit where a union-find over pixels can go wrong: a single
pixel, a single row and a single column, corner contacts, runs that merge far below where they
start, a parent chain as long as its segment, thousands of one-pixel segments, the borders between
rows and between the images of a batch, every add on one address, labels outside the classes, and a
map past the grid caps."""
import ctypes as C
import functools
import glob
import json
import os
import shutil
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import head_cases as HC
from tests import segments_reference as R

pytestmark = pytest.mark.gpu

EDGES = (1, 4, 16, 64, 256)
ALL8 = (1, 2, 4, 8, 16, 64, 256, 1 << 20)
MAX_ROW_BLOCKS, MAX_BLOCKS = 4096, 2048                    # kMaxRowBlocks, kMaxBlocks of segments.hip


@pytest.fixture(scope="module")
def dev():
    return HC.device("segments")


def perturbed(target, n_labels, seed, shift=2, share=0.01):
    """A prediction: the target moved ``shift`` pixels right and down, ``share`` of the pixels redrawn."""
    rng = np.random.default_rng(seed)
    pred = np.roll(target, (shift, shift), axis=(-2, -1))
    flip = rng.random(target.shape) < share
    pred[flip] = rng.integers(0, n_labels, int(flip.sum()), dtype=np.uint8)
    return np.ascontiguousarray(pred)


@functools.lru_cache(maxsize=None)
def procedural(nc):
    from mdil_ss_amd.dataset import ProceduralSeg
    ds = ProceduralSeg(2, 96, 200, nc, seed=2, domain=1)
    target = np.stack([ds[i][1][0].numpy().astype(np.uint8) for i in range(2)])
    return target, perturbed(target, nc, seed=nc)


def one_row():
    """Runs that cross the 64-lane and the 256-pixel chunk of the row pass; 333 is no multiple of 4."""
    return np.repeat(np.array([0, 1, 0, 2, 2], dtype=np.uint8), [70, 200, 1, 61, 1]).reshape(1, 1, 333)


def batch_borders():
    t = R.blocky((2, 37, 131), 20, seed=6, block=11)
    t[:, 1:, 0] = t[:, :-1, -1]                             # every row begins as the row above ends
    t[1, 0] = t[0, -1]                                      # image 1 begins as image 0 ends
    t[1, 1, 0] = t[1, 0, -1]
    return t


def out_of_range(nc):
    """The map holds labels nc and nc + 1 (outside the classes) and a band of 200 (its ignore id);
    the other map a band of 255 (its ignore id) that swallows one segment of the map whole."""
    m = R.blocky((2, 33, 47), nc + 2, seed=4, block=7)
    o = R.blocky((2, 33, 47), nc + 3, seed=3)
    o[0, 5:9, 5:30] = 255
    m[0, 5:9, 5:30] = 1
    m[0, 6:8, 10:14] = 0                                    # eight pixels, all under the other map's 255
    m[1, 20:25, :] = 200
    o[1, 0:4, 0:9] = m[1, 0:4, 0:9]                         # and some segments the other map agrees with
    return m, o


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (map, other u8 [N,H,W], nc, edges, map_ignore, other_ignore, (cover_num, cover_den))."""
    half = (1, 2)
    if name == "one pixel":
        return np.zeros((1, 1, 1), np.uint8), np.ones((1, 1, 1), np.uint8), 2, EDGES, -1, -1, half
    if name == "one row":
        m = one_row()
        return m, perturbed(m, 3, 1, shift=3, share=0.05), 3, EDGES, -1, -1, half
    if name == "one column":
        m = np.ascontiguousarray(one_row().transpose(0, 2, 1))
        return m, perturbed(m, 3, 1, shift=3, share=0.05), 3, EDGES, -1, -1, half
    if name == "checkerboard":
        m = R.checkerboard(33, 47)[None]
        return m, np.ascontiguousarray(1 - m), 2, EDGES, -1, -1, half
    if name == "diagonal":
        m = R.diagonal()[None]
        return m, np.ascontiguousarray(np.roll(m, 1, axis=2)), 3, EDGES, -1, -1, half
    if name == "comb":
        m = R.comb(40, 9)[None]
        return m, perturbed(m, 2, 2, shift=1), 2, EDGES, -1, -1, half
    if name == "spiral":
        m = R.spiral(129)[None]
        return m, perturbed(m, 2, 3, shift=1), 2, ALL8, -1, -1, half
    if name == "noise":
        m = R.noise((1, 200, 300), seed=3)
        return m, R.noise((1, 200, 300), seed=4), 2, EDGES, -1, -1, (3, 4)
    if name == "batch borders":
        m = batch_borders()
        return m, perturbed(m, 20, 6), 20, EDGES, 19, -1, half
    if name == "one label everywhere":
        m = np.full((3, 64, 64), 6, dtype=np.uint8)
        return m, perturbed(m, 8, 7, share=0.3), 8, (64, 4096), -1, -1, half
    if name == "labels outside the classes":
        m, o = out_of_range(6)
        return m, o, 6, EDGES, 200, 255, half
    if name == "two classes":
        m = R.blocky((1, 40, 72), 2, seed=9, block=13)
        return m, perturbed(m, 2, 9), 2, EDGES, -1, -1, (1, 1)
    if name == "32 classes":
        m = R.blocky((1, 40, 72), 32, seed=10, block=6)
        return m, perturbed(m, 32, 10, share=0.05), 32, EDGES, 31, -1, half
    if name == "eight edges":
        m = R.blocky((2, 37, 130), 5, seed=11, block=9)
        return m, perturbed(m, 5, 11), 5, ALL8, -1, 4, (999, 1000)
    if name in ("procedural 20", "procedural 27"):
        nc = int(name.split()[1])
        t, p = procedural(nc)
        return (t, p, nc, EDGES, 19, -1, half) if nc == 20 else (p, t, nc, ALL8, -1, 26, half)
    if name == "past the grid caps":
        m = R.blocky((1, 16500, 136), 9, seed=12, block=23)
        return m, perturbed(m, 9, 12, share=0.002), 9, (512, 2048), 8, -1, half
    raise KeyError(name)


CASES = ["one pixel", "one row", "one column", "checkerboard", "diagonal", "comb", "spiral", "noise", "batch borders",
         "one label everywhere", "labels outside the classes", "two classes", "32 classes", "eight edges",
         "procedural 20", "procedural 27", "past the grid caps"]
RUNS = [(n, c) for n in CASES for c in ((8,) if n == "past the grid caps" else (4, 8))]


@functools.lru_cache(maxsize=None)
def expected(name, connectivity):
    """-> (root, area, hit, void, counters) of the reference; computed once, shared and never modified."""
    m, o, nc, edges, m_ign, o_ign, cover = inputs(name)
    root, area = R.label(m, connectivity)
    if m.size <= 2000:                                      # the definition itself where it is cheap
        assert np.array_equal(root, R.label(m, connectivity, R.roots_flood)[0])
    counters, hit, void = R.counters(m, o, root, area, nc, m_ign, o_ign, edges, *cover)
    return root, area, hit, void, counters


def run(dev, name, connectivity, counters=None, overlap=True, images=None, **kw):
    from mdil_ss_amd import segments as S
    m, o, nc, edges, m_ign, o_ign, cover = inputs(name)
    if images is not None:
        m, o = np.ascontiguousarray(m[images]), np.ascontiguousarray(o[images])
    counters = S.new_counters(nc, len(edges) + 1, dev) if counters is None else counters
    md, od = torch.from_numpy(m).to(dev), torch.from_numpy(o).to(dev)
    root, area = S.label(md, connectivity, **kw)
    hit, void = S.segment_count(md, od, root, area, nc, edges, map_ignore=m_ign, other_ignore=o_ign,
                                coverage=Fraction(*cover), counters=counters, overlap=overlap, **kw)
    torch.cuda.synchronize()
    return (root.cpu().numpy(), area.cpu().numpy(), None if hit is None else hit.cpu().numpy(),
            None if void is None else void.cpu().numpy(), {k: v.cpu().numpy() for k, v in counters.items()})


def check_counters(got, want, times=1):
    assert sorted(got) == sorted(R.COUNTERS)
    for k in R.COUNTERS:
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], times * want[k]), k


def check_maps(got, want):
    for k, what in enumerate(("root", "area", "hit", "void")):
        assert got[k].dtype == np.int32 and got[k].shape == want[k].shape, what
        assert np.array_equal(got[k], want[k]), \
            f"{what} differs at {int((got[k] != want[k]).sum())} of {want[k].size} pixels"


@pytest.mark.parametrize("name, connectivity", RUNS)
def test_segments_and_counters_are_exact(dev, name, connectivity):
    want = expected(name, connectivity)
    got = run(dev, name, connectivity)
    check_maps(got, want)
    check_counters(got[4], want[4])
    m, _, nc, _, m_ign, _, _ = inputs(name)
    assert got[1].sum() == m.size                           # every pixel belongs to exactly one segment
    c = got[4]
    assert c["segments"].sum() + c["unjudged"].sum() == int(((want[1] > 0) & (m != m_ign) & (m < nc)).sum())


def test_the_cases_reach_what_they_are_for():
    """Properties of the inputs, so that a case cannot quietly stop testing its point."""
    def n(name, c):
        return R.n_segments(expected(name, c)[1])
    assert (n("one pixel", 4), n("one pixel", 8)) == (1, 1)
    assert n("one row", 8) == n("one column", 4) == 4 and inputs("one row")[0].shape[2] % 4 != 0
    assert (n("checkerboard", 4), n("checkerboard", 8)) == (33 * 47, 2) == (1551, 2)
    assert (n("diagonal", 4), n("diagonal", 8)) == (5, 3)
    assert n("comb", 4) == n("comb", 8) == 9
    assert n("spiral", 4) == n("spiral", 8) == 2 and expected("spiral", 4)[1].max() > 129 * 129 // 2 - 129
    assert n("noise", 4) > 5000 > 1000 > n("noise", 8) and (expected("noise", 4)[1] == 1).sum() > 1000
    m = inputs("batch borders")[0]
    assert np.array_equal(m[1, 0], m[0, -1]) and np.array_equal(m[:, 1:, 0], m[:, :-1, -1])
    r4 = expected("batch borders", 4)[0]
    assert (r4[0, 1:, 0] != r4[0, :-1, -1]).any()          # equal labels across the row border, other segments
    assert n("one label everywhere", 8) == 3 and (expected("one label everywhere", 8)[1][:, 0, 0] == 4096).all()
    m, o, nc, _, m_ign, o_ign, _ = inputs("labels outside the classes")
    c = expected("labels outside the classes", 8)[4]
    assert c["bad_labels"][0] > 0 and (m == m_ign).any() and (o == o_ign).any() and (m >= nc).any()
    assert c["unjudged"].sum() > 0 and c["missed"].sum() > 0 and c["covered"].sum() > 0
    assert 0 < (c["covered"] + c["missed"]).sum() < c["segments"].sum()          # and some partly hit
    assert inputs("two classes")[2] == 2 and inputs("32 classes")[2] == 32
    edges = inputs("eight edges")[3]
    assert len(edges) == 8 and edges[-1] > expected("eight edges", 4)[1].max()
    assert (inputs("procedural 20")[0] == 19).any()         # the ignore class is there to be ignored
    N, H, W = inputs("past the grid caps")[0].shape
    assert N * H > MAX_ROW_BLOCKS * 4 and N * H * ((W + 3) // 4) > MAX_BLOCKS * 256


@pytest.mark.parametrize("name", ["batch borders", "procedural 20"])
def test_counters_accumulate_and_the_sums_are_optional(dev, name):
    from mdil_ss_amd import segments as S
    m, _, nc, edges = inputs(name)[:4]
    want = expected(name, 8)
    counters = S.new_counters(nc, len(edges) + 1, dev)
    ws = torch.empty(S.workspace_bytes(*m.shape) + 64, dtype=torch.uint8, device=dev)
    a = run(dev, name, 8, counters=counters, overlap=False, workspace=ws)
    assert a[2] is None and a[3] is None
    check_counters(a[4], want[4])                           # without the two maps: the same counts
    b = run(dev, name, 8, counters=counters, overlap=True, workspace=ws)
    check_maps(b, want)
    check_counters(b[4], want[4], times=2)                  # added to, never cleared


@pytest.mark.parametrize("connectivity", (4, 8))
def test_images_of_a_batch_never_see_each_other(dev, connectivity):
    """Each image alone gives the roots and areas it has inside the batch, and the counts add up."""
    want = expected("batch borders", connectivity)
    total = None
    for n in range(2):
        got = run(dev, "batch borders", connectivity, images=slice(n, n + 1))
        for k in range(4):
            assert np.array_equal(got[k][0], want[k][n])
        total = got[4] if total is None else {k: total[k] + got[4][k] for k in total}
    check_counters(total, want[4])


def test_side_stream_gives_the_same(dev):
    want = expected("procedural 27", 8)
    got = HC.side_stream(lambda: run(dev, "procedural 27", 8))
    check_maps(got, want)
    check_counters(got[4], want[4])


@pytest.mark.parametrize("name", ["noise", "spiral", "one label everywhere"])
def test_two_runs_give_identical_bytes(dev, name):
    """The order in which the atomics arrive changes nothing."""
    a, b = run(dev, name, 4), run(dev, name, 4)
    for k in range(4):
        assert a[k].tobytes() == b[k].tobytes()
    assert all(a[4][k].tobytes() == b[4][k].tobytes() for k in a[4])


def least_areas(seed=5):
    least = np.random.default_rng(seed).integers(1, 40, 256).astype(np.int32)
    least[0], least[1], least[3] = 0, 30, 1 << 30           # label 0 always stays, label 3 always goes
    return least


def test_guard_bands_and_the_workspace_bound(dev):
    """Every output inside a 0xA5-filled arena and a workspace of exactly the promised size with a
    guard behind it: nothing outside root, area, hit, void, out and the workspace is written."""
    from mdil_ss_amd import _segments_lib
    from mdil_ss_amd import segments as S
    lib = _segments_lib.load()
    name = "batch borders"
    m, o, nc, edges, m_ign, o_ign, cover = inputs(name)
    want = expected(name, 8)
    N, H, W = m.shape
    assert W % 4 != 0
    need = lib.mdil_segments_workspace_bytes(N, H, W)
    arena = HC.Arena(dev, {"root": 4 * m.size, "area": 4 * m.size, "workspace": need, "hit": 4 * m.size,
                           "void": 4 * m.size, "out": m.size})
    counters = S.new_counters(nc, len(edges) + 1, dev)
    removed = torch.zeros(2, 256, dtype=torch.int64, device=dev)
    md, od = torch.from_numpy(m).to(dev), torch.from_numpy(o).to(dev)
    least = torch.from_numpy(least_areas()).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.mdil_segments_label(md.data_ptr(), N, H, W, 8, arena.ptr("root"), arena.ptr("area"),
                                 arena.ptr("workspace"), need, stream)
    assert rc == 0, lib.mdil_segments_last_error()
    rc = lib.mdil_segments_count(md.data_ptr(), od.data_ptr(), arena.ptr("root"), arena.ptr("area"), N, H, W, nc,
                                 m_ign, o_ign, (C.c_int * len(edges))(*edges), len(edges), cover[0], cover[1],
                                 arena.ptr("workspace"), need, arena.ptr("hit"), arena.ptr("void"),
                                 *(counters[k].data_ptr() for k in S.COUNTERS), stream)
    assert rc == 0, lib.mdil_segments_last_error()
    rc = lib.mdil_segments_filter(md.data_ptr(), arena.ptr("root"), arena.ptr("area"), N, H, W, least.data_ptr(), 19,
                                  255, arena.ptr("out"), removed[0].data_ptr(), removed[1].data_ptr(), stream)
    assert rc == 0, lib.mdil_segments_last_error()
    torch.cuda.synchronize()
    arena.read()
    arena.assert_untouched(("root", "area", "workspace", "hit", "void", "out"))
    for k, what in enumerate(("root", "area", "hit", "void")):
        got = arena.cut(what).numpy().view(np.int32).reshape(m.shape)
        assert np.array_equal(got, want[k]), what
    check_counters({k: v.cpu().numpy() for k, v in counters.items()}, want[4])
    out, seg, pix = R.filter(m, want[0], want[1], least_areas(), 19, 255)
    assert np.array_equal(arena.cut("out").numpy().reshape(m.shape), out)
    assert np.array_equal(removed.cpu().numpy(), np.stack([seg, pix]))
    # without hit and void the sums live in the workspace, and nothing else changes
    again = S.new_counters(nc, len(edges) + 1, dev)
    rc = lib.mdil_segments_count(md.data_ptr(), od.data_ptr(), arena.ptr("root"), arena.ptr("area"), N, H, W, nc,
                                 m_ign, o_ign, (C.c_int * len(edges))(*edges), len(edges), cover[0], cover[1],
                                 arena.ptr("workspace"), need, None, None,
                                 *(again[k].data_ptr() for k in S.COUNTERS), stream)
    assert rc == 0, lib.mdil_segments_last_error()
    torch.cuda.synchronize()
    before = arena.bytes.clone()
    arena.read()
    s, e = arena.off["workspace"], arena.off["workspace"] + need
    assert torch.equal(arena.bytes[:s], before[:s]) and torch.equal(arena.bytes[e:], before[e:])
    check_counters({k: v.cpu().numpy() for k, v in again.items()}, want[4])


@pytest.mark.parametrize("name", ["noise", "procedural 20", "procedural 27"])
@pytest.mark.parametrize("connectivity", (4, 8))
def test_despeckle_equals_the_reference(dev, name, connectivity):
    from mdil_ss_amd import segments as S
    m = inputs(name)[0]
    least = least_areas()
    if name == "noise":
        least[:2] = (3, 9)                                  # both labels lose segments, and keep some
    root, area = expected(name, connectivity)[:2]
    for keep_id, fill in ((255, 255), (1, 0), (-1, 7)):
        want, seg, pix = R.filter(m, root, area, least, keep_id, fill)
        out, removed = S.despeckle(torch.from_numpy(m).to(dev), torch.from_numpy(least), keep_id=keep_id, fill=fill,
                                   connectivity=connectivity)
        assert out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), want)
        assert np.array_equal(removed["segments"].cpu().numpy(), seg), (keep_id, fill)
        assert np.array_equal(removed["pixels"].cpu().numpy(), pix), (keep_id, fill)
        if keep_id >= 0:
            assert seg[keep_id] == 0 and pix[keep_id] == 0 and (out.cpu().numpy()[m == keep_id] == keep_id).all()
    # the cases remove something and keep something, and a kept label survives whatever its area
    want, seg, pix = R.filter(m, root, area, least, 1, 0)
    assert 0 < pix.sum() < m.size and seg.sum() > 0 and (want[m == 1] == 1).all()
    tiny = (area > 0) & (area < least[m]) & (m == 1)
    assert name == "procedural 20" or tiny.any()            # label 1 has segments the filter would remove
    one, gone = S.despeckle(torch.from_numpy(m).to(dev), 1 << 30, keep_id=3, fill=9, connectivity=connectivity)
    assert np.array_equal(one.cpu().numpy(), np.where(m == 3, 3, 9))
    assert int(gone["pixels"].sum()) == int((m != 3).sum())


def test_meter_ties_to_the_confusion_matrix_of_fullres(dev):
    """The same features and target through SegmentMeter and through the shipped ConfusionMeter:
    the pixels the segments are judged on are the matrix's pixels, row by row and column by column."""
    from mdil_ss_amd import fullres as F
    from mdil_ss_amd import segments as S
    nc, size = 20, (45, 77)
    g = torch.Generator().manual_seed(3)
    x = torch.relu(torch.randn(2, 12, 20, 16, generator=g)).to(dev)
    w, b = (torch.randn(16, nc, 2, 2, generator=g) * 0.3).to(dev), (torch.randn(nc, generator=g) * 0.2).to(dev)
    target = torch.from_numpy(R.blocky((2,) + size, nc, seed=11, block=9)).to(dev)
    shipped = F.ConfusionMeter(nc, nc - 1)
    label = shipped.add(x, w, b, target=target)[0]
    meter = S.SegmentMeter(nc, nc - 1, edges=[4, 32, 200])
    pred, seen = meter.add(x, w, b, target=target, overlap=True)
    assert torch.equal(pred, label) and sorted(seen) == ["area", "hit", "root"]
    c, matrix = meter.counters(), shipped.matrix()
    assert torch.equal(c["target"]["hit_pixels"].sum(1), matrix.diagonal())
    assert torch.equal(c["target"]["pixels"].sum(1), matrix.sum(1))
    assert torch.equal(c["pred"]["pixels"].sum(1), matrix.sum(0))
    # (a predicted pixel of the ignore class under an ignored target is both hit and void by the header's
    # definitions, so the prediction side's hit_pixels equal the diagonal only below the ignore class)
    assert torch.equal(c["pred"]["hit_pixels"].sum(1)[:nc - 1], matrix.diagonal()[:nc - 1])
    # and both sides are the reference's on the kernel's own label map
    p, t = pred.cpu().numpy(), target.cpu().numpy()
    for side, a, o, a_ign, o_ign in (("target", t, p, nc - 1, -1), ("pred", p, t, -1, nc - 1)):
        root, area = R.label(a, 8)
        want, hit, _ = R.counters(a, o, root, area, nc, a_ign, o_ign, [4, 32, 200], 1, 2)
        check_counters({k: v.numpy() for k, v in c[side].items()}, want)
        if side == "target":
            assert np.array_equal(seen["root"].cpu().numpy(), root) and np.array_equal(seen["hit"].cpu().numpy(), hit)
    rep = meter.report()
    assert rep["segment_recall"]["total"] == int(c["target"]["covered"].sum()) / int(c["target"]["segments"].sum())
    assert rep["edges"] == [4, 32, 200] and rep["coverage"] == [1, 2] and rep["connectivity"] == 8


def test_meter_accumulates_and_refuses_bad_labels(dev):
    from mdil_ss_amd import segments as S
    t, p = procedural(20)
    td, pd = torch.from_numpy(t).to(dev), torch.from_numpy(p).to(dev)
    meter = S.SegmentMeter(20, 19, edges=EDGES, connectivity=4)
    meter.add(pd, td)
    meter.add(pd[:, :40, :64].contiguous(), td[:, :40, :64].contiguous())
    ts, ps = np.ascontiguousarray(t[:, :40, :64]), np.ascontiguousarray(p[:, :40, :64])
    c = meter.counters()
    for side, pairs, a_ign, o_ign in (("target", ((t, p), (ts, ps)), 19, -1), ("pred", ((p, t), (ps, ts)), -1, 19)):
        want = None
        for a, o in pairs:
            one = R.counters(a, o, *R.label(a, 4), 20, a_ign, o_ign, EDGES, 1, 2)[0]
            want = one if want is None else {k: want[k] + one[k] for k in one}
        check_counters({k: v.numpy() for k, v in c[side].items()}, want)
    bad = td.clone()
    bad[0, 0, :5] = 77
    meter.add(pd, bad)
    with pytest.raises(RuntimeError, match="5 target pixels are outside"):
        meter.report()
    meter = S.SegmentMeter(20, 19)
    worse = pd.clone()
    worse[1, 3, :9] = 99
    meter.add(worse, td)
    with pytest.raises(RuntimeError, match="9 predicted pixels are outside"):
        meter.report()


@pytest.fixture(scope="module")
def tiny_model(dev):
    return HC.tiny_model(dev)


def test_cli_end_to_end(dev, tiny_model, tmp_path):
    """--synthetic 3 at a native size of 96 x 200 through a 64 x 128 network, in-process: once from
    the checkpoint with --score --json --out, once with --pred on the label PNGs that a
    ``fullres --out`` run wrote.  Both reports hold the same counters, those of the reference on the
    label maps of ``predict_fullres``; the PNGs have the native size and only the declared colours."""
    from PIL import Image
    from mdil_ss_amd import fullres as FR
    from mdil_ss_amd import segments as S
    from mdil_ss_amd.dataset import ProceduralSeg
    ckpt, maps, seen = tmp_path / "checkpoint.pth.tar", tmp_path / "maps", tmp_path / "seen"
    first, second = tmp_path / "first.json", tmp_path / "second.json"
    HC.save_checkpoint(tiny_model, ckpt)
    data = ["--num-classes", "20", "20", "--task", "1", "--synthetic", "3", "--native-height", "96",
            "--native-width", "200", "--height", "64", "--width", "128"]
    how = ["--edges", "8", "64", "512", "--coverage", "0.75"]
    a = S.main(S.build_parser().parse_args(data + how + ["--state", str(ckpt), "--score", "--json", str(first), "--out",
                                                         str(seen)]))
    FR.main(FR.build_parser().parse_args(data + ["--state", str(ckpt), "--out", str(maps)]))
    b = S.main(S.build_parser().parse_args(data + how + ["--pred", str(maps), "--score", "--json", str(second)]))
    ja, jb = json.load(open(first)), json.load(open(second))
    assert ja["counters"] == jb["counters"] == a["counters"] == b["counters"]
    for k in ("segment_recall", "missed_share", "pixel_recall", "segment_precision", "hallucinated_share", "unjudged",
              "edges", "coverage", "connectivity", "target_segments", "pred_segments"):
        assert ja[k] == jb[k] == a[k], k
    assert jb["written"] == [] and ja["images"] == 3 and ja["edges"] == [8, 64, 512] and ja["coverage"] == [3, 4]

    ds = ProceduralSeg(3, 96, 200, 20, seed=13, domain=1)
    samples = [FR.synthetic_sample(ds, i, 64, 128) for i in range(3)]
    images = torch.from_numpy(np.stack([im for im, _ in samples])).to(dev).permute(0, 3, 1, 2).float().div(255.0)
    t = np.stack([lab for _, lab in samples])
    p = FR.predict_fullres(tiny_model, images, 1, (96, 200))[0].cpu().numpy()
    root, area = R.label(t, 8)
    want, hit, _ = R.counters(t, p, root, area, 20, 19, -1, [8, 64, 512], 3, 4)
    assert a["counters"]["target"] == {k: want[k].tolist() for k in R.COUNTERS}
    rp, ap = R.label(p, 8)
    assert a["counters"]["pred"] == {k: v.tolist() for k, v in
                                     R.counters(p, t, rp, ap, 20, -1, 19, [8, 64, 512], 3, 4)[0].items()}
    assert a["target_segments"] == int(want["segments"].sum()) > 0

    files = sorted(glob.glob(str(seen / "*.png")))
    assert len(files) == 3 and sorted(a["written"]) == files
    flat = np.arange(3)[:, None, None]
    h = hit.reshape(3, -1)[flat, root].astype(np.int64)
    s = area.reshape(3, -1)[flat, root].astype(np.int64)
    for i, f in enumerate(files):
        assert os.path.basename(f) == f"synthetic_{i:04d}_segments.png"
        with Image.open(f) as im:
            assert im.size == (200, 96) and im.mode == "RGB"
            img = np.array(im)
        ign = t[i] == 19
        assert (img[ign] == S.GREY).all()
        assert (img[~ign & (h[i] == 0)] == S.MISSED).all()
        assert (img[~ign & (4 * h[i] >= 3 * s[i])] == S.COVERED).all()
        assert (img[~ign & (h[i] > 0) & (4 * h[i] < 3 * s[i])] == S.PARTLY).all()

    # a label PNG of another size than its label is refused
    Image.fromarray(np.zeros((96, 100), dtype=np.uint8)).save(maps / "synthetic_0001_label.png")
    with pytest.raises(RuntimeError, match="synthetic_0001_label.png is 96 x 100, its label 96 x 200"):
        S.main(S.build_parser().parse_args(data + ["--pred", str(maps), "--score"]))


def test_cli_cleans_a_tree_of_pseudo_labels(dev, tiny_model, tmp_path):
    """--clean on the maps a ``pseudo --out`` run wrote, two folders deep: the output equals the
    reference's filter file by file, the layout is kept, the source is untouched, and a PNG that is
    no 8-bit single-channel map is refused by name."""
    from PIL import Image
    from mdil_ss_amd import pseudo as P
    from mdil_ss_amd import segments as S
    ckpt, tree, cleaned, report = tmp_path / "checkpoint.pth.tar", tmp_path / "tree", tmp_path / "cleaned", \
        tmp_path / "clean.json"
    HC.save_checkpoint(tiny_model, ckpt)
    P.main(P.build_parser().parse_args(
        ["--state", str(ckpt), "--num-classes", "20", "20", "--task", "1", "--synthetic", "3", "--height", "64",
         "--width", "128", "--batch-size", "3", "--portion", "0.5", "--out", str(tree / "city" / "train")]))
    names = sorted(os.path.relpath(f, tree) for f in glob.glob(str(tree / "**" / "*.png"), recursive=True))
    assert len(names) == 3 and all(n.startswith(os.path.join("city", "train")) for n in names)
    source = {n: open(tree / n, "rb").read() for n in names}
    rep = S.main(S.build_parser().parse_args(["--clean", str(tree), "--out", str(cleaned), "--min-area", "12",
                                              "--min-area-class", "0", "40", "1", "0", "--connectivity", "4",
                                              "--json", str(report)]))
    written = glob.glob(str(cleaned / "**" / "*.png"), recursive=True)
    assert sorted(os.path.relpath(f, cleaned) for f in written) == names
    assert {n: open(tree / n, "rb").read() for n in names} == source
    least = np.full(256, 12)
    least[0], least[1] = 40, 0
    seg_all, pix_all = np.zeros(256, np.int64), np.zeros(256, np.int64)
    for n in names:
        with Image.open(tree / n) as im:
            m = np.array(im)[None]
        with Image.open(cleaned / n) as im:
            assert im.mode == "L"
            got = np.array(im)
        root, area = R.label(m, 4)
        want, seg, pix = R.filter(m, root, area, least, 255, 255)
        assert got.dtype == np.uint8 and np.array_equal(got, want[0]), n
        assert (got[m[0] == 255] == 255).all()
        seg_all, pix_all = seg_all + seg, pix_all + pix
    assert pix_all.sum() > 0, "the thresholded maps hold no speckle: the case tests nothing"
    assert rep["removed_segments"] == {str(c): int(v) for c, v in enumerate(seg_all) if v}
    assert rep["removed_pixels"] == {str(c): int(v) for c, v in enumerate(pix_all) if v}
    assert rep["maps"] == 3 and json.load(open(report))["removed_pixels"] == rep["removed_pixels"]
    assert rep["min_area"][:3] == [40, 0, 12] and (rep["keep_id"], rep["fill"], rep["connectivity"]) == (255, 255, 4)

    shutil.copy(tree / names[0], tree / "city" / "copy.png")
    Image.fromarray(np.zeros((8, 8, 3), dtype=np.uint8)).save(tree / "city" / "rgb.png")
    with pytest.raises(RuntimeError, match=r"city/rgb.png is not an 8-bit single-channel"):
        S.main(S.build_parser().parse_args(["--clean", str(tree), "--out", str(tmp_path / "again")]))
