"""CPU: the segments add-on (include/mdil_segments.h, mdil_ss_amd/segments.py) -- the library exports
exactly what its header declares, every argument check answers before any launch, the command
line's defaults and refusals, the two spellings of the numpy reference against each other (and
against scipy where it is installed), the reference's counters and filter by hand, the meter's
arithmetic on hand-written counters, the coverage rule, the refusal of host tensors, and the rule
the add-on exists under: it leaves the training path's build id alone."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import segments_reference as R
from tests.helpers import declared_names, dynamic_exports

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mdil_segments_count", "mdil_segments_filter", "mdil_segments_label", "mdil_segments_last_error",
         "mdil_segments_version", "mdil_segments_workspace_bytes"]


def test_library_exports_exactly_the_declared_symbols():
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _boundary_lib, _segments_lib
    lib = _segments_lib.load()
    assert declared_names("mdil_segments.h") == NAMES
    for n in NAMES:
        assert hasattr(lib, n), f"{n} declared in include/mdil_segments.h but not exported"
    assert sorted(_segments_lib.EXPORTS) == NAMES
    assert dynamic_exports(_segments_lib.LIB_PATH) == NAMES
    assert lib.mdil_segments_version() >= 100
    # the add-on it is modelled on keeps its four names
    assert dynamic_exports(_boundary_lib.LIB_PATH) == ["mdil_boundary_count", "mdil_boundary_last_error",
                                                        "mdil_boundary_version", "mdil_boundary_workspace_bytes"]


def test_workspace_bytes():
    from mdil_ss_amd import _segments_lib
    lib = _segments_lib.load()
    assert lib.mdil_segments_workspace_bytes(6, 1024, 2048) == 8 * 6 * 1024 * 2048
    assert lib.mdil_segments_workspace_bytes(1, 1, 1) == 16                # 8 bytes, rounded up to 16
    assert lib.mdil_segments_workspace_bytes(2, 37, 131) == (8 * 2 * 37 * 131 + 15) // 16 * 16
    assert lib.mdil_segments_workspace_bytes(1 << 10, 1 << 15, 1 << 15) == 8 << 40
    for bad in ((0, 4, 4), (1, -1, 4), (1, 4, (1 << 15) + 1), (1, (1 << 15) + 1, 4), ((1 << 10) + 1, 1 << 15, 1 << 15)):
        assert lib.mdil_segments_workspace_bytes(*bad) == -1, bad


SIZE = dict(N=1, H=8, W=8)
LABEL = dict(SIZE, map=4096, conn=8, root=8192, area=12288, ws=16384, wsb=512)
COUNT = dict(SIZE, map=4096, other=4352, root=8192, area=12288, nc=20, mign=19, oign=-1, edges=(4, 16), ne=None, num=1,
             den=2, ws=16384, wsb=512, hit=20480, void=24576, seg=28672, pix=32768, hpix=36864, cov=40960, mis=45056,
             unj=49152, bad=53248)
FILTER = dict(SIZE, map=4096, root=8192, area=12288, least=16384, keep=255, fill=255, out=20480, rseg=24576,
              rpix=28672)


def _label(lib, **kw):
    a = dict(LABEL, **kw)
    return lib.mdil_segments_label(a["map"], a["N"], a["H"], a["W"], a["conn"], a["root"], a["area"], a["ws"], a["wsb"],
                                   None)


def _count(lib, **kw):
    a = dict(COUNT, **kw)
    edges = None if a["edges"] is None else (C.c_int * max(1, len(a["edges"])))(*a["edges"])
    ne = len(a["edges"]) if a["ne"] is None else a["ne"]
    return lib.mdil_segments_count(a["map"], a["other"], a["root"], a["area"], a["N"], a["H"], a["W"], a["nc"],
                                   a["mign"], a["oign"], edges, ne, a["num"], a["den"], a["ws"], a["wsb"], a["hit"],
                                   a["void"], a["seg"], a["pix"], a["hpix"], a["cov"], a["mis"], a["unj"], a["bad"],
                                   None)


def _filter(lib, **kw):
    a = dict(FILTER, **kw)
    return lib.mdil_segments_filter(a["map"], a["root"], a["area"], a["N"], a["H"], a["W"], a["least"], a["keep"],
                                    a["fill"], a["out"], a["rseg"], a["rpix"], None)


BIG = [(dict(H=(1 << 15) + 1), b"above 32768"), (dict(W=(1 << 15) + 1), b"above 32768"),
       (dict(N=(1 << 10) + 1, H=1 << 15, W=1 << 15), b"too large"),
       (dict(N=1 << 30, H=1 << 15, W=1 << 15), b"too large"),
       (dict(N=0), b"bad argument"), (dict(H=0), b"bad argument"), (dict(W=-3), b"bad argument")]

BAD = [(_label, bad, text) for bad, text in BIG + [
    (dict(map=None), b"bad argument"), (dict(root=None), b"bad argument"), (dict(area=None), b"bad argument"),
    (dict(conn=6), b"connectivity=6"), (dict(conn=0), b"connectivity=0"),
    (dict(map=4097), b"alignment"), (dict(root=8194), b"alignment"), (dict(area=12289), b"alignment"),
    (dict(ws=16386), b"alignment"),
    (dict(wsb=511), b"workspace of 512 bytes"), (dict(ws=None), b"workspace of 512 bytes"),
]] + [(_count, bad, text) for bad, text in BIG + [
    (dict(nc=1), b"nc=1"), (dict(nc=33), b"nc=33"),
    (dict(map=None), b"bad argument"), (dict(other=None), b"bad argument"), (dict(root=None), b"bad argument"),
    (dict(area=None), b"bad argument"), (dict(edges=None, ne=1), b"bad argument"), (dict(seg=None), b"bad argument"),
    (dict(pix=None), b"bad argument"), (dict(hpix=None), b"bad argument"), (dict(cov=None), b"bad argument"),
    (dict(mis=None), b"bad argument"), (dict(unj=None), b"bad argument"), (dict(bad=None), b"bad argument"),
    (dict(ne=0), b"n_edges=0"), (dict(edges=tuple(range(1, 10))), b"n_edges=9"),
    (dict(edges=(2, 2)), b"strictly increasing"), (dict(edges=(3, 1)), b"strictly increasing"),
    (dict(edges=(0,)), b"strictly increasing"), (dict(edges=((1 << 30) + 1,)), b"strictly increasing"),
    (dict(num=0), b"coverage 0/2"), (dict(num=3, den=2), b"coverage 3/2"), (dict(num=1, den=1001), b"coverage 1/1001"),
    (dict(mign=-2), b"map_ignore=-2"), (dict(mign=256), b"map_ignore=256"),
    (dict(oign=-2), b"other_ignore=-2"), (dict(oign=256), b"other_ignore=256"),
    (dict(wsb=511), b"workspace of 512 bytes"), (dict(ws=None), b"workspace of 512 bytes"),
    (dict(map=4098), b"alignment"), (dict(other=4353), b"alignment"), (dict(root=8193), b"alignment"),
    (dict(area=12290), b"alignment"), (dict(ws=16385), b"alignment"), (dict(hit=20482), b"alignment"),
    (dict(void=24577), b"alignment"), (dict(seg=28676), b"alignment"), (dict(pix=32772), b"alignment"),
    (dict(hpix=36868), b"alignment"), (dict(cov=40964), b"alignment"), (dict(mis=45060), b"alignment"),
    (dict(unj=49156), b"alignment"), (dict(bad=53252), b"alignment"),
]] + [(_filter, bad, text) for bad, text in BIG + [
    (dict(map=None), b"bad argument"), (dict(root=None), b"bad argument"), (dict(area=None), b"bad argument"),
    (dict(least=None), b"bad argument"), (dict(out=None), b"bad argument"), (dict(rseg=None), b"bad argument"),
    (dict(rpix=None), b"bad argument"),
    (dict(keep=-2), b"keep_id=-2"), (dict(keep=256), b"keep_id=256"), (dict(fill=-1), b"fill=-1"),
    (dict(fill=256), b"fill=256"), (dict(out=4096), b"may not alias"),
    (dict(map=4097), b"alignment"), (dict(root=8194), b"alignment"), (dict(area=12291), b"alignment"),
    (dict(least=16385), b"alignment"), (dict(out=20482), b"alignment"), (dict(rseg=24580), b"alignment"),
    (dict(rpix=28676), b"alignment"),
]]


@pytest.mark.parametrize("call, bad, text", BAD, ids=[f"{c.__name__[1:]}-{b}" for c, b, _ in BAD])
def test_library_refuses_bad_arguments_without_a_device(call, bad, text):
    """Argument checks come before the launch, so fake pointers never reach a device."""
    from mdil_ss_amd import _segments_lib
    lib = _segments_lib.load()
    assert call(lib, **bad) == -1, bad
    assert text in lib.mdil_segments_last_error(), (bad, lib.mdil_segments_last_error())


BASE = ["--num-classes", "20", "20", "27", "--task", "2"]
STATE = BASE + ["--state", "ckpt.pth.tar"]


def test_parser_defaults():
    from mdil_ss_amd import boundary as B
    from mdil_ss_amd import segments as S
    p = S.build_parser()
    a = p.parse_args(STATE + ["--dataset", "IDD", "--score"])
    assert (a.state, a.num_classes, a.task, a.dataset, a.subset) == ("ckpt.pth.tar", [20, 20, 27], 2, "IDD", "val")
    assert (a.height, a.width, a.batch_size, a.native_height, a.native_width) == (512, 1024, 6, 1024, 2048)
    assert (a.score, a.json, a.out, a.synthetic, a.pred, a.clean) == (True, None, None, 0, None, None)
    assert (a.edges, a.coverage, a.connectivity) == ([64, 256, 1024, 4096, 16384, 65536], "0.5", 8)
    assert tuple(a.edges) == S.DEFAULT_EDGES and S.check_coverage(a.coverage) == (1, 2)
    assert (a.min_area, a.min_area_class, a.keep_id, a.fill) == (16, None, 255, 255)
    assert not hasattr(a, "colour") and not hasattr(a, "label_ids")
    b = p.parse_args(BASE + ["--pred", "maps", "--synthetic", "3", "--native-height", "96", "--native-width", "200",
                             "--edges", "4", "40", "--coverage", "0.75", "--connectivity", "4", "--score", "--json",
                             "r.json", "--out", "seen"])
    assert (b.state, b.pred, b.edges, b.coverage, b.connectivity, b.json, b.out) == \
        (None, "maps", [4, 40], "0.75", 4, "r.json", "seen")
    c = p.parse_args(["--clean", "maps", "--out", "cleaned", "--min-area", "9", "--min-area-class", "11", "4", "12",
                      "30", "--keep-id", "-1", "--fill", "0", "--json", "r.json"])
    assert (c.clean, c.out, c.min_area, c.min_area_class, c.keep_id, c.fill, c.json, c.num_classes, c.task) == \
        ("maps", "cleaned", 9, [11, 4, 12, 30], -1, 0, "r.json", None, None)
    assert callable(S.main)
    # the command lines whose flags it shares keep their surface
    f = B.build_parser().parse_args(STATE + ["--dataset", "IDD", "--score"])
    assert not hasattr(f, "clean") and not hasattr(f, "edges") and f.ratio == 0.02
    with pytest.raises(SystemExit):
        B.build_parser().parse_args(["--state", "c", "--dataset", "IDD", "--score"])   # --num-classes: required there


@pytest.mark.parametrize("argv", [
    STATE + ["--dataset", "cityscapes"],                                 # nothing to do
    STATE + ["--synthetic", "2"],
    STATE + ["--score"],                                                 # no source of labels
    STATE + ["--dataset", "BDD", "--synthetic", "2", "--score"],
    STATE + ["--dataset", "BDD", "--out", "o", "--json", "r.json"],      # a score file without --score
    STATE + ["--dataset", "BDD", "--score", "--pred", "maps"],           # --pred together with --state
    BASE + ["--dataset", "BDD", "--score"],                              # neither of them
    ["--state", "c", "--dataset", "BDD", "--score"],                     # scoring without --num-classes / --task
    STATE + ["--dataset", "BDD", "--score", "--edges", "2", "2"],
    STATE + ["--dataset", "BDD", "--score", "--edges", "4", "1"],
    STATE + ["--dataset", "BDD", "--score", "--edges", "0"],
    STATE + ["--dataset", "BDD", "--score", "--edges", "1", "2", "3", "4", "5", "6", "7", "8", "9"],
    STATE + ["--dataset", "BDD", "--score", "--coverage", "0"],
    STATE + ["--dataset", "BDD", "--score", "--coverage", "1.5"],
    STATE + ["--dataset", "BDD", "--score", "--coverage", "half"],
    STATE + ["--dataset", "BDD", "--score", "--connectivity", "6"],
    STATE + ["--dataset", "BDD", "--score", "--colour"],                 # flags of the map writers
    ["--clean", "maps", "--out", "o", "--score"],                        # --clean with --score
    BASE + ["--clean", "maps", "--out", "o", "--pred", "p"],
    STATE + ["--clean", "maps", "--out", "o"],
    ["--clean", "maps"],                                                 # --clean without --out
    ["--clean", "maps", "--out", "maps"],                                # --out is --clean
    ["--clean", "maps", "--out", "maps/cleaned"],                        # --out inside --clean
    ["--clean", "maps", "--out", "maps/../maps/deep/er"],
    ["--clean", "maps", "--out", "o", "--min-area-class", "3"],          # not pairs
    ["--clean", "maps", "--out", "o", "--min-area-class", "256", "4"],
    ["--clean", "maps", "--out", "o", "--min-area", "-1"],
    ["--clean", "maps", "--out", "o", "--fill", "256"],
    ["--clean", "maps", "--out", "o", "--keep-id", "-2"],
])
def test_parser_refusals(argv):
    from mdil_ss_amd import segments as S
    with pytest.raises(SystemExit):
        S.build_parser().parse_args(argv)


def test_main_refuses_before_it_opens_anything(tmp_path):
    from argparse import Namespace
    from mdil_ss_amd import segments as S
    with pytest.raises(RuntimeError, match="nothing to do"):
        S.main(Namespace(clean=None, score=False, out=None))
    with pytest.raises(RuntimeError, match="give one of them"):
        S.main(Namespace(clean=None, score=True, out=None, json=None, pred="maps", state="ckpt"))
    with pytest.raises(RuntimeError, match="goes without --score"):
        S.main(Namespace(clean="maps", score=True, pred=None, state=None))
    with pytest.raises(RuntimeError, match="needs --out"):
        S.main(Namespace(clean="maps", score=False, pred=None, state=None, out=None))
    inner = tmp_path / "maps" / "cleaned"
    with pytest.raises(RuntimeError, match="lies inside it"):
        S.main(Namespace(clean=str(tmp_path / "maps"), score=False, pred=None, state=None, out=str(inner)))
    # a sibling whose name merely begins like the source is no such case
    assert not S._inside(str(tmp_path / "maps_cleaned"), str(tmp_path / "maps"))


def test_a_map_that_is_not_8_bit_single_channel_is_refused_by_name(tmp_path):
    from PIL import Image
    from mdil_ss_amd import segments as S
    Image.fromarray(np.zeros((6, 9), dtype=np.uint8)).save(tmp_path / "a.png")
    assert S.read_map_png(str(tmp_path / "a.png"), "a.png").shape == (6, 9)
    Image.fromarray(np.zeros((6, 9, 3), dtype=np.uint8)).save(tmp_path / "b.png")
    with pytest.raises(RuntimeError, match="b.png is not an 8-bit single-channel"):
        S.read_map_png(str(tmp_path / "b.png"), "b.png")
    Image.fromarray(np.zeros((6, 9), dtype=np.uint16)).save(tmp_path / "c.png")
    with pytest.raises(RuntimeError, match="c.png is not an 8-bit single-channel"):
        S.read_map_png(str(tmp_path / "c.png"), "c.png")


def test_the_coverage_rule():
    from mdil_ss_amd import segments as S
    assert S.check_coverage("0.5") == (1, 2) == S.check_coverage(Fraction(1, 2)) == S.check_coverage(0.5)
    assert S.check_coverage("0.75") == (3, 4) and S.check_coverage("1") == (1, 1) and S.check_coverage(Fraction(2, 3)) == (2, 3)
    assert S.check_coverage("0.3333") == (1, 3) == tuple(
        Fraction("0.3333").limit_denominator(1000).as_integer_ratio())      # the nearest share up to /1000
    assert S.check_coverage("0.123") == (123, 1000)
    for bad in ("0", "-0.5", "1.001", "half", None, "1/0", Fraction(1, 1001)):
        with pytest.raises(RuntimeError, match="coverage"):
            S.check_coverage(bad)
    assert S.check_edges(S.DEFAULT_EDGES) == [64, 256, 1024, 4096, 16384, 65536]
    for bad in ((), (0,), (3, 3), (5, 2), tuple(range(1, 10)), ((1 << 30) + 1,), ("a",)):
        with pytest.raises(RuntimeError, match="edges"):
            S.check_edges(bad)
    assert S.min_area_table(7, {3: 0, 255: 9}).tolist() == [7, 7, 7, 0] + [7] * 251 + [9]
    with pytest.raises(RuntimeError, match="256 of them"):
        S.min_area_table([1, 2, 3])


SMALL = {
    "checkerboard": R.checkerboard(9, 13),
    "diagonal": R.diagonal(),
    "comb": R.comb(12, 5),
    "spiral": R.spiral(21),
    "blocky": R.blocky((23, 31), 4, seed=1),
    "noise": R.noise((30, 40), seed=2),
    "one label": np.full((7, 5), 3, dtype=np.uint8),
    "one pixel": np.zeros((1, 1), dtype=np.uint8),
}


@pytest.mark.parametrize("name", sorted(SMALL))
@pytest.mark.parametrize("connectivity", (4, 8))
def test_the_two_reference_spellings_agree(name, connectivity):
    a, b = R.roots_flood(SMALL[name], connectivity), R.roots_propagate(SMALL[name], connectivity)
    assert a.dtype == b.dtype == np.int32 and np.array_equal(a, b)
    flat = a.reshape(-1)
    assert (flat <= np.arange(a.size)).all() and np.array_equal(flat[flat], flat)


def merge_rules(m, eight, seed):
    """The contact rules of ``segments_merge_kernel`` (mdil_ss_amd/ext/segments.hip), one pixel at a
    time in a random order on the host: parents start at the run starts, a vertical contact is
    united unless the contact to its left joins the same two runs, a diagonal one only where no
    vertical contact implies it; ``unite`` as the kernel spells it.  -> the end of every parent chain."""
    H, W = m.shape
    P = np.arange(H * W)
    for y in range(H):
        for x in range(1, W):
            if m[y, x] == m[y, x - 1]:
                P[y * W + x] = P[y * W + x - 1]

    def find(x):
        while P[x] != x:
            x = P[x]
        return x

    def unite(a, b):
        while True:
            a, b = find(a), find(b)
            if a == b:
                return
            a, b = max(a, b), min(a, b)
            old, P[a] = P[a], min(P[a], b)
            if old == a:
                return
            a = old

    def below(y, x):
        return int(m[y, x]) if 0 <= x < W else -1

    def above(y, x):
        return int(m[y - 1, x]) if 0 <= x < W else -2

    order = [(y, x) for y in range(1, H) for x in range(W)]
    np.random.default_rng(seed).shuffle(order)
    for y, x in order:
        lab, p = below(y, x), y * W + x
        if above(y, x) == lab:
            if not (below(y, x - 1) == lab and above(y, x - 1) == lab):
                unite(p, p - W)
        elif eight:
            if above(y, x - 1) == lab and below(y, x - 1) != lab:
                unite(p, p - W - 1)
            if above(y, x + 1) == lab and below(y, x + 1) != lab:
                unite(p, p - W + 1)
    return np.array([find(i) for i in range(H * W)], dtype=np.int32).reshape(H, W)


@pytest.mark.parametrize("name", sorted(SMALL))
@pytest.mark.parametrize("connectivity", (4, 8))
def test_one_union_per_contact_run_is_enough(name, connectivity):
    """The unions the merge kernel skips are implied by those it issues, in whatever order they run."""
    want = R.roots_propagate(SMALL[name], connectivity)
    for seed in (0, 1):
        assert np.array_equal(merge_rules(SMALL[name], connectivity == 8, seed), want)


def test_the_maps_have_the_segments_they_are_named_for():
    def count(m, c):
        return R.n_segments(R.label(m[None], c)[1])
    assert (count(R.checkerboard(33, 47), 4), count(R.checkerboard(33, 47), 8)) == (1551, 2)
    assert (count(R.diagonal(), 4), count(R.diagonal(), 8)) == (5, 3)
    assert count(R.comb(40, 9), 4) == count(R.comb(40, 9), 8) == 9
    assert count(R.spiral(129), 4) == count(R.spiral(129), 8) == 2
    s = R.spiral(21)
    assert s[0].all() and s[:, -1].all() and not s[1, :-1].any() and s[2, 0] == 1
    root, area = R.label(R.comb(6, 3)[None], 4)
    assert root[0, :, 0].tolist() == [0] * 6 and root[0, :5, 2].tolist() == [0] * 5 and area[0, 0, 0] == 6 * 3 + 2
    assert area[0, 0, 1] == 5 and area[0, 0, 3] == 5 and R.n_segments(area) == 3


@pytest.mark.parametrize("name", ["blocky", "noise", "spiral", "checkerboard"])
@pytest.mark.parametrize("connectivity", (4, 8))
def test_reference_against_scipy_where_it_is_installed(name, connectivity):
    try:
        from scipy import ndimage
    except ImportError:
        return                                             # the GPU machines go without it
    m = SMALL[name] if name != "noise" else R.noise((200, 300), seed=3)
    want = np.empty(m.shape, dtype=np.int32)
    own = np.arange(m.size).reshape(m.shape)
    structure = np.ones((3, 3)) if connectivity == 8 else None
    for c in np.unique(m):
        lab, n = ndimage.label(m == c, structure=structure)
        low = ndimage.minimum(own, lab, np.arange(1, n + 1)).astype(np.int32)
        want[lab > 0] = low[lab[lab > 0] - 1]
    assert np.array_equal(R.roots_propagate(m, connectivity), want)


def test_reference_counters_and_filter_by_hand():
    """One image of 3 x 6, three classes, class 2 ignored on the target side:
         map    0 0 1 1 2 2      other  0 0 0 1 7 7
                0 0 1 1 2 5             0 9 1 1 7 7
                5 5 5 1 2 2             9 9 9 9 7 7      (9 = the other side's ignore id)"""
    m = np.array([[[0, 0, 1, 1, 2, 2], [0, 0, 1, 1, 2, 5], [5, 5, 5, 1, 2, 2]]], dtype=np.uint8)
    o = np.array([[[0, 0, 0, 1, 7, 7], [0, 9, 1, 1, 7, 7], [9, 9, 9, 9, 7, 7]]], dtype=np.uint8)
    root, area = R.label(m, 4)
    assert root[0].tolist() == [[0, 0, 2, 2, 4, 4], [0, 0, 2, 2, 4, 11], [12, 12, 12, 2, 4, 4]]
    assert area[0].reshape(-1).tolist() == [4, 0, 5, 0, 5, 0, 0, 0, 0, 0, 0, 1, 3] + [0] * 5
    c, hit, void = R.counters(m, o, root, area, 3, 2, 9, [3, 4], 1, 2)
    assert hit[0].reshape(-1)[[0, 2, 4, 11, 12]].tolist() == [3, 3, 0, 0, 0]
    assert void[0].reshape(-1)[[0, 2, 4, 11, 12]].tolist() == [1, 1, 0, 0, 3]
    # class 0: area 4 (bin 1), judged 3, hit 3; class 1: area 5 (bin 2), judged 4, hit 3; class 2 ignored;
    # label 5: one pixel judged and three pixels not judged at all, both outside the classes
    assert c["segments"].tolist() == [[0, 1, 0], [0, 0, 1], [0, 0, 0]]
    assert c["pixels"].tolist() == [[0, 3, 0], [0, 0, 4], [0, 0, 0]]
    assert c["hit_pixels"].tolist() == [[0, 3, 0], [0, 0, 3], [0, 0, 0]]
    assert c["covered"].tolist() == c["segments"].tolist() and not c["missed"].any() and not c["unjudged"].any()
    assert c["bad_labels"].tolist() == [4]
    # the other way round: 7 is outside, 9 ignored; 0 and 1 judged by m
    ro, ao = R.label(o, 4)
    d, _, _ = R.counters(o, m, ro, ao, 3, 9, 2, [3, 4], 3, 4)
    assert d["bad_labels"].tolist() == [6] and d["segments"].sum() == 2 and d["covered"].tolist()[0] == [0, 1, 0]
    assert d["covered"].tolist()[1] == [1, 0, 0] and d["missed"].sum() == 0
    # with 5 as a class of its own: an unjudged segment (all three pixels void) and a missed one
    e, _, _ = R.counters(m, o, root, area, 6, 2, 9, [3, 4], 1, 2)
    assert e["unjudged"][5].tolist() == [1, 0, 0] and e["missed"][5].tolist() == [1, 0, 0] and e["bad_labels"][0] == 0
    assert e["segments"][5].tolist() == [1, 0, 0] and e["pixels"][5].tolist() == [1, 0, 0]
    # the filter: everything below 5 pixels goes (label 5: below 2), label 1 is kept whatever its size
    least = np.full(256, 5)
    least[5] = 2
    out, seg, pix = R.filter(m, root, area, least, 1, 255)
    assert out[0].tolist() == [[255, 255, 1, 1, 2, 2], [255, 255, 1, 1, 2, 255], [5, 5, 5, 1, 2, 2]]
    assert seg[[0, 5]].tolist() == [1, 1] and pix[[0, 5]].tolist() == [4, 1] and seg.sum() == 2 and pix.sum() == 5
    assert R.bins([1, 3, 4, 5, 9], [3, 4]).tolist() == [0, 0, 1, 2, 2]


def _counters(nc, nb):
    from mdil_ss_amd import segments as S
    return {k: torch.zeros(s, dtype=torch.int64) for k, s in S.counter_shapes(nc, nb).items()}


def test_score_on_hand_written_counters():
    from mdil_ss_amd import segments as S
    t, p = _counters(2, 3), _counters(2, 3)
    t["segments"] = torch.tensor([[4, 2, 0], [10, 0, 0]])
    t["covered"] = torch.tensor([[1, 2, 0], [5, 0, 0]])
    t["missed"] = torch.tensor([[2, 0, 0], [5, 0, 0]])
    t["pixels"] = torch.tensor([[40, 200, 0], [50, 0, 0]])
    t["hit_pixels"] = torch.tensor([[10, 150, 0], [25, 0, 0]])
    t["unjudged"] = torch.tensor([[0, 0, 0], [0, 3, 0]])
    p["segments"] = torch.tensor([[8, 0, 0], [0, 0, 2]])
    p["covered"] = torch.tensor([[2, 0, 0], [0, 0, 2]])
    p["missed"] = torch.tensor([[6, 0, 0], [0, 0, 0]])
    rep = S.score(t, p, [10, 100], (1, 2))
    assert rep["edges"] == [10, 100] and rep["coverage"] == [1, 2]
    assert rep["segment_recall"] == {"total": 8 / 16, "bins": [6 / 14, 2 / 2, None],
                                     "classes": [[1 / 4, 2 / 2, None], [5 / 10, None, None]]}
    assert rep["missed_share"]["total"] == 7 / 16 and rep["missed_share"]["classes"][0] == [2 / 4, 0.0, None]
    assert rep["pixel_recall"]["bins"] == [35 / 90, 150 / 200, None] and rep["pixel_recall"]["total"] == 185 / 290
    assert rep["segment_precision"] == {"total": 4 / 10, "bins": [2 / 8, None, 2 / 2],
                                        "classes": [[2 / 8, None, None], [None, None, 2 / 2]]}
    assert rep["hallucinated_share"]["total"] == 6 / 10 and rep["hallucinated_share"]["bins"] == [6 / 8, None, 0.0]
    assert (rep["target_segments"], rep["pred_segments"]) == (16, 10)
    assert rep["unjudged"] == {"target": [[0, 0, 0], [0, 3, 0]], "pred": [[0, 0, 0], [0, 0, 0]]}
    assert rep["counters"]["target"]["pixels"] == t["pixels"].tolist() and sorted(rep["counters"]["pred"]) == \
        sorted(S.COUNTERS)


def test_meter_without_data_and_its_settings():
    from mdil_ss_amd import segments as S
    m = S.SegmentMeter(20, 19)
    assert (m.edges, m.coverage, m.connectivity, m.nb) == (list(S.DEFAULT_EDGES), (1, 2), 8, 7)
    rep = m.report()
    assert rep["segment_recall"]["total"] is None and rep["target_segments"] == 0 and rep["connectivity"] == 8
    assert rep["counters"]["pred"]["segments"] == torch.zeros(20, 7, dtype=torch.int64).tolist()
    m = S.SegmentMeter(20, 19, edges=[5], coverage="0.9", connectivity=4)
    assert (m.edges, m.coverage, m.connectivity, m.nb) == ([5], (9, 10), 4, 2)
    with pytest.raises(RuntimeError, match="strictly increasing"):
        S.SegmentMeter(20, 19, edges=[3, 3])
    with pytest.raises(RuntimeError, match="coverage"):
        S.SegmentMeter(20, 19, coverage=0)
    with pytest.raises(RuntimeError, match="connectivity must be 4 or 8"):
        S.SegmentMeter(20, 19, connectivity=6)


def test_segments_refuse_cpu_tensors():
    from mdil_ss_amd import segments as S
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    pred, target = torch.zeros(1, 8, 8, dtype=torch.uint8), torch.zeros(1, 8, 8, dtype=torch.uint8)
    ints = torch.zeros(1, 8, 8, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="map must be a contiguous uint8 device tensor.*no CPU fallback in the "
                                           "segments path"):
        S.label(pred)
    with pytest.raises(RuntimeError, match="no CPU fallback in the segments path"):
        S.segment_count(pred, target, ints, ints, 20, counters=_counters(20, 7))
    with pytest.raises(RuntimeError, match="no CPU fallback in the segments path"):
        S.despeckle(pred, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback in the segments path"):
        S.SegmentMeter(20, 19).add(pred, target)
    x, w, b = torch.zeros(1, 2, 2, 16), torch.zeros(16, 20, 2, 2), torch.zeros(20)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.SegmentMeter(20, 19).add(x, w, b, target=target)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.SegmentMeter(20, 19).add(Net([20], 1, 0), torch.zeros(1, 3, 32, 64), 0, target=target)
    with pytest.raises(RuntimeError, match="expects"):
        S.SegmentMeter(20, 19).add(pred)


def test_training_build_id_is_untouched():
    """tests/test_miou_parity.py counts only the recorded mIoU runs that carry the id of the build
    under test and needs 32 of them: the add-on must leave that id where the recorded runs have it."""
    from mdil_ss_amd import segments  # noqa: F401
    from tests import helpers
    tags = [str(t) for t in np.load(os.path.join(REPO, "tests", "golden", "miou_run.npz"),
                                    allow_pickle=False)["hip_build"]]
    build = helpers.kernel_build_id()
    assert tags.count(build) >= 32, f"build id {build} is carried by {tags.count(build)} recorded runs"
