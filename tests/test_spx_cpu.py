"""CPU: the superpixel acquisition add-on (include/mdil_spx.h, mdil_ss_amd/superpixel.py) -- the two forms of the
reference of tests/spx_reference.py against each other and against hand-worked examples, the library's exports
and argument counts against the header, every argument check before any launch, and the command line's defaults
and refusals."""
import os
import re

import numpy as np
import pytest
import torch

from tests import spx_reference as R
from tests.helpers import declared_names, dynamic_exports

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mdil_spx_apply", "mdil_spx_last_error", "mdil_spx_slic", "mdil_spx_table", "mdil_spx_version"]


def grey(codes):
    """A 1 x W image whose three channels hold ``codes`` / 255."""
    return (torch.tensor(codes, dtype=torch.float32) / 255.0).expand(1, 3, 1, len(codes)).contiguous()


# ---------------------------------------------------------------------------------- reference
@pytest.mark.parametrize("shape, S, m, T", (((1, 1, 1), 4, 10, 2), ((2, 9, 7), 4, 1, 2), ((1, 9, 7), 16, 10, 1), ((1, 5, 21), 4, 64, 3),
                                            ((1, 13, 11), 5, 10, 2), ((1, 6, 70), 64, 10, 1)))
def test_the_two_forms_of_the_reference_agree(shape, S, m, T):
    g = torch.Generator().manual_seed(S + shape[1])
    N, H, W = shape
    img = torch.rand(N, 3, H, W, generator=g)
    img[:, :, :, W // 2:] = (img[:, :, :, W // 2:] * 4).floor() / 4             # flat patches: ties
    a, b = R.slic(img, S, m, T, R.assign_loop), R.slic(img, S, m, T, R.assign_fast)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    ids, centres, sums = b
    Gy, Gx = R.grid(H, W, S)
    assert tuple(centres.shape) == (N, Gy * Gx, 5) and tuple(sums.shape) == (N, Gy * Gx, 6)
    assert int(sums[..., 0].sum()) == N * H * W                                # areas sum to the pixels
    yy, xx = torch.arange(H)[:, None] // S, torch.arange(W)[None] // S
    assert bool(((ids // Gx - yy).abs() <= 1).all()) and bool(((ids % Gx - xx).abs() <= 1).all())   # within 3 x 3 of home


def fma_code(v):
    """floor(RN_fp32(v * 255 + 0.5)) of one fp32 value in exact rationals: the fmaf of the header, rounded once."""
    from fractions import Fraction
    x = Fraction(float(v)) * 255 + Fraction(1, 2)
    near = np.float32(float(x))
    cands = sorted({near, np.nextafter(near, np.float32(-1)), np.nextafter(near, np.float32(1e9))}, key=float)
    dist = [abs(Fraction(float(c)) - x) for c in cands]
    best = [c for c, d in zip(cands, dist) if d == min(dist)]
    if len(best) == 2:                                                         # halfway: to the even mantissa
        best = [c for c in best if int(np.array(c).view(np.uint32)) % 2 == 0]
    return int(np.floor(best[0]))


def test_quantiser_by_hand_and_against_exact_rationals():
    v = torch.tensor([0.0, 1.0, 0.5, float("nan"), -3.0, 7.0, float("inf"), float("-inf"), 1e-30, -0.0, 0.25])
    assert R.quantise(v).tolist() == [0, 255, 128, 0, 0, 255, 255, 0, 0, 0, 64]    # 0.5: 127.5 + 0.5; 0.25: 63.75 + 0.5 = 64.25
    k = (torch.arange(256, dtype=torch.float32) / 255.0).numpy()
    assert R.quantise(torch.from_numpy(k)).tolist() == list(range(256))
    # around every k / 255 and every (k + 0.5) / 255, one ulp either way, and random values
    half = ((torch.arange(255, dtype=torch.float32) + 0.5) / 255.0).numpy()
    near = np.concatenate([k, half])
    near = np.concatenate([near, np.nextafter(near, np.float32(-1)), np.nextafter(near, np.float32(2))]).clip(0, 1).astype(np.float32)
    rnd = torch.rand(500, generator=torch.Generator().manual_seed(3)).numpy()
    for values in (near, rnd):
        assert R.quantise(torch.from_numpy(values)).tolist() == [fma_code(x) for x in values]


def test_one_by_eight_by_hand():
    """S = 4, m = 1: centres at x = 2 (code 0) and x = 6 (code 2).  Pixel 4 (code 1) is as far from both in colour
    (16 away) and in space (32 away): a tie, so it goes to centre 0.  Update: centre 0 has 5 pixels, sum x 10, sum of
    codes 3: X = (160 + 2) / 5 = 32, colour (48 + 2) / 5 = 10 (9.6, half up); centre 1 has 3, sum x 18, codes 7:
    X = (288 + 1) / 3 = 96, colour (112 + 1) / 3 = 37 (37.33, down)."""
    img = grey([0, 1, 0, 1, 1, 2, 2, 3])
    for form in (R.assign_loop, R.assign_fast):
        ids, centres, sums = R.slic(img, 4, 1, 0, form)
        assert ids.tolist() == [[[0, 0, 0, 0, 0, 1, 1, 1]]]
        assert centres.tolist() == [[[0, 32, 0, 0, 0], [0, 96, 32, 32, 32]]]
        assert sums.tolist() == [[[5, 0, 10, 3, 3, 3], [3, 0, 18, 7, 7, 7]]]
        ids, centres, sums = R.slic(img, 4, 1, 1, form)
        assert centres.tolist() == [[[0, 32, 10, 10, 10], [0, 96, 37, 37, 37]]]
        assert ids.tolist() == [[[0, 0, 0, 0, 0, 1, 1, 1]]]
    c0 = [0, 32, 0, 0, 0]
    assert R.distance(4, 1, 0, 4, 1, 1, 1, c0) == R.distance(4, 1, 0, 4, 1, 1, 1, [0, 96, 32, 32, 32]) == 16 * 3 * 256 + 1024


def test_an_emptied_centre_keeps_its_state():
    img = R.emptied_image()
    for form in (R.assign_loop, R.assign_fast):
        ids, centres, sums = R.slic(img, 4, 1, 0, form)
        assert ids.tolist() == [[[0] * 5 + [1, 1] + [2] * 5]]
        ids, centres, sums = R.slic(img, 4, 1, 1, form)
        assert centres[0, 1].tolist() == [0, 88, 800, 800, 0]                  # (16 * 11 + 1) / 2, (1600 + 1) / 2
        assert ids.tolist() == [[[0] * 5 + [2, 0] + [2] * 5]] and sums[0, :, 0].tolist() == [6, 0, 6]
        ids, centres, sums = R.slic(img, 4, 1, 2, form)
        assert centres[0, 1].tolist() == [0, 88, 800, 800, 0] and sums[0, 1].tolist() == [0] * 6    # kept
        assert centres[0, 0].tolist() == [0, 43, 1613, 0, 0]                   # (16 * 16 + 3) / 6, (16 * 605 + 3) / 6


@pytest.mark.parametrize("S, m, size", ((4, 1, (36, 52)), (16, 10, (48, 80)), (16, 64, (16, 16)), (64, 64, (128, 192))))
def test_a_constant_image_keeps_the_first_partition(S, m, size):
    """Every D is a tie or purely spatial.  On whole cells the first partition (cell borders moved by the tie rule: pixel
    (a + 1) S is as far from centre a as from centre a + 1 and goes to a) is a fixed point of the update for every T.
    On a ragged grid it is not: the clamped first centre of a narrow last cell is not the mean of its pixels, so the
    borders move with T (37 x 53 at S = 16, m = 10 does); the property is stated and checked on whole cells."""
    img = torch.full((1, 3) + size, 0.3)
    first = R.slic(img, S, m, 0)[0]
    Gx = size[1] // S
    if Gx > 1:
        assert int(first[0, 0, S]) == 0 and int(first[0, S, 0]) == 0 and int(first[0, S + 1, S + 1]) == Gx + 1
    for T in (1, 2, 5):
        assert torch.equal(R.slic(img, S, m, T)[0], first)
    ragged = torch.full((1, 3, 37, 53), 0.3)
    assert not torch.equal(R.slic(ragged, 16, 10, 1)[0], R.slic(ragged, 16, 10, 0)[0])


def test_the_largest_distance_stays_below_2_39():
    """S = 64, m = 64, colours 0 against 255, and a centre as far as the update can take it from a candidate pixel: its
    own pixels lie within its 3 x 3 cells, so it stays within 1.5 S of its cell's middle and a pixel of a neighbouring
    cell is less than 3.5 S from it on either axis."""
    S = m = 64
    far = int(3.5 * S)
    D = R.distance(S, m, far, far, 255, 255, 255, [0, 0, 0, 0, 0])
    assert D == 64 * 64 * 3 * 4080 ** 2 + 64 * 64 * 2 * (16 * far) ** 2 and D < 2 ** 39
    img = torch.zeros(1, 3, 70, 130)
    img[:, :, ::2] = 1.0
    codes = R.quantise(img)
    R.assign_fast(codes, R.init_centres(codes, S), S, m)                       # asserts D < 2^39 inside


def test_table_by_hand():
    ids = torch.tensor([[[0, 0, 1, 1, 5, -1]]])
    label = torch.tensor([[[1, 2, 1, 9, 0, 0]]], dtype=torch.uint8)
    q = torch.tensor([[[10, 20, 30, 40, 50, 60]]])
    target = torch.tensor([[[1, 1, 255, 7, 1, 1]]], dtype=torch.uint8)
    r = R.table_ref(label, q, ids, 2, 3, target, 255)
    assert r["table"].tolist() == [[[2, 30, 1, 2, 0, 1, 1], [2, 70, 0, 0, 0, 1, 0]]]   # the label 9 counts in pixels alone
    assert r["tcount"].tolist() == [[[0, 2, 0], [0, 0, 0]]] and (r["bad_targets"], r["bad_ids"]) == (1, 2)
    r = R.table_ref(label, q, ids, 2, 3)
    assert r["table"].tolist() == [[[2, 30, 0, 0, 0, 1, 1], [2, 70, 0, 0, 0, 1, 0]]] and int(r["tcount"].sum()) == 0


def test_apply_precedence_by_hand():
    """The table of test_ripu_cpu.test_apply_precedence_by_hand, the region read through four superpixels."""
    ids = torch.tensor([[[0, 0, 1, 2, 2, 3]]])
    selected = torch.tensor([[255, 128, 0, 1]], dtype=torch.uint8)           # only 255 is chosen
    target = torch.tensor([[[0, 9, 2, 1, 255, 1]]], dtype=torch.uint8)
    previous = torch.tensor([[[2, 2, 1, 250, 7, 250]]], dtype=torch.uint8)
    fill = torch.tensor([[[0, 0, 0, 2, 2, 250]]], dtype=torch.uint8)
    label = torch.tensor([[[1, 1, 2, 0, 0, 1]]], dtype=torch.uint8)
    r = R.apply_ref(ids, selected, 3, None, target, previous, fill, label, 255, 250)
    assert r["out"].tolist() == [[[0, 9, 1, 2, 7, 250]]] and r["mask"].tolist() == [[[255, 255, 128, 64, 128, 0]]]
    assert r["shown"] == 2 and r["bad_targets"] == 1 and r["annotated"].tolist() == [1, 0, 0]
    assert r["kept"].tolist() == [0, 1, 0] and r["filled"].tolist() == [0, 0, 1]   # the kept 7 is no class
    assert (r["wrong_shown"], r["wrong_all"]) == (1, 2) and (r["noisy"], r["bad_ids"]) == (0, 0)
    # one click: superpixel 0 is answered 2; pixel 0 (target 0) is noisy, pixel 1 (target 9) has no valid target
    answer = torch.tensor([[2, 0, 0, 0]], dtype=torch.uint8)
    r = R.apply_ref(ids, selected, 3, answer, target, previous, fill, label, 255, 250)
    assert r["out"].tolist() == [[[2, 2, 1, 2, 7, 250]]] and r["mask"].tolist() == [[[255, 255, 128, 64, 128, 0]]]
    assert r["annotated"].tolist() == [0, 0, 2] and r["noisy"] == 1 and r["bad_targets"] == 1 and r["shown"] == 2
    assert (r["wrong_shown"], r["wrong_all"]) == (1, 2)
    # an answer that is the ignore class or no class is written and not counted
    r = R.apply_ref(ids, selected, 3, torch.tensor([[255, 0, 0, 0]], dtype=torch.uint8), target, ignore=255, drop_id=250)
    assert r["out"].tolist() == [[[255, 255, 250, 250, 250, 250]]] and r["annotated"].tolist() == [0, 0, 0] and r["noisy"] == 1
    # an id outside [0, K) is never chosen
    r = R.apply_ref(torch.tensor([[[0, 4, 1, 2, 2, -1]]]), selected, 3, answer, target, previous, fill, label, 255, 250)
    assert r["out"].tolist() == [[[2, 2, 1, 2, 7, 250]]] and r["mask"].tolist() == [[[255, 128, 128, 64, 128, 0]]]
    assert r["bad_ids"] == 2 and r["shown"] == 1 and r["bad_targets"] == 0 and (r["wrong_shown"], r["wrong_all"]) == (1, 2)
    r = R.apply_ref(ids, selected, 3)
    assert r["out"].tolist() == [[[255] * 6]] and r["mask"].tolist() == [[[255, 255, 0, 0, 0, 0]]]


def test_host_helpers_on_a_hand_table():
    from mdil_ss_amd import superpixel as P
    tcount = torch.tensor([[5, 1, 0], [2, 2, 1], [0, 0, 0], [0, 3, 3]])
    assert P.dominant_answers(tcount, 250).tolist() == [0, 0, 250, 1] == R.dominant(tcount, 250).tolist()   # ties: the lowest class
    assert P.dominant_answers(tcount).dtype == torch.uint8 and P.dominant_answers(tcount)[2] == 255
    assert P.achievable_accuracy(tcount) == (5 + 2 + 0 + 3) / 17 == R.achievable_accuracy(tcount)
    assert P.achievable_accuracy(torch.zeros(2, 3, dtype=torch.int64)) == 0.0
    table = torch.cat([torch.full((4, 4), 9), tcount.flip(1)], 1)
    assert P.majority_labels(table, 7).tolist() == [2, 1, 7, 0] == R.dominant(tcount.flip(1), 7).tolist()
    assert P.dominant_answers(tcount.reshape(2, 2, 3), 250).tolist() == [[0, 0], [250, 1]]
    with pytest.raises(RuntimeError, match="drop_id 256"):
        P.dominant_answers(tcount, 256)
    ids = torch.tensor([[[0, 0, 1], [0, 2, 2]]])
    assert P.superpixel_edges(ids).tolist() == [[[0, 255, 255], [255, 0, 0]]] == R.edges(ids).tolist()
    assert P.grid((9, 7), 4) == (3, 2) == R.grid(9, 7, 4)


# -------------------------------------------------------------------------------------- library
def header():
    text = open(os.path.join(REPO, "include", "mdil_spx.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_library_exports_exactly_the_declared_symbols():
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _spx_lib
    lib = _spx_lib.load()
    assert declared_names("mdil_spx.h") == NAMES
    for n in NAMES:
        assert hasattr(lib, n), f"{n} declared in include/mdil_spx.h but not exported"
    assert sorted(_spx_lib.EXPORTS) == NAMES
    assert dynamic_exports(_spx_lib.LIB_PATH) == NAMES
    assert lib.mdil_spx_version() >= 100


def test_header_export_map_and_binding_name_the_same_entry_points():
    from mdil_ss_amd import _spx_lib
    from mdil_ss_amd import superpixel as P
    hdr = header()
    declared = {}
    for name, params in re.findall(r"\b(mdil_spx_\w+)\s*\(([^)]*)\)\s*;", hdr):
        params = params.strip()
        declared[name] = 0 if params == "void" else params.count(",") + 1
    mapped = re.findall(r"^\s*(mdil_spx_\w+);", open(os.path.join(REPO, "mdil_ss_amd", "ext", "spx_exports.map")).read(),
                        flags=re.M)
    assert sorted(declared) == sorted(mapped) == sorted(_spx_lib._SIGNATURES) == NAMES
    for name, (_, argtypes) in _spx_lib._SIGNATURES.items():
        assert declared[name] == len(argtypes), (name, declared[name], len(argtypes))
    assert (declared["mdil_spx_slic"], declared["mdil_spx_table"], declared["mdil_spx_apply"]) == (11, 15, 26)
    macros = {k: int(v) for k, v in re.findall(r"#define\s+MDIL_SPX_(\w+)\s+\(?(-?\d+)\)?\s", hdr)}
    assert (macros["MIN_CLASSES"], macros["MAX_CLASSES"]) == (_spx_lib.MIN_CLASSES, _spx_lib.MAX_CLASSES) == (2, 32)
    assert (macros["MIN_STEP"], macros["MAX_STEP"]) == (_spx_lib.MIN_STEP, _spx_lib.MAX_STEP) == (4, 64)
    assert (macros["MIN_COMPACTNESS"], macros["MAX_COMPACTNESS"]) == (_spx_lib.MIN_COMPACTNESS, _spx_lib.MAX_COMPACTNESS) == (1, 64)
    assert macros["MAX_ITERATIONS"] == _spx_lib.MAX_ITERATIONS == 32 and macros["MAX_SIDE"] == _spx_lib.MAX_SIDE == 4096
    assert macros["FRACTION_BITS"] == _spx_lib.FRACTION_BITS == 4 and macros["FIELDS"] == _spx_lib.FIELDS == P.FIELDS == R.FIELDS == 4
    assert (macros["OK"], macros["ERR_INVALID"], macros["ERR_LAUNCH"]) == (0, -1, -2)
    from mdil_ss_amd import acquire as A
    assert P.FIELDS == A.FIELDS                                                # acquire's scores read the table as it is


def test_build_checks_the_binding_and_the_makefile_builds_it():
    assert "_spx_lib" in open(os.path.join(REPO, "__graft_entry__.py")).read()
    make = open(os.path.join(REPO, "mdil_ss_amd", "ext", "Makefile")).read()
    assert re.search(r"^PLAIN := .*\bripu\b.*\bspx\b", make, flags=re.M) and re.search(r"^NAMES \+= acquire$", make, flags=re.M)
    assert re.search(r"spx\.o.*: head_common\.h", make) and re.search(r"spx\.o.*: map_common\.h", make)
    # no head code: the library takes the shared headers as they are and no head kernel
    src = open(os.path.join(REPO, "mdil_ss_amd", "ext", "spx.hip")).read()
    assert "map_common.h" in src and "stage_parity" not in src and "logits4" not in src and "annotate_pixel" in src


SLIC_OK = dict(image=4096, N=1, H=8, W=8, step=4, m=10, T=2, id=8192, centres=12288, sums=16384)
TABLE_OK = dict(label=4096, qmap=8192, tgt=12288, ign=19, id=16384, N=1, H=8, W=8, K=4, nc=20, table=20480, tcount=24576,
                badt=28672, badi=32768)
APPLY_OK = dict(id=4096, sel=8192, ans=12288, tgt=16384, prev=20480, fill=24576, label=28672, N=1, H=8, W=8, K=4, nc=20, ign=19,
                drop=255, out=32768, mask=36864, shown=40960, ann=45056, kept=49152, filled=53248, badt=57344, ws=61440,
                wa=65536, noisy=69632, badi=73728)


def _slic(lib, **kw):
    a = dict(SLIC_OK, **kw)
    return lib.mdil_spx_slic(a["image"], a["N"], a["H"], a["W"], a["step"], a["m"], a["T"], a["id"], a["centres"], a["sums"], None)


def _table(lib, **kw):
    a = dict(TABLE_OK, **kw)
    return lib.mdil_spx_table(a["label"], a["qmap"], a["tgt"], a["ign"], a["id"], a["N"], a["H"], a["W"], a["K"], a["nc"],
                              a["table"], a["tcount"], a["badt"], a["badi"], None)


def _apply(lib, **kw):
    a = dict(APPLY_OK, **kw)
    return lib.mdil_spx_apply(a["id"], a["sel"], a["ans"], a["tgt"], a["prev"], a["fill"], a["label"], a["N"], a["H"], a["W"],
                              a["K"], a["nc"], a["ign"], a["drop"], a["out"], a["mask"], a["shown"], a["ann"], a["kept"],
                              a["filled"], a["badt"], a["ws"], a["wa"], a["noisy"], a["badi"], None)


_NO_OUTPUTS = dict(out=None, mask=None, shown=None, ann=None, kept=None, filled=None, badt=None, ws=None, wa=None, noisy=None,
                   badi=None)


@pytest.mark.parametrize("call, bad, text", [
    (_slic, dict(step=3), b"step=3"), (_slic, dict(step=65), b"step=65"), (_slic, dict(m=0), b"compactness=0"),
    (_slic, dict(m=65), b"compactness=65"), (_slic, dict(T=-1), b"iterations=-1"), (_slic, dict(T=33), b"iterations=33"),
    (_slic, dict(image=None), b"bad argument"), (_slic, dict(id=None), b"all required"), (_slic, dict(centres=None), b"all required"),
    (_slic, dict(sums=None), b"all required"), (_slic, dict(N=0), b"bad argument"), (_slic, dict(H=-1), b"bad argument"),
    (_slic, dict(W=0), b"bad argument"), (_slic, dict(H=4097), b"too large"), (_slic, dict(W=4097), b"too large"),
    (_slic, dict(N=1 << 17, H=4096, W=4096), b"too large"),
    (_slic, dict(image=4100), b"alignment"), (_slic, dict(id=8196), b"alignment"), (_slic, dict(centres=12292), b"alignment"),
    (_slic, dict(sums=16388), b"alignment"),
    (_table, dict(nc=1), b"nc=1"), (_table, dict(nc=33), b"nc=33"), (_table, dict(label=None), b"bad argument"),
    (_table, dict(qmap=None), b"bad argument"), (_table, dict(id=None), b"bad argument"), (_table, dict(N=0), b"bad argument"),
    (_table, dict(W=-3), b"bad argument"), (_table, dict(H=4097), b"too large"), (_table, dict(K=0), b"K=0"),
    (_table, dict(N=1 << 10, K=1 << 17), b"2^31 cells"), (_table, dict(ign=-2), b"ignore_index=-2"),
    (_table, dict(ign=256), b"ignore_index=256"),
    (_table, dict(table=None, tcount=None, badt=None, badi=None), b"nothing to write"),
    (_table, dict(tgt=None), b"need a target"), (_table, dict(tgt=None, tcount=None), b"need a target"),
    (_table, dict(tgt=None, badt=None), b"need a target"),
    (_table, dict(label=4097), b"alignment"), (_table, dict(qmap=8194), b"alignment"), (_table, dict(tgt=12292), b"alignment"),
    (_table, dict(id=16388), b"alignment"), (_table, dict(table=20484), b"alignment"), (_table, dict(tcount=24580), b"alignment"),
    (_table, dict(badt=28676), b"alignment"), (_table, dict(badi=32772), b"alignment"),
    (_apply, dict(nc=1), b"nc=1"), (_apply, dict(nc=33), b"nc=33"), (_apply, dict(id=None), b"bad argument"),
    (_apply, dict(sel=None), b"bad argument"), (_apply, dict(N=0), b"bad argument"), (_apply, dict(W=-3), b"bad argument"),
    (_apply, dict(H=1 << 13, W=1 << 12), b"too large"), (_apply, dict(K=0), b"K=0"), (_apply, dict(ign=-2), b"ignore_index=-2"),
    (_apply, dict(drop=-1), b"drop_id=-1"), (_apply, dict(drop=256), b"drop_id=256"), (_apply, _NO_OUTPUTS, b"nothing to write"),
    (_apply, dict(tgt=None, ans=None), b"annotated needs an answer or a target"),
    (_apply, dict(tgt=None), b"bad_targets and noisy need a target"),
    (_apply, dict(tgt=None, badt=None, ws=None, wa=None), b"bad_targets and noisy need a target"),
    (_apply, dict(tgt=None, badt=None, noisy=None), b"need a target and a label"),
    (_apply, dict(label=None), b"need a target and a label"), (_apply, dict(label=None, ws=None), b"need a target and a label"),
    (_apply, dict(id=4100), b"alignment"), (_apply, dict(sel=8193), b"alignment"), (_apply, dict(ans=12289), b"alignment"),
    (_apply, dict(tgt=16388), b"alignment"), (_apply, dict(prev=20484), b"alignment"), (_apply, dict(fill=24580), b"alignment"),
    (_apply, dict(label=28676), b"alignment"), (_apply, dict(out=32772), b"alignment"), (_apply, dict(mask=36868), b"alignment"),
    (_apply, dict(shown=40964), b"alignment"), (_apply, dict(ann=45060), b"alignment"), (_apply, dict(kept=49156), b"alignment"),
    (_apply, dict(filled=53252), b"alignment"), (_apply, dict(badt=57348), b"alignment"), (_apply, dict(ws=61444), b"alignment"),
    (_apply, dict(wa=65540), b"alignment"), (_apply, dict(noisy=69636), b"alignment"), (_apply, dict(badi=73732), b"alignment"),
])
def test_library_refuses_bad_arguments_without_a_device(call, bad, text):
    """Argument checks come before the launch, so fake pointers never reach a device."""
    from mdil_ss_amd import _spx_lib
    lib = _spx_lib.load()
    assert call(lib, **bad) == -1, bad
    assert text in lib.mdil_spx_last_error(), (bad, lib.mdil_spx_last_error())


# -------------------------------------------------------------------------------------- wrappers
def test_wrappers_refuse_cpu_tensors_and_bad_values():
    from mdil_ss_amd import superpixel as P
    image = torch.zeros(1, 3, 8, 8)
    ids = torch.zeros(1, 8, 8, dtype=torch.int32)
    label = torch.zeros(1, 8, 8, dtype=torch.uint8)
    sel = torch.zeros(1, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="image must be a contiguous float32 device tensor.*no CPU fallback in the superpixel path"):
        P.spx_slic(image)
    with pytest.raises(RuntimeError, match="id must be a contiguous int32 device tensor.*no CPU fallback in the superpixel path"):
        P.spx_table(label, label, ids, 4, 20)
    with pytest.raises(RuntimeError, match="id must be a contiguous int32 device tensor.*no CPU fallback in the superpixel path"):
        P.spx_apply(ids, sel, 20)
    for name, kw, lo, hi in (("step", dict(step=3), 4, 64), ("step", dict(step=65), 4, 64), ("compactness", dict(compactness=0), 1, 64),
                             ("compactness", dict(compactness=65), 1, 64), ("iterations", dict(iterations=-1), 0, 32),
                             ("iterations", dict(iterations=33), 0, 32), ("step", dict(step=4.5), 4, 64)):
        with pytest.raises(RuntimeError, match=f"{name} .* outside \\[{lo}, {hi}\\]"):
            P.spx_slic(image, **kw)
    for nc in (1, 33):
        with pytest.raises(RuntimeError, match=f"{nc} classes \\(supported: 2 to 32\\)"):
            P.spx_table(label, label, ids, 4, nc)
        with pytest.raises(RuntimeError, match=f"{nc} classes \\(supported: 2 to 32\\)"):
            P.spx_apply(ids, sel, nc)
    with pytest.raises(RuntimeError, match="K 0"):
        P.spx_table(label, label, ids, 0, 20)
    with pytest.raises(RuntimeError, match="drop_id 256"):
        P.spx_apply(ids, sel, 20, drop_id=256)
    with pytest.raises(RuntimeError, match="ignore_index 300"):
        P.spx_apply(ids, sel, 20, ignore_index=300)
    assert set(P.apply_counter_shapes(20)) == set(P.APPLY_COUNTERS) and P.apply_counter_shapes(20)["annotated"] == (20,)


def test_read_selection(tmp_path):
    import json
    from mdil_ss_amd import superpixel as P
    f = tmp_path / "selection.json"
    params = {"step": 16, "compactness": 10, "iterations": 10}
    f.write_text(json.dumps(dict(params, size=[16, 24], superpixels={"a": [[3, 4, 6, 99, 0.5, 2], [0, 1, 1, 40, 0.25, None]]})))
    assert P.read_selection(str(f), params, (16, 24)) == {"a": {0, 3}}
    with pytest.raises(RuntimeError, match="this run has"):
        P.read_selection(str(f), params, (8, 8))
    for other in ({"step": 8}, {"compactness": 9}, {"iterations": 0}):
        with pytest.raises(RuntimeError, match="selected with"):
            P.read_selection(str(f), dict(params, **other), (16, 24))
    f.write_text("{}")
    with pytest.raises(RuntimeError, match="not a selection.json"):
        P.read_selection(str(f), params, (16, 24))


# ---------------------------------------------------------------------------------- command line
BASE = ["--state", "ckpt.pth.tar", "--num-classes", "20", "20", "--task", "1"]


def test_parser_defaults():
    from mdil_ss_amd import superpixel as P
    a = P.build_parser().parse_args(BASE + ["--dataset", "BDD", "--budget", "0.05", "--json", "r.json"])
    assert (a.dataset, a.subset, a.synthetic, a.images, a.json, a.out, a.out_root, a.layout) == \
        ("BDD", "train", 0, None, "r.json", None, None, None)
    assert (a.budget, a.step, a.compactness, a.iterations, a.answer, a.max_per_image, a.vote, a.kind, a.by, a.seed, a.previous,
            a.previous_root, a.fill_root) == (0.05, 16, 10, 10, "dominant", None, False, "entropy", "ripu", 0, None, None, None)
    assert (a.height, a.width, a.batch_size) == (512, 1024, 6)
    b = P.build_parser().parse_args(BASE + ["--synthetic", "2", "--budget", "0.1", "--step", "8", "--compactness", "20",
                                            "--iterations", "0", "--answer", "exact", "--max-per-image", "0.5", "--kind", "margin",
                                            "--by", "oracle", "--previous", "s.json", "--previous-root", "r0", "--fill-root", "p",
                                            "--out-root", "r1", "--layout", "BDD", "--out", "o", "--seed", "4"])
    assert (b.step, b.compactness, b.iterations, b.answer, b.max_per_image, b.kind, b.by, b.previous, b.previous_root, b.fill_root,
            b.out_root, b.layout, b.out, b.seed) == (8, 20, 0, "exact", 0.5, "margin", "oracle", "s.json", "r0", "p", "r1", "BDD", "o", 4)
    c = P.build_parser().parse_args(BASE + ["--synthetic", "2", "--budget", "1", "--vote", "--out", "o"])
    assert c.vote and callable(P.main)


@pytest.mark.parametrize("argv, text", [
    (["--budget", "0.1", "--json", "r"], "give one source"),
    (["--dataset", "BDD", "--synthetic", "2", "--budget", "0.1", "--json", "r"], "give one source"),
    (["--dataset", "BDD", "--json", "r"], "--budget"),
    (["--dataset", "BDD", "--budget", "0.1"], "nothing to do"),
    (["--dataset", "BDD", "--budget", "0", "--json", "r"], "--budget 0"),
    (["--dataset", "BDD", "--budget", "1.5", "--json", "r"], "--budget 1.5"),
    (["--dataset", "BDD", "--budget", "0.1", "--json", "r", "--step", "3"], "step 3 outside \\[4, 64\\]"),
    (["--dataset", "BDD", "--budget", "0.1", "--json", "r", "--step", "65"], "step 65 outside"),
    (["--dataset", "BDD", "--budget", "0.1", "--json", "r", "--compactness", "0"], "compactness 0 outside \\[1, 64\\]"),
    (["--dataset", "BDD", "--budget", "0.1", "--json", "r", "--iterations", "33"], "iterations 33 outside \\[0, 32\\]"),
    (["--dataset", "BDD", "--budget", "0.1", "--json", "r", "--answer", "guess"], "invalid choice"),
    (["--dataset", "BDD", "--budget", "0.1", "--json", "r", "--max-per-image", "0"], "--max-per-image 0"),
    (["--dataset", "BDD", "--budget", "0.1", "--json", "r", "--kind", "energy"], "invalid choice"),
    (["--dataset", "BDD", "--budget", "0.1", "--json", "r", "--by", "best"], "invalid choice"),
    (["--images", "d", "--budget", "0.1", "--json", "r", "--by", "oracle"], "needs labels"),
    (["--images", "d", "--budget", "0.1", "--out-root", "c", "--layout", "BDD"], "needs labels"),
    (["--dataset", "BDD", "--budget", "0.1", "--out-root", "c"], "go together"),
    (["--dataset", "BDD", "--budget", "0.1", "--json", "r", "--layout", "BDD"], "go together"),
    (["--dataset", "IDD", "--budget", "0.1", "--out-root", "c", "--layout", "BDD"], "does not take --dataset IDD"),
    (["--dataset", "BDD", "--budget", "0.1", "--json", "r", "--fill-root", "p"], "need --out-root"),
    (["--dataset", "BDD", "--budget", "0.1", "--out-root", "c", "--layout", "BDD", "--previous-root", "p"], "goes with --previous"),
    (["--dataset", "BDD", "--budget", "0.1", "--json", "r", "--batch-size", "0"], "must be positive"),
    (["--dataset", "BDD", "--budget", "0.1", "--json", "r", "--height", "511"], "must be even"),
    (["--dataset", "BDD", "--budget", "0.1", "--json", "r", "--height", "8192", "--width", "4096"], "sides of at most 4096"),
    (["--dataset", "BDD", "--budget", "0.1", "--vote", "--out-root", "c", "--layout", "BDD"], "--vote writes"),
    (["--dataset", "BDD", "--budget", "0.1", "--vote", "--json", "r", "--previous", "s.json"], "--vote writes"),
])
def test_parser_refusals(argv, text, capsys):
    from mdil_ss_amd import superpixel as P
    with pytest.raises(SystemExit):
        P.build_parser().parse_args(BASE + argv)
    assert re.search(text, capsys.readouterr().err)


def test_main_refuses_before_it_opens_anything():
    """The checkpoint does not exist: every refusal below comes before it would be opened."""
    from mdil_ss_amd import superpixel as P
    args = P.build_parser().parse_args(BASE + ["--dataset", "BDD", "--budget", "0.1", "--json", "r.json"])
    args.json = None
    with pytest.raises(RuntimeError, match="nothing to do"):
        P.main(args)
    args.json, args.step = "r.json", 2
    with pytest.raises(RuntimeError, match="step 2 outside"):
        P.main(args)
    args.step, args.task = 16, 2
    with pytest.raises(RuntimeError, match="--task 2: the model has tasks 0 to 1"):
        P.main(args)
    args.task, args.previous = 1, "no_such_file.json"
    with pytest.raises(RuntimeError, match="--previous no_such_file.json: no such file"):
        P.main(args)
    args.previous, args.fill_root, args.out_root, args.layout = None, "no_such_folder", "x", "BDD"
    with pytest.raises(RuntimeError, match="--fill-root no_such_folder: no such folder"):
        P.main(args)
    assert not os.path.exists("r.json") and not os.path.exists("x")


def test_docstring_readme_and_design_say_what_is_not_measured():
    from mdil_ss_amd import superpixel as P
    texts = [P.__doc__] + [open(os.path.join(REPO, f)).read() for f in ("README.md", "DESIGN.md")]
    for text in texts:
        flat = " ".join(text.split()).lower()
        assert "not cielab" in flat
        assert "no connectivity enforcement" in flat and "may be disconnected" in flat
        assert "untuned" in flat
        assert "randomly initialised network" in flat
        assert "no retraining" in flat
        assert "which criterion" in flat
    for f in ("README.md", "DESIGN.md"):
        flat = " ".join(open(os.path.join(REPO, f)).read().split())
        assert "mdil_ss_amd.superpixel" in flat and "libmdil_spx.so" in flat
    assert "spx_bench.json" in open(os.path.join(REPO, "profiles", "README.md")).read()
    assert "not CIELAB" in " ".join(open(os.path.join(REPO, "include", "mdil_spx.h")).read().replace(" * ", " ").split())


def test_training_build_id_is_untouched():
    """tests/test_miou_parity.py counts only the recorded mIoU runs that carry the id of the build
    under test and needs 32 of them: the add-on must leave that id where the recorded runs have it."""
    from mdil_ss_amd import superpixel  # noqa: F401
    from tests import helpers
    tags = [str(t) for t in np.load(os.path.join(REPO, "tests", "golden", "miou_run.npz"),
                                    allow_pickle=False)["hip_build"]]
    build = helpers.kernel_build_id()
    assert tags.count(build) >= 32, f"build id {build} is carried by {tags.count(build)} recorded runs"
