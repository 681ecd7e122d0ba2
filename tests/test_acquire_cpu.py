"""CPU: the acquisition add-on (include/mdil_acquire.h, mdil_ss_amd/acquire.py) -- the reference of
tests/acquire_reference.py against hand-worked examples, the package's host arithmetic against that
reference, the library's exports and argument counts against the header, every argument check before
any launch, and the command line's defaults and refusals."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import acquire_reference as R
from tests.helpers import declared_names, dynamic_exports

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mdil_acquire_apply", "mdil_acquire_head", "mdil_acquire_last_error", "mdil_acquire_version"]


# ------------------------------------------------------------------------------------ by hand
def test_q_and_uncertainties_by_hand():
    u = torch.tensor([-0.5, 0.0, 2.0 ** -17, 2.0 ** -16, 0.5, 1.0 - 2.0 ** -17, 1.0, 1.5])
    assert R.q_of(u).tolist() == [0, 0, 0, 1, 32768, 65535, 65535, 65535]
    # two classes, logits (ln 3, 0): p = (3/4, 1/4)
    logits = torch.tensor([math.log(3.0), 0.0], dtype=torch.float64).reshape(1, 2, 1, 1)
    assert abs(float(R.scores(logits, "msp")) - 0.25) < 1e-15
    assert abs(float(R.scores(logits, "margin")) - 0.5) < 1e-15
    H = -(0.75 * math.log(0.75) + 0.25 * math.log(0.25)) / math.log(2.0)
    assert abs(float(R.scores(logits, "entropy")) - H) < 1e-15
    flat = torch.zeros(1, 4, 1, 1, dtype=torch.float64)                # uniform: every uncertainty at its top
    assert abs(float(R.scores(flat, "msp")) - 0.75) < 1e-15 and abs(float(R.scores(flat, "entropy")) - 1.0) < 1e-15
    assert abs(float(R.scores(flat, "margin")) - 1.0) < 1e-15


def hand_maps():
    """One image of 4 x 6 pixels, 3 classes, tiles of 2 x 4: a 2 x 2 grid whose last column is ragged (2 wide)."""
    label = torch.tensor([[[0, 0, 0, 0, 1, 1],
                           [0, 0, 1, 1, 1, 1],
                           [2, 2, 2, 2, 0, 1],
                           [2, 2, 2, 2, 1, 0]]], dtype=torch.uint8)
    q = torch.tensor([[[100, 100, 100, 100, 7, 7],
                       [100, 100, 300, 300, 7, 7],
                       [0, 0, 0, 0, 65535, 65535],
                       [0, 0, 0, 0, 65535, 1]]])
    target = torch.tensor([[[0, 0, 0, 0, 1, 0],
                            [0, 0, 0, 255, 1, 9],
                            [2, 2, 2, 2, 1, 1],
                            [2, 2, 2, 1, 1, 0]]], dtype=torch.uint8)
    return label, q, target


def test_tile_table_by_hand():
    label, q, target = hand_maps()
    t = R.tile_table(label, q, target, 3, 255, (2, 4))
    assert tuple(t.shape) == (1, 2, 2, 7)
    assert t[0, 0, 0].tolist() == [8, 1200, 1, 7, 6, 2, 0]           # one ignored pixel, one wrong (1 given 0)
    assert t[0, 0, 1].tolist() == [4, 28, 1, 3, 0, 4, 0]             # the 9 is out of range: not valid
    assert t[0, 1, 0].tolist() == [8, 0, 1, 8, 0, 0, 8]
    assert t[0, 1, 1].tolist() == [4, 3 * 65535 + 1, 1, 4, 2, 2, 0]
    none = R.tile_table(label, q, None, 3, 255, (2, 4))
    assert none[..., 2:4].sum() == 0 and torch.equal(none[..., :2], t[..., :2]) and torch.equal(none[..., 4:], t[..., 4:])
    finite = torch.ones(1, 4, 6, dtype=torch.bool)
    finite[0, 0, 0] = False
    assert R.tile_table(label, q, target, 3, 255, (2, 4), finite)[0, 0, 0].tolist() == [7, 1100, 1, 6, 5, 2, 0]


def test_scores_ties_budget_and_cap_by_hand():
    label, q, target = hand_maps()
    t = R.tile_table(label, q, target, 3, 255, (2, 4))
    U = [s for s, *_ in R.all_scores(t, "uncertainty")]
    assert U == [1200 / (65536 * 8), 28 / (65536 * 4), 0.0, (3 * 65535 + 1) / (65536 * 4)]
    I = [s for s, *_ in R.all_scores(t, "impurity")]
    h = -(0.75 * math.log(0.75) + 0.25 * math.log(0.25)) / math.log(3)
    assert I[0] == h and I[1] == 0.0 and I[2] == 0.0 and abs(I[3] - math.log(2) / math.log(3)) < 1e-15
    assert [s for s, *_ in R.all_scores(t, "ripu")] == [U[0] * I[0], 0.0, 0.0, U[3] * I[3]]
    assert [s for s, *_ in R.all_scores(t, "oracle")] == [1 / 8, 1 / 4, 1 / 8, 1 / 4]
    # ties by (image, ty, tx): oracle ranks (0,1) before (1,1), then (0,0) before (1,0)
    assert R.rank(R.all_scores(t, "oracle")) == [(0, 0, 1), (0, 1, 1), (0, 0, 0), (0, 1, 0)]
    assert R.rank(R.all_scores(t, "ripu")) == [(0, 1, 1), (0, 0, 0), (0, 0, 1), (0, 1, 0)]
    assert R.rank(R.all_scores(t, "ripu"), removed={(0, 1, 1)}) == [(0, 0, 0), (0, 0, 1), (0, 1, 0)]
    order = R.rank(R.all_scores(t, "oracle"))
    # 24 pixels; half of them: the two ragged tiles (4 + 4) fit, the next (8) would make 16 > 12: the walk ENDS there
    assert R.select(order, (4, 6), (2, 4), 1, 0.5) == ([(0, 0, 1), (0, 1, 1)], 8)
    assert R.select(order, (4, 6), (2, 4), 1, 1.0) == (order, 24)
    assert R.select(order, (4, 6), (2, 4), 1, 0.1) == ([], 0)
    # two images, a cap of a third of an image (8 pixels): image 0 gives its two small tiles, then the walk goes on
    two = torch.cat([t, t])
    order2 = R.rank(R.all_scores(two, "oracle"))
    assert order2[:4] == [(0, 0, 1), (0, 1, 1), (1, 0, 1), (1, 1, 1)]
    chosen, spent = R.select(order2, (4, 6), (2, 4), 2, 1.0, max_per_image=1 / 3)
    assert chosen == [(0, 0, 1), (0, 1, 1), (1, 0, 1), (1, 1, 1)] and spent == 16
    # a cap of 0.7 (16.8 pixels) under a budget of half the split (24): image 0's first large tile fits (16), its
    # second is skipped (24 > 16.8), image 1's first large tile would pass the budget (32 > 24): the walk ends
    chosen, spent = R.select(order2, (4, 6), (2, 4), 2, 0.5, max_per_image=0.7)
    assert chosen == [(0, 0, 1), (0, 1, 1), (1, 0, 1), (1, 1, 1), (0, 0, 0)] and spent == 24
    assert R.select(order2, (4, 6), (2, 4), 2, 0.5, max_per_image=0.5) == (chosen[:4], 16)   # every large tile skipped


def test_random_scores_are_a_fixed_hash():
    assert R.mix(0, 1) == 0xE220A8397B1DCDAF                           # SplitMix64's first output from seed 0
    a = [R.tile_score([1, 0, 0, 0, 1, 0], "random", 2, 7, i, j) for i in range(3) for j in range(4)]
    assert len(set(a)) == 12 and all(0.0 <= v < 1.0 for v in a)
    assert a == [R.tile_score([9, 9, 9, 9, 9, 0], "random", 2, 7, i, j) for i in range(3) for j in range(4)]
    assert a != [R.tile_score([1, 0, 0, 0, 1, 0], "random", 2, 8, i, j) for i in range(3) for j in range(4)]


def test_apply_precedence_by_hand():
    sel = torch.tensor([[[1, 0]]], dtype=torch.uint8)                  # one image, 2 x 6, tiles 2 x 4: left chosen
    target = torch.tensor([[[0, 1, 2, 255, 0, 0], [9, 1, 1, 1, 0, 0]]], dtype=torch.uint8)
    previous = torch.tensor([[[2, 2, 2, 2, 1, 250], [2, 2, 2, 2, 250, 7]]], dtype=torch.uint8)
    fill = torch.tensor([[[0, 0, 0, 0, 0, 2], [0, 0, 0, 0, 250, 2]]], dtype=torch.uint8)
    r = R.apply_ref(sel, (2, 6), (2, 4), 3, target, previous, fill, 255, 250)
    assert r["out"].tolist() == [[[0, 1, 2, 255, 1, 2], [9, 1, 1, 1, 250, 7]]]
    assert r["mask"].tolist() == [[[255, 255, 255, 255, 128, 64], [255, 255, 255, 255, 0, 128]]]
    assert r["shown"] == 8 and r["bad_targets"] == 1 and r["annotated"].tolist() == [1, 4, 1]
    assert r["kept"].tolist() == [0, 1, 0] and r["filled"].tolist() == [0, 0, 1]       # the kept 7 is no class
    r = R.apply_ref(sel, (2, 6), (2, 4), 3, None, None, fill, 255, 250)
    assert r["out"].tolist() == [[[250, 250, 250, 250, 0, 2], [250, 250, 250, 250, 250, 2]]]
    assert r["mask"].tolist() == [[[255, 255, 255, 255, 64, 64], [255, 255, 255, 255, 0, 64]]]
    r = R.apply_ref(sel, (2, 6), (2, 4), 3, target)
    assert r["out"].tolist() == [[[0, 1, 2, 255, 255, 255], [9, 1, 1, 1, 255, 255]]] and int(r["mask"].sum()) == 8 * 255


# ------------------------------------------------------------ the package's host arithmetic
def seeded_table(M=3, Ty=4, Tx=5, nc=6, seed=3):
    g = torch.Generator().manual_seed(seed)
    hist = torch.randint(0, 40, (M, Ty, Tx, nc), generator=g)
    hist[0, 0, 0] = 0                                                  # a tile without a finite pixel
    hist[1, 2, 3, 1:] = 0                                              # a pure tile
    cnt = hist.sum(-1)
    qsum = (torch.rand(M, Ty, Tx, generator=g, dtype=torch.float64) * cnt * 65535).long()
    valid = (torch.rand(M, Ty, Tx, generator=g) * (cnt + 1)).long().clamp(max=cnt)
    wrong = (torch.rand(M, Ty, Tx, generator=g) * (valid + 1)).long().clamp(max=valid)
    wrong[2, 1, 1], wrong[2, 1, 2], valid[2, 1, 1], valid[2, 1, 2] = 5, 5, 5, 5      # an exact tie where cnt agrees
    hist[2, 1, 1], hist[2, 1, 2] = torch.tensor([10, 0, 0, 0, 0, 0]), torch.tensor([0, 10, 0, 0, 0, 0])
    cnt = hist.sum(-1)
    return torch.cat([torch.stack([cnt, qsum.clamp(max=cnt * 65535), wrong.clamp(max=cnt), valid.clamp(max=cnt)], -1), hist], -1)


@pytest.mark.parametrize("by", R.CRITERIA)
def test_package_scores_ranking_and_budget_match_the_reference(by):
    from mdil_ss_amd import acquire as A
    t = seeded_table()
    M, Ty, Tx, width = t.shape
    nc, T = width - 4, Ty * Tx
    flat = t.reshape(-1, width)
    image, tidx = np.repeat(np.arange(M), T), np.tile(np.arange(T), M)
    got = A.tile_scores(flat, by, image, tidx, seed=11)
    want = R.all_scores(t, by, seed=11)
    assert np.allclose(got.numpy(), [s for s, *_ in want], rtol=1e-14, atol=0)
    size, tile = (4 * 6 - 2, 5 * 8 - 4), (6, 8)                          # ragged last row and column
    assert A.tile_grid(size, tile) == (Ty, Tx) == R.grid(size, tile)
    boxes, pixels = A.tile_boxes(size, tile)
    assert pixels == [R.tile_pixels(size, tile, y, x) for y in range(Ty) for x in range(Tx)]
    assert boxes[-1] == (18, 32, 22, 36) and sum(pixels) == size[0] * size[1]
    usable = flat[:, 0].numpy() > 0
    removed = {(1, 0, 0), (2, 3, 4)}
    for i, y, x in removed:
        usable[i * T + y * Tx + x] = False
    order = A.rank_tiles(got.numpy(), image, tidx // Tx, tidx % Tx, usable)
    ref_order = R.rank([w for w in want if flat[(w[1] * Ty + w[2]) * Tx + w[3], 0] > 0], removed)
    assert [(int(image[i]), int(tidx[i] // Tx), int(tidx[i] % Tx)) for i in order] == ref_order
    for budget, cap in ((0.05, None), (0.3, None), (0.5, 0.25), (1.0, 0.1), (1.0, None)):
        chosen, spent = A.select_tiles(order, np.tile(pixels, M), image, [size[0] * size[1]] * M,
                                       budget * M * size[0] * size[1], cap)
        ref_chosen, ref_spent = R.select(ref_order, size, tile, M, budget, cap)
        assert [(int(image[i]), int(tidx[i] // Tx), int(tidx[i] % Tx)) for i in chosen] == ref_chosen
        assert spent == ref_spent <= budget * M * size[0] * size[1]
        if cap is None and budget < 1.0:
            assert spent > budget * M * size[0] * size[1] - max(pixels)
    assert A.error_recall(flat, torch.tensor(order[:7].copy())) == int(flat[order[:7].copy(), 2].sum()) / int(flat[:, 2].sum())


def test_package_hash_and_constants():
    from mdil_ss_amd import acquire as A
    assert A.mix64(0, 1) == R.mix(0, 1) == 0xE220A8397B1DCDAF
    assert all(A.random_score(s, i, j) == R.tile_score([1], "random", 2, s, i, j) for s in (0, 5, 2 ** 63 + 1)
               for i in (0, 3) for j in (0, 17))
    assert A.inv_log_nc(20) == float(np.float32(1.0 / math.log(20)))
    assert (A.KINDS, A.CRITERIA, A.FIELDS) == (R.KINDS, R.CRITERIA, R.FIELDS)
    with pytest.raises(RuntimeError, match="oracle criterion needs labels"):
        A.tile_scores(seeded_table().reshape(-1, 10), "oracle", labelled=False)
    with pytest.raises(RuntimeError, match="criterion 'best'"):
        A.tile_scores(seeded_table().reshape(-1, 10), "best")
    with pytest.raises(RuntimeError, match="host int64"):
        A.uncertainty_of(torch.zeros(3, 10))


def test_read_selection(tmp_path):
    import json
    from mdil_ss_amd import acquire as A
    f = tmp_path / "selection.json"
    f.write_text(json.dumps({"tile": [4, 6], "size": [16, 24], "tiles": {"a": [[4, 6, 8, 12, 0.5], [12, 18, 16, 24, 0.1]]}}))
    assert A.read_selection(str(f), (4, 6), (16, 24)) == {"a": {(1, 1), (3, 3)}}
    with pytest.raises(RuntimeError, match="selected with tiles of"):
        A.read_selection(str(f), (8, 8), (16, 24))
    f.write_text("{}")
    with pytest.raises(RuntimeError, match="not a selection.json"):
        A.read_selection(str(f), (4, 6), (16, 24))


# -------------------------------------------------------------------------------------- library
def header():
    text = open(os.path.join(REPO, "include", "mdil_acquire.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_library_exports_exactly_the_declared_symbols():
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _acquire_lib
    lib = _acquire_lib.load()
    assert declared_names("mdil_acquire.h") == NAMES
    for n in NAMES:
        assert hasattr(lib, n), f"{n} declared in include/mdil_acquire.h but not exported"
    assert sorted(_acquire_lib.EXPORTS) == NAMES
    assert dynamic_exports(_acquire_lib.LIB_PATH) == NAMES
    assert lib.mdil_acquire_version() >= 100


def test_header_export_map_and_binding_name_the_same_entry_points():
    from mdil_ss_amd import _acquire_lib
    hdr = header()
    declared = {}
    for name, params in re.findall(r"\b(mdil_acquire_\w+)\s*\(([^)]*)\)\s*;", hdr):
        params = params.strip()
        declared[name] = 0 if params == "void" else params.count(",") + 1
    mapped = re.findall(r"^\s*(mdil_acquire_\w+);", open(os.path.join(REPO, "mdil_ss_amd", "ext", "acquire_exports.map")).read(),
                        flags=re.M)
    assert sorted(declared) == sorted(mapped) == sorted(_acquire_lib._SIGNATURES) == NAMES
    for name, (_, argtypes) in _acquire_lib._SIGNATURES.items():
        assert declared[name] == len(argtypes), (name, declared[name], len(argtypes))
    assert (declared["mdil_acquire_head"], declared["mdil_acquire_apply"]) == (19, 20)
    macros = {k: int(v) for k, v in re.findall(r"#define\s+MDIL_ACQUIRE_(\w+)\s+\(?(-?\d+)\)?", hdr)}
    assert (macros["MIN_CLASSES"], macros["MAX_CLASSES"]) == (_acquire_lib.MIN_CLASSES, _acquire_lib.MAX_CLASSES) == (2, 32)
    assert (macros["MIN_TILE"], macros["MAX_TILE"]) == (_acquire_lib.MIN_TILE, _acquire_lib.MAX_TILE) == (2, 256)
    assert (macros["OK"], macros["ERR_INVALID"], macros["ERR_LAUNCH"], macros["Q_ONE"]) == (0, -1, -2, 65536)
    assert (macros["MSP"], macros["ENTROPY"], macros["MARGIN"], macros["KINDS"]) == (0, 1, 2, 3)
    assert macros["TILE_FIELDS"] == _acquire_lib.TILE_FIELDS == 4


def test_build_checks_the_binding_and_the_makefile_builds_it():
    assert "_acquire_lib" in open(os.path.join(REPO, "__graft_entry__.py")).read()
    assert re.search(r"^NAMES \+= acquire$", open(os.path.join(REPO, "mdil_ss_amd", "ext", "Makefile")).read(), flags=re.M)


HEAD_OK = dict(x=4096, w=8192, b=12288, N=1, H=4, W=4, nc=20, th=4, tw=4, kind=1, inv=0.33, tgt=16384, ign=19,
               label=20480, qmap=24576, tiles=28672, nonf=32768, badt=36864)
APPLY_OK = dict(sel=4096, tgt=8192, prev=12288, fill=16384, N=1, Hl=8, Wl=8, th=4, tw=4, nc=20, ign=19, drop=255,
                out=20480, mask=24576, shown=28672, ann=32768, kept=36864, filled=40960, badt=45056)


def _head(lib, **kw):
    a = dict(HEAD_OK, **kw)
    return lib.mdil_acquire_head(a["x"], a["w"], a["b"], a["N"], a["H"], a["W"], a["nc"], a["th"], a["tw"], a["kind"],
                                 a["inv"], a["tgt"], a["ign"], a["label"], a["qmap"], a["tiles"], a["nonf"], a["badt"], None)


def _apply(lib, **kw):
    a = dict(APPLY_OK, **kw)
    return lib.mdil_acquire_apply(a["sel"], a["tgt"], a["prev"], a["fill"], a["N"], a["Hl"], a["Wl"], a["th"], a["tw"],
                                  a["nc"], a["ign"], a["drop"], a["out"], a["mask"], a["shown"], a["ann"], a["kept"],
                                  a["filled"], a["badt"], None)


@pytest.mark.parametrize("call, bad, text", [
    (_head, dict(nc=1), b"nc=1"), (_head, dict(nc=33), b"nc=33"),
    (_head, dict(x=None), b"bad argument"), (_head, dict(w=None), b"bad argument"), (_head, dict(b=None), b"bad argument"),
    (_head, dict(N=0), b"bad argument"), (_head, dict(H=-1), b"bad argument"), (_head, dict(W=0), b"bad argument"),
    (_head, dict(label=None, qmap=None, tiles=None, nonf=None, badt=None), b"nothing to write"),
    (_head, dict(th=3), b"tile 3 x 4"), (_head, dict(tw=5), b"tile 4 x 5"), (_head, dict(th=0), b"tile 0 x 4"),
    (_head, dict(tw=258), b"tile 4 x 258"), (_head, dict(th=-2), b"tile -2 x 4"), (_head, dict(th=257, tw=257), b"tile 257"),
    (_head, dict(kind=-1), b"kind=-1"), (_head, dict(kind=3), b"kind=3"),
    (_head, dict(inv=-1.0), b"inv_log_nc"), (_head, dict(inv=float("inf")), b"inv_log_nc"),
    (_head, dict(inv=float("nan")), b"inv_log_nc"),
    (_head, dict(ign=-2), b"ignore_index=-2"), (_head, dict(ign=256), b"ignore_index=256"),
    (_head, dict(tgt=None), b"needs a target"),
    (_head, dict(x=4100), b"alignment"), (_head, dict(w=8194), b"alignment"), (_head, dict(b=12290), b"alignment"),
    (_head, dict(tgt=16385), b"alignment"), (_head, dict(label=20481), b"alignment"), (_head, dict(qmap=24578), b"alignment"),
    (_head, dict(tiles=28676), b"alignment"), (_head, dict(nonf=32772), b"alignment"), (_head, dict(badt=36868), b"alignment"),
    (_head, dict(W=1 << 30), b"too large"), (_head, dict(N=1 << 20, H=1 << 10, W=1 << 10), b"too large"),
    (_head, dict(N=1 << 12, H=1 << 10, W=1 << 10, th=2, tw=2), b"2^31 cells"),
    (_apply, dict(nc=1), b"nc=1"), (_apply, dict(nc=33), b"nc=33"),
    (_apply, dict(sel=None), b"bad argument"), (_apply, dict(N=0), b"bad argument"), (_apply, dict(Hl=0), b"bad argument"),
    (_apply, dict(Wl=-3), b"bad argument"), (_apply, dict(N=1 << 20, Hl=1 << 20, Wl=1 << 10), b"too large"),
    (_apply, dict(th=3), b"tile 3 x 4"), (_apply, dict(tw=300), b"tile 4 x 300"),
    (_apply, dict(ign=-2), b"ignore_index=-2"), (_apply, dict(drop=-1), b"drop_id=-1"), (_apply, dict(drop=256), b"drop_id=256"),
    (_apply, dict(out=None, mask=None, shown=None, ann=None, kept=None, filled=None, badt=None), b"nothing to write"),
    (_apply, dict(tgt=None), b"need a target"), (_apply, dict(tgt=None, ann=None), b"need a target"),
    (_apply, dict(tgt=None, badt=None), b"need a target"),
    (_apply, dict(tgt=8196), b"alignment"), (_apply, dict(prev=12292), b"alignment"), (_apply, dict(fill=16388), b"alignment"),
    (_apply, dict(out=20484), b"alignment"), (_apply, dict(mask=24580), b"alignment"), (_apply, dict(shown=28676), b"alignment"),
    (_apply, dict(ann=32772), b"alignment"), (_apply, dict(kept=36868), b"alignment"), (_apply, dict(filled=40964), b"alignment"),
    (_apply, dict(badt=45060), b"alignment"),
])
def test_library_refuses_bad_arguments_without_a_device(call, bad, text):
    """Argument checks come before the launch, so fake pointers never reach a device."""
    from mdil_ss_amd import _acquire_lib
    lib = _acquire_lib.load()
    assert call(lib, **bad) == -1, bad
    assert text in lib.mdil_acquire_last_error(), (bad, lib.mdil_acquire_last_error())


# -------------------------------------------------------------------------------------- wrappers
def test_wrappers_refuse_cpu_tensors_and_bad_values():
    from mdil_ss_amd import acquire as A
    x, w, b = torch.zeros(1, 2, 2, 16), torch.zeros(16, 20, 2, 2), torch.zeros(20)
    with pytest.raises(RuntimeError, match="features must be a contiguous float32 device tensor.*no CPU fallback in "
                                           "the acquisition path"):
        A.acquire_head(x, w, b, (4, 4), want_label=True)
    sel = torch.zeros(1, 2, 2, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="selected must be a contiguous uint8.*no CPU fallback in the acquisition path"):
        A.acquire_apply(sel, (8, 8), (4, 4), 20)
    for nc in (1, 33):
        with pytest.raises(RuntimeError, match=f"{nc} classes \\(supported: 2 to 32\\)"):
            A.acquire_apply(sel, (8, 8), (4, 4), nc)
    for tile in ((3, 4), (4, 258), (0, 4), (4,), "ab"):
        with pytest.raises(RuntimeError, match="tile"):
            A.acquire_apply(sel, (8, 8), tile, 20)
    with pytest.raises(RuntimeError, match="drop_id 256"):
        A.acquire_apply(sel, (8, 8), (4, 4), 20, drop_id=256)
    with pytest.raises(RuntimeError, match="ignore_index 300"):
        A.acquire_apply(sel, (8, 8), (4, 4), 20, ignore_index=300)
    with pytest.raises(RuntimeError, match="kind 'energy'"):
        A.check_kind("acquire_head", "energy")
    assert A.check_tile("t", [32, 64]) == (32, 64) and A.tile_grid((18, 14), (4, 6)) == (5, 3)


# ---------------------------------------------------------------------------------- command line
BASE = ["--state", "ckpt.pth.tar", "--num-classes", "20", "20", "--task", "1"]


def test_parser_defaults():
    from mdil_ss_amd import acquire as A
    a = A.build_parser().parse_args(BASE + ["--dataset", "BDD", "--budget", "0.05", "--json", "r.json"])
    assert (a.dataset, a.subset, a.synthetic, a.images, a.json, a.out, a.out_root, a.layout) == \
        ("BDD", "train", 0, None, "r.json", None, None, None)
    assert (a.budget, a.tile, a.kind, a.by, a.seed, a.max_per_image, a.previous, a.previous_root, a.fill_root) == \
        (0.05, [32, 32], "entropy", "ripu", 0, None, None, None, None)
    assert (a.height, a.width, a.batch_size) == (512, 1024, 6)
    assert all(hasattr(a, k) for k in ("cs_datadir", "bdd_datadir", "idd_datadir", "cache_resized"))
    b = A.build_parser().parse_args(BASE + ["--synthetic", "2", "--budget", "0.1", "--tile", "16", "64", "--kind", "margin",
                                            "--by", "oracle", "--max-per-image", "0.25", "--previous", "s.json",
                                            "--previous-root", "r0", "--fill-root", "p", "--out-root", "r1", "--layout", "BDD",
                                            "--out", "o", "--seed", "4"])
    assert (b.tile, b.kind, b.by, b.max_per_image, b.previous, b.previous_root, b.fill_root, b.out_root, b.layout, b.out,
            b.seed) == ([16, 64], "margin", "oracle", 0.25, "s.json", "r0", "p", "r1", "BDD", "o", 4)
    assert callable(A.main)


@pytest.mark.parametrize("argv, text", [
    (["--budget", "0.1", "--json", "r"], "give one source"),
    (["--dataset", "BDD", "--synthetic", "2", "--budget", "0.1", "--json", "r"], "give one source"),
    (["--dataset", "BDD", "--json", "r"], "--budget"),
    (["--dataset", "BDD", "--budget", "0.1"], "nothing to do"),
    (["--dataset", "BDD", "--budget", "0", "--json", "r"], "--budget 0"),
    (["--dataset", "BDD", "--budget", "1.5", "--json", "r"], "--budget 1.5"),
    (["--dataset", "BDD", "--budget", "0.1", "--json", "r", "--max-per-image", "0"], "--max-per-image"),
    (["--dataset", "BDD", "--budget", "0.1", "--json", "r", "--tile", "31", "32"], "tile 31 x 32"),
    (["--dataset", "BDD", "--budget", "0.1", "--json", "r", "--tile", "32", "512"], "tile 32 x 512"),
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
])
def test_parser_refusals(argv, text, capsys):
    from mdil_ss_amd import acquire as A
    with pytest.raises(SystemExit):
        A.build_parser().parse_args(BASE + argv)
    assert re.search(text, capsys.readouterr().err)


def test_main_refuses_before_it_opens_anything():
    """The checkpoint does not exist: every refusal below comes before it would be opened."""
    from mdil_ss_amd import acquire as A
    args = A.build_parser().parse_args(BASE + ["--dataset", "BDD", "--budget", "0.1", "--json", "r.json"])
    args.json = None
    with pytest.raises(RuntimeError, match="nothing to do"):
        A.main(args)
    args.json, args.task = "r.json", 2
    with pytest.raises(RuntimeError, match="--task 2: the model has tasks 0 to 1"):
        A.main(args)
    args.task, args.previous = 1, "no_such_file.json"
    with pytest.raises(RuntimeError, match="--previous no_such_file.json: no such file"):
        A.main(args)
    assert not os.path.exists("r.json")


def test_docstring_readme_and_design_say_what_is_not_measured():
    from mdil_ss_amd import acquire as A
    texts = [A.__doc__] + [open(os.path.join(REPO, f)).read() for f in ("README.md", "DESIGN.md")]
    for text in texts:
        flat = " ".join(text.split()).lower()
        assert "randomly initialised network" in flat
        assert "sliding (2k+1)" in flat and "not built" in flat
        assert "no retraining" in flat
        assert "which criterion" in flat


def test_training_build_id_is_untouched():
    """tests/test_miou_parity.py counts only the recorded mIoU runs that carry the id of the build
    under test and needs 32 of them: the add-on must leave that id where the recorded runs have it."""
    from mdil_ss_amd import acquire  # noqa: F401
    from tests import helpers
    tags = [str(t) for t in np.load(os.path.join(REPO, "tests", "golden", "miou_run.npz"),
                                    allow_pickle=False)["hip_build"]]
    build = helpers.kernel_build_id()
    assert tags.count(build) >= 32, f"build id {build} is carried by {tags.count(build)} recorded runs"
