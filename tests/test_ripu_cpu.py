"""CPU: the sliding-region acquisition add-on (include/mdil_ripu.h, mdil_ss_amd/ripu.py) -- the reference of
tests/ripu_reference.py against brute force and hand-worked examples, the library's exports and argument counts
against the header, every argument check before any launch, and the command line's defaults and refusals."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import ripu_reference as R
from tests.helpers import declared_names, dynamic_exports

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mdil_ripu_apply", "mdil_ripu_last_error", "mdil_ripu_score", "mdil_ripu_select", "mdil_ripu_version"]


# ---------------------------------------------------------------------------------- reference
@pytest.mark.parametrize("shape", ((1, 1, 1), (2, 5, 12), (1, 12, 7), (3, 9, 9)))
@pytest.mark.parametrize("k", (1, 2, 5, 32))
def test_cumsum_box_sums_equal_the_window_loop(shape, k):
    v = torch.randint(0, 70000, shape, generator=torch.Generator().manual_seed(k + shape[1]))
    assert torch.equal(R.box_sums(v, k), R.box_sums_brute(v, k))
    ones = torch.ones(shape, dtype=torch.int64)
    H, W = shape[1:]
    cnt = torch.tensor([[(min(y + k, H - 1) - max(y - k, 0) + 1) * (min(x + k, W - 1) - max(x - k, 0) + 1)
                         for x in range(W)] for y in range(H)])
    assert torch.equal(R.box_sums(ones, k), cnt.expand(shape))                 # the closed form of the header


def test_tlog_table_by_hand():
    from mdil_ss_amd import ripu as P
    t = P.tlog_table(1)
    assert t.dtype == torch.int32 and tuple(t.shape) == (10,)
    # 2 ln 2 = 1.3862943611, x 16384 = 22713.05;  3 ln 3 = 3.2958368660, x 16384 = 53998.99;  4 ln 4 = 4 x 22713.05
    assert t[:5].tolist() == [0, 0, 22713, 53999, 90852]
    for k in (1, 3, 32):
        assert P.tlog_table(k).tolist() == R.tlog(k) and len(R.tlog(k)) == (2 * k + 1) ** 2 + 1
    assert R.tlog(32)[-1] == int(round(4225 * math.log(4225) * 16384)) < 2 ** 30
    for k in (0, 33, 1.5, "a"):
        with pytest.raises(RuntimeError, match="outside \\[1, 32\\]"):
            P.tlog_table(k)


@pytest.mark.parametrize("nc", (2, 32))
@pytest.mark.parametrize("k", (1, 32))
def test_every_key_stays_below_2_32_at_the_largest_products(nc, k):
    H, W = (7, 9) if k == 1 else (70, 67)
    label = ((torch.arange(H)[:, None] * 5 + torch.arange(W)[None] * 3) % nc).to(torch.uint8)[None]   # balanced labels
    q = torch.full((1, H, W), 65535)
    target = ((label.long() + 1) % nc).to(torch.uint8)                        # every pixel wrong
    top = 0
    for by in ("uncertainty", "impurity", "ripu", "oracle"):
        cnt, h = R.window_counts(label, k, nc)
        t = torch.tensor(R.tlog(k))
        E = (t[cnt] - t[h].sum(0)).clamp(min=0)
        raw = {"uncertainty": (R.box_sums(q, k) << 16) // cnt, "impurity": (E << 16) // cnt,
               "ripu": (R.box_sums(q, k) * E) // (cnt * cnt), "oracle": (cnt << 32) // (cnt + 1)}[by]
        assert int(raw.max()) < 2 ** 32, by                                    # nothing to saturate
        assert torch.equal(R.keys_fast(label, k, nc, by, q, target), raw)
        top = max(top, int(raw.max()))
        assert int((R.box_sums(q, k) * E).max()) < 2 ** 57
    assert top >= 65535 * 65536                                               # uncertainty's key at q = 65535 everywhere


def test_keys_by_hand_and_one_label_gives_zero():
    # 1 x 3, k = 1, two classes: windows {0,1}, {0,1,2}, {1,2}
    label = torch.tensor([[[0, 1, 1]]], dtype=torch.uint8)
    q = torch.tensor([[[10, 20, 60]]])
    t = R.tlog(1)
    assert R.keys(label, 1, 2, "uncertainty", q).tolist() == [[[(30 << 16) // 2, (90 << 16) // 3, (80 << 16) // 2]]]
    E = [t[2], t[3] - t[2], 0]                                               # (1,1), (1,2), (0,2)
    assert R.keys(label, 1, 2, "impurity").tolist() == [[[(E[0] << 16) // 2, (E[1] << 16) // 3, 0]]]
    assert R.keys(label, 1, 2, "ripu", q).tolist() == [[[30 * E[0] // 4, 90 * E[1] // 9, 0]]]
    target = torch.tensor([[[1, 1, 255]]], dtype=torch.uint8)
    assert R.keys(label, 1, 2, "oracle", target=target, ignore=255).tolist() == [[[(1 << 32) // 3, (1 << 32) // 4, 0]]]
    taken = torch.tensor([[[0, 7, 0]]], dtype=torch.uint8)
    assert R.keys(label, 1, 2, "uncertainty", q, taken=taken).tolist() == [[[(30 << 16) // 2, 0, (80 << 16) // 2]]]
    rnd = R.keys(label, 1, 2, "random", seed=5, image0=3)
    assert rnd.tolist() == [[[max(1, R.mix(R.mix(5, 4), i + 1) >> 32) for i in range(3)]]] and R.mix(0, 1) == 0xE220A8397B1DCDAF
    # a label >= nc counts in cnt and in no h_c: for the window (1, 9), E = tlog[2] - tlog[1]
    assert R.keys(torch.tensor([[[1, 9]]], dtype=torch.uint8), 1, 2, "impurity").tolist() == [[[t[2] << 16 >> 1] * 2]]
    for shape, k in (((2, 9, 7), 1), ((1, 6, 11), 3), ((1, 9, 7), 32)):
        one = torch.full(shape, 4, dtype=torch.uint8)
        qq = torch.randint(0, 65536, shape, generator=torch.Generator().manual_seed(k))
        for by in ("impurity", "ripu"):
            assert int(R.keys(one, k, 20, by, qq).abs().sum()) == 0 and int(R.keys_fast(one, k, 20, by, qq).abs().sum()) == 0
    # the tensor form is the integer form
    g = torch.Generator().manual_seed(2)
    label = torch.randint(0, 5, (2, 6, 8), generator=g, dtype=torch.uint8)
    qq, target = torch.randint(0, 65536, (2, 6, 8), generator=g), torch.randint(0, 5, (2, 6, 8), generator=g, dtype=torch.uint8)
    taken = (torch.rand(2, 6, 8, generator=g) < 0.2).to(torch.uint8)
    for by in R.CRITERIA:
        for tk in (None, taken):
            assert torch.equal(R.keys(label, 2, 4, by, qq, target, 3, tk, seed=9), R.keys_fast(label, 2, 4, by, qq, target, 3, tk, seed=9))


def test_greedy_pick_by_hand():
    key = torch.tensor([[[5, 0, 0, 0, 9],
                         [0, 0, 0, 0, 0],
                         [0, 0, 7, 0, 0],
                         [0, 0, 0, 0, 0],
                         [9, 0, 0, 0, 3]]])
    taken = torch.zeros(1, 5, 5, dtype=torch.uint8)
    taken[0, 0, 3] = 128                                                      # an earlier round's mark
    # the 9s tie: (0, 4) comes first in raster order; its clipped 2 x 2 region holds the mark: 3 fresh.  (4, 0): 4 fresh.
    # (2, 2): 9 pixels, (1, 3) and (3, 1) already taken: 7 fresh, 14 shown.  (0, 0): (1, 1) taken: 3 fresh, 17.  (4, 4): 3, 20.
    full = [(0, 4, 9, 3), (4, 0, 9, 4), (2, 2, 7, 7), (0, 0, 5, 3), (4, 4, 3, 3)]
    after, picks, shown, stop = R.select(key, taken, 1, 20, 10)
    assert picks == [full] and shown == [20] and stop == [R.STOP_EMPTY]       # what is left has key 0
    assert int(after[0, 0, 3]) == 128 and int((after == 255).sum()) == 20 and int(after[0, 2, 0]) == 0
    assert R.select(key, taken, 1, 14, 10)[1:] == ([full[:3]], [14], [R.STOP_BUDGET])   # 14 + 3 > 14
    assert R.select(key, taken, 1, 13, 10)[1:] == ([full[:2]], [7], [R.STOP_BUDGET])    # 7 + 7 > 13: the walk ENDS
    assert R.select(key, taken, 1, 100, 2)[1:] == ([full[:2]], [7], [R.STOP_PICKS])
    assert R.select(key, taken, 1, 2, 10)[1:] == ([[]], [0], [R.STOP_BUDGET])
    marked = taken.clone()
    marked[0, 2, 2] = 1                                                       # a taken pixel is no centre
    assert R.select(key, marked, 1, 100, 10)[1] == [[full[0], full[1], (0, 0, 5, 4), (4, 4, 3, 4)]]
    pixel = R.select(key, taken, 0, 3, 10)                                    # pixel mode: one pixel per pick
    assert pixel[1:] == ([[(0, 4, 9, 1), (4, 0, 9, 1), (2, 2, 7, 1)]], [3], [R.STOP_BUDGET])
    assert R.select(torch.zeros(1, 5, 5, dtype=torch.int64), taken, 1, 100, 10)[1:] == ([[]], [0], [R.STOP_EMPTY])
    assert R.select(key, torch.ones(1, 5, 5, dtype=torch.uint8), 1, 100, 10)[1:] == ([[]], [0], [R.STOP_EMPTY])


def test_apply_precedence_by_hand():
    sel = torch.tensor([[[255, 255, 128, 0, 0, 1]]], dtype=torch.uint8)       # only 255 is chosen
    target = torch.tensor([[[0, 9, 2, 1, 255, 1]]], dtype=torch.uint8)
    previous = torch.tensor([[[2, 2, 1, 250, 7, 250]]], dtype=torch.uint8)
    fill = torch.tensor([[[0, 0, 0, 2, 2, 250]]], dtype=torch.uint8)
    label = torch.tensor([[[1, 1, 2, 0, 0, 1]]], dtype=torch.uint8)
    r = R.apply_ref(sel, 3, target, previous, fill, label, 255, 250)
    assert r["out"].tolist() == [[[0, 9, 1, 2, 7, 250]]] and r["mask"].tolist() == [[[255, 255, 128, 64, 128, 0]]]
    assert r["shown"] == 2 and r["bad_targets"] == 1 and r["annotated"].tolist() == [1, 0, 0]
    assert r["kept"].tolist() == [0, 1, 0] and r["filled"].tolist() == [0, 0, 1]   # the kept 7 is no class
    assert (r["wrong_shown"], r["wrong_all"]) == (1, 2)                       # (0: 1 given 0), (3: 0 given 1); the 9 is not valid
    r = R.apply_ref(sel, 3)
    assert r["out"].tolist() == [[[255] * 6]] and r["mask"].tolist() == [[[255, 255, 0, 0, 0, 0]]]


# -------------------------------------------------------------------------------------- library
def header():
    text = open(os.path.join(REPO, "include", "mdil_ripu.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_library_exports_exactly_the_declared_symbols():
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _ripu_lib
    lib = _ripu_lib.load()
    assert declared_names("mdil_ripu.h") == NAMES
    for n in NAMES:
        assert hasattr(lib, n), f"{n} declared in include/mdil_ripu.h but not exported"
    assert sorted(_ripu_lib.EXPORTS) == NAMES
    assert dynamic_exports(_ripu_lib.LIB_PATH) == NAMES
    assert lib.mdil_ripu_version() >= 100


def test_header_export_map_and_binding_name_the_same_entry_points():
    from mdil_ss_amd import _ripu_lib
    from mdil_ss_amd import ripu as P
    hdr = header()
    declared = {}
    for name, params in re.findall(r"\b(mdil_ripu_\w+)\s*\(([^)]*)\)\s*;", hdr):
        params = params.strip()
        declared[name] = 0 if params == "void" else params.count(",") + 1
    mapped = re.findall(r"^\s*(mdil_ripu_\w+);", open(os.path.join(REPO, "mdil_ss_amd", "ext", "ripu_exports.map")).read(),
                        flags=re.M)
    assert sorted(declared) == sorted(mapped) == sorted(_ripu_lib._SIGNATURES) == NAMES
    for name, (_, argtypes) in _ripu_lib._SIGNATURES.items():
        assert declared[name] == len(argtypes), (name, declared[name], len(argtypes))
    assert (declared["mdil_ripu_score"], declared["mdil_ripu_select"], declared["mdil_ripu_apply"]) == (16, 13, 21)
    macros = {k: int(v) for k, v in re.findall(r"#define\s+MDIL_RIPU_(\w+)\s+\(?(-?\d+)\)?\s", hdr)}
    assert (macros["MIN_CLASSES"], macros["MAX_CLASSES"]) == (_ripu_lib.MIN_CLASSES, _ripu_lib.MAX_CLASSES) == (2, 32)
    assert (macros["MIN_RADIUS"], macros["MAX_RADIUS"]) == (_ripu_lib.MIN_RADIUS, _ripu_lib.MAX_RADIUS) == (1, 32)
    assert (macros["OK"], macros["ERR_INVALID"], macros["ERR_LAUNCH"]) == (0, -1, -2)
    assert macros["MAX_PICKS"] == _ripu_lib.MAX_PICKS == 65536 and macros["TLOG_SHIFT"] == _ripu_lib.TLOG_SHIFT == 14
    assert [macros[c.upper()] for c in P.CRITERIA] == list(range(macros["CRITERIA"])) == list(range(len(R.CRITERIA)))
    assert P.CRITERIA == R.CRITERIA
    assert [macros["STOP_" + s.upper().replace("MAX_", "")] for s in P.STOPS] == [R.STOP_EMPTY, R.STOP_BUDGET, R.STOP_PICKS]


def test_build_checks_the_binding_and_the_makefile_builds_it():
    assert "_ripu_lib" in open(os.path.join(REPO, "__graft_entry__.py")).read()
    make = open(os.path.join(REPO, "mdil_ss_amd", "ext", "Makefile")).read()
    assert re.search(r"^PLAIN := .*\bripu\b", make, flags=re.M) and re.search(r"^NAMES \+= acquire$", make, flags=re.M)
    # no head code: the library takes the shared headers as they are and no head kernel
    src = open(os.path.join(REPO, "mdil_ss_amd", "ext", "ripu.hip")).read()
    assert "map_common.h" in src and "stage_parity" not in src and "logits4" not in src


SCORE_OK = dict(label=4096, qmap=8192, tgt=12288, ign=19, taken=16384, tlog=20480, N=1, Hl=8, Wl=8, nc=20, k=2, by=2, seed=0,
                image0=0, key=24576)
SELECT_OK = dict(key=4096, taken=8192, N=1, Hl=8, Wl=8, r=2, budget=10, P=16, picks=12288, count=16384, shown=20480,
                 stop=24576)
APPLY_OK = dict(sel=4096, tgt=8192, prev=12288, fill=16384, label=20480, N=1, Hl=8, Wl=8, nc=20, ign=19, drop=255, out=24576,
                mask=28672, shown=32768, ann=36864, kept=40960, filled=45056, badt=49152, ws=53248, wa=57344)


def _score(lib, **kw):
    a = dict(SCORE_OK, **kw)
    return lib.mdil_ripu_score(a["label"], a["qmap"], a["tgt"], a["ign"], a["taken"], a["tlog"], a["N"], a["Hl"], a["Wl"],
                               a["nc"], a["k"], a["by"], a["seed"], a["image0"], a["key"], None)


def _select(lib, **kw):
    a = dict(SELECT_OK, **kw)
    return lib.mdil_ripu_select(a["key"], a["taken"], a["N"], a["Hl"], a["Wl"], a["r"], a["budget"], a["P"], a["picks"],
                                a["count"], a["shown"], a["stop"], None)


def _apply(lib, **kw):
    a = dict(APPLY_OK, **kw)
    return lib.mdil_ripu_apply(a["sel"], a["tgt"], a["prev"], a["fill"], a["label"], a["N"], a["Hl"], a["Wl"], a["nc"], a["ign"],
                               a["drop"], a["out"], a["mask"], a["shown"], a["ann"], a["kept"], a["filled"], a["badt"], a["ws"],
                               a["wa"], None)


@pytest.mark.parametrize("call, bad, text", [
    (_score, dict(nc=1), b"nc=1"), (_score, dict(nc=33), b"nc=33"), (_score, dict(k=0), b"k=0"), (_score, dict(k=33), b"k=33"),
    (_score, dict(by=5), b"by=5"), (_score, dict(by=-1), b"by=-1"),
    (_score, dict(qmap=None), b"needs a qmap"), (_score, dict(qmap=None, by=0), b"needs a qmap"),
    (_score, dict(tgt=None, by=3), b"needs a target"), (_score, dict(tlog=None), b"needs the tlog"),
    (_score, dict(tlog=None, by=1), b"needs the tlog"),
    (_score, dict(label=None), b"bad argument"), (_score, dict(key=None), b"nothing to write"),
    (_score, dict(N=0), b"bad argument"), (_score, dict(Hl=-1), b"bad argument"), (_score, dict(Wl=0), b"bad argument"),
    (_score, dict(ign=-2), b"ignore_index=-2"), (_score, dict(ign=256), b"ignore_index=256"), (_score, dict(image0=-1), b"image0"),
    (_score, dict(label=4097), b"alignment"), (_score, dict(qmap=8194), b"alignment"), (_score, dict(tgt=12292), b"alignment"),
    (_score, dict(taken=16388), b"alignment"), (_score, dict(tlog=20484), b"alignment"), (_score, dict(key=24580), b"alignment"),
    (_score, dict(Hl=4096, Wl=4097), b"2^24 pixels per image"), (_score, dict(N=1 << 17, Hl=4096, Wl=4096), b"too large"),
    (_select, dict(r=-1), b"r=-1"), (_select, dict(r=33), b"r=33"), (_select, dict(P=0), b"max_picks=0"),
    (_select, dict(P=65537), b"max_picks=65537"), (_select, dict(budget=-1), b"budget_pixels=-1"),
    (_select, dict(key=None), b"bad argument"), (_select, dict(taken=None), b"bad argument"), (_select, dict(N=0), b"bad argument"),
    (_select, dict(Hl=4097, Wl=4096), b"2^24 pixels per image"),
    (_select, dict(key=4100), b"alignment"), (_select, dict(taken=8193), b"alignment"), (_select, dict(picks=12292), b"alignment"),
    (_select, dict(count=16388), b"alignment"), (_select, dict(shown=20484), b"alignment"), (_select, dict(stop=24580), b"alignment"),
    (_apply, dict(nc=1), b"nc=1"), (_apply, dict(nc=33), b"nc=33"), (_apply, dict(sel=None), b"bad argument"),
    (_apply, dict(N=0), b"bad argument"), (_apply, dict(Wl=-3), b"bad argument"), (_apply, dict(Hl=1 << 13, Wl=1 << 12), b"too large"),
    (_apply, dict(ign=-2), b"ignore_index=-2"), (_apply, dict(drop=-1), b"drop_id=-1"), (_apply, dict(drop=256), b"drop_id=256"),
    (_apply, dict(out=None, mask=None, shown=None, ann=None, kept=None, filled=None, badt=None, ws=None, wa=None),
     b"nothing to write"),
    (_apply, dict(tgt=None), b"need a target"), (_apply, dict(tgt=None, ann=None, ws=None, wa=None), b"need a target"),
    (_apply, dict(label=None), b"need a target and a label"), (_apply, dict(label=None, ws=None), b"need a target and a label"),
    (_apply, dict(sel=4097), b"alignment"), (_apply, dict(tgt=8196), b"alignment"), (_apply, dict(prev=12292), b"alignment"),
    (_apply, dict(fill=16388), b"alignment"), (_apply, dict(label=20484), b"alignment"), (_apply, dict(out=24580), b"alignment"),
    (_apply, dict(mask=28676), b"alignment"), (_apply, dict(shown=32772), b"alignment"), (_apply, dict(ann=36868), b"alignment"),
    (_apply, dict(kept=40964), b"alignment"), (_apply, dict(filled=45060), b"alignment"), (_apply, dict(badt=49156), b"alignment"),
    (_apply, dict(ws=53252), b"alignment"), (_apply, dict(wa=57348), b"alignment"),
])
def test_library_refuses_bad_arguments_without_a_device(call, bad, text):
    """Argument checks come before the launch, so fake pointers never reach a device."""
    from mdil_ss_amd import _ripu_lib
    lib = _ripu_lib.load()
    assert call(lib, **bad) == -1, bad
    assert text in lib.mdil_ripu_last_error(), (bad, lib.mdil_ripu_last_error())


# -------------------------------------------------------------------------------------- wrappers
def test_wrappers_refuse_cpu_tensors_and_bad_values():
    from mdil_ss_amd import ripu as P
    label = torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="label must be a contiguous uint8 device tensor.*no CPU fallback in the ripu path"):
        P.ripu_score(label, 1, 20)
    with pytest.raises(RuntimeError, match="key must be a contiguous uint32 device tensor.*no CPU fallback in the ripu path"):
        P.ripu_select(torch.zeros(1, 4, 4, dtype=torch.uint32), label, 1, 4, 4)
    with pytest.raises(RuntimeError, match="selected must be a contiguous uint8.*no CPU fallback in the ripu path"):
        P.ripu_apply(label, 20)
    for nc in (1, 33):
        with pytest.raises(RuntimeError, match=f"{nc} classes \\(supported: 2 to 32\\)"):
            P.ripu_score(label, 1, nc)
        with pytest.raises(RuntimeError, match=f"{nc} classes \\(supported: 2 to 32\\)"):
            P.ripu_apply(label, nc)
    for k in (0, 33):
        with pytest.raises(RuntimeError, match=f"k {k} outside \\[1, 32\\]"):
            P.ripu_score(label, k, 20)
    for r in (-1, 33):
        with pytest.raises(RuntimeError, match=f"r {r} outside \\[0, 32\\]"):
            P.ripu_select(label, label, r, 4, 4)
    with pytest.raises(RuntimeError, match="criterion 'best'"):
        P.ripu_score(label, 1, 20, "best")
    with pytest.raises(RuntimeError, match="drop_id 256"):
        P.ripu_apply(label, 20, drop_id=256)
    with pytest.raises(RuntimeError, match="ignore_index 300"):
        P.ripu_apply(label, 20, ignore_index=300)
    assert P.key_values(torch.tensor([0xffffffff, 7], dtype=torch.uint32)).tolist() == [0xffffffff, 7]
    assert P.earlier_marks(["a", "b"], {"b": [(0, 1)]}, 1, (3, 4)).tolist() == \
        [[[0] * 4] * 3, [[128, 128, 128, 0], [128, 128, 128, 0], [0] * 4]]


def test_read_selection(tmp_path):
    import json
    from mdil_ss_amd import ripu as P
    f = tmp_path / "selection.json"
    f.write_text(json.dumps({"select_radius": 3, "size": [16, 24], "picks": {"a": [[4, 6, 99, 49], [12, 18, 5, 40]]}}))
    assert P.read_selection(str(f), (16, 24)) == ({"a": [(4, 6), (12, 18)]}, 3)
    with pytest.raises(RuntimeError, match="selected on maps of"):
        P.read_selection(str(f), (8, 8))
    f.write_text("{}")
    with pytest.raises(RuntimeError, match="not a selection.json"):
        P.read_selection(str(f), (16, 24))


# ---------------------------------------------------------------------------------- command line
BASE = ["--state", "ckpt.pth.tar", "--num-classes", "20", "20", "--task", "1"]


def test_parser_defaults():
    from mdil_ss_amd import ripu as P
    a = P.build_parser().parse_args(BASE + ["--dataset", "BDD", "--budget", "0.05", "--json", "r.json"])
    assert (a.dataset, a.subset, a.synthetic, a.images, a.json, a.out, a.out_root, a.layout) == \
        ("BDD", "train", 0, None, "r.json", None, None, None)
    assert (a.budget, a.radius, a.select_radius, a.kind, a.by, a.seed, a.max_picks, a.previous, a.previous_root, a.fill_root) == \
        (0.05, 16, None, "entropy", "ripu", 0, 4096, None, None, None)
    assert (a.height, a.width, a.batch_size) == (512, 1024, 6)
    b = P.build_parser().parse_args(BASE + ["--synthetic", "2", "--budget", "0.0001", "--radius", "1", "--select-radius", "0",
                                            "--kind", "margin", "--by", "oracle", "--max-picks", "9", "--previous", "s.json",
                                            "--previous-root", "r0", "--fill-root", "p", "--out-root", "r1", "--layout", "BDD",
                                            "--out", "o", "--seed", "4"])
    assert (b.radius, b.select_radius, b.kind, b.by, b.max_picks, b.previous, b.previous_root, b.fill_root, b.out_root, b.layout,
            b.out, b.seed) == (1, 0, "margin", "oracle", 9, "s.json", "r0", "p", "r1", "BDD", "o", 4)
    assert callable(P.main)


@pytest.mark.parametrize("argv, text", [
    (["--budget", "0.1", "--json", "r"], "give one source"),
    (["--dataset", "BDD", "--synthetic", "2", "--budget", "0.1", "--json", "r"], "give one source"),
    (["--dataset", "BDD", "--json", "r"], "--budget"),
    (["--dataset", "BDD", "--budget", "0.1"], "nothing to do"),
    (["--dataset", "BDD", "--budget", "0", "--json", "r"], "--budget 0"),
    (["--dataset", "BDD", "--budget", "1.5", "--json", "r"], "--budget 1.5"),
    (["--dataset", "BDD", "--budget", "0.1", "--json", "r", "--radius", "0"], "radius 0 outside \\[1, 32\\]"),
    (["--dataset", "BDD", "--budget", "0.1", "--json", "r", "--radius", "33"], "radius 33 outside"),
    (["--dataset", "BDD", "--budget", "0.1", "--json", "r", "--select-radius", "-1"], "radius -1 outside \\[0, 32\\]"),
    (["--dataset", "BDD", "--budget", "0.1", "--json", "r", "--max-picks", "0"], "--max-picks 0"),
    (["--dataset", "BDD", "--budget", "0.1", "--json", "r", "--max-picks", "65537"], "--max-picks 65537"),
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
    (["--dataset", "BDD", "--budget", "0.1", "--json", "r", "--height", "8192", "--width", "4096"], "2\\^24 pixels per image"),
])
def test_parser_refusals(argv, text, capsys):
    from mdil_ss_amd import ripu as P
    with pytest.raises(SystemExit):
        P.build_parser().parse_args(BASE + argv)
    assert re.search(text, capsys.readouterr().err)


def test_main_refuses_before_it_opens_anything():
    """The checkpoint does not exist: every refusal below comes before it would be opened."""
    from mdil_ss_amd import ripu as P
    args = P.build_parser().parse_args(BASE + ["--dataset", "BDD", "--budget", "0.1", "--json", "r.json"])
    args.json = None
    with pytest.raises(RuntimeError, match="nothing to do"):
        P.main(args)
    args.json, args.task = "r.json", 2
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
    from mdil_ss_amd import ripu as P
    texts = [P.__doc__] + [open(os.path.join(REPO, f)).read() for f in ("README.md", "DESIGN.md")]
    for text in texts:
        flat = " ".join(text.split()).lower()
        assert "randomly initialised network" in flat
        assert "untuned" in flat
        assert "no retraining" in flat
        assert "which criterion" in flat
        assert "per image" in flat
    for f in ("README.md", "DESIGN.md"):
        flat = " ".join(open(os.path.join(REPO, f)).read().split())
        assert "mdil_ss_amd.ripu" in flat and "sliding (2k+1)" in flat and "not built" in flat
    assert "ripu_bench.json" in open(os.path.join(REPO, "profiles", "README.md")).read()


def test_training_build_id_is_untouched():
    """tests/test_miou_parity.py counts only the recorded mIoU runs that carry the id of the build
    under test and needs 32 of them: the add-on must leave that id where the recorded runs have it."""
    from mdil_ss_amd import ripu  # noqa: F401
    from tests import helpers
    tags = [str(t) for t in np.load(os.path.join(REPO, "tests", "golden", "miou_run.npz"),
                                    allow_pickle=False)["hip_build"]]
    build = helpers.kernel_build_id()
    assert tags.count(build) >= 32, f"build id {build} is carried by {tags.count(build)} recorded runs"
