"""CPU: the open-set add-on (include/mdil_openset.h, mdil_ss_amd/openset.py) -- the 16-bit key and
its inverse, the report arithmetic against brute-force pairwise counting in exact Fractions, the
threshold and CDF table by hand, the library's exports and argument checks (every refusal before any
launch), the wrappers' and the command line's refusals, and the rule the add-on exists under: it
leaves the training path's build id alone."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import openset_reference as R
from tests.helpers import declared_names, dynamic_exports

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mdil_openset_apply", "mdil_openset_head", "mdil_openset_last_error", "mdil_openset_version"]
FLT_MAX = 3.4028234663852886e38
SPECIAL = [0.0, -0.0, float("inf"), float("-inf"), FLT_MAX, -FLT_MAX, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38,
           1.17549435e-38, -1.17549435e-38]


# ------------------------------------------------------------------------------------- the key
def test_key16_is_monotone_and_parameter_free():
    from mdil_ss_amd import openset as O
    g = torch.Generator().manual_seed(0)
    v = torch.cat([torch.randn(40000, generator=g) * 10.0 ** torch.randint(-30, 30, (40000,), generator=g).float(),
                   torch.randn(20000, generator=g), torch.tensor(SPECIAL)])
    v = v.sort()[0]
    code = O.key16(v)
    assert code.dtype == torch.int64 and bool((code[1:] >= code[:-1]).all())
    assert torch.equal(code, R.key16(v.numpy()))
    finite = torch.isfinite(v)
    assert int(code[finite].min()) >= 128 and int(code[finite].max()) <= 65407
    assert O.key16(torch.tensor([float("-inf"), float("inf")])).tolist() == [127, 65408]
    assert O.key16(torch.tensor([-FLT_MAX, FLT_MAX])).tolist() == [128, 65407] == list(O.FINITE_CODES)
    zeros = O.key16(torch.tensor([0.0, -0.0]))
    assert zeros.tolist() == [0x8000, 0x8000]
    assert O.key16(torch.tensor([-1e-45])).item() == 0x7fff


def test_code_floor_inverts_the_key():
    from mdil_ss_amd import openset as O
    c = torch.arange(128, 65408)
    floor = O.code_floor(c)
    assert floor.dtype == torch.float32 and torch.equal(O.key16(floor), c)
    assert bool((floor[1:] > floor[:-1]).all())
    # the floor is the SMALLEST float of its bin: the float just below it lies in the bin before
    below = torch.from_numpy(np.nextafter(floor[1:].numpy(), np.float32(-np.inf)))
    assert torch.equal(O.key16(below), c[1:] - 1)
    assert O.code_floor(0x8000) == 0.0 and isinstance(O.code_floor(0x8000), float)
    assert O.code_floor(65408) == float("inf")
    assert O.threshold_score(65536) is None and O.threshold_score(0) is None and O.threshold_score(128) == -FLT_MAX
    with pytest.raises(RuntimeError, match="codes lie in"):
        O.code_floor(65536)


# ------------------------------------------------------------------------------------ metrics
def _table(neg_codes, pos_codes):
    return torch.stack([torch.bincount(torch.as_tensor(neg_codes), minlength=65536),
                        torch.bincount(torch.as_tensor(pos_codes), minlength=65536)])


def _brute(neg, pos, tpr=0.95):
    """AUROC, AUPR, FPR at TPR and the tie mass by counting over pairs and thresholds."""
    import math
    neg, pos = np.asarray(neg), np.asarray(pos)
    N, P = len(neg), len(pos)
    auroc = R.pairwise_auroc(neg, pos)
    ties = Fraction(int(sum(int((neg == v).sum()) for v in pos)), P * N)
    aupr = Fraction(0)
    for v in np.unique(pos):
        tp, fp = int((pos >= v).sum()), int((neg >= v).sum())
        aupr += Fraction(int((pos == v).sum()), P) * Fraction(tp, tp + fp)
    need = math.ceil(Fraction(str(tpr)) * P)
    t = max(int(v) for v in np.unique(np.concatenate([neg, pos])) if int((pos >= v).sum()) >= need)
    return auroc, aupr, Fraction(int((neg >= t).sum()), N), t, ties


def _cases():
    from mdil_ss_amd import openset as O
    g = torch.Generator().manual_seed(1)
    spread_neg, spread_pos = torch.randn(2000, generator=g), torch.randn(1500, generator=g) + 0.7
    five = torch.tensor([0.1, 0.2, 0.3, 0.4, 0.5])
    few_neg = five[torch.randint(0, 5, (1800,), generator=g)]
    few_pos = five[torch.multinomial(torch.tensor([1., 1., 2., 4., 8.]), 900, True, generator=g)]
    return {"spread": (spread_neg, spread_pos), "five codes": (few_neg, few_pos),
            "disjoint above": (torch.rand(300, generator=g), torch.rand(200, generator=g) + 2.0),
            "disjoint below": (torch.rand(300, generator=g) + 2.0, torch.rand(200, generator=g)),
            "one code": (torch.full((700,), 0.25), torch.full((300,), 0.25))}, O


@pytest.mark.parametrize("name", ("spread", "five codes", "disjoint above", "disjoint below", "one code"))
def test_metrics_equal_brute_force_counting(name):
    cases, O = _cases()
    neg, pos = cases[name]
    cn, cp = O.key16(neg), O.key16(pos)
    table = _table(cn, cp)
    got = O.metrics(table)
    auroc, aupr, fpr, t, ties = _brute(cn.numpy(), cp.numpy())
    ref = R.metrics(table)
    assert (ref["auroc"], ref["aupr"], ref["fpr_at_tpr"], ref["threshold_code"], ref["tie_mass"]) == \
        (auroc, aupr, fpr, t, ties)                                  # the reference itself, against pairs
    assert got["auroc"] == float(auroc) and got["tie_mass"] == float(ties) and got["fpr_at_tpr"] == float(fpr)
    assert got["threshold_code"] == t and got["threshold_score"] == O.code_floor(t)
    assert (got["P"], got["N"]) == (len(pos), len(neg))
    # the step sum: every term and the last division are correctly rounded, the sum itself is exact (fsum)
    assert abs(got["aupr"] - float(aupr)) <= 4 * 2.0 ** -53
    # half the tie mass bounds what the 16 bits can do to the AUROC of the unquantised scores
    exact = R.pairwise_auroc(neg.numpy(), pos.numpy())
    assert abs(auroc - exact) <= ties / 2, (name, float(auroc), float(exact), float(ties))
    if name == "disjoint above":
        assert got["auroc"] == 1.0 and got["aupr"] == 1.0 and got["fpr_at_tpr"] == 0.0 and got["tie_mass"] == 0.0
    if name == "disjoint below":
        assert got["auroc"] == 0.0 and got["fpr_at_tpr"] == 1.0
    if name == "one code":
        assert got["auroc"] == 0.5 and got["tie_mass"] == 1.0 and got["fpr_at_tpr"] == 1.0 and got["aupr"] == 0.3
    for tpr in (0.5, 1.0):
        assert O.metrics(table, tpr)["fpr_at_tpr"] == float(_brute(cn.numpy(), cp.numpy(), tpr)[2])


def test_metrics_refuse_an_empty_group_and_other_tables():
    from mdil_ss_amd import openset as O
    table = _table([5, 6], [7])
    for g, name in ((0, "known"), (1, "unknown")):
        t = table.clone()
        t[g] = 0
        with pytest.raises(RuntimeError, match=f"the {name} group is empty"):
            O.metrics(t)
    with pytest.raises(RuntimeError, match=r"host int64 \[2,65536\]"):
        O.metrics(table.float())
    with pytest.raises(RuntimeError, match=r"host int64 \[2,65536\]"):
        O.metrics(table[0])
    with pytest.raises(RuntimeError, match="tpr 1.5"):
        O.metrics(table, 1.5)


def test_threshold_and_cdf_by_hand():
    from mdil_ss_amd import openset as O
    known = torch.zeros(65536, dtype=torch.int64)
    bins = [1000, 1001, 1002, 1003, 1004, 1005]
    known[bins] = torch.tensor([10, 20, 30, 25, 10, 5])               # N = 100; tails 100 90 70 40 15 5
    assert O.threshold_at_known_fpr(known, 0.05) == 1005
    assert O.threshold_at_known_fpr(known, 0.049) == 1006
    assert O.threshold_at_known_fpr(known, 0.15) == 1004
    assert O.threshold_at_known_fpr(known, 0.39) == 1004
    assert O.threshold_at_known_fpr(known, 0.4) == 1003
    assert O.threshold_at_known_fpr(known, 0.999) == 1001
    assert O.threshold_at_known_fpr(known, 1.0) == 0                  # everything may go
    assert O.threshold_at_known_fpr(known, 0.0) == 1006               # nothing known is rejected
    lut = O.cdf_lut(known)
    assert lut.dtype == torch.uint8 and tuple(lut.shape) == (65536,)
    assert lut[bins].tolist() == [25, 76, 153, 216, 242, 255]         # floor(255 * (10, 30, 60, 85, 95, 100) / 100)
    assert int(lut[999]) == 0 and int(lut[0]) == 0 and int(lut[1006]) == 255 and int(lut[65535]) == 255
    assert torch.equal(O.cdf_from_starts(O.cdf_starts(lut)), lut) and len(O.cdf_starts(lut)) == 256
    top = torch.zeros(65536, dtype=torch.int64)
    top[65535] = 3
    assert O.threshold_at_known_fpr(top, 0.0) == 65536 and O.threshold_at_known_fpr(top, 1.0) == 0
    for fn in (lambda: O.threshold_at_known_fpr(torch.zeros(65536, dtype=torch.int64), 0.1),
               lambda: O.cdf_lut(torch.zeros(65536, dtype=torch.int64))):
        with pytest.raises(RuntimeError, match="the known group is empty"):
            fn()
    with pytest.raises(RuntimeError, match="fpr -0.1"):
        O.threshold_at_known_fpr(known, -0.1)


def test_group_lut_and_kinds():
    from mdil_ss_amd import openset as O
    lut = O.group_lut([19, 200], [7])
    assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256,)
    assert (int(lut[19]), int(lut[200]), int(lut[7]), int(lut[0]), int(lut.sum())) == (1, 1, 2, 0, 4)
    with pytest.raises(RuntimeError, match="both unknown and ignored"):
        O.group_lut([3], [3])
    with pytest.raises(RuntimeError, match="ids lie in"):
        O.group_lut([256])
    assert O.kinds_mask(O.KINDS) == 15 and O.kinds_mask(["energy"]) == 4 and O.kinds_mask([0, "entropy"]) == 9
    assert O.KINDS == R.KINDS
    for bad in (["softmax"], [4], []):
        with pytest.raises(RuntimeError, match="score kind"):
            O.kinds_mask(bad)


def test_apply_rule_by_hand():
    label = torch.tensor([0, 0, 1, 1, 2, 5, 2], dtype=torch.uint8)
    code = torch.tensor([10, 20, 30, 40, 50, 60, 5])
    target = torch.tensor([0, 1, 9, 9, 2, 0, 7], dtype=torch.uint8)
    lut = torch.zeros(256, dtype=torch.uint8)
    lut[9], lut[7] = 1, 2
    cdf = (torch.arange(65536) % 256).to(torch.uint8)
    r = R.apply_rule(label, code, 3, 30, torch.tensor([7, 8, 9], dtype=torch.uint8), 255, cdf, target, lut)
    assert r["out"].tolist() == [7, 7, 255, 255, 255, 255, 9] and r["score"].tolist() == [10, 20, 30, 40, 50, 60, 5]
    assert r["seen"].tolist() == [2, 2, 2] and r["rejected"].tolist() == [0, 2, 1]
    assert r["detect"].tolist() == [[2, 1], [0, 2]]
    assert r["confusion"].tolist() == [[1, 0, 0], [1, 0, 0], [0, 0, 0]]
    assert (r["bad_targets"], r["bad_labels"]) == (0, 1)


# -------------------------------------------------------------------------------------- library
def test_library_exports_exactly_the_declared_symbols():
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _openset_lib
    lib = _openset_lib.load()
    assert declared_names("mdil_openset.h") == NAMES
    for n in NAMES:
        assert hasattr(lib, n), f"{n} declared in include/mdil_openset.h but not exported"
    assert sorted(_openset_lib.EXPORTS) == NAMES
    assert dynamic_exports(_openset_lib.LIB_PATH) == NAMES
    assert lib.mdil_openset_version() >= 100
    assert (_openset_lib.MIN_CLASSES, _openset_lib.MAX_CLASSES) == (2, 32)


HEAD_OK = dict(x=4096, w=8192, b=12288, N=1, H=4, W=4, nc=20, tgt=16384, lut=20480, cg=0, kinds=15, mk=2,
               label=24576, code=28672, hist=32768, nonf=36864)
APPLY_OK = dict(label=4096, code=8192, npix=64, nc=20, thr=40000, ids=12288, unk=255, cdf=16384, tgt=20480, lut=24576,
                out=28672, score=32768, seen=36864, rej=40960, det=45056, conf=49152, badt=53248, badl=57344)


def _head(lib, **kw):
    a = dict(HEAD_OK, **kw)
    return lib.mdil_openset_head(a["x"], a["w"], a["b"], a["N"], a["H"], a["W"], a["nc"], a["tgt"], a["lut"], a["cg"],
                                 a["kinds"], a["mk"], a["label"], a["code"], a["hist"], a["nonf"], None)


def _apply(lib, **kw):
    a = dict(APPLY_OK, **kw)
    return lib.mdil_openset_apply(a["label"], a["code"], a["npix"], a["nc"], a["thr"], a["ids"], a["unk"], a["cdf"],
                                  a["tgt"], a["lut"], a["out"], a["score"], a["seen"], a["rej"], a["det"], a["conf"],
                                  a["badt"], a["badl"], None)


@pytest.mark.parametrize("call, bad, text", [
    (_head, dict(nc=1), b"nc=1"), (_head, dict(nc=33), b"nc=33"),
    (_head, dict(x=None), b"bad argument"), (_head, dict(w=None), b"bad argument"), (_head, dict(b=None), b"bad argument"),
    (_head, dict(N=0), b"bad argument"), (_head, dict(H=-1), b"bad argument"), (_head, dict(W=0), b"bad argument"),
    (_head, dict(label=None, code=None, mk=-1, hist=None, nonf=None), b"nothing to write"),
    (_head, dict(kinds=0), b"kinds=0"), (_head, dict(kinds=16), b"kinds=16"),
    (_head, dict(mk=4), b"map_kind=4"), (_head, dict(mk=-2), b"map_kind=-2"),
    (_head, dict(mk=-1), b"map_kind=-1"), (_head, dict(code=None), b"map_kind=2"),
    (_head, dict(cg=3), b"const_group=3"), (_head, dict(cg=-1), b"const_group=-1"),
    (_head, dict(lut=None), b"a target needs its group_lut"),
    (_head, dict(x=4100), b"alignment"), (_head, dict(w=8194), b"alignment"), (_head, dict(b=12290), b"alignment"),
    (_head, dict(tgt=16385), b"alignment"), (_head, dict(label=24577), b"alignment"), (_head, dict(code=28674), b"alignment"),
    (_head, dict(hist=32772), b"alignment"), (_head, dict(nonf=36868), b"alignment"),
    (_head, dict(W=1 << 30), b"too large"), (_head, dict(N=1 << 20, H=1 << 10, W=1 << 10), b"too large"),
    (_apply, dict(nc=1), b"nc=1"), (_apply, dict(nc=33), b"nc=33"),
    (_apply, dict(label=None), b"bad argument"), (_apply, dict(code=None), b"bad argument"),
    (_apply, dict(npix=0), b"bad argument"), (_apply, dict(npix=-4), b"bad argument"),
    (_apply, dict(npix=(1 << 40) + 1), b"too large"),
    (_apply, dict(thr=-1), b"thr=-1"), (_apply, dict(thr=65537), b"thr=65537"),
    (_apply, dict(unk=-1), b"unknown_id=-1"), (_apply, dict(unk=256), b"unknown_id=256"),
    (_apply, dict(cdf=None), b"go together"), (_apply, dict(score=None), b"go together"),
    (_apply, dict(lut=None), b"a target needs"), (_apply, dict(det=None), b"a target needs"),
    (_apply, dict(conf=None), b"a target needs"), (_apply, dict(badt=None), b"a target needs"),
    (_apply, dict(tgt=None, out=None, score=None, cdf=None, seen=None, rej=None, det=None, conf=None, badt=None,
                  badl=None), b"nothing to write"),
    (_apply, dict(label=4100), b"alignment"), (_apply, dict(code=8200), b"alignment"), (_apply, dict(tgt=20484), b"alignment"),
    (_apply, dict(out=28676), b"alignment"), (_apply, dict(score=32772), b"alignment"), (_apply, dict(seen=36868), b"alignment"),
    (_apply, dict(rej=40964), b"alignment"), (_apply, dict(det=45060), b"alignment"), (_apply, dict(conf=49156), b"alignment"),
    (_apply, dict(badt=53252), b"alignment"), (_apply, dict(badl=57348), b"alignment"),
])
def test_library_refuses_bad_arguments_without_a_device(call, bad, text):
    """Argument checks come before the launch, so fake pointers never reach a device."""
    from mdil_ss_amd import _openset_lib
    lib = _openset_lib.load()
    assert call(lib, **bad) == -1, bad
    assert text in lib.mdil_openset_last_error(), (bad, lib.mdil_openset_last_error())


# -------------------------------------------------------------------------------------- wrappers
def test_openset_refuses_cpu_tensors():
    from mdil_ss_amd import openset as O
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    x, w, b = torch.zeros(1, 2, 2, 16), torch.zeros(16, 20, 2, 2), torch.zeros(20)
    with pytest.raises(RuntimeError, match="features must be a contiguous float32 device tensor.*no CPU fallback in "
                                           "the open-set path"):
        O.openset_head(x, w, b)
    label, code = torch.zeros(8, dtype=torch.uint8), torch.zeros(8, dtype=torch.uint16)
    with pytest.raises(RuntimeError, match="label must be a contiguous uint8.*no CPU fallback in the open-set path"):
        O.openset_apply(label, code, 20, 100)
    with pytest.raises(RuntimeError, match="no CPU fallback in the open-set path"):
        O.OpenSetMeter(20).add(x, w, b)
    with pytest.raises(RuntimeError, match="no CPU fallback in the open-set path"):
        O.OpenSetMeter(20).add(Net([20], 1, 0), torch.zeros(1, 3, 32, 64), 0)
    with pytest.raises(RuntimeError, match="expects"):
        O.OpenSetMeter(20).add(x, w)


def test_wrappers_refuse_classes_thresholds_and_ids():
    from mdil_ss_amd import openset as O
    label, code = torch.zeros(8, dtype=torch.uint8), torch.zeros(8, dtype=torch.uint16)
    for nc in (1, 33):
        with pytest.raises(RuntimeError, match=f"{nc} classes \\(supported: 2 to 32\\)"):
            O.openset_apply(label, code, nc, 0)
        with pytest.raises(RuntimeError, match=f"{nc} classes \\(supported: 2 to 32\\)"):
            O.OpenSetMeter(nc)
    for thr in (-1, 65537, "abc", None):
        with pytest.raises(RuntimeError, match="thr must be an integer in \\[0, 65536\\]"):
            O.openset_apply(label, code, 20, thr)
    with pytest.raises(RuntimeError, match="unknown_id 256"):
        O.openset_apply(label, code, 20, 0, unknown_id=256)
    with pytest.raises(RuntimeError, match="const_group 3"):
        O.OpenSetMeter(20, const_group=3)
    with pytest.raises(RuntimeError, match="score kind"):
        O.OpenSetMeter(20, ["margin"])
    with pytest.raises(RuntimeError, match="lut must be"):
        O.OpenSetMeter(20, lut=torch.zeros(255, dtype=torch.uint8))
    empty = O.OpenSetMeter(20, ["energy", "msp"])
    assert empty.kinds == ("msp", "energy") and empty.nonfinite() == 0 and int(empty.hist().sum()) == 0
    with pytest.raises(RuntimeError, match="group is empty"):
        empty.report()


# ---------------------------------------------------------------------------------- command line
BASE = ["--state", "ckpt.pth.tar", "--num-classes", "20", "20", "27", "--task", "0"]


def test_parser_defaults():
    from mdil_ss_amd import openset as O
    a = O.build_parser().parse_args(BASE + ["--dataset", "IDD", "--score", "--json", "r.json"])
    assert (a.dataset, a.subset, a.synthetic, a.score, a.json, a.fit, a.images, a.out, a.threshold) == \
        ("IDD", "val", 0, True, "r.json", None, None, None, None)
    assert (a.unknown_ids, a.ignore_ids, a.kinds, a.tpr, a.known_fpr, a.kind, a.unknown_id, a.colour) == \
        ([], [], ["msp", "maxlogit", "energy", "entropy"], 0.95, 0.05, "energy", 255, False)
    assert (a.data_task, a.foreign_dataset, a.foreign_task, a.foreign_synthetic, a.height, a.width, a.batch_size) == \
        (None, None, None, 0, 512, 1024, 6)
    assert all(hasattr(a, k) for k in ("cs_datadir", "bdd_datadir", "idd_datadir", "cache_resized"))
    b = O.build_parser().parse_args(BASE + ["--dataset", "IDD", "--data-task", "2", "--unknown-ids", "18", "25",
                                            "--ignore-ids", "26", "--kinds", "energy", "msp", "--tpr", "0.9", "--score",
                                            "--json", "r.json"])
    assert (b.data_task, b.unknown_ids, b.ignore_ids, b.kinds, b.tpr) == (2, [18, 25], [26], ["energy", "msp"], 0.9)
    c = O.build_parser().parse_args(BASE + ["--dataset", "cityscapes", "--foreign-dataset", "BDD", "--foreign-task", "1",
                                            "--score", "--json", "r.json"])
    assert (c.foreign_dataset, c.foreign_task) == ("BDD", 1)
    d = O.build_parser().parse_args(BASE + ["--dataset", "cityscapes", "--fit", "t.json", "--known-fpr", "0.01"])
    assert (d.fit, d.known_fpr) == ("t.json", 0.01)
    e = O.build_parser().parse_args(BASE + ["--images", "pics", "--threshold", "t.json", "--kind", "msp", "--out", "o",
                                            "--unknown-id", "254", "--colour"])
    assert (e.images, e.threshold, e.kind, e.out, e.unknown_id, e.colour) == ("pics", "t.json", "msp", "o", 254, True)
    assert callable(O.main)


@pytest.mark.parametrize("argv, text", [
    (["--dataset", "BDD"], "give one of --score"),
    (["--dataset", "BDD", "--score", "--json", "r", "--fit", "t"], "give one of --score"),
    (["--dataset", "BDD", "--score"], "--score writes its report to --json"),
    (["--score", "--json", "r"], "give --dataset"),
    (["--dataset", "BDD", "--synthetic", "2", "--score", "--json", "r"], "give --dataset"),
    (["--images", "p", "--score", "--json", "r"], "--images DIR has no labels"),
    (["--images", "p", "--out", "o"], "--out DIR needs --threshold"),
    (["--dataset", "BDD", "--fit", "t", "--threshold", "x"], "--threshold FILE goes with --out"),
    (["--dataset", "BDD", "--threshold", "t", "--out", "o"], "one source of images"),
    (["--threshold", "t", "--out", "o"], "one source of images"),
    (["--images", "p", "--threshold", "t", "--out", "o", "--kind", "margin"], "--kind margin"),
    (["--images", "p", "--threshold", "t", "--out", "o", "--unknown-id", "256"], "--unknown-id 256"),
    (["--dataset", "BDD", "--fit", "t", "--foreign-dataset", "IDD"], "--foreign-dataset goes with --score"),
    (["--dataset", "BDD", "--score", "--json", "r", "--foreign-dataset", "IDD", "--foreign-synthetic", "2"], "exclude each other"),
    (["--dataset", "BDD", "--score", "--json", "r", "--foreign-dataset", "IDD", "--unknown-ids", "3"], "does not go with it"),
    (["--dataset", "BDD", "--score", "--json", "r", "--tpr", "0"], "--tpr"),
    (["--dataset", "BDD", "--score", "--json", "r", "--tpr", "1.5"], "--tpr"),
    (["--dataset", "BDD", "--fit", "t", "--known-fpr", "1.5"], "--known-fpr"),
    (["--dataset", "BDD", "--fit", "t", "--batch-size", "0"], "must be positive"),
    (["--dataset", "BDD", "--score", "--json", "r", "--unknown-ids", "3", "--ignore-ids", "3"], "share an id"),
])
def test_parser_refusals(argv, text, capsys):
    from mdil_ss_amd import openset as O
    with pytest.raises(SystemExit):
        O.build_parser().parse_args(BASE + argv)
    assert re.search(text, capsys.readouterr().err)


def test_main_refuses_before_it_opens_anything():
    """The checkpoint does not exist: every refusal below comes before it would be opened."""
    from mdil_ss_amd import openset as O
    args = O.build_parser().parse_args(BASE + ["--dataset", "BDD", "--score", "--json", "r.json"])
    args.json = None
    with pytest.raises(RuntimeError, match="--score writes its report"):
        O.main(args)
    args.json, args.task = "r.json", 3
    with pytest.raises(RuntimeError, match="--task 3: the model has tasks 0 to 2"):
        O.main(args)
    args.task, args.data_task = 0, 5
    with pytest.raises(RuntimeError, match="--data-task 5: the model has tasks 0 to 2"):
        O.main(args)
    args.data_task, args.unknown_ids = 2, [27]
    with pytest.raises(RuntimeError, match=r"--unknown-ids \[27\]: task 2's labels lie in \[0, 27\)"):
        O.main(args)
    args.unknown_ids, args.data_task, args.dataset, args.synthetic, args.foreign_synthetic = [], None, None, 2, 2
    with pytest.raises(RuntimeError, match="the same images"):
        O.main(args)
    maps = O.build_parser().parse_args(BASE + ["--images", "p", "--threshold", "no_such_file.json", "--out", "o"])
    with pytest.raises(RuntimeError, match="--threshold no_such_file.json: no such file"):
        O.main(maps)
    assert not os.path.exists("o")


def test_training_build_id_is_untouched():
    """tests/test_miou_parity.py counts only the recorded mIoU runs that carry the id of the build
    under test and needs 32 of them: the add-on must leave that id where the recorded runs have it."""
    from mdil_ss_amd import openset  # noqa: F401
    from tests import helpers
    tags = [str(t) for t in np.load(os.path.join(REPO, "tests", "golden", "miou_run.npz"),
                                    allow_pickle=False)["hip_build"]]
    build = helpers.kernel_build_id()
    assert tags.count(build) >= 32, f"build id {build} is carried by {tags.count(build)} recorded runs"
