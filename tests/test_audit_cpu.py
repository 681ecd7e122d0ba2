"""CPU: the label-audit add-on (include/mdil_audit.h, mdil_ss_amd/audit.py) -- the reference of
tests/audit_reference.py against hand-worked examples, the package's host arithmetic against that
reference, the library's exports and argument counts against the header, every argument check before
any launch, the command line's defaults and refusals, and the exclusion conditions of the GPU suite on
the reference alone."""
import os
import re

import numpy as np
import pytest
import torch

from tests import audit_reference as R
from tests import head_cases as HC
from tests.helpers import declared_names, dynamic_exports

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mdil_audit_apply", "mdil_audit_head", "mdil_audit_last_error", "mdil_audit_version"]
K = 17
BIG = (3, 16, 48)
SCALE = 8.0


# ------------------------------------------------------------------------------------ by hand
def test_q_and_thresholds_by_hand():
    from mdil_ss_amd import audit as A
    p = torch.tensor([0.0, 2.0 ** -17, 2.0 ** -16, 0.5, 1.0 - 2.0 ** -17, 1.0])
    assert R.q_of(p).tolist() == [0, 0, 1, 32768, 65535, 65535]
    count, qsum = torch.tensor([0, 1, 4, 3, 2]), torch.tensor([0, 40000, 8, 10, 2 * 65535])
    want = [65536, 40000, 2, 4, 65535]              # no pixel; one pixel; a sum the count divides; rounded up; the top
    assert R.thresholds(count, qsum) == want and A.thresholds(count, qsum) == want
    with pytest.raises(RuntimeError, match="not the counters of one sweep"):
        A.thresholds(torch.tensor([1]), torch.tensor([65536]))
    with pytest.raises(RuntimeError, match="host int64"):
        A.thresholds(torch.tensor([1.0]), torch.tensor([1]))
    assert [A.max_q_of(v) for v in (0.0, 0.5, 1.0)] == [0, 32768, 65535]


def test_suggest_joint_and_per_image_by_hand():
    # two images of 1 x 3 pixels, 3 classes
    logits = torch.tensor([[[[2.0, 0.0, 1.0]], [[1.0, 0.0, 1.0]], [[0.0, 0.0, 3.0]]],
                           [[[0.0, 5.0, 0.0]], [[0.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]]]])       # [2,3,1,3]
    q = torch.tensor([[[[40000, 100, 7000]], [[20000, 100, 7000]], [[5000, 100, 50000]]],
                      [[[100, 60000, 100]], [[100, 100, 100]], [[100, 100, 100]]]])
    thr = [30000, 200, 7000]
    # image 0: pixel 0 -> {0}: 0; pixel 1 -> nobody; pixel 2 -> {2} (class 0's 7000 < 30000): 2
    # image 1: pixel 0 -> nobody; pixel 1 -> {0}: 0; pixel 2 -> nobody
    s = R.suggest_from(q, thr, logits)
    assert s.tolist() == [[[0, 3, 2]], [[3, 0, 3]]]
    # ties go to the lowest confident class
    assert R.suggest_from(q, [0, 0, 0], logits).tolist() == [[[0, 0, 2]], [[0, 0, 0]]]
    assert R.suggest_from(q, [65536, 0, 0], logits).tolist() == [[[1, 1, 2]], [[1, 1, 1]]]
    target = torch.tensor([[[0, 1, 0]], [[9, 2, 255]]], dtype=torch.uint8)
    joint = R.joint_of(target, s, 3, 255)
    assert joint.tolist() == [[1, 0, 1, 0], [0, 0, 0, 1], [1, 0, 0, 0]]
    assert R.per_image_of(target, s, 3, 255).tolist() == [[[2, 1], [1, 0], [0, 0]], [[0, 0], [0, 0], [1, 1]]]
    assert R.issues_of(target, s, 3, 255).tolist() == [[[False, False, True]], [[False, True, False]]]
    sq = R.self_q(q, target, 3, 255)
    assert sq.tolist() == [[[40000, 100, 7000]], [[0, 100, 0]]]
    count, qsum = R.count_qsum(sq, target, 3, 255)
    assert count.tolist() == [2, 1, 1] and qsum.tolist() == [47000, 100, 100]


def test_calibrated_joint_by_hand():
    """Three classes.  C = [[8,2,0],[1,9,0],[0,0,0]] (+ a "none" column), counts 20, 10, 5: the rows scale to
    [16,4,0], [1,9,0], [0,0,0], 30 pixels in all, so Q = [[16,4,0],[1,9,0],[0,0,0]] / 30."""
    from fractions import Fraction as F
    from mdil_ss_amd import audit as A
    joint, count = torch.tensor([[8, 2, 0, 1], [1, 9, 0, 0], [0, 0, 0, 3]]), torch.tensor([20, 10, 5])
    Q, given, missed, issues = R.calibrated(joint, count)
    assert Q == [[F(16, 30), F(4, 30), 0], [F(1, 30), F(9, 30), 0], [0, 0, 0]]
    assert given == [F(1, 5), F(1, 10), 0] and missed == [F(1, 17), F(4, 13), 0] and issues == 5
    rep = A.confident_joint_report(joint, count, top=5)
    assert np.allclose(rep["calibrated_joint"], [[float(v) for v in r] for r in Q], rtol=0, atol=1e-15)
    assert np.allclose(rep["noise_given"], [float(v) for v in given], rtol=0, atol=1e-15)
    assert np.allclose(rep["noise_missed"], [float(v) for v in missed], rtol=0, atol=1e-15)
    assert abs(rep["estimated_issues"] - 5.0) < 1e-12 and rep["confident_issues"] == 3
    assert rep["no_confident_class"] == [1, 0, 3]
    assert [(p["given"], p["suggested"], p["confident_pixels"]) for p in rep["top_pairs"]] == [(0, 1, 2), (1, 0, 1)]
    assert len(A.confident_joint_report(joint, count, top=1)["top_pairs"]) == 1
    with pytest.raises(RuntimeError, match="expects joint"):
        A.confident_joint_report(joint[:, :3], count)


def test_calibrated_joint_on_a_seeded_matrix():
    from mdil_ss_amd import audit as A
    g = torch.Generator().manual_seed(5)
    nc = 20
    joint = torch.randint(0, 1000, (nc, nc + 1), generator=g)
    joint[7] = 0
    count = joint.sum(1) + torch.randint(0, 50, (nc,), generator=g)
    Q, given, missed, issues = R.calibrated(joint, count)
    rep = A.confident_joint_report(joint, count)
    assert np.allclose(rep["calibrated_joint"], [[float(v) for v in r] for r in Q], rtol=1e-13, atol=0)
    assert np.allclose(rep["noise_given"], [float(v) for v in given], rtol=1e-12, atol=1e-15)
    assert np.allclose(rep["noise_missed"], [float(v) for v in missed], rtol=1e-12, atol=1e-15)
    assert abs(rep["estimated_issues"] - float(issues)) <= 1e-9 * float(issues)
    assert rep["noise_given"][7] == 0.0 and len(rep["top_pairs"]) == 20
    joints = [p["joint"] for p in rep["top_pairs"]]
    assert joints == sorted(joints, reverse=True)


def test_apply_rule_by_hand():
    target = torch.tensor([0, 0, 1, 1, 2, 9, 255, 2], dtype=torch.uint8)
    suggest = torch.tensor([0, 1, 0, 254, 1, 0, 0, 7], dtype=torch.uint8)
    selfq = torch.tensor([9, 100, 300, 5, 65535, 1, 1, 1])
    r = R.apply_ref(target, suggest, selfq, 3, 255, 254, "prune", [100, 200, 65535], 250)
    #        pixel: 0 agrees; 1 issue 100 <= 100; 2 issue 300 > 200; 3 none; 4 issue; 5 bad; 6 ignored; 7 suggest >= nc
    assert r["out"].tolist() == [0, 250, 1, 1, 250, 9, 255, 2]
    assert r["mask"].tolist() == [0, 255, 128, 0, 255, 0, 0, 0]
    assert r["seen"].tolist() == [2, 2, 2] and r["bad_targets"] == 1
    assert r["acted"].tolist() == [[0, 1, 0], [0, 0, 0], [0, 1, 0]]
    r = R.apply_ref(target, suggest, selfq, 3, 255, 254, "relabel", [-1, 65535, 65535], 250)
    assert r["out"].tolist() == [0, 0, 0, 1, 1, 9, 255, 2] and r["mask"].tolist() == [0, 128, 255, 0, 255, 0, 0, 0]


def test_top_images_by_hand():
    from mdil_ss_amd import audit as A
    per_image = torch.tensor([[[10, 1], [10, 0]], [[0, 0], [4, 2]], [[0, 0], [0, 0]], [[5, 5], [5, 0]]])
    top = A.top_images(per_image, ["a", "b", "c", "d"], 3)
    assert [t["image"] for t in top] == ["b", "d", "a"]
    assert top[0]["issues"] == 2 and top[0]["labelled"] == 4 and top[0]["issues_per_class"] == [0, 2]
    assert A.top_images(per_image, ["a", "b", "c", "d"], 0) == []


# -------------------------------------------------------------------------------------- library
def header():
    text = open(os.path.join(REPO, "include", "mdil_audit.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_library_exports_exactly_the_declared_symbols():
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _audit_lib
    lib = _audit_lib.load()
    assert declared_names("mdil_audit.h") == NAMES
    for n in NAMES:
        assert hasattr(lib, n), f"{n} declared in include/mdil_audit.h but not exported"
    assert sorted(_audit_lib.EXPORTS) == NAMES
    assert dynamic_exports(_audit_lib.LIB_PATH) == NAMES
    assert lib.mdil_audit_version() >= 100


def test_header_export_map_and_binding_name_the_same_entry_points():
    from mdil_ss_amd import _audit_lib
    hdr = header()
    declared = {}
    for name, params in re.findall(r"\b(mdil_audit_\w+)\s*\(([^)]*)\)\s*;", hdr):
        params = params.strip()
        declared[name] = 0 if params == "void" else params.count(",") + 1
    mapped = re.findall(r"^\s*(mdil_audit_\w+);", open(os.path.join(REPO, "mdil_ss_amd", "ext", "audit_exports.map")).read(),
                        flags=re.M)
    assert sorted(declared) == sorted(mapped) == sorted(_audit_lib._SIGNATURES) == NAMES
    for name, (_, argtypes) in _audit_lib._SIGNATURES.items():
        assert declared[name] == len(argtypes), (name, declared[name], len(argtypes))
    assert (declared["mdil_audit_head"], declared["mdil_audit_apply"]) == (21, 16)
    macros = {k: int(v) for k, v in re.findall(r"#define\s+MDIL_AUDIT_(\w+)\s+\(?(-?\d+)\)?", hdr)}
    assert (macros["MIN_CLASSES"], macros["MAX_CLASSES"]) == (_audit_lib.MIN_CLASSES, _audit_lib.MAX_CLASSES) == (2, 32)
    assert (macros["OK"], macros["ERR_INVALID"], macros["ERR_LAUNCH"], macros["Q_ONE"]) == (0, -1, -2, 65536)
    assert (macros["PRUNE"], macros["RELABEL"]) == (0, 1)


def test_build_checks_the_binding():
    assert "_audit_lib" in open(os.path.join(REPO, "__graft_entry__.py")).read()


HEAD_OK = dict(x=4096, w=8192, b=12288, N=1, H=4, W=4, nc=20, tgt=16384, ign=19, thr=20480, qc=20, none=255,
               qmap=24576, sug=28672, count=32768, qsum=36864, joint=40960, pi=45056, badt=49152, nonf=53248)
APPLY_OK = dict(tgt=4096, sug=8192, sq=12288, npix=64, nc=20, ign=19, none=255, mode=0, maxq=16384, drop=255,
                out=20480, mask=24576, seen=28672, acted=32768, badt=36864)


def _head(lib, **kw):
    a = dict(HEAD_OK, **kw)
    return lib.mdil_audit_head(a["x"], a["w"], a["b"], a["N"], a["H"], a["W"], a["nc"], a["tgt"], a["ign"], a["thr"],
                               a["qc"], a["none"], a["qmap"], a["sug"], a["count"], a["qsum"], a["joint"], a["pi"],
                               a["badt"], a["nonf"], None)


def _apply(lib, **kw):
    a = dict(APPLY_OK, **kw)
    return lib.mdil_audit_apply(a["tgt"], a["sug"], a["sq"], a["npix"], a["nc"], a["ign"], a["none"], a["mode"], a["maxq"],
                                a["drop"], a["out"], a["mask"], a["seen"], a["acted"], a["badt"], None)


NO_COUNTERS = dict(count=None, qsum=None, joint=None, pi=None, badt=None)


@pytest.mark.parametrize("call, bad, text", [
    (_head, dict(nc=1), b"nc=1"), (_head, dict(nc=33), b"nc=33"),
    (_head, dict(x=None), b"bad argument"), (_head, dict(w=None), b"bad argument"), (_head, dict(b=None), b"bad argument"),
    (_head, dict(N=0), b"bad argument"), (_head, dict(H=-1), b"bad argument"), (_head, dict(W=0), b"bad argument"),
    (_head, dict(qmap=None, sug=None, nonf=None, **NO_COUNTERS), b"nothing to write"),
    (_head, dict(ign=-2), b"ignore_index=-2"), (_head, dict(ign=256), b"ignore_index=256"),
    (_head, dict(none=-1), b"none_id=-1"), (_head, dict(none=256), b"none_id=256"),
    (_head, dict(tgt=None), b"need a target"), (_head, dict(tgt=None, qc=3, joint=None, pi=None, qsum=None, badt=None), b"need a target"),
    (_head, dict(tgt=None, qc=3, count=None, pi=None, qsum=None, badt=None), b"need a target"),
    (_head, dict(tgt=None, qc=3, count=None, joint=None, qsum=None, pi=None), b"need a target"),
    (_head, dict(tgt=None, **NO_COUNTERS), b"q_class=20"),
    (_head, dict(thr=None), b"need thr"), (_head, dict(thr=None, sug=None, pi=None), b"need thr"),
    (_head, dict(thr=None, sug=None, joint=None), b"need thr"), (_head, dict(thr=None, joint=None, pi=None), b"need thr"),
    (_head, dict(qc=-1), b"q_class=-1"), (_head, dict(qc=21), b"q_class=21"),
    (_head, dict(x=4100), b"alignment"), (_head, dict(w=8194), b"alignment"), (_head, dict(b=12290), b"alignment"),
    (_head, dict(tgt=16385), b"alignment"), (_head, dict(thr=20482), b"alignment"), (_head, dict(qmap=24578), b"alignment"),
    (_head, dict(sug=28673), b"alignment"), (_head, dict(count=32772), b"alignment"), (_head, dict(qsum=36868), b"alignment"),
    (_head, dict(joint=40964), b"alignment"), (_head, dict(pi=45060), b"alignment"), (_head, dict(badt=49156), b"alignment"),
    (_head, dict(nonf=53252), b"alignment"),
    (_head, dict(W=1 << 30), b"too large"), (_head, dict(N=1 << 20, H=1 << 10, W=1 << 10), b"too large"),
    (_apply, dict(nc=1), b"nc=1"), (_apply, dict(nc=33), b"nc=33"),
    (_apply, dict(tgt=None), b"bad argument"), (_apply, dict(sug=None), b"bad argument"), (_apply, dict(sq=None), b"bad argument"),
    (_apply, dict(maxq=None), b"bad argument"), (_apply, dict(npix=0), b"bad argument"), (_apply, dict(npix=-4), b"bad argument"),
    (_apply, dict(npix=(1 << 40) + 1), b"too large"),
    (_apply, dict(ign=-2), b"ignore_index=-2"), (_apply, dict(none=256), b"none_id=256"), (_apply, dict(drop=-1), b"drop_id=-1"),
    (_apply, dict(mode=2), b"mode=2"), (_apply, dict(mode=-1), b"mode=-1"),
    (_apply, dict(out=None, mask=None, seen=None, acted=None, badt=None), b"nothing to write"),
    (_apply, dict(tgt=4100), b"alignment"), (_apply, dict(sug=8196), b"alignment"), (_apply, dict(sq=12296), b"alignment"),
    (_apply, dict(maxq=16386), b"alignment"), (_apply, dict(out=20484), b"alignment"), (_apply, dict(mask=24580), b"alignment"),
    (_apply, dict(seen=28676), b"alignment"), (_apply, dict(acted=32772), b"alignment"), (_apply, dict(badt=36868), b"alignment"),
])
def test_library_refuses_bad_arguments_without_a_device(call, bad, text):
    """Argument checks come before the launch, so fake pointers never reach a device."""
    from mdil_ss_amd import _audit_lib
    lib = _audit_lib.load()
    assert call(lib, **bad) == -1, bad
    assert text in lib.mdil_audit_last_error(), (bad, lib.mdil_audit_last_error())


# -------------------------------------------------------------------------------------- wrappers
def test_audit_refuses_cpu_tensors_and_bad_values():
    from mdil_ss_amd import audit as A
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    x, w, b = torch.zeros(1, 2, 2, 16), torch.zeros(16, 20, 2, 2), torch.zeros(20)
    with pytest.raises(RuntimeError, match="features must be a contiguous float32 device tensor.*no CPU fallback in "
                                           "the label-audit path"):
        A.audit_head(x, w, b, q_class=0)
    t, q = torch.zeros(8, dtype=torch.uint8), torch.zeros(8, dtype=torch.uint16)
    with pytest.raises(RuntimeError, match="target must be a contiguous uint8.*no CPU fallback in the label-audit path"):
        A.audit_apply(t, t, q, 20, [0] * 20)
    target = torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback in the label-audit path"):
        A.LabelAuditor(20).fit(x, w, b, target=target)
    with pytest.raises(RuntimeError, match="no CPU fallback in the label-audit path"):
        A.LabelAuditor(20).fit(Net([20], 1, 0), torch.zeros(1, 3, 32, 64), 0, target=target)
    with pytest.raises(RuntimeError, match="expects"):
        A.LabelAuditor(20).fit(x, w, target=target)
    with pytest.raises(RuntimeError, match="needs the batch's target"):
        A.LabelAuditor(20).fit(x, w, b)
    with pytest.raises(RuntimeError, match="thr must be 20 integers"):
        A.LabelAuditor(20).set_thresholds([0] * 19)
    for nc in (1, 33):
        with pytest.raises(RuntimeError, match=f"{nc} classes \\(supported: 2 to 32\\)"):
            A.audit_apply(t, t, q, nc, [0] * nc)
        with pytest.raises(RuntimeError, match=f"{nc} classes \\(supported: 2 to 32\\)"):
            A.LabelAuditor(nc)
    with pytest.raises(RuntimeError, match="mode 'drop'"):
        A.audit_apply(t, t, q, 20, [0] * 20, mode="drop")
    with pytest.raises(RuntimeError, match="none_id 256"):
        A.audit_apply(t, t, q, 20, [0] * 20, none_id=256)
    with pytest.raises(RuntimeError, match="ignore_index 300"):
        A.LabelAuditor(20, ignore_index=300)
    with pytest.raises(RuntimeError, match="thr must be 20 integers in \\[0, 65536\\]"):
        A.LabelAuditor(20).set_thresholds([65537] * 20)
    with pytest.raises(RuntimeError, match="fit\\(\\) has seen no batch"):
        A.LabelAuditor(20).thresholds()
    with pytest.raises(RuntimeError, match="audit\\(\\) has seen no batch"):
        A.LabelAuditor(20).counters()


def test_read_thresholds_refuses_other_files(tmp_path):
    import json
    from mdil_ss_amd import audit as A
    f = tmp_path / "t.json"
    f.write_text(json.dumps({"mode": "fit", "num_classes": 3, "thr": [1, 2, 65536]}))
    assert A.read_thresholds(str(f), 3) == [1, 2, 65536]
    with pytest.raises(RuntimeError, match="fitted on a head of 3 classes, this one has 20"):
        A.read_thresholds(str(f), 20)
    f.write_text(json.dumps({"mode": "score"}))
    with pytest.raises(RuntimeError, match="not a file written by --fit"):
        A.read_thresholds(str(f), 3)


# ---------------------------------------------------------------------------------- command line
BASE = ["--state", "ckpt.pth.tar", "--num-classes", "20", "20", "--task", "1"]


def test_parser_defaults():
    from mdil_ss_amd import audit as A
    a = A.build_parser().parse_args(BASE + ["--dataset", "BDD", "--json", "r.json"])
    assert (a.dataset, a.subset, a.synthetic, a.json, a.fit, a.thresholds, a.out, a.clean_root, a.layout) == \
        ("BDD", "val", 0, "r.json", None, None, None, None, None)
    assert (a.top, a.mode, a.max_self_confidence, a.height, a.width, a.batch_size) == (20, "prune", 1.0, 512, 1024, 6)
    assert all(hasattr(a, k) for k in ("cs_datadir", "bdd_datadir", "idd_datadir", "cache_resized"))
    b = A.build_parser().parse_args(BASE + ["--synthetic", "2", "--thresholds", "t.json", "--clean-root", "root", "--layout",
                                            "cityscapes", "--mode", "relabel", "--max-self-confidence", "0.25", "--top", "3",
                                            "--out", "o"])
    assert (b.synthetic, b.thresholds, b.clean_root, b.layout, b.mode, b.max_self_confidence, b.top, b.out) == \
        (2, "t.json", "root", "cityscapes", "relabel", 0.25, 3, "o")
    assert callable(A.main)


@pytest.mark.parametrize("argv, text", [
    (["--json", "r"], "give --dataset"),
    (["--dataset", "BDD", "--synthetic", "2", "--json", "r"], "exclude each other"),
    (["--dataset", "BDD"], "nothing to do"),
    (["--dataset", "BDD", "--fit", "t", "--thresholds", "u"], "give one"),
    (["--dataset", "BDD", "--json", "r", "--clean-root", "c"], "go together"),
    (["--dataset", "BDD", "--json", "r", "--layout", "BDD"], "go together"),
    (["--dataset", "IDD", "--clean-root", "c", "--layout", "BDD"], "does not take --dataset IDD"),
    (["--dataset", "BDD", "--clean-root", "c", "--layout", "IDD"], "invalid choice"),
    (["--dataset", "BDD", "--json", "r", "--mode", "drop"], "invalid choice"),
    (["--dataset", "BDD", "--json", "r", "--max-self-confidence", "1.5"], "--max-self-confidence"),
    (["--dataset", "BDD", "--json", "r", "--top", "-1"], "--top"),
    (["--dataset", "BDD", "--json", "r", "--batch-size", "0"], "must be positive"),
])
def test_parser_refusals(argv, text, capsys):
    from mdil_ss_amd import audit as A
    with pytest.raises(SystemExit):
        A.build_parser().parse_args(BASE + argv)
    assert re.search(text, capsys.readouterr().err)


def test_main_refuses_before_it_opens_anything():
    """The checkpoint does not exist: every refusal below comes before it would be opened."""
    from mdil_ss_amd import audit as A
    args = A.build_parser().parse_args(BASE + ["--dataset", "BDD", "--json", "r.json"])
    args.json = None
    with pytest.raises(RuntimeError, match="nothing to do"):
        A.main(args)
    args.json, args.task = "r.json", 2
    with pytest.raises(RuntimeError, match="--task 2: the model has tasks 0 to 1"):
        A.main(args)
    args.task, args.thresholds = 1, "no_such_file.json"
    with pytest.raises(RuntimeError, match="--thresholds no_such_file.json: no such file"):
        A.main(args)
    assert not os.path.exists("r.json")


def test_docstring_and_readme_carry_the_two_cautions():
    from mdil_ss_amd import audit as A
    readme = open(os.path.join(REPO, "README.md")).read()
    for text in (A.__doc__, readme):
        flat = " ".join(text.split()).lower()
        assert "out-of-sample" in flat and "class-weighted cross-entropy" in flat
        assert "randomly initialised network" in flat


def test_training_build_id_is_untouched():
    """tests/test_miou_parity.py counts only the recorded mIoU runs that carry the id of the build
    under test and needs 32 of them: the add-on must leave that id where the recorded runs have it."""
    from mdil_ss_amd import audit  # noqa: F401
    from tests import helpers
    tags = [str(t) for t in np.load(os.path.join(REPO, "tests", "golden", "miou_run.npz"),
                                    allow_pickle=False)["hip_build"]]
    build = helpers.kernel_build_id()
    assert tags.count(build) >= 32, f"build id {build} is carried by {tags.count(build)} recorded runs"


# ------------------------------------------------------- the exclusion conditions of the GPU suite
CASES = [(nc, shape, 1.0) for nc in HC.CLASSES for shape in HC.SHAPES] + [(nc, BIG, SCALE) for nc in HC.CLASSES]


def reference_case(nc, shape, scale):
    """The reference's own q, thresholds, confident sets and near-ties of one case."""
    x, w, b = HC.head_inputs(nc, shape)
    logits, S = HC.head64(x, w * scale if scale != 1.0 else w, b)
    q = R.q_of(R.probs64(logits))
    target = HC.make_target(nc, (shape[0], 2 * shape[1], 2 * shape[2]), 255, seed=nc + shape[1])
    count, qsum = R.count_qsum(R.self_q(q, target, nc, 255), target, nc, 255)
    thr = R.thresholds(count, qsum)
    inside = R.confident(q, thr)
    return logits, S, q, target, thr, inside, R.near_tie_confident(logits, S, inside, HC.gamma(K))


@pytest.mark.parametrize("nc, shape, scale", CASES)
def test_exclusions_of_the_gpu_suite_stay_under_the_cap(nc, shape, scale):
    logits, S, q, target, thr, inside, excluded = reference_case(nc, shape, scale)
    HC.count_cap(excluded, f"nc {nc} shape {shape} scale {scale}")
    # the case means something: thresholds inside the range, and issues to count.  (Over the suite the
    # confident sets come in every size: empty at nc 2, one class at nc 2 and with the weights times 8,
    # nearly all classes at random targets and many classes, where a threshold is about 1 / nc.)
    suggest = R.suggest_from(q, thr, logits)
    if target.numel() >= 1000:
        assert all(0 < t <= 65535 for t in thr)
        joint = R.joint_of(target, suggest, nc, 255)
        assert int(joint.sum()) == int(R.valid_of(target, nc, 255).sum())
        assert int(joint[:, :nc].sum() - joint[:, :nc].diagonal().sum()) > 0
