"""CPU: the drift add-on (include/mdil_drift.h, mdil_ss_amd/drift.py) -- the library exports exactly
what its header declares, every argument check answers before any launch, the command line's
defaults and refusals, the refusal of host tensors, and ``drift_report`` on a three-class example
whose every output is worked out by hand below."""
import pytest
import torch

from tests.helpers import declared_names, dynamic_exports

NAMES = ["mdil_drift_head", "mdil_drift_last_error", "mdil_drift_version", "mdil_drift_workspace_bytes"]


def test_library_exports_exactly_the_declared_symbols():
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _drift_lib
    lib = _drift_lib.load()
    assert declared_names("mdil_drift.h") == NAMES
    for n in NAMES:
        assert hasattr(lib, n), f"{n} declared in include/mdil_drift.h but not exported"
    assert sorted(_drift_lib.EXPORTS) == NAMES
    assert dynamic_exports(_drift_lib.LIB_PATH) == NAMES
    assert lib.mdil_drift_version() >= 100
    assert (_drift_lib.MIN_CLASSES, _drift_lib.MAX_CLASSES) == (2, 32)


def test_workspace_bytes_is_one_row_per_work_group():
    """ceil(N H W / 256) work-groups, at most 2048, of nc + 1 doubles each."""
    from mdil_ss_amd import _drift_lib
    lib = _drift_lib.load()
    assert lib.mdil_drift_workspace_bytes(1, 1, 1, 2) == 1 * 3 * 8
    assert lib.mdil_drift_workspace_bytes(2, 12, 20, 20) == 2 * 21 * 8
    assert lib.mdil_drift_workspace_bytes(6, 256, 512, 27) == 2048 * 28 * 8
    assert lib.mdil_drift_workspace_bytes(1, 513, 1023, 32) == 2048 * 33 * 8
    for bad in ((0, 1, 1, 20), (1, 1, 1, 1), (1, 1, 1, 33), (1, -1, 1, 20)):
        assert lib.mdil_drift_workspace_bytes(*bad) == -1


OK = dict(xa=4096, wa=8192, ba=12288, xb=16384, wb=20480, bb=24576, N=1, H=2, W=2, nc=20, tgt=28672, ign=19,
          la=32768, lb=36864, kl=40960, ch=45056, tr=49152, ca=53248, cb=57344, oc=61440, bad=65536, sums=69632,
          ws=73728, wsb=21 * 8)


def _call(lib, **kw):
    a = dict(OK, **kw)
    return lib.mdil_drift_head(a["xa"], a["wa"], a["ba"], a["xb"], a["wb"], a["bb"], a["N"], a["H"], a["W"], a["nc"],
                               a["tgt"], a["ign"], a["la"], a["lb"], a["kl"], a["ch"], a["tr"], a["ca"], a["cb"],
                               a["oc"], a["bad"], a["sums"], a["ws"], a["wsb"], None)


@pytest.mark.parametrize("bad, text", [
    (dict(nc=1), b"nc=1"), (dict(nc=33), b"nc=33"),
    (dict(xa=None), b"bad argument"), (dict(xb=None), b"bad argument"), (dict(wa=None), b"bad argument"),
    (dict(bb=None), b"bad argument"), (dict(N=0), b"bad argument"), (dict(W=0), b"bad argument"),
    (dict(H=1 << 30, W=1 << 29), b"too large"),
    (dict(xa=4100), b"alignment"), (dict(xb=16392), b"alignment"), (dict(tgt=28673), b"alignment"),
    (dict(la=32769), b"alignment"), (dict(ch=45057), b"alignment"), (dict(kl=40964), b"alignment"),
    (dict(tr=49156), b"alignment"), (dict(sums=69636), b"alignment"), (dict(ws=73732), b"alignment"),
    (dict(tgt=None), b"need a target"),                                   # confusion_a (and the others) given
    (dict(tgt=None, ca=None, cb=None), b"need a target"),                 # outcome alone
    (dict(ws=None), b"sums need a workspace of 168 bytes"), (dict(wsb=167), b"sums need a workspace of 168 bytes"),
    (dict(ign=256), b"ignore_index=256"), (dict(ign=-2), b"ignore_index=-2"),
])
def test_library_refuses_bad_arguments_without_a_device(bad, text):
    """Argument checks come before the launch, so fake pointers never reach a device."""
    from mdil_ss_amd import _drift_lib
    lib = _drift_lib.load()
    assert _call(lib, **bad) == -1, bad
    assert text in lib.mdil_drift_last_error(), (bad, lib.mdil_drift_last_error())


BASE = ["--before", "a.pth.tar", "--before-num-classes", "20", "--after", "b.pth.tar", "--after-num-classes", "20",
        "20", "--task", "0"]


def test_parser_defaults():
    from mdil_ss_amd import drift as D
    p = D.build_parser()
    a = p.parse_args(BASE + ["--dataset", "BDD", "--report"])
    assert (a.before, a.before_num_classes, a.after, a.after_num_classes, a.task) == \
        ("a.pth.tar", [20], "b.pth.tar", [20, 20], 0)
    assert (a.dataset, a.subset, a.synthetic) == ("BDD", "val", 0)
    assert (a.height, a.width, a.batch_size) == (512, 1024, 6)
    assert (a.report, a.score, a.json, a.out, a.kl_max, a.labels) == (True, False, None, None, 1.0, False)
    assert all(hasattr(a, k) for k in ("cs_datadir", "bdd_datadir", "idd_datadir", "cache_resized"))
    b = p.parse_args(BASE + ["--synthetic", "3", "--height", "64", "--width", "128", "--batch-size", "2", "--score",
                             "--json", "r.json", "--out", "maps", "--kl-max", "0.5", "--labels"])
    assert (b.synthetic, b.dataset, b.height, b.width, b.batch_size) == (3, None, 64, 128, 2)
    assert (b.report, b.score, b.json, b.out, b.kl_max, b.labels) == (False, True, "r.json", "maps", 0.5, True)
    assert callable(D.main)


def _with(**kw):
    argv = list(BASE)
    for flag, value in kw.items():
        i = argv.index(flag)
        j = i + 1
        while j < len(argv) and not argv[j].startswith("--"):
            j += 1
        argv[i + 1:j] = value
    return argv


@pytest.mark.parametrize("argv", [
    _with(**{"--task": ["1"]}) + ["--dataset", "BDD", "--report"],       # the model before has no task 1
    _with(**{"--task": ["2"]}) + ["--dataset", "BDD", "--report"],       # neither has task 2
    _with(**{"--after-num-classes": ["27", "20"]}) + ["--dataset", "BDD", "--report"],   # 20 classes against 27
    BASE + ["--dataset", "cityscapes"],                                  # nothing to do
    BASE + ["--synthetic", "2"],                                         # the same, synthetic
    BASE + ["--dataset", "BDD", "--out", "o", "--json", "r.json"],       # a report file without any report
    BASE + ["--report"],                                                 # no source
    BASE + ["--dataset", "BDD", "--synthetic", "2", "--report"],         # two sources
    BASE + ["--dataset", "KITTI", "--report"],                           # unknown dataset
    BASE + ["--dataset", "BDD", "--report", "--labels"],                 # label maps without --out
    BASE + ["--dataset", "BDD", "--out", "o", "--kl-max", "0"],
    BASE[2:] + ["--dataset", "BDD", "--report"],                         # no checkpoint before
])
def test_parser_refusals(argv):
    from mdil_ss_amd import drift as D
    with pytest.raises(SystemExit):
        D.build_parser().parse_args(argv)


@pytest.mark.parametrize("kw, text", [
    (dict(task=1), "the --before model has tasks 0 to 0"),
    (dict(after_num_classes=[27, 20]), "20 classes before and 27 after"),
    (dict(report=False), "nothing to do"),
    (dict(report=False, out="o", json="r.json"), "--json writes the report"),
])
def test_main_names_the_refusal(kw, text):
    from mdil_ss_amd import drift as D
    args = D.build_parser().parse_args(BASE + ["--dataset", "BDD", "--report"])
    for k, v in kw.items():
        setattr(args, k, v)
    with pytest.raises(RuntimeError, match=text):
        D.main(args)


def test_drift_refuses_cpu_tensors():
    from mdil_ss_amd import drift as D
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    x, w, b = torch.zeros(1, 2, 2, 16), torch.zeros(16, 20, 2, 2), torch.zeros(20)
    with pytest.raises(RuntimeError, match="feat_a must be a contiguous float32 device tensor.*no CPU fallback in "
                                           "the drift path"):
        D.drift_head(x, w, b, x, w, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.compare(Net([20], 1, 0), Net([20, 20], 2, 1), torch.zeros(1, 3, 32, 64), 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.DriftMeter(20, 19).add(x, w, b, x, w, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.DriftMeter(20, 19).add(Net([20], 1, 0), Net([20, 20], 2, 1), torch.zeros(1, 3, 32, 64), 0)


# Three classes, 24 pixels of which 20 are counted.
#   confusion_a (target x before)   confusion_b (target x after)   outcome (target x both right, forgotten,
#     4 1 0   | 5                     3 2 0   | 5                     3 1 0 1   | 5       gained, both wrong)
#     1 5 1   | 7                     0 6 1   | 7                     4 1 2 0   | 7
#     0 2 6   | 8                     1 1 6   | 8                     5 1 1 1   | 8
#     -----                           -----
#     5 8 7                           4 9 7
#   transition (before x after): rows sum to confusion_a's columns (5 8 7), columns to confusion_b's (4 9 7)
#     3 2 0
#     1 6 1
#     0 1 6        trace 15 of 20
CONF_A = [[4, 1, 0], [1, 5, 1], [0, 2, 6]]
CONF_B = [[3, 2, 0], [0, 6, 1], [1, 1, 6]]
OUTCOME = [[3, 1, 0, 1], [4, 1, 2, 0], [5, 1, 1, 1]]
TRANSITION = [[3, 2, 0], [1, 6, 1], [0, 1, 6]]
SUMS = [0.5, 1.4, 0.8, 6.0]


def approx(v):
    return pytest.approx(v, rel=1e-12, abs=0)


def test_drift_report_by_hand():
    from mdil_ss_amd.drift import drift_report
    t = lambda m: torch.tensor(m, dtype=torch.int64)  # noqa: E731
    r = drift_report(3, t(TRANSITION), torch.tensor(SUMS, dtype=torch.float64), 24, confusion_a=t(CONF_A),
                     confusion_b=t(CONF_B), outcome=t(OUTCOME), ignore_index=-1, top=3)
    assert (r["classes"], r["pixels"], r["counted_pixels"]) == (3, 24, 20)
    assert r["agreement"] == 15 / 20
    assert r["mean_kl"] == approx((0.5 + 1.4 + 0.8) / 20)
    assert r["kl_classes"] == [approx(0.5 / 5), approx(1.4 / 7), approx(0.8 / 8)]       # over the target's rows
    assert r["kd_loss"] == approx(6.0 / (24 * 3))
    assert r["top_transitions"] == [[0, 1, 2], [1, 0, 1], [1, 2, 1]]                    # ties: lowest (from, to)
    assert r["transition"] == TRANSITION
    # iouEval: tp / (tp + fp + fn), fp = column sum - tp, fn = row sum - tp
    before, after = [4 / 6, 5 / 10, 6 / 9], [3 / 6, 6 / 10, 6 / 9]
    assert r["iou_before"] == [approx(v) for v in before] and r["iou_after"] == [approx(v) for v in after]
    assert r["mIoU_before"] == approx(11 / 18) and r["mIoU_after"] == approx(53 / 90)
    assert r["mIoU_change"] == approx(53 / 90 - 11 / 18)
    assert r["iou_change"] == [approx(3 / 6 - 4 / 6), approx(0.1), pytest.approx(0.0, abs=1e-15)]
    assert r["forgotten"] == [approx(1 / 5), approx(1 / 7), approx(1 / 8)]
    assert r["gained"] == [0.0, approx(2 / 7), approx(1 / 8)]
    assert (r["outcome"], r["confusion_before"], r["confusion_after"]) == (OUTCOME, CONF_A, CONF_B)
    # the last class as the ignore class: it leaves the IoU lists and the means
    r2 = drift_report(3, TRANSITION, SUMS, 24, confusion_a=CONF_A, confusion_b=CONF_B, outcome=OUTCOME, ignore_index=2)
    assert r2["iou_before"] == [approx(4 / 6), approx(5 / 10)] and r2["mIoU_before"] == approx(7 / 12)
    assert r2["mIoU_after"] == approx(11 / 20) and len(r2["top_transitions"]) == 4


def test_drift_report_without_a_target():
    """The label-free half: the class of a pixel is its label before (the transition's rows)."""
    from mdil_ss_amd.drift import drift_report
    r = drift_report(3, TRANSITION, SUMS, 20)
    assert r["kl_classes"] == [approx(0.5 / 5), approx(1.4 / 8), approx(0.8 / 7)]
    assert r["agreement"] == 0.75 and r["kd_loss"] == approx(6.0 / 60)
    assert not any(k in r for k in ("mIoU_before", "mIoU_after", "forgotten", "gained", "outcome"))
    # a class without pixels has no mean; nothing seen at all: no rates
    r = drift_report(3, [[2, 0, 0], [0, 0, 0], [1, 0, 1]], [0.2, 0.0, 0.4, 1.2], 4)
    assert r["kl_classes"] == [approx(0.1), None, approx(0.2)] and r["top_transitions"] == [[2, 0, 1]]
    empty = drift_report(3, [[0] * 3] * 3, [0.0] * 4, 0)
    assert (empty["agreement"], empty["mean_kl"], empty["kd_loss"], empty["top_transitions"]) == (None, None, None, [])
    with pytest.raises(RuntimeError, match="come together"):
        drift_report(3, TRANSITION, SUMS, 20, confusion_a=CONF_A)
    with pytest.raises(RuntimeError, match=r"expected transition \[3,3\]"):
        drift_report(3, [[1, 0], [0, 1]], SUMS, 20)


def test_change_palette_and_kl_bytes():
    import numpy as np
    from mdil_ss_amd import drift as D
    codes = np.array([[0, 1, 2], [3, 4, 255]], dtype=np.uint8)
    rgb = D.change_colours(codes)
    assert rgb.dtype == np.uint8 and rgb.shape == (2, 3, 3)
    assert [tuple(v) for v in rgb.reshape(-1, 3).tolist()] == [D.CHANGE_PALETTE[c] for c in (0, 1, 2, 3, 4, 255)]
    assert len(set(D.CHANGE_PALETTE.values())) == 6
    kl = torch.tensor([0.0, 0.1, 0.25, 0.5, 7.0, float("nan"), -1e-9])
    assert D.kl_bytes(kl, 0.5).tolist() == [0, 51, 128, 255, 255, 0, 0]
