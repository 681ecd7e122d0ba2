"""CPU: the calibration add-on (include/mdil_calib.h, mdil_ss_amd/calibrate.py) -- the library exports
exactly what its header declares, every argument check answers before any launch, the report's
arithmetic against the fp64 reference of tests/calib_reference.py, the temperature search on a numpy
NLL, the inputs of the GPU tests (every case has a unimodal NLL; where its minimum lies), the
command line's defaults and refusals and the refusal of host tensors."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from tests import calib_reference as R
from tests.helpers import declared_names, dynamic_exports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mdil_calib_head", "mdil_calib_last_error", "mdil_calib_version", "mdil_calib_workspace_bytes"]


def header():
    text = open(os.path.join(ROOT, "include", "mdil_calib.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_library_exports_exactly_the_declared_symbols():
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _calib_lib
    lib = _calib_lib.load()
    assert declared_names("mdil_calib.h") == NAMES
    for n in NAMES:
        assert hasattr(lib, n), f"{n} declared in include/mdil_calib.h but not exported"
    assert sorted(_calib_lib.EXPORTS) == NAMES
    assert dynamic_exports(_calib_lib.LIB_PATH) == NAMES
    assert lib.mdil_calib_version() >= 100


def test_argument_counts_and_macros_match_the_header():
    from mdil_ss_amd import _calib_lib
    hdr = header()
    for name, (_, argtypes) in _calib_lib._SIGNATURES.items():
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr).group(1).strip()
        count = 0 if params == "void" else params.count(",") + 1
        assert count == len(argtypes), (name, count, len(argtypes))
    macros = {k: int(v) for k, v in re.findall(r"#define\s+MDIL_CALIB_(\w+)\s+\(?(-?\d+)\)?", hdr)}
    assert (macros["MIN_CLASSES"], macros["MAX_CLASSES"]) == (_calib_lib.MIN_CLASSES, _calib_lib.MAX_CLASSES) == (2, 32)
    assert (macros["MAX_TEMPS"], macros["MAX_BINS"]) == (_calib_lib.MAX_TEMPS, _calib_lib.MAX_BINS) == (16, 32)
    assert (macros["OK"], macros["ERR_INVALID"], macros["ERR_LAUNCH"]) == (0, -1, -2)


def test_build_checks_the_binding():
    assert "_calib_lib" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_workspace_bytes_is_one_row_per_work_group():
    """ceil(N H W / 256) work-groups, at most 512, of 3 K doubles each."""
    from mdil_ss_amd import _calib_lib
    lib = _calib_lib.load()
    assert lib.mdil_calib_workspace_bytes(1, 1, 1, 2, 1) == 1 * 3 * 8
    assert lib.mdil_calib_workspace_bytes(2, 12, 20, 20, 16) == 2 * 48 * 8
    assert lib.mdil_calib_workspace_bytes(6, 256, 512, 27, 16) == 512 * 48 * 8
    assert lib.mdil_calib_workspace_bytes(1, 257, 511, 32, 3) == 512 * 9 * 8
    for bad in ((0, 1, 1, 20, 1), (1, 1, 1, 1, 1), (1, 1, 1, 33, 1), (1, -1, 1, 20, 1), (1, 1, 1, 20, 0), (1, 1, 1, 20, 17)):
        assert lib.mdil_calib_workspace_bytes(*bad) == -1


OK = dict(x=4096, w=8192, b=12288, N=1, H=2, W=2, nc=20, tgt=16384, ign=19, temps=(0.5, 1.0, 2.0), K=None, bins=15,
          ct=1, lab=20480, conf=24576, nll=28672, hist=32768, ch=36864, sums=40960, nf=45056, bad=49152, ws=53248,
          wsb=9 * 8)


def _call(lib, **kw):
    a = dict(OK, **kw)
    temps = None if a["temps"] is None else (C.c_float * len(a["temps"]))(*a["temps"])
    K = a["K"] if a["K"] is not None else len(a["temps"])
    return lib.mdil_calib_head(a["x"], a["w"], a["b"], a["N"], a["H"], a["W"], a["nc"], a["tgt"], a["ign"], temps, K,
                               a["bins"], a["ct"], a["lab"], a["conf"], a["nll"], a["hist"], a["ch"], a["sums"], a["nf"],
                               a["bad"], a["ws"], a["wsb"], None)


@pytest.mark.parametrize("bad, text", [
    (dict(nc=1), b"nc=1"), (dict(nc=33), b"nc=33"),
    (dict(x=None), b"bad argument"), (dict(w=None), b"bad argument"), (dict(b=None), b"bad argument"),
    (dict(N=0), b"bad argument"), (dict(W=0), b"bad argument"), (dict(H=1 << 30, W=1 << 29), b"too large"),
    (dict(temps=(), K=0), b"K=0"), (dict(temps=(1.0,) * 16, K=17), b"K=17"), (dict(temps=None, K=1), b"temps NULL"),
    (dict(bins=0), b"bins=0"), (dict(bins=33), b"bins=33"),
    (dict(ct=3), b"class_temp=3 outside [-1, K=3)"), (dict(ct=-2), b"class_temp=-2"),
    (dict(ct=-1), b"class_hist needs class_temp >= 0"),
    (dict(temps=(1.0, 0.0, 2.0)), b"temperature 1 is 0"), (dict(temps=(-1.5, 1.0)), b"temperature 0 is -1.5"),
    (dict(temps=(1.0, 2.0, float("nan"))), b"temperature 2 is nan"), (dict(temps=(float("inf"),), ct=0), b"temperature 0 is inf"),
    (dict(tgt=None), b"a target is required"),
    (dict(ws=None), b"sums need a workspace of 72 bytes"), (dict(wsb=71), b"sums need a workspace of 72 bytes"),
    (dict(x=4100), b"alignment"), (dict(tgt=16385), b"alignment"), (dict(lab=20481), b"alignment"),
    (dict(conf=24578), b"alignment"), (dict(nll=28674), b"alignment"), (dict(hist=32772), b"alignment"),
    (dict(ch=36868), b"alignment"), (dict(sums=40964), b"alignment"), (dict(nf=45060), b"alignment"),
    (dict(bad=49156), b"alignment"), (dict(ws=53252), b"alignment"),
    (dict(ign=256), b"ignore_index=256"), (dict(ign=-2), b"ignore_index=-2"),
])
def test_library_refuses_bad_arguments_without_a_device(bad, text):
    """Argument checks come before the launch, so fake pointers never reach a device."""
    from mdil_ss_amd import _calib_lib
    lib = _calib_lib.load()
    assert _call(lib, **bad) == -1, bad
    assert text in lib.mdil_calib_last_error(), (bad, lib.mdil_calib_last_error())


# ------------------------------------------------------------------------------ report arithmetic
def flat_case(nc=20, shape=(2, 12, 20), T=1.0):
    c = R.case(nc, shape, False)
    conf, label, nll, brier, ent = R.stats64(c["logits"], c["target"], c["counted"], T)
    k = c["counted"]
    return conf[k], (label == c["target"].long())[k], nll[k], brier[k], ent[k]


@pytest.mark.parametrize("T", (0.5, 1.0, 2.5))
def test_report_matches_the_textbook_metrics(T):
    """fp64 confidences quantised by the library's q rule: each confidence loses less than 2^-24, so
    per bin |correct - confsum| moves by less than n_b 2^-24 and the ECE by less than 2^-24."""
    from mdil_ss_amd.calibrate import calibration_report
    conf, correct, nll, brier, ent = flat_case(T=T)
    n = conf.numel()
    hist = R.pack(conf, correct, 15)
    sums = torch.tensor([[nll.sum(), brier.sum(), ent.sum()]], dtype=torch.float64)
    row = calibration_report(hist[None], sums, [T])["temperatures"][0]
    ece, mce = R.textbook(conf, correct, 15)
    assert row["pixels"] == n and row["temperature"] == T
    assert row["accuracy"] == pytest.approx(correct.double().mean().item(), rel=1e-14)
    assert abs(row["ece"] - ece) <= 2.0 ** -24 and abs(row["mce"] - mce) <= 2.0 ** -24
    assert row["nll"] == pytest.approx(nll.mean().item(), rel=1e-13)
    assert row["brier"] == pytest.approx(brier.mean().item(), rel=1e-13)
    assert row["entropy"] == pytest.approx(ent.mean().item(), rel=1e-13)
    table = row["reliability"]
    assert len(table) == 15 and sum(c["pixels"] for c in table) == n
    b = (conf * 15).long().clamp(max=14)
    for i, cell in enumerate(table):
        if cell["pixels"]:
            assert cell["accuracy"] == pytest.approx(correct[b == i].double().mean().item(), rel=1e-13)
            assert abs(cell["confidence"] - conf[b == i].mean().item()) <= 2.0 ** -24
            assert i / 15 <= cell["confidence"] <= (i + 1) / 15
        else:
            assert cell["accuracy"] is None and cell["confidence"] is None


def test_a_calibrated_histogram_has_no_error_and_one_bin_gives_the_overall_gap():
    from mdil_ss_amd.calibrate import calibration_report
    # bin b of 10: 1000 pixels at confidence (2b + 1) / 20 exactly, of which that share is right
    cells = [[1000, 50 * (2 * b + 1), 1000 * ((2 * b + 1) * R.Q_ONE // 20)] for b in range(10)]
    exact = [[1000, 50 * (2 * b + 1), 50 * (2 * b + 1) * R.Q_ONE] for b in range(10)]
    row = calibration_report([exact], [[0.0, 0.0, 0.0]], [1.0])["temperatures"][0]
    assert row["ece"] == 0.0 and row["mce"] == 0.0 and row["pixels"] == 10000 and row["accuracy"] == 0.5
    row = calibration_report([cells], [[0.0, 0.0, 0.0]], [1.0])["temperatures"][0]
    assert row["ece"] < 2.0 ** -24
    conf, correct, *_ = flat_case()
    one = calibration_report(R.pack(conf, correct, 1)[None], [[0.0, 0.0, 0.0]], [1.0])["temperatures"][0]
    gap = abs(correct.double().mean().item() - conf.mean().item())
    assert abs(one["ece"] - gap) <= 2.0 ** -24 and one["ece"] == one["mce"]
    empty = calibration_report(torch.zeros(2, 15, 3, dtype=torch.int64), torch.zeros(2, 3), [1.0, 2.0])
    assert [r["ece"] for r in empty["temperatures"]] == [None, None] and empty["bins"] == 15
    with pytest.raises(RuntimeError, match=r"expected hist \[2,bins,3\]"):
        calibration_report(torch.zeros(1, 15, 3), torch.zeros(2, 3), [1.0, 2.0])


def test_class_wise_ece_is_the_mean_over_the_predicted_classes():
    from mdil_ss_amd.calibrate import calibration_report
    c = R.case(20, (2, 12, 20), False)
    conf, label, *_ = R.stats64(c["logits"], c["target"], c["counted"], 1.0)
    k = c["counted"]
    conf, label, correct = conf[k], label[k], (label == c["target"].long())[k]
    ch = torch.stack([R.pack(conf[label == cl], correct[label == cl], 15) for cl in range(20)])
    r = calibration_report(R.pack(conf, correct, 15)[None], [[0.0, 0.0, 0.0]], [1.0], class_hist=ch,
                           names=[f"c{i}" for i in range(20)])
    want = [R.textbook(conf[label == cl], correct[label == cl], 15)[0] if (label == cl).any() else None for cl in range(20)]
    assert torch.equal(ch.sum(0), R.pack(conf, correct, 15))
    for got, w in zip(r["class_ece"], want):
        assert (got is None) == (w is None) and (w is None or abs(got - w) <= 2.0 ** -24)
    seen = [v for v in r["class_ece"] if v is not None]
    assert len(seen) >= 10 and r["classwise_ece"] == pytest.approx(sum(seen) / len(seen), rel=1e-14)
    assert r["class_names"][3] == "c3"


# -------------------------------------------------------------------------------------- the fit
def fit_case(t0, scale=1.0):
    c = R.case(20, (3, 16, 48), False)
    logits = c["logits"]
    target = R.sample_targets(logits, 20, 11, 255, t0=t0, salt=False)
    counted = torch.ones_like(target, dtype=torch.bool)
    return logits * scale, target, counted


@pytest.mark.parametrize("t0", (0.6, 1.7))
def test_fit_lands_within_one_cell_of_the_dense_minimiser(t0):
    from mdil_ss_amd.calibrate import fit_temperature
    logits, target, counted = fit_case(t0)
    fit = fit_temperature(lambda temps: R.nll_curve(logits, target, counted, temps))
    best = R.dense_minimiser(logits, target, counted)
    assert abs(math.log(best / t0)) < 0.1                        # the sample's own optimum is near t0
    assert fit["cell"] == pytest.approx(16 ** ((2 / 15) ** 3 / 15), rel=1e-9)
    assert abs(math.log(fit["temperature"] / best)) <= math.log(fit["cell"]) * (1 + 1e-9)
    lo, hi = fit["bracket"]
    assert lo < best < hi and hi / lo == pytest.approx(16 ** ((2 / 15) ** 4), rel=1e-9)     # 1.0009
    assert len(fit["trace"]) == 64 and fit["trace"][0][0] == 0.25 and fit["trace"][15][0] == 4.0
    # scale equivariance: three times the logits on three times the range gives three times the temperature
    fit3 = fit_temperature(lambda temps: R.nll_curve(3 * logits, target, counted, temps), lo=0.75, hi=12.0)
    assert abs(math.log(fit3["temperature"] / (3 * fit["temperature"]))) <= math.log(fit["cell"]) * (1 + 1e-9)


def test_fit_moves_out_at_an_end_point():
    """Targets sampled at T0 = 6 with hi = 4: every round whose argmin is the last point lengthens
    the range by one cell, until the minimum is inside; the round that finds it inside brackets it."""
    from mdil_ss_amd.calibrate import fit_temperature
    logits, target, counted = fit_case(6.0)
    best = R.dense_minimiser(logits, target, counted)
    assert best > 4.5
    fit = fit_temperature(lambda temps: R.nll_curve(logits, target, counted, temps), hi=4.0)
    lo, hi = fit["bracket"]
    assert hi > 4.0 and lo < best < hi
    assert abs(math.log(fit["temperature"] / best)) <= math.log(fit["cell"]) * (1 + 1e-9)
    with pytest.raises(RuntimeError, match="needs 0 < lo < hi"):
        fit_temperature(lambda temps: [0.0] * len(temps), lo=2.0, hi=1.0)


@pytest.mark.parametrize("ignore_last", (True, False))
@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("nc", R.CLASSES)
def test_every_gpu_case_has_a_unimodal_nll(nc, shape, ignore_last):
    """The 32 inputs of tests/test_calib_gpu.py: the NLL falls and then rises along 64 temperatures
    on [0.25, 4], and three rounds of 16 points bracket its minimum to a ratio of 1.0066.  The
    minimum lies inside [0.25, 4] in 30 cases.  The other two are two-class cases whose ignore index
    is class 1: only pixels of class 0 are counted there, nothing is ever wrong at a high
    confidence, and the optimum moves past 4 (5.28 and 11.37)."""
    from mdil_ss_amd.calibrate import fit_temperature
    c = R.case(nc, shape, ignore_last)
    temps = [0.25 * 16 ** (i / 63) for i in range(64)]
    v = R.nll_curve(c["logits"], c["target"], c["counted"], temps)
    i = min(range(64), key=lambda j: v[j])
    slack = 1e-12 * max(abs(x) for x in v)
    assert all(a >= b - slack for a, b in zip(v[:i], v[1:i + 1])) and all(a <= b + slack for a, b in zip(v[i:], v[i + 1:]))
    best = R.dense_minimiser(c["logits"], c["target"], c["counted"])
    outside = nc == 2 and ignore_last and shape in ((1, 9, 7), (2, 12, 20))
    assert (best > 4.0) == outside and best > 0.25
    if not outside:
        fit = fit_temperature(lambda t: R.nll_curve(c["logits"], c["target"], c["counted"], t), rounds=3)
        lo, hi = fit["bracket"]
        assert lo <= best <= hi and hi / lo == pytest.approx(16 ** ((2 / 15) ** 3), rel=1e-9)    # 1.0066


# ------------------------------------------------------------------------------------------ CLI
BASE = ["--state", "a.pth.tar", "--num-classes", "20", "20", "--task", "0", "--json", "r.json"]


def test_parser_defaults():
    from mdil_ss_amd import calibrate as K
    p = K.build_parser()
    a = p.parse_args(BASE + ["--dataset", "cityscapes"])
    assert (a.state, a.num_classes, a.task, a.json) == ("a.pth.tar", [20, 20], 0, "r.json")
    assert (a.dataset, a.subset, a.synthetic) == ("cityscapes", "val", 0)
    assert (a.height, a.width, a.batch_size) == (512, 1024, 6)
    assert (a.bins, a.temperature, a.fit, a.fit_rounds, a.feature_cache_gb, a.out) == (15, None, False, 4, 16.0, None)
    assert all(hasattr(a, k) for k in ("cs_datadir", "bdd_datadir", "idd_datadir", "cache_resized"))
    b = p.parse_args(BASE + ["--synthetic", "2", "--height", "64", "--width", "128", "--fit", "--fit-rounds", "3",
                             "--feature-cache-gb", "0", "--out", "o", "--bins", "10"])
    assert (b.synthetic, b.dataset, b.height, b.width) == (2, None, 64, 128)
    assert (b.fit, b.fit_rounds, b.feature_cache_gb, b.out, b.bins) == (True, 3, 0.0, "o", 10)
    c = p.parse_args(BASE + ["--dataset", "BDD", "--temperature", "1.5", "2"])
    assert c.temperature == [1.5, 2.0]
    assert callable(K.main)


@pytest.mark.parametrize("argv", [
    BASE,                                                                # no source
    BASE + ["--dataset", "BDD", "--synthetic", "2"],                     # two sources
    BASE + ["--dataset", "KITTI"],                                       # unknown dataset
    BASE[:-2] + ["--dataset", "BDD"],                                    # no --json
    BASE[2:] + ["--dataset", "BDD"],                                     # no checkpoint
    BASE + ["--dataset", "BDD", "--fit", "--temperature", "2"],          # fit or given, not both
    BASE + ["--dataset", "BDD", "--temperature", "0"],
    BASE + ["--dataset", "BDD", "--temperature", "-1"],
    BASE + ["--dataset", "BDD", "--temperature"] + ["1.5"] * 17,
    BASE + ["--dataset", "BDD", "--bins", "0"],
    BASE + ["--dataset", "BDD", "--bins", "33"],
    BASE + ["--dataset", "BDD", "--fit", "--fit-rounds", "0"],
    BASE + ["--dataset", "BDD", "--feature-cache-gb", "-1"],
    [a if a != "0" else "2" for a in BASE] + ["--dataset", "BDD"],       # the model has no task 2
])
def test_parser_refusals(argv):
    from mdil_ss_amd import calibrate as K
    with pytest.raises(SystemExit):
        K.build_parser().parse_args(argv)


def test_main_names_the_refusal():
    from mdil_ss_amd import calibrate as K
    args = K.build_parser().parse_args(BASE + ["--dataset", "BDD"])
    args.task = 2
    with pytest.raises(RuntimeError, match="the model has tasks 0 to 1"):
        K.main(args)
    args.task, args.fit, args.temperature = 0, True, [2.0]
    with pytest.raises(RuntimeError, match="--fit and --temperature exclude each other"):
        K.main(args)


def test_calibration_refuses_cpu_tensors():
    from mdil_ss_amd import calibrate as K
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    x, w, b = torch.zeros(1, 2, 2, 16), torch.zeros(16, 20, 2, 2), torch.zeros(20)
    t = torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="feat must be a contiguous float32 device tensor.*no CPU fallback in "
                                           "the calibration path"):
        K.calib_head(x, w, b, t, [1.0])
    with pytest.raises(RuntimeError, match="no CPU fallback in the calibration path"):
        K.calibrate(Net([20], 1, 0), torch.zeros(1, 3, 32, 64), 0, t, [1.0])
    with pytest.raises(RuntimeError, match="no CPU fallback in the calibration path"):
        K.CalibrationMeter(20, [1.0]).add(x, w, b, target=t)
    with pytest.raises(RuntimeError, match="no CPU fallback in the calibration path"):
        K.CalibrationMeter(20, [1.0]).add(Net([20], 1, 0), torch.zeros(1, 3, 32, 64), 0, target=t)
    with pytest.raises(RuntimeError, match="1 to 16"):
        K.CalibrationMeter(20, [1.0] * 17)
    with pytest.raises(RuntimeError, match="finite and > 0"):
        K.CalibrationMeter(20, [1.0, 0.0])
