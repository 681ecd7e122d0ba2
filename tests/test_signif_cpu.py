"""CPU: the significance add-on (include/mdil_signif.h, mdil_ss_amd/significance.py) -- the library
exports exactly what its header declares, every argument check answers before any launch, the
command line's defaults and refusals, the two spellings of the numpy reference against each other,
the generator's published outputs, a three-image case worked by hand, the interval arithmetic, a
predictor paired with itself, the coverage of the percentile interval on synthetic sets, the refusal
of host tensors, and the rule the add-on exists under: it leaves the training path's build id alone."""
import os

import numpy as np
import pytest
import torch

from tests import signif_reference as R
from tests.helpers import declared_names, dynamic_exports

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mdil_signif_count", "mdil_signif_last_error", "mdil_signif_resample", "mdil_signif_version"]


def test_library_exports_exactly_the_declared_symbols():
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _segments_lib, _signif_lib
    lib = _signif_lib.load()
    assert declared_names("mdil_signif.h") == NAMES
    for n in NAMES:
        assert hasattr(lib, n), f"{n} declared in include/mdil_signif.h but not exported"
    assert sorted(_signif_lib.EXPORTS) == NAMES
    assert dynamic_exports(_signif_lib.LIB_PATH) == NAMES
    assert lib.mdil_signif_version() >= 100
    assert (_signif_lib.BOOTSTRAP, _signif_lib.JACKKNIFE, _signif_lib.SWAP) == (0, 1, 2)
    # the add-on it is modelled on keeps its six names
    assert len(dynamic_exports(_segments_lib.LIB_PATH)) == 6


COUNT = dict(pred=4096, target=8192, N=1, H=8, W=8, nc=20, ign=19, first=0, M=4, G=1, g=0, counts=12288, bad=16384,
             unp=16392)
RESAMPLE = dict(counts=4096, M=4, G=2, nc=20, ign=19, mode=0, first=0, B=8, seed=0, sums=8192, miou=12288, iou=16384,
                empty=20480)


def _count(lib, **kw):
    a = dict(COUNT, **kw)
    return lib.mdil_signif_count(a["pred"], a["target"], a["N"], a["H"], a["W"], a["nc"], a["ign"], a["first"], a["M"],
                                 a["G"], a["g"], a["counts"], a["bad"], a["unp"], None)


def _resample(lib, **kw):
    a = dict(RESAMPLE, **kw)
    return lib.mdil_signif_resample(a["counts"], a["M"], a["G"], a["nc"], a["ign"], a["mode"], a["first"], a["B"],
                                    a["seed"], a["sums"], a["miou"], a["iou"], a["empty"], None)


BAD = [(_count, bad, text) for bad, text in [
    (dict(pred=None), b"bad argument"), (dict(target=None), b"bad argument"), (dict(counts=None), b"bad argument"),
    (dict(bad=None), b"bad argument"), (dict(unp=None), b"bad argument"),
    (dict(N=0), b"bad argument"), (dict(H=0), b"bad argument"), (dict(W=-3), b"bad argument"),
    (dict(nc=1), b"nc=1"), (dict(nc=33), b"nc=33"),
    (dict(H=(1 << 15) + 1), b"above 32768"), (dict(W=(1 << 15) + 1), b"above 32768"),
    (dict(N=(1 << 10) + 1, H=1 << 15, W=1 << 15, M=1 << 20), b"too large"),
    (dict(ign=-2), b"ignore_index=-2"), (dict(ign=256), b"ignore_index=256"),
    (dict(M=0), b"M=0"), (dict(M=(1 << 20) + 1), b"M=1048577"),
    (dict(G=0), b"G=0"), (dict(G=3), b"G=3"), (dict(g=1), b"group g=1"), (dict(g=-1), b"group g=-1"),
    (dict(G=2, g=2), b"group g=2"),
    (dict(first=-1), b"first_image=-1"), (dict(first=4), b"first_image=4"), (dict(N=3, first=2), b"first_image=2"),
    (dict(N=5), b"first_image=0"),
    (dict(pred=4097), b"alignment"), (dict(target=8194), b"alignment"), (dict(counts=12292), b"alignment"),
    (dict(bad=16388), b"alignment"), (dict(unp=16396), b"alignment"),
]] + [(_resample, bad, text) for bad, text in [
    (dict(counts=None), b"bad argument"), (dict(miou=None), b"bad argument"),
    (dict(nc=1), b"nc=1"), (dict(nc=33), b"nc=33"),
    (dict(M=0), b"M=0"), (dict(M=-5), b"M=-5"), (dict(M=(1 << 20) + 1), b"M=1048577"),
    (dict(G=0), b"G=0"), (dict(G=3), b"G=3"),
    (dict(mode=3), b"mode=3"), (dict(mode=-1), b"mode=-1"),
    (dict(ign=-2), b"ignore_index=-2"), (dict(ign=256), b"ignore_index=256"),
    (dict(ign=0), b"must be the last one"), (dict(ign=18), b"must be the last one"), (dict(ign=7), b"must be the last"),
    (dict(mode=2, G=1), b"needs G=2"),
    (dict(mode=1, B=5), b"the jackknife has M=4"), (dict(mode=1, first=3, B=2), b"the jackknife has M=4"),
    (dict(first=-1), b"replicates first_replicate=-1"), (dict(B=0), b"B=0"), (dict(B=-2), b"B=-2"),
    (dict(first=(1 << 32) - 7), b"first + B <= 2^32"), (dict(B=(1 << 32) + 1), b"first + B <= 2^32"),
    (dict(first=1 << 40), b"first + B <= 2^32"),
    (dict(counts=4100), b"alignment"), (dict(sums=8196), b"alignment"), (dict(miou=12292), b"alignment"),
    (dict(iou=16388), b"alignment"), (dict(empty=20482), b"alignment"),
]]


@pytest.mark.parametrize("call, bad, text", BAD, ids=[f"{c.__name__[1:]}-{b}" for c, b, _ in BAD])
def test_library_refuses_bad_arguments_without_a_device(call, bad, text):
    """Argument checks come before the launch, so fake pointers never reach a device."""
    from mdil_ss_amd import _signif_lib
    lib = _signif_lib.load()
    assert call(lib, **bad) == -1, bad
    assert text in lib.mdil_signif_last_error(), (bad, lib.mdil_signif_last_error())


BASE = ["--num-classes", "20", "20", "27", "--task", "2"]
STATE = BASE + ["--state", "ckpt.pth.tar"]
PAIR = ["--before", "a.pth.tar", "--before-num-classes", "20", "--after", "b.pth.tar", "--after-num-classes", "20",
        "20", "--task", "0"]


def test_parser_defaults():
    from mdil_ss_amd import significance as S
    p = S.build_parser()
    a = p.parse_args(STATE + ["--dataset", "IDD"])
    assert (a.state, a.num_classes, a.task, a.dataset, a.subset) == ("ckpt.pth.tar", [20, 20, 27], 2, "IDD", "val")
    assert (a.height, a.width, a.batch_size, a.native_height, a.native_width) == (512, 1024, 6, 1024, 2048)
    assert (a.replicates, a.seed, a.level, a.influence, a.json, a.synthetic) == (10000, 0, 0.95, 10, None, 0)
    assert (a.before, a.after, a.before_num_classes, a.after_num_classes, a.pred, a.pred_b) == (None,) * 6
    b = p.parse_args(PAIR + ["--synthetic", "5", "--native-height", "96", "--native-width", "200", "--replicates",
                             "500", "--seed", "7", "--level", "0.9", "--influence", "3", "--json", "r.json"])
    assert (b.before, b.before_num_classes, b.after, b.after_num_classes, b.task, b.num_classes) == \
        ("a.pth.tar", [20], "b.pth.tar", [20, 20], 0, None)
    assert (b.synthetic, b.native_height, b.native_width, b.replicates, b.seed, b.level, b.influence, b.json) == \
        (5, 96, 200, 500, 7, 0.9, 3, "r.json")
    c = p.parse_args(BASE + ["--pred", "maps", "--pred-b", "other", "--dataset", "BDD"])
    assert (c.pred, c.pred_b, c.state) == ("maps", "other", None)
    assert callable(S.main)


@pytest.mark.parametrize("argv", [
    BASE + ["--dataset", "BDD"],                                         # no source
    STATE + ["--pred", "maps", "--dataset", "BDD"],                      # two sources
    STATE + PAIR[:-2] + ["--dataset", "BDD"],
    STATE,                                                               # no data
    STATE + ["--dataset", "BDD", "--synthetic", "2"],
    ["--state", "c", "--task", "0", "--dataset", "BDD"],                 # --state without --num-classes
    ["--state", "c", "--num-classes", "20", "--dataset", "BDD"],         # no --task
    STATE[:3] + ["--task", "3", "--state", "c", "--dataset", "BDD"],     # --task outside the model
    PAIR[:6] + ["--task", "0", "--dataset", "BDD"],                      # half a pair
    PAIR + ["--num-classes", "20", "--dataset", "BDD"],
    PAIR[:-1] + ["1", "--dataset", "BDD"],                               # --task outside the --before model
    PAIR[:3] + ["19"] + PAIR[4:] + ["--dataset", "BDD"],                 # heads of two widths
    BASE + ["--pred-b", "other", "--dataset", "BDD"],                    # --pred-b alone
    BASE + ["--pred", "maps", "--pred-b", "maps/../maps", "--dataset", "BDD"],
    STATE + ["--dataset", "BDD", "--replicates", "1"],
    STATE + ["--dataset", "BDD", "--replicates", str((1 << 32) + 1)],
    STATE + ["--dataset", "BDD", "--seed", "-1"],
    STATE + ["--dataset", "BDD", "--level", "1"],
    STATE + ["--dataset", "BDD", "--level", "0"],
    STATE + ["--dataset", "BDD", "--influence", "-1"],
    STATE + ["--synthetic", "2", "--native-height", "0"],
    STATE + ["--dataset", "BDD", "--score"],                             # flags of the other command lines
])
def test_parser_refusals(argv):
    from mdil_ss_amd import significance as S
    with pytest.raises(SystemExit):
        S.build_parser().parse_args(argv)


def test_main_refuses_before_it_opens_anything():
    from mdil_ss_amd import significance as S
    p = S.build_parser()
    ok = p.parse_args(STATE + ["--synthetic", "2"])

    def change(**kw):
        a = p.parse_args(STATE + ["--synthetic", "2"])
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert ok.state == "ckpt.pth.tar"
    for kw, flag in ((dict(state=None), "give one source"), (dict(pred="maps"), "--state, --pred"),
                     (dict(num_classes=None), "--state needs --num-classes"), (dict(task=None), "--task is needed"),
                     (dict(task=5), "--task 5"), (dict(state=None, pred_b="x"), "give one source"),
                     (dict(state=None, pred="x", pred_b="x"), "--pred-b is --pred"),
                     (dict(replicates=1), "--replicates 1"), (dict(seed=1 << 64), "--seed"),
                     (dict(level=1.5), "--level 1.5"), (dict(influence=-2), "--influence -2"),
                     (dict(synthetic=0), "--dataset"), (dict(native_width=0), "--native-height and --native-width"),
                     (dict(state=None, before="a", after="b", before_num_classes=[20]), "a pair needs"),
                     (dict(state=None, num_classes=None, before="a", after="b", before_num_classes=[20],
                           after_num_classes=[19], task=0), "the heads must agree")):
        with pytest.raises(RuntimeError, match=flag):
            S.main(change(**kw))


def test_the_generator_gives_its_published_first_outputs():
    """SplitMix64 from state 0: 0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4 -- counters 1 and 2."""
    assert (R.splitmix(0, 0, 0), R.splitmix(0, 0, 1)) == (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4)
    assert R.hashes(0, 0, 1, 2)[0].tolist() == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4]
    seed, b = (1 << 63) + 5, (1 << 32) - 1
    assert [int(v) for v in R.hashes(seed, b, 1, 70)[0]] == [R.splitmix(seed, b, j) for j in range(70)]
    assert R.draws(seed, b, 1, 1)[0].tolist() == [0] and set(R.bits(seed, 3, 1, 200)[0].tolist()) == {0, 1}
    d = R.draws(3, 0, 200, 37)
    assert d.min() == 0 and d.max() == 36 and abs(d.mean() - 18.0) < 0.5


@pytest.mark.parametrize("mode", (R.BOOTSTRAP, R.JACKKNIFE, R.SWAP))
@pytest.mark.parametrize("M, nc", ((1, 2), (7, 5), (65, 3)))
def test_the_two_reference_spellings_agree(mode, M, nc):
    rng = np.random.default_rng(M + nc)
    table = rng.integers(0, 1 << 31, size=(M, 2, 3, nc))
    table[0] = (1 << 31) - 1
    for seed in (0, (1 << 63) + 5):
        for b in sorted({0, M // 2, M - 1}):
            got = R.replicate_gather(table, mode, b, seed)
            assert got.dtype == np.int64 and got.tolist() == R.replicate_multiplicity(table, mode, b, seed)
    one = R.replicate_gather(table[:, :1], mode, 0, 9) if mode != R.SWAP else None
    assert one is None or one.tolist() == R.replicate_multiplicity(table[:, :1], mode, 0, 9)


# three images of 1 x 4 pixels, three classes, 255 ignored
TARGET = np.array([[[0, 0, 1, 2]], [[0, 0, 0, 0]], [[1, 2, 2, 255]]], dtype=np.uint8)
PRED_A = np.array([[[0, 1, 1, 2]], [[0, 0, 0, 0]], [[2, 2, 2, 0]]], dtype=np.uint8)
PRED_B = np.array([[[0, 0, 1, 2]], [[1, 0, 0, 0]], [[1, 2, 2, 0]]], dtype=np.uint8)
ROWS_A = [[[1, 1, 1], [1, 2, 1], [2, 1, 1]], [[4, 0, 0], [4, 0, 0], [4, 0, 0]], [[0, 0, 2], [0, 0, 3], [0, 1, 2]]]
ROWS_B = [[[2, 1, 1], [2, 1, 1], [2, 1, 1]], [[3, 0, 0], [3, 1, 0], [4, 0, 0]], [[0, 1, 2], [0, 1, 2], [0, 1, 2]]]


def test_three_images_by_hand():
    a, bad, unpredicted = R.counts(PRED_A, TARGET, 3, 255)
    b, _, _ = R.counts(PRED_B, TARGET, 3, 255)
    assert a.tolist() == ROWS_A and b.tolist() == ROWS_B and (bad, unpredicted) == (0, 0)
    # 255 not ignored: a bad target; two classes only: targets 2 are bad, predictions 2 unpredicted
    assert R.counts(PRED_A, TARGET, 3, -1)[1:] == (1, 0)
    two, bad, unpredicted = R.counts(PRED_A, TARGET, 2, 255)
    assert (bad, unpredicted) == (3, 1) and two.tolist() == [[[1, 1], [1, 2], [2, 1]], [[4, 0], [4, 0], [4, 0]],
                                                             [[0, 0], [0, 0], [0, 1]]]
    table = np.stack([a, b], axis=1)
    miou, iou, empty = R.score(table.sum(0), 3, 255)
    assert iou[0].tolist() == pytest.approx([5 / 6, 1 / 3, 3 / 4], abs=1e-15) and miou[0] == pytest.approx(23 / 36)
    assert empty.tolist() == [0, 0]
    # seed 0, replicate 2 draws the images 2, 1, 1
    assert R.draws(0, 2, 1, 3)[0].tolist() == [2, 1, 1]
    boot = R.replicates(table, 3, 255, R.BOOTSTRAP, 1, 0, first=2)
    assert boot["sums"][0, 0].tolist() == [[8, 0, 2], [8, 0, 3], [8, 1, 2]]
    assert boot["iou"][0, 0].tolist() == pytest.approx([1.0, 0.0, 2 / 3], abs=1e-15)
    assert boot["miou"][0, 0] == pytest.approx(5 / 9, abs=1e-15)
    # without image 1
    jack = R.replicates(table, 3, 255, R.JACKKNIFE, 1, 0, first=1)
    assert jack["sums"][0, 0].tolist() == [[1, 1, 3], [1, 2, 4], [2, 2, 3]]
    assert jack["miou"][0, 0] == pytest.approx(19 / 36, abs=1e-15)
    only = R.replicates(table, 3, 255, R.JACKKNIFE, 1, 0, first=0)["sums"][0, 0]
    assert only.tolist() == [[4, 0, 2], [4, 0, 3], [4, 1, 2]]
    # seed 0, replicate 2 exchanges the predictors of images 0 and 2
    assert R.bits(0, 2, 1, 3)[0].tolist() == [1, 0, 1]
    swap = R.replicates(table, 3, 255, R.SWAP, 1, 0, first=2)
    assert swap["sums"][0].tolist() == [[[6, 2, 3], [6, 2, 3], [6, 2, 3]], [[4, 1, 3], [4, 3, 4], [6, 2, 3]]]
    assert swap["miou"][0, 0] == pytest.approx(1.0, abs=1e-15)
    assert swap["miou"][0, 1] == pytest.approx((4 / 6 + 1 / 4 + 3 / 4) / 3, abs=1e-15)
    # a class that lives in one image only is empty where that image is not drawn; the ignore class is no class
    lone = np.zeros((2, 1, 3, 3), dtype=np.int64)
    lone[0, 0, :, 0] = 5
    lone[1, 0, :, 1] = 7
    _, iou, empty = R.score(lone[0], 3, 2)
    assert iou.shape == (1, 2) and empty.tolist() == [0b110] and iou[0].tolist() == pytest.approx([1.0, 0.0])


def test_the_module_scores_as_the_reference_does():
    from mdil_ss_amd import significance as S
    rng = np.random.default_rng(5)
    sums = rng.integers(0, 1 << 40, size=(50, 2, 3, 20))
    sums[:, :, 0] = np.minimum(sums[:, :, 0], np.minimum(sums[:, :, 1], sums[:, :, 2]))
    sums[3, 1, :, 4] = 0
    for ignore in (19, 255, -1):
        want, got = R.score(sums, 20, ignore), S.score_counts(sums, 20, ignore)
        for w, g in zip(want, got):
            assert np.array_equal(w, g)
    assert got[2][3, 1] == 1 << 4
    with pytest.raises(RuntimeError, match="must be the last one"):
        S.score_counts(sums, 20, 3)
    # fullres.iou_rule (numpy's pairwise mean) agrees within the rounding of 19 adds
    from mdil_ss_amd import fullres as FR
    t = torch.from_numpy(sums[0, 0]).double()
    mean, per_class = FR.iou_rule(20, 19, t[0], t[1], t[2])
    ref_mean, ref_classes, _ = R.score(sums[0, 0], 20, 19)
    assert np.array_equal(per_class.numpy(), ref_classes) and abs(float(mean) - ref_mean) < 1e-14


def test_intervals():
    from mdil_ss_amd import significance as S
    rng = np.random.default_rng(0)
    boot = rng.normal(0.5, 0.01, 4001)
    theta = float(np.median(boot))                       # as many replicates below as above: z0 = 0
    jack = np.array([0.4, 0.6])                          # symmetric: a = 0
    out = S.intervals(theta, boot, jack, 0.95)
    assert out["z0"] == 0.0 and out["acceleration"] == 0.0
    assert out["se"] == pytest.approx(boot.std(ddof=1), rel=1e-15)
    assert out["percentile"] == [float(v) for v in np.quantile(boot, [0.025, 0.975])]
    assert out["bca"] == pytest.approx(out["percentile"], abs=1e-12) and out["bca_reason"] is None
    # a skewed jackknife and an estimate off the median move the BCa interval
    skew = S.intervals(theta + 0.005, boot, np.array([0.1, 0.5, 0.5, 0.5, 0.52]), 0.9)
    assert skew["z0"] > 0 and skew["acceleration"] > 0 and skew["bca"][0] > skew["percentile"][0]
    # identical images: every replicate is the estimate
    flat = S.intervals(0.25, np.full(100, 0.25), np.full(7, 0.25), 0.95)
    assert flat["se"] == 0.0 and flat["percentile"] == [0.25, 0.25] == flat["bca"] and flat["z0"] == 0.0
    # z0 infinite: null with a reason
    none = S.intervals(1.0, boot, jack, 0.95)
    assert none["bca"] is None and "every bootstrap replicate" in none["bca_reason"] and none["z0"] is None
    none = S.intervals(0.0, boot, jack, 0.95)
    assert none["bca"] is None and "no bootstrap replicate" in none["bca_reason"]
    assert none["percentile"] == out["percentile"]
    for bad in (dict(boot=boot[:1]), dict(level=1.0), dict(level=0.0), dict(jack=np.array([]))):
        with pytest.raises(RuntimeError, match="significance"):
            S.intervals(**dict(dict(theta_hat=0.5, boot=boot, jack=jack, level=0.95), **bad))


def _host_report(table, nc, ignore, B, seed, **kw):
    from mdil_ss_amd import significance as S
    G = table.shape[1]
    boot = R.replicates(table, nc, ignore, R.BOOTSTRAP, B, seed)
    jack = R.replicates(table, nc, ignore, R.JACKKNIFE, table.shape[0], seed)
    swap = R.replicates(table, nc, ignore, R.SWAP, B, seed) if G == 2 else None
    return S.build_report(table.sum(0), boot, jack, swap, nc, ignore, [f"s{i}" for i in range(table.shape[0])],
                          seed=seed, **kw)


def test_a_predictor_paired_with_itself():
    table = R.synthetic_tables(np.random.default_rng(3), 40, 6)
    rep = _host_report(np.concatenate([table, table], axis=1), 6, -1, 500, 1)
    d = rep["delta"]
    assert d["value"] == 0.0 and d["se"] == 0.0 and d["percentile"] == [0.0, 0.0] and d["bca"] == [0.0, 0.0]
    assert d["p_boot"] == 1.0 and d["p_swap"] == 1.0
    assert all(c["value"] == 0.0 and c["percentile"] == [0.0, 0.0] for c in d["classes"])
    assert rep["predictors"][0]["mIoU"] == rep["predictors"][1]["mIoU"] and rep["paired"]


def test_report_fields_on_identical_images_and_on_a_clear_difference():
    row = R.synthetic_tables(np.random.default_rng(4), 1, 6)
    rep = _host_report(np.repeat(row, 12, axis=0), 6, -1, 200, 0, influence=3)
    m = rep["predictors"][0]["mIoU"]
    # every replicate is 12 times the one image: the ratio is the same up to the rounding of the divide
    assert m["se"] < 1e-15 and m["percentile"][1] - m["percentile"][0] < 1e-15
    assert (rep["images"], rep["classes"], rep["replicates"], rep["paired"]) == (12, 6, 200, False)
    assert len(rep["predictors"][0]["influence"]) == 3 and "delta" not in rep
    assert [e["image"] for e in rep["predictors"][0]["influence"]] == [0, 1, 2]      # all equal: by index
    assert rep["predictors"][0]["empty_replicates"] == [0] * 6
    # B is A with a tenth of every image's hits taken away: B - A is negative in every replicate
    a = R.synthetic_tables(np.random.default_rng(5), 50, 6)
    b = a.copy()
    b[:, 0, 0] -= b[:, 0, 0] // 10
    rep = _host_report(np.concatenate([a, b], axis=1), 6, -1, 999, 2, influence=50)
    d = rep["delta"]
    assert d["value"] < 0 and d["percentile"][1] < 0 and d["p_boot"] == 2 / 1000 and d["p_swap"] == 1 / 1000
    assert d["bca"] is None or d["bca"][1] < 0
    worst = d["influence"][0]
    assert worst["stem"] == f"s{worst['image']}"
    assert abs(worst["change"]) == max(abs(e["change"]) for e in d["influence"])
    assert len(d["influence"]) == 50 and len(d["classes"]) == 6
    # classes that live in few images are missing from some replicates
    rare = R.synthetic_tables(np.random.default_rng(6), 8, 6)
    rare[1:, :, :, 5] = 0
    rep = _host_report(rare, 6, -1, 400, 0)
    gone = rep["predictors"][0]["empty_replicates"]
    assert gone[:5] == [0] * 5 and 100 < gone[5] < 180                    # (7/8)^8 = 0.34 of 400


def test_percentile_interval_covers_the_population_value():
    """300 synthetic sets of 60 i.i.d. images and 6 classes, B = 1000: the 95 % percentile interval
    must cover the population mIoU (200,000 images) in a share within [0.88, 0.99]."""
    truth = R.score(R.synthetic_tables(np.random.default_rng(2024), 200000, 6).sum(0), 6, -1)[0][0]
    covered = 0
    for s in range(300):
        table = R.synthetic_tables(np.random.default_rng(1000 + s), 60, 6)
        miou = R.replicates(table, 6, -1, R.BOOTSTRAP, 1000, s)["miou"][:, 0]
        lo, hi = np.quantile(miou, [0.025, 0.975])
        covered += bool(lo <= truth <= hi)
    print(f"population mIoU {truth:.4f}: covered by {covered} of 300 intervals")
    assert 0.88 <= covered / 300 <= 0.99


def test_meter_settings_and_refusals_of_cpu_tensors():
    from mdil_ss_amd import significance as S
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    m = S.SignificanceMeter(20, 19)
    assert (m.nc, m.ignore_index, m.k, m.G, m.paired, m.images) == (20, 19, 19, 1, False, 0)
    assert S.SignificanceMeter(27, 255, paired=True).k == 27 and S.SignificanceMeter(27, -1, paired=True).G == 2
    with pytest.raises(RuntimeError, match="must be the last one"):
        S.SignificanceMeter(20, 3)
    with pytest.raises(RuntimeError, match="33 classes"):
        S.SignificanceMeter(33, 32)
    with pytest.raises(RuntimeError, match="no image was added"):
        m.report()
    with pytest.raises(RuntimeError, match="replicates 1"):
        m.report(replicates=1)
    pred, target = torch.zeros(1, 8, 8, dtype=torch.uint8), torch.zeros(1, 8, 8, dtype=torch.uint8)
    table = torch.zeros(4, 1, 3, 20, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="pred must be a contiguous uint8 device tensor.*no CPU fallback in the "
                                           "significance path"):
        S.image_counts(pred, target, 20, ignore_index=19, counts=table, first_image=0)
    with pytest.raises(RuntimeError, match="counts must be a contiguous int64 device tensor.*no CPU fallback"):
        S.resample(table, 20, 19, "bootstrap", 10, 0)
    with pytest.raises(RuntimeError, match="target must be a contiguous uint8 device tensor.*no CPU fallback"):
        m.add(pred, target)
    x, w, b = torch.zeros(1, 2, 2, 16), torch.zeros(16, 20, 2, 2), torch.zeros(20)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.add(x, w, b, target=target)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.add(Net([20], 1, 0), torch.zeros(1, 3, 32, 64), 0, target=target)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.SignificanceMeter(20, 19, paired=True).add(pred, (x, w, b), target=target)
    with pytest.raises(RuntimeError, match="expects"):
        m.add(pred)
    with pytest.raises(RuntimeError, match="expects .a, b, target"):
        S.SignificanceMeter(20, 19, paired=True).add(pred, target)
    assert S.scored_classes(20, 19) == 19 and S.scored_classes(20, 255) == 20 and S.scored_classes(20, -1) == 20


def test_training_build_id_is_untouched():
    """tests/test_miou_parity.py counts only the recorded mIoU runs that carry the id of the build
    under test and needs 32 of them: the add-on must leave that id where the recorded runs have it."""
    from mdil_ss_amd import significance  # noqa: F401
    from tests import helpers
    tags = [str(t) for t in np.load(os.path.join(REPO, "tests", "golden", "miou_run.npz"),
                                    allow_pickle=False)["hip_build"]]
    build = helpers.kernel_build_id()
    assert tags.count(build) >= 32, f"build id {build} is carried by {tags.count(build)} recorded runs"
