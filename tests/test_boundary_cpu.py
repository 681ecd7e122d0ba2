"""CPU: the boundary add-on (include/mdil_boundary.h, mdil_ss_amd/boundary.py) -- the library
exports exactly what its header declares, every argument check answers before any launch, the
command line's defaults and refusals, the published ratio -> width rule, the two spellings of the
numpy reference against each other, the meter's arithmetic on hand-written counters, the refusal of
host tensors, and the rule the add-on exists under: it leaves the training path's build id alone."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import boundary_reference as R
from tests.helpers import declared_names, dynamic_exports

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mdil_boundary_count", "mdil_boundary_last_error", "mdil_boundary_version", "mdil_boundary_workspace_bytes"]


def test_library_exports_exactly_the_declared_symbols():
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _boundary_lib, _fullres_lib
    lib = _boundary_lib.load()
    assert declared_names("mdil_boundary.h") == NAMES
    for n in NAMES:
        assert hasattr(lib, n), f"{n} declared in include/mdil_boundary.h but not exported"
    assert sorted(_boundary_lib.EXPORTS) == NAMES
    assert dynamic_exports(_boundary_lib.LIB_PATH) == NAMES
    assert lib.mdil_boundary_version() >= 100
    # the library it takes its label maps from keeps its three names
    assert dynamic_exports(_fullres_lib.LIB_PATH) == ["mdil_fullres_head", "mdil_fullres_last_error",
                                                       "mdil_fullres_version"]


def test_workspace_bytes():
    from mdil_ss_amd import _boundary_lib
    lib = _boundary_lib.load()
    assert lib.mdil_boundary_workspace_bytes(6, 1024, 2048) == 2 * 6 * 1024 * 2048
    assert lib.mdil_boundary_workspace_bytes(1, 1, 1) == 16               # 2 bytes, rounded up to 16
    assert lib.mdil_boundary_workspace_bytes(2, 37, 130) == (2 * 2 * 37 * 130 + 15) // 16 * 16
    for bad in ((0, 4, 4), (1, -1, 4), (1, 4, (1 << 22) + 1), (1 << 20, 1 << 11, 1 << 11)):
        assert lib.mdil_boundary_workspace_bytes(*bad) == -1, bad


OK = dict(pred=4096, tgt=8192, N=1, H=8, W=8, nc=20, widths=(1, 3), nw=None, ign=19, ws=12288, wsb=128, dp=16384,
          dt=20480, th=24576, ph=28672, bh=32768, conf=36864, badt=40960, badp=45056)


def _call(lib, **kw):
    a = dict(OK, **kw)
    widths = None if a["widths"] is None else (C.c_int * max(1, len(a["widths"])))(*a["widths"])
    nw = len(a["widths"]) if a["nw"] is None else a["nw"]
    return lib.mdil_boundary_count(a["pred"], a["tgt"], a["N"], a["H"], a["W"], a["nc"], widths, nw, a["ign"], a["ws"],
                                   a["wsb"], a["dp"], a["dt"], a["th"], a["ph"], a["bh"], a["conf"], a["badt"],
                                   a["badp"], None)


@pytest.mark.parametrize("bad, text", [
    (dict(nc=1), b"nc=1"), (dict(nc=33), b"nc=33"),
    (dict(pred=None), b"bad argument"), (dict(tgt=None), b"bad argument"), (dict(widths=None, nw=1), b"bad argument"),
    (dict(th=None), b"bad argument"), (dict(ph=None), b"bad argument"), (dict(bh=None), b"bad argument"),
    (dict(conf=None), b"bad argument"), (dict(badt=None), b"bad argument"), (dict(badp=None), b"bad argument"),
    (dict(N=0), b"bad argument"), (dict(H=0), b"bad argument"), (dict(W=-3), b"bad argument"),
    (dict(H=(1 << 22) + 1), b"above 4194304"), (dict(W=(1 << 22) + 1), b"above 4194304"),
    (dict(N=1 << 20, H=1 << 11, W=1 << 11), b"too large"), (dict(N=1 << 30, H=1 << 20, W=1 << 20), b"too large"),
    (dict(nw=0), b"n_widths=0"), (dict(widths=tuple(range(1, 10))), b"n_widths=9"),
    (dict(widths=(2, 2)), b"strictly increasing"), (dict(widths=(3, 1)), b"strictly increasing"),
    (dict(widths=(0,)), b"strictly increasing"), (dict(widths=(129,)), b"strictly increasing"),
    (dict(wsb=127), b"workspace of 128 bytes"), (dict(ws=None), b"workspace of 128 bytes"),
    (dict(pred=4098), b"alignment"), (dict(tgt=8193), b"alignment"), (dict(ws=12290), b"alignment"),
    (dict(dp=16385), b"alignment"), (dict(dt=20482), b"alignment"), (dict(th=24580), b"alignment"),
    (dict(ph=28676), b"alignment"), (dict(bh=32772), b"alignment"), (dict(conf=36868), b"alignment"),
    (dict(badt=40964), b"alignment"), (dict(badp=45060), b"alignment"),
    (dict(ign=-2), b"ignore_index=-2"), (dict(ign=256), b"ignore_index=256"),
])
def test_library_refuses_bad_arguments_without_a_device(bad, text):
    """Argument checks come before the launch, so fake pointers never reach a device."""
    from mdil_ss_amd import _boundary_lib
    lib = _boundary_lib.load()
    assert _call(lib, **bad) == -1, bad
    assert text in lib.mdil_boundary_last_error(), (bad, lib.mdil_boundary_last_error())


BASE = ["--num-classes", "20", "20", "27", "--task", "2"]
STATE = BASE + ["--state", "ckpt.pth.tar"]


def test_parser_defaults():
    from mdil_ss_amd import boundary as B
    p = B.build_parser()
    a = p.parse_args(STATE + ["--dataset", "IDD", "--score"])
    assert (a.state, a.num_classes, a.task, a.dataset, a.subset) == ("ckpt.pth.tar", [20, 20, 27], 2, "IDD", "val")
    assert (a.height, a.width, a.batch_size, a.native_height, a.native_width) == (512, 1024, 6, 1024, 2048)
    assert (a.score, a.json, a.out, a.synthetic, a.pred) == (True, None, None, 0, None)
    assert (a.ratio, a.widths) == (0.02, None)
    assert not hasattr(a, "colour") and not hasattr(a, "label_ids")
    assert all(hasattr(a, k) for k in ("cs_datadir", "bdd_datadir", "idd_datadir", "cache_resized"))
    b = p.parse_args(BASE + ["--pred", "maps", "--synthetic", "3", "--native-height", "96", "--native-width", "200",
                             "--widths", "1", "2", "4", "--score", "--json", "r.json", "--out", "bands"])
    assert (b.state, b.pred, b.widths, b.json, b.out, b.synthetic) == (None, "maps", [1, 2, 4], "r.json", "bands", 3)
    c = p.parse_args(STATE + ["--dataset", "BDD", "--out", "bands", "--ratio", "0.005"])
    assert (c.ratio, c.widths, c.score) == (0.005, None, False)
    assert callable(B.main)
    # the flags it shares keep their old surface in the command line they come from
    from mdil_ss_amd import fullres as F
    f = F.build_parser().parse_args(STATE + ["--dataset", "IDD", "--score"])
    assert (f.colour, f.label_ids) == (False, None)
    with pytest.raises(SystemExit):
        F.build_parser().parse_args(BASE + ["--dataset", "IDD", "--score"])          # --state stays required there


@pytest.mark.parametrize("argv", [
    STATE + ["--dataset", "cityscapes"],                                 # nothing to do
    STATE + ["--synthetic", "2"],                                        # the same, synthetic
    STATE + ["--score"],                                                 # no source of labels
    STATE + ["--dataset", "BDD", "--synthetic", "2", "--score"],         # two of them
    STATE + ["--dataset", "BDD", "--out", "o", "--json", "r.json"],      # a score file without --score
    STATE + ["--dataset", "BDD", "--score", "--pred", "maps"],           # --pred together with --state
    BASE + ["--dataset", "BDD", "--score"],                              # neither of them
    STATE + ["--dataset", "BDD", "--score", "--widths", "2", "2"],       # non-increasing widths
    STATE + ["--dataset", "BDD", "--score", "--widths", "4", "1"],
    STATE + ["--dataset", "BDD", "--score", "--widths", "0"],
    STATE + ["--dataset", "BDD", "--score", "--widths", "129"],
    STATE + ["--dataset", "BDD", "--score", "--widths", "1", "2", "3", "4", "5", "6", "7", "8", "9"],
    STATE + ["--dataset", "BDD", "--score", "--widths", "4", "--ratio", "0.02"],
    STATE + ["--dataset", "BDD", "--score", "--ratio", "0"],
    STATE + ["--dataset", "BDD", "--score", "--colour"],                 # flags of the map writers
    STATE + ["--dataset", "BDD", "--score", "--label-ids", "cityscapes"],
])
def test_parser_refusals(argv):
    from mdil_ss_amd import boundary as B
    with pytest.raises(SystemExit):
        B.build_parser().parse_args(argv)


def test_main_refuses_before_it_opens_anything():
    from argparse import Namespace
    from mdil_ss_amd import boundary as B
    with pytest.raises(RuntimeError, match="nothing to do"):
        B.main(Namespace(score=False, out=None))
    with pytest.raises(RuntimeError, match="give one of them"):
        B.main(Namespace(score=True, out=None, json=None, pred="maps", state="ckpt"))


def test_a_label_png_of_another_size_is_refused(tmp_path):
    from PIL import Image
    from mdil_ss_amd import boundary as B
    Image.fromarray(np.zeros((6, 9), dtype=np.uint8)).save(tmp_path / "a_label.png")
    assert B.read_label_png(str(tmp_path), "a", (6, 9)).shape == (6, 9)
    with pytest.raises(RuntimeError, match="a_label.png is 6 x 9, its label 9 x 6"):
        B.read_label_png(str(tmp_path), "a", (9, 6))
    with pytest.raises(RuntimeError, match="b_label.png not found"):
        B.read_label_png(str(tmp_path), "b", (6, 9))
    Image.fromarray(np.zeros((6, 9, 3), dtype=np.uint8)).save(tmp_path / "c_label.png")
    with pytest.raises(RuntimeError, match="not an 8-bit single-channel"):
        B.read_label_png(str(tmp_path), "c", (6, 9))


def test_ratio_gives_the_published_widths():
    from mdil_ss_amd import boundary as B
    assert B.ratio_width(0.02, 1024, 2048) == 46 == int(round(0.02 * (1024 ** 2 + 2048 ** 2) ** 0.5))
    assert B.ratio_width(0.02, 720, 1280) == 29 == int(round(0.02 * (720 ** 2 + 1280 ** 2) ** 0.5))
    assert B.ratio_width(0.02, 8, 8) == 1                                  # never below one pixel
    assert B.ratio_width(0.02, 1080, 1920) == 44
    with pytest.raises(RuntimeError, match=r"4096 x 8192 image is a width of 183 pixels"):
        B.ratio_width(0.02, 4096, 8192)


SMALL = [
    R.blocky((23, 31), 4, seed=1),
    R.blocky((40, 50), 3, seed=2, block=9),
    np.pad(np.full((9, 14), 7, dtype=np.uint8), 4, constant_values=2),     # a rectangle inside a frame
]


@pytest.mark.parametrize("k", range(len(SMALL)))
@pytest.mark.parametrize("cap", (1, 3, 12))
def test_the_two_reference_spellings_agree(k, cap):
    a, b = R.distance_brute(SMALL[k], cap), R.distance_erode(SMALL[k], cap)
    assert a.dtype == b.dtype == np.uint8 and np.array_equal(a, b)
    assert a.min() == 1 and a.max() <= cap + 1


def test_reference_distance_by_hand():
    """A 5 x 7 map of one label: the distance to the border; a one-pixel stripe: 1 everywhere on it."""
    want = np.array([[1, 1, 1, 1, 1, 1, 1], [1, 2, 2, 2, 2, 2, 1], [1, 2, 3, 3, 3, 2, 1], [1, 2, 2, 2, 2, 2, 1],
                     [1, 1, 1, 1, 1, 1, 1]], dtype=np.uint8)
    one = np.zeros((5, 7), dtype=np.uint8)
    assert np.array_equal(R.distance_erode(one, 8), want) and np.array_equal(R.distance_brute(one, 8), want)
    assert np.array_equal(R.distance_erode(one, 2), np.minimum(want, 3))
    one[:, 3] = 5
    d = R.distance_erode(one, 8)
    assert (d[:, 3] == 1).all() and d[2].tolist() == [1, 2, 1, 1, 1, 2, 1]
    assert R.bins(np.array([1, 2, 3, 4, 7, 8, 9]), [2, 3, 8]).tolist() == [0, 0, 1, 2, 2, 2, 3]


def _counters(nc, nb):
    from mdil_ss_amd import boundary as B
    return {k: torch.zeros(s, dtype=torch.int64) for k, s in B.counter_shapes(nc, nb).items()}


def test_score_on_hand_written_counters():
    """Three classes, the last one ignored, widths [2, 5]: class 1 is absent from both maps."""
    from mdil_ss_amd import boundary as B
    from mdil_ss_amd import fullres as F
    c = _counters(3, 3)
    c["target_hist"][0] = torch.tensor([4, 6, 10])
    c["pred_hist"][0] = torch.tensor([5, 5, 8])
    c["both_hist"][0] = torch.tensor([2, 3, 7])
    c["target_hist"][2] = torch.tensor([9, 9, 9])                          # the ignore class: never reported
    c["confusion"][0] = torch.tensor([[3, 1, 0], [0, 0, 0], [0, 0, 0]])
    c["confusion"][1] = torch.tensor([[4, 2, 0], [0, 0, 0], [0, 0, 0]])
    c["confusion"][2] = torch.tensor([[10, 0, 0], [0, 0, 0], [0, 0, 0]])
    rep = B.score(c, 3, 2, [2, 5])
    assert rep["widths"] == [2, 5] and len(rep["boundary_iou"]) == len(rep["trimap_iou"]) == 2
    # cumulative: T = 4, 10; P = 5, 10; B = 2, 5
    assert rep["boundary_iou"][0]["classes"] == [2 / (4 + 5 - 2 + 1e-15), 0.0]
    assert rep["boundary_iou"][1]["classes"] == [5 / (10 + 10 - 5 + 1e-15), 0.0]
    assert rep["boundary_iou"][1]["mean"] == (5 / (15 + 1e-15)) / 2
    # trimap: C_0 = [[3, 1], ...]: class 0 tp 3, fn 1; class 1 fp 1
    assert rep["trimap_iou"][0]["classes"] == [3 / (4 + 1e-15), 0.0]
    assert rep["trimap_iou"][1]["classes"] == [7 / (10 + 1e-15), 0.0]
    assert rep["interior_iou"]["classes"] == [10 / (10 + 1e-15), 0.0]
    assert rep["pixels"] == 20 and rep["counters"]["confusion"] == c["confusion"].tolist()
    # every bin together is the ordinary matrix, scored as ConfusionMeter scores it
    mean, per_class = F.ConfusionMeter(3, 2).iou(c["confusion"].sum(0))
    assert rep["mIoU"] == mean.item() and rep["iou_classes"] == per_class.tolist() == [17 / (20 + 1e-15), 0.0]
    # without an ignore class all three are reported
    assert len(B.score(c, 3, -1, [2, 5])["boundary_iou"][0]["classes"]) == 3
    with pytest.raises(RuntimeError, match="the ignore class must be the last one"):
        B.score(c, 3, 1, [2, 5])


def test_score_against_random_counters():
    from mdil_ss_amd import boundary as B
    from mdil_ss_amd import fullres as F
    nc, widths = 6, [1, 4, 9, 30]
    g = torch.Generator().manual_seed(4)
    c = _counters(nc, 5)
    for k in ("target_hist", "pred_hist", "confusion"):
        c[k] = torch.randint(0, 1000, c[k].shape, generator=g)
    c["both_hist"] = torch.minimum(c["target_hist"], c["pred_hist"]) // 2
    rep = B.score(c, nc, nc - 1, widths)
    meter = F.ConfusionMeter(nc, nc - 1)
    for k in range(4):
        T, P, Bh = (c[n][:, :k + 1].sum(1).double() for n in ("target_hist", "pred_hist", "both_hist"))
        want = (Bh / (T + P - Bh + 1e-15))[:nc - 1]
        assert rep["boundary_iou"][k]["classes"] == want.tolist() and rep["boundary_iou"][k]["mean"] == want.mean().item()
        mean, per_class = meter.iou(c["confusion"][:k + 1].sum(0))
        assert rep["trimap_iou"][k] == {"mean": mean.item(), "classes": per_class.tolist()}
    mean, per_class = meter.iou(c["confusion"][4])
    assert rep["interior_iou"] == {"mean": mean.item(), "classes": per_class.tolist()}
    assert rep["mIoU"] == meter.iou(c["confusion"].sum(0))[0].item()


def test_meter_without_data_and_its_modes():
    from mdil_ss_amd import boundary as B
    m = B.BoundaryMeter(20, 19)
    assert (m.ratio, m.widths, m.nb) == (0.02, None, 2)
    rep = m.report()
    assert rep["widths"] == [None] and rep["ratio"] == 0.02 and rep["widths_used"] == [] and rep["pixels"] == 0
    m = B.BoundaryMeter(20, 19, widths=[1, 2, 4])
    assert (m.ratio, m.widths, m.nb) == (None, [1, 2, 4], 4)
    assert m.report()["counters"]["confusion"] == torch.zeros(4, 20, 20, dtype=torch.int64).tolist()
    with pytest.raises(RuntimeError, match="widths or ratio, not both"):
        B.BoundaryMeter(20, 19, widths=[1], ratio=0.02)
    with pytest.raises(RuntimeError, match="strictly increasing"):
        B.BoundaryMeter(20, 19, widths=[3, 3])
    with pytest.raises(RuntimeError, match="must be positive"):
        B.BoundaryMeter(20, 19, ratio=0.0)


def test_boundary_refuses_cpu_tensors():
    from mdil_ss_amd import boundary as B
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    pred, target = torch.zeros(1, 8, 8, dtype=torch.uint8), torch.zeros(1, 8, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="pred must be a contiguous uint8 device tensor.*no CPU fallback in the "
                                           "boundary path"):
        B.boundary_count(pred, target, 20, [3], counters=_counters(20, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback in the boundary path"):
        B.BoundaryMeter(20, 19).add(pred, target)
    x, w, b = torch.zeros(1, 2, 2, 16), torch.zeros(16, 20, 2, 2), torch.zeros(20)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.BoundaryMeter(20, 19).add(x, w, b, target=target)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.BoundaryMeter(20, 19).add(Net([20], 1, 0), torch.zeros(1, 3, 32, 64), 0, target=target)
    with pytest.raises(RuntimeError, match="expects"):
        B.BoundaryMeter(20, 19).add(pred)


def test_training_build_id_is_untouched():
    """tests/test_miou_parity.py counts only the recorded mIoU runs that carry the id of the build
    under test and needs 32 of them: the add-on must leave that id where the recorded runs have it."""
    from mdil_ss_amd import boundary  # noqa: F401
    from tests import helpers
    tags = [str(t) for t in np.load(os.path.join(REPO, "tests", "golden", "miou_run.npz"),
                                    allow_pickle=False)["hip_build"]]
    build = helpers.kernel_build_id()
    assert tags.count(build) >= 32, f"build id {build} is carried by {tags.count(build)} recorded runs"
