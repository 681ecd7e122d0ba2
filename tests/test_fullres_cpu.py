"""CPU: the full-resolution add-on (include/mdil_fullres.h, mdil_ss_amd/fullres.py) -- the library
exports exactly what its header declares, every argument check answers before any launch, the
command line's defaults and refusals, the iouEval rule of ConfusionMeter, the Cityscapes label ids,
the refusal of host tensors, and the rule the add-on exists under: it leaves the training path's
build id alone."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import declared_names, dynamic_exports

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mdil_fullres_head", "mdil_fullres_last_error", "mdil_fullres_version"]


def test_library_exports_exactly_the_declared_symbols():
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _fullres_lib, _predict_lib
    lib = _fullres_lib.load()
    assert declared_names("mdil_fullres.h") == NAMES
    for n in NAMES:
        assert hasattr(lib, n), f"{n} declared in include/mdil_fullres.h but not exported"
    assert sorted(_fullres_lib.EXPORTS) == NAMES
    assert dynamic_exports(_fullres_lib.LIB_PATH) == NAMES
    assert lib.mdil_fullres_version() >= 100
    # the first add-on keeps its three names
    assert dynamic_exports(_predict_lib.LIB_PATH) == ["mdil_predict_head", "mdil_predict_last_error",
                                                       "mdil_predict_version"]


OK = dict(x=4096, w=8192, b=12288, N=1, H=2, W=2, nc=20, Ho=8, Wo=8, ids=16384, pal=20480, tgt=24576, ign=19,
          lab=28672, col=32768, conf=36864, bad=40960)


def _call(lib, **kw):
    a = dict(OK, **kw)
    return lib.mdil_fullres_head(a["x"], a["w"], a["b"], a["N"], a["H"], a["W"], a["nc"], a["Ho"], a["Wo"], a["ids"],
                                 a["pal"], a["tgt"], a["ign"], a["lab"], a["col"], a["conf"], a["bad"], None)


@pytest.mark.parametrize("bad, text", [
    (dict(nc=1), b"nc=1"), (dict(nc=33), b"nc=33"),
    (dict(x=None), b"bad argument"), (dict(w=None), b"bad argument"), (dict(b=None), b"bad argument"),
    (dict(lab=None), b"bad argument"), (dict(N=0), b"bad argument"), (dict(W=0), b"bad argument"),
    (dict(Ho=0), b"bad argument"), (dict(Wo=-3), b"bad argument"),
    (dict(Ho=(1 << 22) + 1), b"above 4194304"), (dict(Wo=(1 << 22) + 1), b"above 4194304"),
    (dict(N=1 << 20, Ho=1 << 22, Wo=1 << 22), b"too large"), (dict(N=1 << 30, H=1 << 20, W=1 << 20), b"too large"),
    (dict(H=(1 << 29) + 1), b"too large"),
    (dict(pal=None), b"palette"),
    (dict(conf=None), b"a target needs"), (dict(bad=None), b"a target needs"),
    (dict(ign=-2), b"ignore_index=-2"), (dict(ign=256), b"ignore_index=256"),
    (dict(x=4100), b"alignment"), (dict(lab=28674), b"alignment"), (dict(col=32769), b"alignment"),
    (dict(tgt=24578), b"alignment"), (dict(conf=36868), b"alignment"), (dict(bad=40964), b"alignment"),
])
def test_library_refuses_bad_arguments_without_a_device(bad, text):
    """Argument checks come before the launch, so fake pointers never reach a device."""
    from mdil_ss_amd import _fullres_lib
    lib = _fullres_lib.load()
    assert _call(lib, **bad) == -1, bad
    assert text in lib.mdil_fullres_last_error(), (bad, lib.mdil_fullres_last_error())


BASE = ["--state", "ckpt.pth.tar", "--num-classes", "20", "20", "27", "--task", "2"]


def test_parser_defaults():
    from mdil_ss_amd import fullres as F
    p = F.build_parser()
    a = p.parse_args(BASE + ["--dataset", "IDD", "--score"])
    assert (a.state, a.num_classes, a.task, a.dataset, a.subset) == ("ckpt.pth.tar", [20, 20, 27], 2, "IDD", "val")
    assert (a.height, a.width, a.batch_size) == (512, 1024, 6)
    assert (a.score, a.json, a.out, a.colour, a.label_ids, a.synthetic) == (True, None, None, False, None, 0)
    assert (a.native_height, a.native_width) == (1024, 2048)
    assert all(hasattr(a, k) for k in ("cs_datadir", "bdd_datadir", "idd_datadir", "cache_resized"))
    b = p.parse_args(BASE + ["--synthetic", "3", "--native-height", "96", "--native-width", "200", "--height", "64",
                             "--width", "128", "--batch-size", "2", "--score", "--json", "r.json", "--out", "maps",
                             "--colour", "--label-ids", "cityscapes"])
    assert (b.synthetic, b.dataset, b.native_height, b.native_width) == (3, None, 96, 200)
    assert (b.height, b.width, b.batch_size) == (64, 128, 2)
    assert (b.score, b.json, b.out, b.colour, b.label_ids) == (True, "r.json", "maps", True, "cityscapes")
    assert callable(F.main)


@pytest.mark.parametrize("argv", [
    BASE + ["--dataset", "cityscapes"],                                  # neither --score nor --out
    BASE + ["--synthetic", "2"],                                         # the same, synthetic
    BASE + ["--score"],                                                  # no source
    BASE + ["--dataset", "BDD", "--synthetic", "2", "--score"],          # two sources
    BASE + ["--dataset", "KITTI", "--score"],                            # unknown dataset
    BASE + ["--dataset", "BDD", "--score", "--colour"],                  # a colour map without --out
    BASE + ["--dataset", "BDD", "--score", "--label-ids", "cityscapes"],
    BASE + ["--dataset", "BDD", "--out", "o", "--json", "r.json"],       # a score file without --score
    ["--num-classes", "20", "--task", "0", "--dataset", "BDD", "--score"],   # no checkpoint
])
def test_parser_refusals(argv):
    from mdil_ss_amd import fullres as F
    with pytest.raises(SystemExit):
        F.build_parser().parse_args(argv)


def test_main_refuses_without_score_and_out():
    from argparse import Namespace
    from mdil_ss_amd import fullres as F
    with pytest.raises(RuntimeError, match="nothing to do"):
        F.main(Namespace(score=False, out=None))


def test_confusion_meter_iou_is_the_iouEval_rule():
    """Against the reference's formulas written out on one-hot tensors (iouEval.addBatch / getIoU):
    ignored pixels leave every count, the ignore class leaves the mean."""
    from mdil_ss_amd import fullres as F
    nc, ignore = 5, 4
    g = torch.Generator().manual_seed(3)
    target = torch.randint(0, nc, (4000,), generator=g)
    pred = torch.randint(0, nc, (4000,), generator=g)
    keep = target != ignore
    matrix = torch.bincount(target[keep] * nc + pred[keep], minlength=nc * nc).reshape(nc, nc)
    x = torch.nn.functional.one_hot(pred, nc)[:, :ignore].double()
    y = torch.nn.functional.one_hot(target, nc).double()
    ignores, y = y[:, ignore:ignore + 1], y[:, :ignore]
    tp = (x * y).sum(0)
    fp = (x * (1 - y - ignores)).sum(0)
    fn = ((1 - x) * y).sum(0)
    want = tp / (tp + fp + fn + 1e-15)
    meter = F.ConfusionMeter(nc, ignore)
    mean, per_class = meter.iou(matrix)
    assert per_class.dtype == torch.float64 and tuple(per_class.shape) == (ignore,)
    assert torch.equal(per_class, want) and mean.item() == want.mean().item()
    # a hand-made matrix without an ignore class: [[5, 1], [2, 3]] -> 5/8 and 3/6
    mean, per_class = F.ConfusionMeter(2, -1).iou(torch.tensor([[5, 1], [2, 3]]))
    assert per_class.tolist() == [5 / (8 + 1e-15), 3 / (6 + 1e-15)] and mean.item() == per_class.mean().item()
    # nothing added yet: an all-zero matrix on the host
    assert torch.equal(meter.matrix(), torch.zeros(nc, nc, dtype=torch.int64))


def test_cityscapes_label_ids():
    from mdil_ss_amd import fullres as F
    ids = F.LABEL_IDS["cityscapes"]
    assert isinstance(ids, bytes) and len(ids) == 20
    assert list(ids) == [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33, 0]
    t = F.load_label_ids("cityscapes", 20)
    assert t.dtype == torch.uint8 and t.tolist() == list(ids)
    with pytest.raises(RuntimeError, match="expected 27 integers"):
        F.load_label_ids("cityscapes", 27)
    with pytest.raises(RuntimeError, match="neither"):
        F.load_label_ids("no_such_dataset", 20)


def test_label_ids_from_a_file(tmp_path):
    import json
    from mdil_ss_amd import fullres as F
    f = tmp_path / "ids.json"
    f.write_text(json.dumps(list(range(100, 127))))
    assert F.load_label_ids(str(f), 27).tolist() == list(range(100, 127))
    f.write_text(json.dumps(list(range(250, 277))))
    with pytest.raises(RuntimeError, match=r"integers in \[0, 255\]"):
        F.load_label_ids(str(f), 27)


def test_resize_is_pil_bilinear():
    from PIL import Image
    from mdil_ss_amd import fullres as F
    arr = np.random.default_rng(0).integers(0, 256, (96, 200, 3), dtype=np.uint8)
    got = F.resize_image(arr, 64, 128)
    assert got.dtype == np.uint8 and got.shape == (64, 128, 3)
    assert np.array_equal(got, np.asarray(Image.fromarray(arr).resize((128, 64), Image.BILINEAR)))


def test_fullres_refuses_cpu_tensors():
    from mdil_ss_amd import fullres as F
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    x, w, b = torch.zeros(1, 2, 2, 16), torch.zeros(16, 20, 2, 2), torch.zeros(20)
    with pytest.raises(RuntimeError, match="features must be a contiguous float32 device tensor.*no CPU fallback"):
        F.fullres_head(x, w, b, (8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.predict_fullres(Net([20], 1, 0), torch.zeros(1, 3, 32, 64), 0, (64, 128))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.ConfusionMeter(20, 19).add(x, w, b, target=torch.zeros(1, 8, 8, dtype=torch.uint8))


def test_training_build_id_is_untouched():
    """tests/test_miou_parity.py counts only the recorded mIoU runs that carry the id of the build
    under test and needs 32 of them: the add-on must leave that id where the recorded runs have it."""
    from tests import helpers
    tags = [str(t) for t in np.load(os.path.join(REPO, "tests", "golden", "miou_run.npz"),
                                    allow_pickle=False)["hip_build"]]
    build = helpers.kernel_build_id()
    assert tags.count(build) >= 32, f"build id {build} is carried by {tags.count(build)} recorded runs"
