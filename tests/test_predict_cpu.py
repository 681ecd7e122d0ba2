"""CPU: the prediction add-on (include/mdil_predict.h, mdil_ss_amd/predict.py) -- the library
exports exactly what its header declares, the command line's defaults, the palettes, the refusal of
host tensors, and the rule the add-on exists under: it leaves the training path's build id alone."""
import os

import pytest
import torch

from tests.helpers import declared_names, dynamic_exports

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tests/test_miou_parity.py counts only recorded mIoU runs that carry the id of the build under
# test; this is the id the recorded runs in tests/golden/miou_run.npz carry.
RECORDED_BUILD_ID = "dfd5957e7955"


def test_library_exports_exactly_the_declared_symbols():
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _predict_lib
    lib = _predict_lib.load()
    names = declared_names("mdil_predict.h")
    assert names == ["mdil_predict_head", "mdil_predict_last_error", "mdil_predict_version"]
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/mdil_predict.h but not exported"
    assert sorted(_predict_lib.EXPORTS) == names
    assert dynamic_exports(_predict_lib.LIB_PATH) == names
    assert lib.mdil_predict_version() >= 100


def test_library_refuses_bad_arguments_without_a_device():
    """Argument checks come before the launch: class count, NULL pointers, a colour map without
    a palette, alignment."""
    from mdil_ss_amd import _predict_lib
    lib = _predict_lib.load()
    ok = dict(x=4096, w=8192, b=12288, N=1, H=2, W=2, nc=20, pal=16384, lab=20480, col=24576, conf=28672)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mdil_predict_head(a["x"], a["w"], a["b"], a["N"], a["H"], a["W"], a["nc"], a["pal"],
                                     a["lab"], a["col"], a["conf"], None)
    for bad, text in ((dict(nc=1), b"nc=1"), (dict(nc=33), b"nc=33"), (dict(x=None), b"bad argument"),
                      (dict(lab=None), b"bad argument"), (dict(W=0), b"bad argument"),
                      (dict(pal=None), b"palette"), (dict(x=4100), b"alignment"),
                      (dict(conf=28676), b"alignment"), (dict(col=24577), b"alignment")):
        assert call(**bad) == -1, bad
        assert text in lib.mdil_predict_last_error(), (bad, lib.mdil_predict_last_error())


def test_parser_defaults():
    from mdil_ss_amd import predict as P
    p = P.build_parser()
    a = p.parse_args(["--state", "ckpt.pth.tar", "--num-classes", "20", "20", "27", "--task", "2",
                      "--images", "in", "--out", "maps"])
    assert (a.state, a.num_classes, a.task, a.images, a.out) == ("ckpt.pth.tar", [20, 20, 27], 2, "in", "maps")
    assert (a.height, a.width, a.batch_size) == (512, 1024, 6)
    assert (a.synthetic, a.colour, a.confidence, a.palette) == (0, False, False, None)
    b = p.parse_args(["--state", "c", "--num-classes", "20", "--task", "0", "--synthetic", "3", "--out", "o",
                      "--colour", "--confidence", "--palette", "p.json", "--height", "64", "--width", "128",
                      "--batch-size", "2"])
    assert (b.synthetic, b.images, b.colour, b.confidence, b.palette) == (3, None, True, True, "p.json")
    assert (b.height, b.width, b.batch_size) == (64, 128, 2)
    for argv in (["--state", "c", "--num-classes", "20", "--task", "0", "--out", "o"],               # no source
                 ["--state", "c", "--num-classes", "20", "--task", "0", "--out", "o", "--images", "d",
                  "--synthetic", "2"]):                                                              # two
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    assert callable(P.main)


def test_default_palettes():
    from mdil_ss_amd import predict as P
    from mdil_ss_amd.transform import colormap, colormap_cityscapes
    for nc in (20, 27):
        pal = P.default_palette(nc)
        assert isinstance(pal, torch.Tensor) and pal.dtype == torch.uint8 and tuple(pal.shape) == (nc, 3)
        assert pal.is_contiguous()
    p20 = P.default_palette(20)
    assert p20[19].tolist() == [0, 0, 0]
    assert p20[0].tolist() == [128, 64, 128] and p20[13].tolist() == [0, 0, 142]      # road, car
    assert torch.equal(p20[:19], torch.from_numpy(colormap_cityscapes(19)))
    p27 = P.default_palette(27)
    assert torch.equal(p27, torch.from_numpy(colormap(27)))
    assert p27[0].tolist() == [0, 0, 0] and p27[1].tolist() == [128, 0, 0] and p27[2].tolist() == [0, 128, 0]
    assert len({tuple(r) for r in p27.tolist()}) == 27


def test_predict_refuses_cpu_tensors():
    from mdil_ss_amd import predict as P
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    x, w, b = torch.zeros(1, 2, 2, 16), torch.zeros(16, 20, 2, 2), torch.zeros(20)
    with pytest.raises(RuntimeError, match="features must be a contiguous float32 device tensor.*no CPU fallback"):
        P.predict_head(x, w, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.predict(Net([20], 1, 0), torch.zeros(1, 3, 32, 64), 0)


def test_training_build_id_is_untouched():
    from tests import helpers
    assert helpers.kernel_build_id() == RECORDED_BUILD_ID
