"""CPU: the ensemble add-on (include/mdil_ensemble.h, mdil_ss_amd/ensemble.py) -- the library exports
exactly what its header declares and the three other libraries keep their names, the fp64 reference
alone stays within the cap of excluded pixels for every case with the constants the kernel's header
states, every argument check answers before any launch, the command line's defaults and refusals,
the refusal of host tensors, and the rule every add-on exists under: the training path's build id
stays where the recorded runs have it."""
import os

import numpy as np
import pytest
import torch

from tests import ensemble_reference as R
from tests.helpers import declared_names, dynamic_exports

REPO = R.REPO
NAMES = ["mdil_ensemble_head", "mdil_ensemble_last_error", "mdil_ensemble_version"]


def test_library_exports_exactly_the_declared_symbols():
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _ensemble_lib, _fullres_lib, _lib, _predict_lib
    lib = _ensemble_lib.load()
    assert declared_names("mdil_ensemble.h") == NAMES
    for n in NAMES:
        assert hasattr(lib, n), f"{n} declared in include/mdil_ensemble.h but not exported"
    assert sorted(_ensemble_lib.EXPORTS) == NAMES
    assert dynamic_exports(_ensemble_lib.LIB_PATH) == NAMES
    assert lib.mdil_ensemble_version() >= 100
    # the other three keep their names
    assert dynamic_exports(_fullres_lib.LIB_PATH) == ["mdil_fullres_head", "mdil_fullres_last_error",
                                                       "mdil_fullres_version"]
    assert dynamic_exports(_predict_lib.LIB_PATH) == ["mdil_predict_head", "mdil_predict_last_error",
                                                       "mdil_predict_version"]
    assert set(_lib.EXPORTS) <= set(dynamic_exports(_lib.LIB_PATH))


def test_header_states_the_constants():
    k, cs = R.header_constants()
    assert k <= R.K_MAX and cs <= R.CS_MAX
    hdr = open(os.path.join(REPO, "include", "mdil_ensemble.h")).read()
    for text in ("#define MDIL_ENSEMBLE_MAX_VIEWS 8", "#define MDIL_ENSEMBLE_MODE_PROB  0",
                 "#define MDIL_ENSEMBLE_MODE_LOGIT 1",
                 "typedef struct { const float* x; int H; int W; int mirrored; } mdil_ensemble_view;"):
        assert text in hdr, text


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("index", range(len(R.CASES)))
@pytest.mark.parametrize("nc", R.CLASSES)
def test_reference_alone_stays_within_the_cap(nc, index, mode):
    """The exclusion is a property of the reference and of the header's two constants; it must not
    swallow the cases."""
    k, cs = R.header_constants()
    assert k <= R.K_MAX and cs <= R.CS_MAX
    excluded = R.case(nc, index, mode)[7]
    n_ex = int(excluded.sum())
    print(f"nc {nc} case {index} {mode}: {n_ex} of {excluded.numel()} excluded (cap {R.cap(excluded.numel())})")
    assert n_ex <= R.cap(excluded.numel())


@pytest.mark.parametrize("mode", R.MODES)
def test_reference_alone_stays_within_the_cap_bounded_grid_case(mode):
    excluded = R.case(R.BIG_NC, -1, mode)[7]
    assert excluded.numel() == 2102275
    print(f"bounded-grid case {mode}: {int(excluded.sum())} of {excluded.numel()} excluded")
    assert int(excluded.sum()) <= R.cap(excluded.numel())


OK = dict(views=((4096, 2, 2, 0), (8192, 3, 3, 1)), n=None, w=12288, b=16384, N=1, nc=20, Ho=8, Wo=8, mode=0,
          ids=20480, pal=24576, tgt=28672, ign=19, lab=32768, col=36864, cf=40960, conf=45056, bad=49152)


def _call(lib, **kw):
    from mdil_ss_amd import _ensemble_lib
    a = dict(OK, **kw)
    table = _ensemble_lib.view_table(a["views"]) if a["views"] is not None else None
    n = len(a["views"]) if a["n"] is None else a["n"]
    return lib.mdil_ensemble_head(table, n, a["w"], a["b"], a["N"], a["nc"], a["Ho"], a["Wo"], a["mode"], a["ids"],
                                  a["pal"], a["tgt"], a["ign"], a["lab"], a["col"], a["cf"], a["conf"], a["bad"],
                                  None)


V = (4096, 2, 2, 0)


@pytest.mark.parametrize("bad, text", [
    (dict(views=()), b"nviews=0"), (dict(views=(V,) * 9), b"nviews=9"), (dict(n=-1), b"nviews=-1"),
    (dict(nc=1), b"nc=1"), (dict(nc=33), b"nc=33"), (dict(mode=2), b"mode=2"), (dict(mode=-1), b"mode=-1"),
    (dict(views=None, n=2), b"bad argument"), (dict(w=None), b"bad argument"), (dict(b=None), b"bad argument"),
    (dict(lab=None), b"bad argument"), (dict(N=0), b"bad argument"), (dict(Ho=0), b"bad argument"),
    (dict(Wo=-3), b"bad argument"),
    (dict(views=(V, (None, 2, 2, 0))), b"view 1: bad argument"), (dict(views=((4096, 0, 2, 0),)), b"view 0: bad argument"),
    (dict(views=(V, V, (4096, 2, -1, 1))), b"view 2: bad argument"),
    (dict(Ho=(1 << 22) + 1), b"above 4194304"), (dict(Wo=(1 << 22) + 1), b"above 4194304"),
    (dict(N=1 << 20, Ho=1 << 22, Wo=1 << 22), b"too large"),
    (dict(N=1 << 30, views=((4096, 1 << 20, 1 << 20, 0),)), b"view 0: too large"),
    (dict(views=(V, (4096, (1 << 29) + 1, 1, 0))), b"view 1: too large"),
    (dict(views=(V, (4100, 2, 2, 0))), b"view 1: alignment"),
    (dict(pal=None), b"palette"),
    (dict(conf=None), b"a target needs"), (dict(bad=None), b"a target needs"),
    (dict(ign=-2), b"ignore_index=-2"), (dict(ign=256), b"ignore_index=256"),
    (dict(lab=32770), b"alignment"), (dict(col=36865), b"alignment"), (dict(cf=40962), b"alignment"),
    (dict(tgt=28674), b"alignment"), (dict(conf=45060), b"alignment"), (dict(bad=49156), b"alignment"),
])
def test_library_refuses_bad_arguments_without_a_device(bad, text):
    """Argument checks come before the launch, so fake pointers never reach a device."""
    from mdil_ss_amd import _ensemble_lib
    lib = _ensemble_lib.load()
    assert _call(lib, **bad) == -1, bad
    assert text in lib.mdil_ensemble_last_error(), (bad, lib.mdil_ensemble_last_error())


BASE = ["--state", "ckpt.pth.tar", "--num-classes", "20", "20", "27", "--task", "2"]


def test_parser_defaults():
    from mdil_ss_amd import ensemble as E
    from mdil_ss_amd import fullres as FR
    p = E.build_parser()
    a = p.parse_args(BASE + ["--dataset", "IDD", "--score"])
    assert (a.state, a.num_classes, a.task, a.dataset, a.subset) == ("ckpt.pth.tar", [20, 20, 27], 2, "IDD", "val")
    assert (a.height, a.width, a.batch_size) == (512, 1024, 6)
    assert (a.score, a.json, a.out, a.colour, a.label_ids, a.synthetic) == (True, None, None, False, None, 0)
    assert (a.native_height, a.native_width) == (1024, 2048)
    assert (a.scales, a.flip, a.mode, a.confidence) == ([1.0], False, "prob", False)
    assert all(hasattr(a, k) for k in ("cs_datadir", "bdd_datadir", "idd_datadir", "cache_resized"))
    # every flag of fullres is a flag here, with the same default
    f = FR.build_parser().parse_args(BASE + ["--dataset", "IDD", "--score"])
    assert all(getattr(a, k) == v for k, v in vars(f).items())
    b = p.parse_args(BASE + ["--synthetic", "3", "--native-height", "96", "--native-width", "200", "--height", "64",
                             "--width", "128", "--batch-size", "2", "--score", "--json", "r.json", "--out", "maps",
                             "--colour", "--confidence", "--scales", "0.75", "1", "1.25", "--flip", "--mode", "logit"])
    assert (b.synthetic, b.dataset, b.native_height, b.native_width) == (3, None, 96, 200)
    assert (b.scales, b.flip, b.mode, b.confidence, b.colour) == ([0.75, 1.0, 1.25], True, "logit", True, True)
    c = p.parse_args(BASE + ["--dataset", "BDD", "--score", "--scales", "0.5", "0.75", "1", "1.25", "--flip"])
    assert len(c.scales) * 2 == 8
    assert callable(E.main)


@pytest.mark.parametrize("argv, text", [
    (["--dataset", "BDD", "--score", "--scales", "0.5", "0.75", "1", "1.25", "1.5", "--flip"], "--scales with --flip"),
    (["--dataset", "BDD", "--score", "--scales"] + [str(0.5 + 0.1 * i) for i in range(9)], "at most 8"),
    (["--dataset", "BDD", "--score", "--scales", "1", "0.75", "1.0"], "--scales holds a duplicate"),
    (["--dataset", "BDD", "--score", "--scales", "1", "0"], "--scales must be positive"),
    (["--dataset", "BDD", "--score", "--scales", "-0.5"], "--scales must be positive"),
    (["--dataset", "BDD", "--score", "--scales", "nan"], "--scales must be positive"),
    (["--dataset", "BDD", "--score", "--confidence"], "--confidence needs --out"),
    (["--dataset", "BDD", "--score", "--mode", "mean"], "--mode"),
    (["--dataset", "cityscapes"], "nothing to do"),                      # fullres's own refusals hold too
    (["--dataset", "BDD", "--score", "--colour"], "--colour"),
])
def test_parser_refusals(argv, text, capsys):
    from mdil_ss_amd import ensemble as E
    with pytest.raises(SystemExit):
        E.build_parser().parse_args(BASE + argv)
    assert text in capsys.readouterr().err


def test_main_refuses_before_touching_the_gpu():
    from argparse import Namespace
    from mdil_ss_amd import ensemble as E
    ok = dict(score=True, out=None, colour=False, label_ids=None, json=None, synthetic=2, dataset=None, height=64,
              width=128, batch_size=2, native_height=96, native_width=200, confidence=False, flip=True)
    with pytest.raises(RuntimeError, match="at most 8"):
        E.main(Namespace(scales=[0.5, 0.75, 1.0, 1.25, 1.5], **ok))
    with pytest.raises(RuntimeError, match="duplicate"):
        E.main(Namespace(scales=[1.0, 1.0], **ok))
    with pytest.raises(RuntimeError, match="must be positive"):
        E.main(Namespace(scales=[1.0, -1.0], **ok))
    with pytest.raises(RuntimeError, match="nothing to do"):
        E.main(Namespace(score=False, out=None))


def test_scaled_size_is_a_multiple_of_eight():
    from mdil_ss_amd.ensemble import scaled_size
    assert [scaled_size(512, s) for s in (0.5, 0.75, 1.0, 1.25, 1.5, 2.0)] == [256, 384, 512, 640, 768, 1024]
    assert [scaled_size(1024, s) for s in (0.75, 1.25)] == [768, 1280]
    assert [scaled_size(64, s) for s in (0.75, 1.0, 1.25)] == [48, 64, 80]
    assert scaled_size(100, 1.0) == 104 and scaled_size(100, 0.9) == 88      # 12.5 -> 13, 11.25 -> 11
    assert scaled_size(64, 0.01) == 8 and scaled_size(3, 1.0) == 8           # at least 8
    for size in (64, 100, 513):
        for s in (0.3, 0.77, 1.0, 1.9):
            v = scaled_size(size, s)
            assert v % 8 == 0 and v >= 8 and abs(v - s * size) <= 4 + 8 * (s * size < 4)


def test_ensemble_refuses_cpu_tensors_and_mismatched_views():
    from mdil_ss_amd import ensemble as E
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    x, w, b = torch.zeros(1, 2, 2, 16), torch.zeros(16, 20, 2, 2), torch.zeros(20)
    with pytest.raises(RuntimeError, match=r"views\[0\] must be a contiguous float32 device tensor.*no CPU fallback"):
        E.ensemble_head([(x, False)], w, b, (8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.predict_ensemble(Net([20], 1, 0), [torch.zeros(1, 3, 32, 64)], 0, (64, 128))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.EnsembleMeter(20, 19).add([(x, False)], w, b, target=torch.zeros(1, 8, 8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="mode must be one of"):
        E.ensemble_head([(x, False)], w, b, (8, 8), mode="mean")
    with pytest.raises(RuntimeError, match="views holds 0 entries"):
        E.ensemble_head([], w, b, (8, 8))
    with pytest.raises(RuntimeError, match="views holds 9 entries"):
        E.ensemble_head([(x, False)] * 9, w, b, (8, 8))
    with pytest.raises(RuntimeError, match="views must be a sequence"):
        E.ensemble_head([x], w, b, (8, 8))
    with pytest.raises(RuntimeError, match="2 image tensors for 3 scales"):
        E.predict_ensemble(Net([20], 1, 0), [torch.zeros(1, 3, 32, 64)] * 2, 0, (64, 128), scales=(0.75, 1, 1.25))
    with pytest.raises(RuntimeError, match="10 views"):
        E.predict_ensemble(Net([20], 1, 0), [torch.zeros(1, 3, 32, 64)] * 5, 0, (64, 128), scales=(1, 2, 3, 4, 5),
                           flip=True)


def test_ensemble_refuses_mismatched_views():
    """Shapes are judged before the device, so these refusals need none."""
    from mdil_ss_amd import ensemble as E
    w, b = torch.zeros(16, 20, 2, 2), torch.zeros(20)
    views = [(torch.zeros(2, 2, 2, 16), False), (torch.zeros(3, 2, 2, 16), True)]
    with pytest.raises(RuntimeError, match=r"views\[1\] has N = 3, views\[0\] has N = 2"):
        E.ensemble_head(views, w, b, (8, 8))
    with pytest.raises(RuntimeError, match=r"views\[1\] must be NHWC features"):
        E.ensemble_head([views[0], (torch.zeros(2, 16, 2, 2), False)], w, b, (8, 8))


def test_training_build_id_is_untouched():
    from tests import helpers
    tags = [str(t) for t in np.load(os.path.join(REPO, "tests", "golden", "miou_run.npz"),
                                    allow_pickle=False)["hip_build"]]
    build = helpers.kernel_build_id()
    assert tags.count(build) >= 32, f"build id {build} is carried by {tags.count(build)} recorded runs"
