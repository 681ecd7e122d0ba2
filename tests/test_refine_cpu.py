"""CPU: the refinement add-on (include/mdil_refine.h, mdil_ss_amd/refine.py) -- the host reference
of tests/refine_reference.py on a case worked by hand and on its two degenerate settings, the
library's exports and argument checks (every refusal before any launch), the workspace sizes, the
wrappers' and the command line's refusals, and the rule the add-on exists under: it leaves the
training path's build id alone."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import refine_reference as R
from tests.helpers import declared_names, dynamic_exports

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mdil_refine_head", "mdil_refine_last_error", "mdil_refine_version", "mdil_refine_workspace_bytes"]


def params(**kw):
    from mdil_ss_amd.refine import RefineParams
    return RefineParams(**kw)


# ------------------------------------------------------------------------------------ reference
def test_reference_on_a_two_by_two_case_worked_by_hand():
    """A 2 x 2 grid, two classes, r = 1, d = 1, one step, a flat image (the colour term is 1).  Every
    pixel has its three neighbours inside: two at distance 1, one at distance sqrt(2); the window's
    normalisers run over all eight taps."""
    p = params(iterations=1, radius=1, dilation=1, w_appearance=2.0, w_smooth=0.5, theta_alpha=1.5, theta_beta=0.1,
               theta_gamma=0.8)
    l = [[[0.3, -1.0], [2.0, 0.1]], [[0.0, 0.4], [-0.5, 1.2]]]                    # [c][y][x]
    ea1, ea2 = math.exp(-1 / (2 * 1.5 ** 2)), math.exp(-2 / (2 * 1.5 ** 2))
    es1, es2 = math.exp(-1 / (2 * 0.8 ** 2)), math.exp(-2 / (2 * 0.8 ** 2))
    za, zs = 4 * ea1 + 4 * ea2, 4 * es1 + 4 * es2
    assert R.normalisers(p) == pytest.approx((za, zs), rel=1e-15)
    k1, k2 = 2.0 / za * ea1 + 0.5 / zs * es1, 2.0 / za * ea2 + 0.5 / zs * es2
    q0 = [[[math.exp(l[c][y][x]) / (math.exp(l[0][y][x]) + math.exp(l[1][y][x])) for x in range(2)]
           for y in range(2)] for c in range(2)]
    want = torch.zeros(1, 2, 2, 2, dtype=torch.float64)
    for y in range(2):
        for x in range(2):
            u = [l[c][y][x] + k1 * (q0[c][y][1 - x] + q0[c][1 - y][x]) + k2 * q0[c][1 - y][1 - x] for c in range(2)]
            for c in range(2):
                want[0, c, y, x] = math.exp(u[c]) / (math.exp(u[0]) + math.exp(u[1]))
    got = R.mean_field(torch.tensor([l], dtype=torch.float64), torch.full((1, 3, 2, 2), 0.25), p)
    assert torch.allclose(got, want, rtol=0, atol=1e-15)
    # a colour step between the columns: the horizontal and the diagonal neighbour lose their appearance part
    img = torch.zeros(1, 3, 2, 2)
    img[:, :, :, 1] = 1.0
    far = math.exp(-3.0 / (2 * 0.1 ** 2))
    kx, kd, ky = 2.0 / za * ea1 * far + 0.5 / zs * es1, 2.0 / za * ea2 * far + 0.5 / zs * es2, k1
    u = [l[c][0][0] + kx * q0[c][0][1] + ky * q0[c][1][0] + kd * q0[c][1][1] for c in range(2)]
    got = R.mean_field(torch.tensor([l], dtype=torch.float64), img, p)
    assert got[0, 0, 0, 0].item() == pytest.approx(math.exp(u[0]) / (math.exp(u[0]) + math.exp(u[1])), abs=1e-15)


def test_reference_degenerate_settings():
    g = torch.Generator().manual_seed(0)
    l = torch.randn(2, 5, 9, 14, generator=g, dtype=torch.float64) * 3
    img = R.block_image(2, 9, 14, 3)
    assert torch.equal(R.mean_field(l, img, params(iterations=0)), F.softmax(l, 1))
    for T in (1, 3, 16):
        got = R.mean_field(l, img, params(iterations=T, w_appearance=0.0, w_smooth=0.0))
        assert torch.equal(got, F.softmax(l, 1)), T
    moved = R.mean_field(l, img, params(iterations=2))
    assert (moved - F.softmax(l, 1)).abs().max() > 1e-3
    assert torch.allclose(moved.sum(1), torch.ones(2, 9, 14, dtype=torch.float64), atol=1e-14)
    assert len(R.taps(params())) == 120 and R.taps(params(radius=1))[0] == (-1, -1, 8.0)
    assert R.mean_field(l, img, params(iterations=2), torch.float32).dtype == torch.float32


def test_block_image_spreads_the_appearance_kernel():
    img = R.block_image(1, 32, 96, 1)
    assert img.dtype == torch.float32 and tuple(img.shape) == (1, 3, 32, 96)
    assert 0.0 <= float(img.min()) and float(img.max()) <= 1.0
    k = torch.exp(-((img[:, :, :, 1:] - img[:, :, :, :-1]) ** 2).sum(1) / (2 * 0.05 ** 2))
    assert float((k > 0.5).double().mean()) > 0.3 and float((k < 1e-3).double().mean()) > 0.03
    assert torch.equal(img, R.block_image(1, 32, 96, 1)) and not torch.equal(img, R.block_image(1, 32, 96, 2))


# -------------------------------------------------------------------------------------- library
def test_library_exports_exactly_the_declared_symbols():
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _refine_lib
    lib = _refine_lib.load()
    assert declared_names("mdil_refine.h") == NAMES
    for n in NAMES:
        assert hasattr(lib, n), f"{n} declared in include/mdil_refine.h but not exported"
    assert sorted(_refine_lib.EXPORTS) == NAMES
    assert dynamic_exports(_refine_lib.LIB_PATH) == NAMES
    assert lib.mdil_refine_version() >= 100
    assert (_refine_lib.MIN_CLASSES, _refine_lib.MAX_CLASSES) == (2, 32)
    assert (_refine_lib.MAX_ITERATIONS, _refine_lib.MAX_RADIUS, _refine_lib.MAX_DILATION) == (16, 5, 4)


Q_BYTES = 1 * 8 * 8 * 20 * 4                       # one Q buffer of the case below
OK = dict(x=4096, w=8192, b=12288, img=16384, N=1, H=4, W=4, nc=20, T=5, r=5, d=2, wa=3.0, ws=1.0, ta=8.0, tb=0.05,
          tg=3.0, wsp=1 << 20, wsb=2 * Q_BYTES, label=20480, conf=24576, q=28672, tgt=32768, ign=19, confusion=36864,
          badt=40960, changed=45056)


def _head(lib, **kw):
    a = dict(OK, **kw)
    return lib.mdil_refine_head(a["x"], a["w"], a["b"], a["img"], a["N"], a["H"], a["W"], a["nc"], a["T"], a["r"],
                                a["d"], a["wa"], a["ws"], a["ta"], a["tb"], a["tg"], a["wsp"], a["wsb"], a["label"],
                                a["conf"], a["q"], a["tgt"], a["ign"], a["confusion"], a["badt"], a["changed"], None)


INF, NAN = float("inf"), float("nan")


@pytest.mark.parametrize("bad, text", [
    (dict(nc=1), b"nc=1 outside [2, 32]"), (dict(nc=33), b"nc=33 outside [2, 32]"),
    (dict(T=-1), b"iterations=-1 outside [0, 16]"), (dict(T=17), b"iterations=17 outside [0, 16]"),
    (dict(r=0), b"radius=0 outside [1, 5]"), (dict(r=6), b"radius=6 outside [1, 5]"),
    (dict(d=0), b"dilation=0 outside [1, 4]"), (dict(d=5), b"dilation=5 outside [1, 4]"),
    (dict(ta=0.0), b"theta_alpha=0 must be finite and > 0"), (dict(ta=INF), b"theta_alpha=inf must be finite"),
    (dict(tb=-0.05), b"theta_beta=-0.05 must be finite and > 0"), (dict(tb=NAN), b"theta_beta="),
    (dict(tg=0.0), b"theta_gamma=0 must be finite and > 0"), (dict(tg=NAN), b"theta_gamma="),
    (dict(wa=-1.0), b"w_app=-1 must be finite and >= 0"), (dict(wa=INF), b"w_app=inf must be finite"),
    (dict(ws=-0.5), b"w_smooth=-0.5 must be finite and >= 0"), (dict(ws=NAN), b"w_smooth="),
    (dict(x=None), b"bad argument"), (dict(w=None), b"bad argument"), (dict(b=None), b"bad argument"),
    (dict(label=None), b"bad argument"), (dict(img=None), b"bad argument (image"),
    (dict(N=0), b"bad argument"), (dict(H=-1), b"bad argument"), (dict(W=0), b"bad argument"),
    (dict(confusion=None), b"a target needs"), (dict(badt=None), b"a target needs"),
    (dict(ign=-2), b"ignore_index=-2"), (dict(ign=256), b"ignore_index=256"),
    (dict(x=4100), b"alignment"), (dict(img=16386), b"alignment"), (dict(wsp=(1 << 20) + 8), b"alignment"),
    (dict(conf=24578), b"alignment"), (dict(q=28680), b"alignment"), (dict(confusion=36868), b"alignment"),
    (dict(badt=40964), b"alignment"), (dict(changed=45060), b"alignment"),
    (dict(W=1 << 29), b"too large"), (dict(N=1 << 20, H=1 << 10, W=1 << 10), b"too large"),
    (dict(wsp=None), b"need a workspace of 10240 bytes"), (dict(wsb=2 * Q_BYTES - 1), b"need a workspace of 10240 bytes"),
    (dict(T=1, wsb=Q_BYTES - 1), b"need a workspace of 5120 bytes"),
])
def test_library_refuses_bad_arguments_without_a_device(bad, text):
    """Argument checks come before the launch, so fake pointers never reach a device."""
    from mdil_ss_amd import _refine_lib
    lib = _refine_lib.load()
    assert _head(lib, **bad) == -1, bad
    assert text in lib.mdil_refine_last_error(), (bad, lib.mdil_refine_last_error())


def test_workspace_bytes():
    from mdil_ss_amd import _refine_lib
    from mdil_ss_amd import refine as RF
    lib = _refine_lib.load()
    one = 6 * 512 * 1024 * 20 * 4
    assert [lib.mdil_refine_workspace_bytes(6, 256, 512, 20, T) for T in (0, 1, 2, 5, 16)] == [0, one, 2 * one, 2 * one, 2 * one]
    assert lib.mdil_refine_workspace_bytes(1, 1, 1, 2, 1) == 32
    assert RF.workspace_bytes(1, 4, 4, 20, 2) == 2 * Q_BYTES
    for bad, text in ((dict(nc=33), b"nc=33"), (dict(T=17), b"iterations=17"), (dict(N=0), b"bad argument"),
                      (dict(W=1 << 29), b"too large")):
        a = dict(dict(N=1, H=4, W=4, nc=20, T=2), **bad)
        assert lib.mdil_refine_workspace_bytes(a["N"], a["H"], a["W"], a["nc"], a["T"]) == -1
        assert text in lib.mdil_refine_last_error()
    with pytest.raises(RuntimeError, match="mdil_refine_workspace_bytes failed.*nc=40"):
        RF.workspace_bytes(1, 4, 4, 40, 2)


# -------------------------------------------------------------------------------------- wrappers
def test_refine_refuses_cpu_tensors():
    from mdil_ss_amd import refine as RF
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    x, w, b, img = torch.zeros(1, 2, 2, 16), torch.zeros(16, 20, 2, 2), torch.zeros(20), torch.zeros(1, 3, 4, 4)
    with pytest.raises(RuntimeError, match="features must be a contiguous float32 device tensor.*no CPU fallback in "
                                           "the refinement path"):
        RF.refine_head(x, w, b, img)
    with pytest.raises(RuntimeError, match="images must be a float32 \\[N,3,H,W\\] device tensor.*no CPU fallback in "
                                           "the refinement path"):
        RF.refine(Net([20], 1, 0), torch.zeros(1, 3, 32, 64), 0)
    with pytest.raises(RuntimeError, match="no CPU fallback in the refinement path"):
        RF.RefineMeter(20, 19).add(Net([20], 1, 0), torch.zeros(1, 3, 32, 64), 0)


def test_wrappers_refuse_bad_parameters():
    from mdil_ss_amd import refine as RF
    assert RF.check_params(None) == RF.DEFAULTS == RF.RefineParams(5, 5, 2, 3.0, 1.0, 8.0, 0.05, 3.0)
    assert RF.check_params(params(iterations=0, radius=1, dilation=4, w_appearance=0, w_smooth=0)).iterations == 0
    x, w, b, img = torch.zeros(1, 2, 2, 16), torch.zeros(16, 20, 2, 2), torch.zeros(20), torch.zeros(1, 3, 4, 4)
    for kw, text in ((dict(iterations=17), "iterations 17 outside \\[0, 16\\]"), (dict(iterations=-1), "iterations -1"),
                     (dict(iterations=2.0), "iterations 2.0"), (dict(radius=0), "radius 0 outside \\[1, 5\\]"),
                     (dict(radius=6), "radius 6"), (dict(dilation=0), "dilation 0 outside \\[1, 4\\]"),
                     (dict(dilation=5), "dilation 5"), (dict(theta_alpha=0.0), "theta_alpha 0.0 must be finite and > 0"),
                     (dict(theta_beta=float("nan")), "theta_beta nan must be finite"),
                     (dict(theta_gamma=float("inf")), "theta_gamma inf must be finite"),
                     (dict(w_appearance=-1.0), "w_appearance -1.0 must be finite and >= 0"),
                     (dict(w_smooth=float("inf")), "w_smooth inf must be finite")):
        with pytest.raises(RuntimeError, match="mdil refine_head: " + text):
            RF.refine_head(x, w, b, img, params(**kw))                  # refused before the tensors are looked at
    with pytest.raises(RuntimeError, match="params must be a RefineParams"):
        RF.refine_head(x, w, b, img, (5, 5, 2))
    empty = RF.RefineMeter(20, 19).report()
    assert (empty["pixels"], empty["changed"], empty["changed_share"], empty["bad_targets"]) == (0, 0, 0.0, 0)
    assert empty["mIoU_plain"] == empty["mIoU_refined"] == 0.0 and len(empty["iou_classes_refined"]) == 19


# ---------------------------------------------------------------------------------- command line
BASE = ["--state", "ckpt.pth.tar", "--num-classes", "20", "20", "27", "--task", "2"]


def test_parser_defaults():
    from mdil_ss_amd import refine as RF
    a = RF.build_parser().parse_args(BASE + ["--images", "pics", "--out", "maps"])
    assert (a.images, a.dataset, a.synthetic, a.subset, a.out, a.colour, a.confidence, a.score, a.json) == \
        ("pics", None, 0, "val", "maps", False, False, False, None)
    assert (a.height, a.width, a.batch_size) == (512, 1024, 6)
    assert RF.params_of(a) == RF.DEFAULTS
    b = RF.build_parser().parse_args(BASE + ["--dataset", "BDD", "--subset", "val", "--score", "--json", "r.json",
                                             "--iterations", "3", "--radius", "2", "--dilation", "1", "--w-appearance",
                                             "4", "--w-smooth", "0", "--theta-alpha", "5", "--theta-beta", "0.1",
                                             "--theta-gamma", "2"])
    assert RF.params_of(b) == RF.RefineParams(3, 2, 1, 4.0, 0.0, 5.0, 0.1, 2.0) and b.score and b.json == "r.json"
    assert all(hasattr(b, k) for k in ("cs_datadir", "bdd_datadir", "idd_datadir", "cache_resized"))
    c = RF.build_parser().parse_args(BASE + ["--synthetic", "5", "--out", "maps", "--colour", "--confidence"])
    assert (c.synthetic, c.colour, c.confidence) == (5, True, True) and callable(RF.main)


@pytest.mark.parametrize("argv, text", [
    (["--out", "o"], "one source of images"),
    (["--images", "p", "--synthetic", "2", "--out", "o"], "one source of images"),
    (["--images", "p", "--dataset", "BDD", "--out", "o"], "one source of images"),
    (["--images", "p", "--out", "o", "--score"], "--score needs labels"),
    (["--synthetic", "2", "--out", "o", "--json", "r.json"], "--json writes the score"),
    (["--images", "p"], "nothing to do"),
    (["--synthetic", "2", "--score", "--colour"], "need --out DIR"),
    (["--synthetic", "2", "--score", "--confidence"], "need --out DIR"),
    (["--images", "p", "--out", "o", "--batch-size", "0"], "must be positive"),
    (["--images", "p", "--out", "o", "--iterations", "17"], "iterations 17 outside \\[0, 16\\]"),
    (["--images", "p", "--out", "o", "--radius", "6"], "radius 6 outside \\[1, 5\\]"),
    (["--images", "p", "--out", "o", "--dilation", "0"], "dilation 0 outside \\[1, 4\\]"),
    (["--images", "p", "--out", "o", "--theta-beta", "0"], "theta_beta 0.0 must be finite and > 0"),
    (["--images", "p", "--out", "o", "--w-smooth", "-1"], "w_smooth -1.0 must be finite and >= 0"),
])
def test_parser_refusals(argv, text, capsys):
    from mdil_ss_amd import refine as RF
    with pytest.raises(SystemExit):
        RF.build_parser().parse_args(BASE + argv)
    assert re.search(text, capsys.readouterr().err)


def test_main_refuses_before_it_opens_anything():
    from mdil_ss_amd import refine as RF
    args = RF.build_parser().parse_args(BASE + ["--images", "p", "--out", "o"])
    args.score = True
    with pytest.raises(RuntimeError, match="--score needs labels"):
        RF.main(args)
    args.score, args.task = False, 3
    with pytest.raises(RuntimeError, match="--task 3: the model has tasks 0 to 2"):
        RF.main(args)


def test_training_build_id_is_untouched():
    """tests/test_miou_parity.py counts only the recorded mIoU runs that carry the id of the build
    under test and needs 32 of them: the add-on must leave that id where the recorded runs have it."""
    from mdil_ss_amd import refine  # noqa: F401
    from tests import helpers
    tags = [str(t) for t in np.load(os.path.join(REPO, "tests", "golden", "miou_run.npz"),
                                    allow_pickle=False)["hip_build"]]
    build = helpers.kernel_build_id()
    assert tags.count(build) >= 32, f"build id {build} is carried by {tags.count(build)} recorded runs"
