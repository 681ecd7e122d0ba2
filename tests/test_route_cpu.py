"""CPU: the routing add-on (include/mdil_route.h, mdil_ss_amd/route.py) -- the library's exports and
argument checks (every refusal before any launch), the host arithmetic of the routes (the statistics
score against a hand-written loop, the tie / NaN / lowest-task rules of ``choose``, the entropy
normalisation, the ``misrouted_unscored`` rule), the command line's defaults and refusals, the
conditions on the reference that the GPU routing test stands on, and the rule the add-on exists
under: it leaves the training path's build id alone."""
import math
import os
import re

import numpy as np
import pytest
import torch

from mdil_ss_amd import route as P  # noqa: F401  (every test here stands on the feature, the reference's too)
from tests import route_reference as R
from tests.helpers import declared_names, dynamic_exports

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mdil_route_head", "mdil_route_head_workspace_bytes", "mdil_route_last_error", "mdil_route_stem",
         "mdil_route_stem_workspace_bytes", "mdil_route_version"]


# -------------------------------------------------------------------------------------- library
def test_library_exports_exactly_the_declared_symbols():
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _route_lib
    lib = _route_lib.load()
    assert declared_names("mdil_route.h") == NAMES
    for n in NAMES:
        assert hasattr(lib, n), f"{n} declared in include/mdil_route.h but not exported"
    assert sorted(_route_lib.EXPORTS) == NAMES
    assert dynamic_exports(_route_lib.LIB_PATH) == NAMES
    assert lib.mdil_route_version() >= 100
    assert (_route_lib.MIN_CLASSES, _route_lib.MAX_CLASSES) == (2, 32)


def test_build_loads_the_route_binding(monkeypatch):
    """``build()`` with ``make`` stubbed out: both Makefiles are asked for, and the route binding is loaded
    like the others; a dry run of the add-ons' Makefile compiles route_head.hip and links libmdil_route.so."""
    import subprocess
    import __graft_entry__ as g
    from mdil_ss_amd import _route_lib
    real_run, real_load, made, loads = subprocess.run, _route_lib.load, [], []
    monkeypatch.setattr(subprocess, "run", lambda cmd, **kw: made.append(cmd))
    monkeypatch.setattr(_route_lib, "load", lambda: (loads.append(1), real_load())[1])
    g.build()
    assert [os.path.basename(c[2]) for c in made] == ["csrc", "ext"] and loads
    dry = real_run(["make", "-n", "-B", "-C", os.path.join(REPO, "mdil_ss_amd", "ext")], check=True,
                   capture_output=True, text=True).stdout
    assert "-c route_head.hip -o route_head.o" in dry and "route_head.o -o ../libmdil_route.so" in dry
    assert P.STEM_CHANNELS == R.STEM_CHANNELS == _route_lib.STEM_CHANNELS == 16


def test_kernels_use_no_scratch(tmp_path):
    """The stem kernel reaches its register allocation through two empty ``asm`` statements (the weights stay in
    LDS, the 27 loads are issued together): what the compiler makes of them is pinned here.  No kernel of the
    library may spill to scratch, and the stem kernel keeps at least three waves per SIMD."""
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(REPO, "mdil_ss_amd", "ext", "route_head.hip")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden",
                          "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o",
                          str(tmp_path / "route_head.o")], check=True, capture_output=True, text=True).stderr
    kernels = re.findall(r"Function Name: (\S+)", out)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out)]
    waves = [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", out)]
    assert len(kernels) == len(scratch) == len(waves) == 3, out[-2000:]
    assert scratch == [0, 0, 0], dict(zip(kernels, scratch))
    assert all(w >= 3 for k, w in zip(kernels, waves) if "route_stem_kernel" in k), dict(zip(kernels, waves))


def test_workspace_sizes_depend_on_one_image_alone():
    """One row per work-group, and the work-groups of an image are min(ceil(H W / 256), 256): N only multiplies."""
    from mdil_ss_amd import _route_lib
    lib = _route_lib.load()
    for (Hi, Wi), bpi in (((2, 2), 1), ((32, 32), 1), ((32, 34), 2), ((34, 62), 3), ((512, 1024), 256), ((1024, 2048), 256)):
        for N in (1, 6):
            assert lib.mdil_route_stem_workspace_bytes(N, Hi, Wi) == N * bpi * 32 * 8
            assert lib.mdil_route_head_workspace_bytes(N, Hi // 2, Wi // 2, 20) == N * bpi * 3 * 8
    for bad in ((0, 4, 4), (1, 3, 4), (1, 4, 5), (1, 0, 4), (1, 4, -2), (1, 1 << 17, 1 << 17), (1 << 25, 2, 2)):
        assert lib.mdil_route_stem_workspace_bytes(*bad) == -1
    for bad in ((0, 4, 4, 20), (1, 4, 4, 1), (1, 4, 4, 33), (1, 1 << 20, 1 << 20, 20), (1 << 30, 1, 1, 20), (1 << 24, 1, 1, 20)):
        assert lib.mdil_route_head_workspace_bytes(*bad) == -1


STEM_OK = dict(img=4096, w=8192, b=12288, N=2, Hi=8, Wi=8, mom=16384, act=20480, nonf=24576, ws=28672, wsb=2 * 32 * 8)
HEAD_OK = dict(x=4096, w=8192, b=12288, N=2, H=4, W=4, nc=20, label=16384, conf=20480, ent=24576, margin=28672,
               scores=32768, nonf=36864, ws=40960, wsb=2 * 3 * 8)


def _stem(lib, **kw):
    a = dict(STEM_OK, **kw)
    return lib.mdil_route_stem(a["img"], a["w"], a["b"], a["N"], a["Hi"], a["Wi"], a["mom"], a["act"], a["nonf"], a["ws"],
                               a["wsb"], None)


def _head(lib, **kw):
    a = dict(HEAD_OK, **kw)
    return lib.mdil_route_head(a["x"], a["w"], a["b"], a["N"], a["H"], a["W"], a["nc"], a["label"], a["conf"], a["ent"],
                               a["margin"], a["scores"], a["nonf"], a["ws"], a["wsb"], None)


@pytest.mark.parametrize("call, bad, text", [
    (_stem, dict(img=None), b"bad argument"), (_stem, dict(w=None), b"bad argument"), (_stem, dict(b=None), b"bad argument"),
    (_stem, dict(N=0), b"bad argument"), (_stem, dict(Hi=0), b"bad argument"), (_stem, dict(Wi=-2), b"bad argument"),
    (_stem, dict(Hi=7), b"must be even"), (_stem, dict(Wi=9), b"must be even"),
    (_stem, dict(Wi=1 << 30), b"too large"), (_stem, dict(N=1 << 12, Hi=1 << 15, Wi=1 << 15), b"too large"),
    (_stem, dict(N=1, Hi=1 << 17, Wi=1 << 17), b"too large"), (_stem, dict(N=1 << 27, Hi=2, Wi=2), b"too large"),
    (_stem, dict(N=1 << 25, Hi=2, Wi=2), b"2^32 work-items"), (_head, dict(N=1 << 24, H=1, W=1), b"2^32 work-items"),
    (_stem, dict(mom=None, act=None, nonf=None), b"nothing to write"),
    (_stem, dict(img=4098), b"alignment"), (_stem, dict(w=8193), b"alignment"), (_stem, dict(b=12290), b"alignment"),
    (_stem, dict(act=20488), b"alignment"), (_stem, dict(mom=16388), b"alignment"), (_stem, dict(nonf=24580), b"alignment"),
    (_stem, dict(ws=28676), b"alignment"),
    (_stem, dict(ws=None), b"need a workspace"), (_stem, dict(wsb=2 * 32 * 8 - 8), b"need a workspace"),
    (_stem, dict(N=3), b"need a workspace"),
    (_head, dict(nc=1), b"nc=1"), (_head, dict(nc=33), b"nc=33"),
    (_head, dict(x=None), b"bad argument"), (_head, dict(w=None), b"bad argument"), (_head, dict(b=None), b"bad argument"),
    (_head, dict(N=0), b"bad argument"), (_head, dict(H=-1), b"bad argument"), (_head, dict(W=0), b"bad argument"),
    (_head, dict(W=1 << 30), b"too large"), (_head, dict(N=1 << 20, H=1 << 10, W=1 << 10), b"too large"),
    (_head, dict(N=1, H=1 << 16, W=1 << 16), b"too large"),
    (_head, dict(label=None, conf=None, ent=None, margin=None, scores=None, nonf=None), b"nothing to write"),
    (_head, dict(x=4100), b"alignment"), (_head, dict(label=16385), b"alignment"), (_head, dict(conf=20482), b"alignment"),
    (_head, dict(ent=24577), b"alignment"), (_head, dict(margin=28674), b"alignment"), (_head, dict(scores=32772), b"alignment"),
    (_head, dict(nonf=36868), b"alignment"), (_head, dict(ws=40964), b"alignment"),
    (_head, dict(ws=None), b"need a workspace"), (_head, dict(wsb=2 * 3 * 8 - 8), b"need a workspace"),
    (_head, dict(H=17, W=16), b"need a workspace"),
])
def test_library_refuses_bad_arguments_without_a_device(call, bad, text):
    """Argument checks come before the launch, so fake pointers never reach a device."""
    from mdil_ss_amd import _route_lib
    lib = _route_lib.load()
    assert call(lib, **bad) == -1, bad
    assert text in lib.mdil_route_last_error(), (bad, lib.mdil_route_last_error())


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from mdil_ss_amd import route as P
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    img, w, b = torch.zeros(1, 3, 4, 4), torch.zeros(13, 3, 3, 3), torch.zeros(13)
    with pytest.raises(RuntimeError, match="images must be a contiguous float32 device tensor.*no CPU fallback in the "
                                           "routing path"):
        P.stem_moments(img, w, b)
    x, hw, hb = torch.zeros(1, 2, 2, 16), torch.zeros(16, 20, 2, 2), torch.zeros(20)
    with pytest.raises(RuntimeError, match="features must be a contiguous float32 device tensor.*no CPU fallback in the "
                                           "routing path"):
        P.route_head(x, hw, hb)
    model = Net([20, 20], 2, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback in the routing path"):
        P.Router(model, "stats").choose(img)
    with pytest.raises(RuntimeError, match="by must be one of"):
        P.Router(model, "loudest")
    for tasks in ([0, 0], [2], [], [-1]):
        with pytest.raises(RuntimeError, match="tasks must be distinct and within 0 to 1"):
            P.Router(model, "entropy", tasks)
    assert P.Router(model, "margin").tasks == [0, 1] and P.Router(model, "margin", [1]).classes == [20]


# ------------------------------------------------------------------------------ host arithmetic
def test_stats_scores_match_a_hand_written_loop():
    from mdil_ss_amd import route as P
    g = torch.Generator().manual_seed(5)
    act = torch.randn(4, 16, 6, 10, generator=g, dtype=torch.float64) * 2 + torch.randn(1, 16, 1, 1, generator=g)
    mean = torch.randn(3, 16, generator=g, dtype=torch.float64)
    var = torch.rand(3, 16, generator=g, dtype=torch.float64) * 3 + 0.01
    m = R.moments(act)
    got = P.stats_scores(m, 60, mean, var, 1e-3)
    want = torch.tensor(R.stats_scores_loop(m, 60, mean, var, 1e-3), dtype=torch.float64)
    assert got.dtype == torch.float64 and tuple(got.shape) == (4, 3)
    assert torch.allclose(got, want, rtol=1e-12, atol=0)
    assert (got > 0).all()                                             # a KL divergence
    # an image whose moments ARE a domain's statistics scores 0 there
    own = torch.stack([60 * mean[1], 60 * (var[1] + mean[1] ** 2)], 1)[None]
    s = P.stats_scores(own, 60, mean, var, 1e-3)
    assert abs(float(s[0, 1])) < 1e-12 and int(P.choose(s)) == 1


def test_domain_stats_reads_the_stems_batchnorm():
    from mdil_ss_amd import route as P
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    model = Net([20, 20, 27], 3, 2)
    for t, bn in enumerate(model.encoder.initial_block.bn_ini):
        bn.running_mean.fill_(t + 0.5)
        bn.running_var.fill_(2 * t + 1.0)
    mean, var, eps = P.domain_stats(model, [2, 0])
    assert mean.dtype == var.dtype == torch.float64 and tuple(mean.shape) == tuple(var.shape) == (2, 16)
    assert mean[:, 0].tolist() == [2.5, 0.5] and var[:, 3].tolist() == [5.0, 1.0] and eps == 1e-3


def test_choose_rules():
    from mdil_ss_amd import route as P
    nan, inf = float("nan"), float("inf")
    s = torch.tensor([[3.0, 1.0, 2.0], [1.0, 1.0, 2.0], [2.0, 1.0, 1.0], [nan, 5.0, 4.0], [-inf, 5.0, 4.0],
                      [nan, inf, 7.0], [nan, nan, nan], [0.0, -1.0, nan]])
    assert P.choose(s).tolist() == [1, 0, 1, 2, 2, 2, 0, 1]
    assert P.choose(s.float()).dtype == torch.int64


def test_head_scores_and_the_entropy_normalisation():
    from mdil_ss_amd import route as P
    pixels = 50
    # a head that is uniform over its nc classes has entropy ln(nc): the normalised score is 1 for 20 and for 27
    for nc in (20, 27):
        sums = torch.tensor([[pixels * math.log(nc), pixels / nc, 0.0]], dtype=torch.float64)
        assert P.head_scores(sums, pixels, nc, "entropy").item() == pytest.approx(1.0, rel=1e-15)
        assert P.head_scores(sums, pixels, nc, "confidence").item() == pytest.approx(1 - 1 / nc, rel=1e-15)
        assert P.head_scores(sums, pixels, nc, "margin").item() == 1.0
    sure = torch.tensor([[0.0, float(pixels), float(pixels)]], dtype=torch.float64)
    assert [P.head_scores(sure, pixels, 20, by).item() for by in ("entropy", "confidence", "margin")] == [0.0, 0.0, 0.0]
    with pytest.raises(RuntimeError, match="head scores are"):
        P.head_scores(sure, pixels, 20, "stats")
    # a head with non-finite pixels on an image sums over fewer pixels: it scores inf there and loses the route
    sums = torch.tensor([[10.0, 20.0, 5.0], [10.0, 20.0, 5.0]], dtype=torch.float64)
    for by in ("entropy", "confidence", "margin"):
        with_nan = P.head_scores(sums, pixels, 20, by, torch.tensor([0, 3]))
        assert with_nan[0] == P.head_scores(sums, pixels, 20, by)[0] and with_nan[1] == float("inf")
        assert P.choose(torch.stack([with_nan, P.head_scores(sums * 2, pixels, 20, by)], 1)).tolist()[1] == 1


def test_misrouted_unscored_rule_by_hand():
    from mdil_ss_amd import route as P
    num_classes = [20, 20, 27]
    scored, lost = P.routed_set([0, 1, 2, 1, 2], 1, num_classes)
    assert scored == [True, True, False, True, False] and lost == 2      # task 0 has 20 classes too: scored
    scored, lost = P.routed_set([2, 2, 0], 2, num_classes)
    assert scored == [True, True, False] and lost == 1
    label = torch.tensor([[0, 1], [2, 2]], dtype=torch.uint8)
    target = torch.tensor([[0, 2], [2, 3]], dtype=torch.uint8)
    m, bad = P.confusion(label, target, 3, 2)                            # class 2 is the ignore class; 3 is out of range
    assert m.tolist() == [[1, 0, 0], [0, 0, 0], [0, 0, 0]] and int(bad) == 1


# ---------------------------------------------------------------------------------- command line
BASE = ["--state", "ckpt.pth.tar", "--num-classes", "20", "20", "27"]


def test_parser_defaults():
    from mdil_ss_amd import route as P
    a = P.build_parser().parse_args(BASE + ["--images", "pics", "--out", "maps"])
    assert (a.by, a.tasks, a.images, a.dataset, a.synthetic, a.task, a.score, a.out, a.colour, a.json) == \
        ("stats", None, "pics", None, 0, None, False, "maps", False, None)
    assert (a.height, a.width, a.batch_size, a.subset) == (512, 1024, 6, "val")
    b = P.build_parser().parse_args(BASE + ["--by", "entropy", "--tasks", "0", "2", "--dataset", "IDD", "--task", "2",
                                            "--score", "--json", "r.json"])
    assert (b.by, b.tasks, b.dataset, b.task, b.score, b.json) == ("entropy", [0, 2], "IDD", 2, True, "r.json")
    assert all(hasattr(b, k) for k in ("cs_datadir", "bdd_datadir", "idd_datadir", "cache_resized"))
    c = P.build_parser().parse_args(BASE + ["--synthetic", "4", "--task", "1", "--out", "o", "--colour"])
    assert (c.synthetic, c.task, c.colour) == (4, 1, True) and callable(P.main)


@pytest.mark.parametrize("argv, text", [
    (["--out", "o"], "one source of images"),
    (["--images", "p", "--synthetic", "2", "--out", "o"], "one source of images"),
    (["--images", "p", "--dataset", "BDD", "--out", "o"], "one source of images"),
    (["--images", "p", "--out", "o", "--task", "1"], "unknown domain"),
    (["--synthetic", "2", "--out", "o"], "need --task"),
    (["--dataset", "BDD", "--json", "j"], "need --task"),
    (["--synthetic", "2", "--task", "3", "--out", "o"], "--task 3"),
    (["--images", "p", "--out", "o", "--score"], "--score needs labels"),
    (["--synthetic", "2", "--task", "1", "--tasks", "0", "2", "--score", "--json", "j"], "not among --tasks"),
    (["--images", "p", "--out", "o", "--tasks", "0", "3"], "tasks must be distinct"),
    (["--images", "p", "--out", "o", "--tasks", "1", "1"], "tasks must be distinct"),
    (["--images", "p"], "nothing to do"),
    (["--images", "p", "--json", "j", "--colour"], "needs --out"),
    (["--images", "p", "--out", "o", "--batch-size", "0"], "must be positive"),
    (["--images", "p", "--out", "o", "--height", "511"], "must be even"),
    (["--images", "p", "--out", "o", "--by", "loudest"], "invalid choice"),
])
def test_parser_refusals(argv, text, capsys):
    from mdil_ss_amd import route as P
    with pytest.raises(SystemExit):
        P.build_parser().parse_args(BASE + argv)
    assert re.search(text, capsys.readouterr().err)


def test_main_refuses_before_it_opens_anything():
    from mdil_ss_amd import route as P
    args = P.build_parser().parse_args(BASE + ["--images", "p", "--out", "o"])
    args.score = True
    with pytest.raises(RuntimeError, match="--score needs labels"):
        P.main(args)
    args.score, args.images, args.synthetic = False, None, 3
    with pytest.raises(RuntimeError, match="need --task"):
        P.main(args)
    args.task, args.tasks = 1, [0, 0]
    with pytest.raises(RuntimeError, match="tasks must be distinct"):
        P.main(args)


# ------------------------------------------------- conditions of the GPU routing test's reference
def test_reference_stem_and_moments_by_hand():
    """The fp64 stem of tests/route_reference.py at one position against the definition written out."""
    images, w, b = R.stem_case((2, 24, 40))
    act, S = R.stem64(images, w, b)
    assert tuple(act.shape) == (2, 16, 12, 20) and tuple(S.shape) == (2, 13, 12, 20)
    x, wd = images.double(), w.double()
    for n, c, h, v in ((0, 0, 0, 0), (1, 12, 11, 19), (1, 5, 3, 0), (0, 7, 0, 9)):
        a, s = float(b[c]), abs(float(b[c]))
        for ci in range(3):
            for ky in range(3):
                for kx in range(3):
                    y, xx = 2 * h - 1 + ky, 2 * v - 1 + kx
                    if y >= 0 and xx >= 0:
                        a += float(x[n, ci, y, xx]) * float(wd[c, ci, ky, kx])
                        s += abs(float(x[n, ci, y, xx]) * float(wd[c, ci, ky, kx]))
        assert float(act[n, c, h, v]) == pytest.approx(a, rel=1e-12) and float(S[n, c, h, v]) == pytest.approx(s, rel=1e-12)
    assert torch.equal(act[:, 13:], torch.nn.functional.max_pool2d(x, 2))
    assert float(act[1, 14, 4, 6]) == float(x[1, 1, 8:10, 12:14].max())
    m = R.moments(act)
    assert tuple(m.shape) == (2, 16, 2) and float(m[1, 3, 1]) == pytest.approx(float((act[1, 3] ** 2).sum()), rel=1e-12)


def test_the_extra_stem_shapes_are_what_the_docstring_says():
    N, Hi, Wi = R.STEM_SHAPES[-1]
    pos = (Hi // 2) * (Wi // 2)
    assert 2 * 256 < pos < 3 * 256 and pos % 256 != 0 and len(R.STEM_SHAPES) == 5       # three work-groups, the last partial
    pos = (R.STRIDE_SHAPE[1] // 2) * (R.STRIDE_SHAPE[2] // 2)
    assert pos > 256 * 256 and ((R.STRIDE_SHAPE[1] - 2) // 2) ** 2 <= 256 * 256           # the loop strides, just


def test_photometric_reference_routes_every_image_with_a_clear_gap():
    """Two facts about the reference alone, which the GPU test rests on: with the seed-0 stem (the one
    ``HC.tiny_model`` builds) all 36 images route to their own domain, and the relative gap between
    the best and the second score is at least 0.1 (measured here: 0.31 at the worst image)."""
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    from tests import head_cases as HC
    c = R.photometric_case()
    assert tuple(c["images"].shape) == (36, 3, 16, 32) and c["true"].tolist() == [0] * 12 + [1] * 12 + [2] * 12
    assert torch.equal(c["choice"], c["true"])
    print(f"photometric reference: worst relative gap {float(c['gap'].min()):.4f}")
    assert float(c["gap"].min()) >= R.MIN_GAP
    w, b = R.stem_params()
    tiny = HC.tiny_model(torch.device("cpu")).encoder.initial_block.conv
    assert torch.equal(tiny.weight, w) and torch.equal(tiny.bias, b)
    torch.manual_seed(0)
    three = Net([20, 20, 20], 3, 2).encoder.initial_block.conv
    assert torch.equal(three.weight, w) and torch.equal(three.bias, b)


def test_training_build_id_is_untouched():
    """tests/test_miou_parity.py counts only the recorded mIoU runs that carry the id of the build
    under test and needs 32 of them: the add-on must leave that id where the recorded runs have it."""
    from mdil_ss_amd import route  # noqa: F401
    from tests import helpers
    tags = [str(t) for t in np.load(os.path.join(REPO, "tests", "golden", "miou_run.npz"),
                                    allow_pickle=False)["hip_build"]]
    build = helpers.kernel_build_id()
    assert tags.count(build) >= 32, f"build id {build} is carried by {tags.count(build)} recorded runs"
