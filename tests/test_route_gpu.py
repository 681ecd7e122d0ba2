"""GPU: the routing kernels (mdil_ss_amd/ext/route_head.hip) and the entry points over them
(mdil_ss_amd/route.py), against the fp64 reference of tests/route_reference.py.

Stem.  Shapes: the images of ``HC.SHAPES`` -- (1,2,2), (1,18,14), (2,24,40), (3,32,96) -- and
(2,34,62): 17 x 31 = 527 positions per image are three work-groups of 256 with 15 positions in the
last.  One more case, (1,514,514), has 66,049 positions: more than 256 work-groups of 256, so the
loop strides.  Tolerances are derived: the pool channels are exact; a conv channel is 27 FMA
roundings on an exact bias, so within gamma(27) S of the exact value, S = |b_c| + sum |x||w|; the
moments are held within the summed per-element bounds (tol for the first, 2 |a| tol + tol^2 for the
second) plus n 2^-53 sum |v| for the fp64 order, and within that order term alone of the kernel's own
activation summed exactly.

Head.  ``HC.CLASSES x HC.SHAPES`` with ``head_inputs``.  With S = max_c (|b| + sum |x||w|) of the pixel
and U = 2^-24:
    conf    K_CONF   U (1 + S)
    ent     K_ENT    U (1 + S) (1 + ent64)
    margin  K_MARGIN U (1 + S)
Each K is 4 x the worst per-pixel constant of the DENSE FP32 TORCH ROUTE on the same MI355X against
the same fp64 values over the 16 cases (stored fp32 logits from ``F.conv_transpose2d`` on the device,
``log_softmax``, the formulas): the kernel's exp, log and summation order differ from torch's by a
few ulps per term.  Measured (K_*_TORCH below; per case the tests print both routes' constants)."""
import functools
import itertools
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import head_cases as HC
from tests import route_reference as R
from tests.head_cases import CLASSES, SHAPES, U, as_bytes, gamma, nhwc

pytestmark = pytest.mark.gpu

# Worst per-pixel constants of the dense fp32 torch route measured on an MI355X over the 16 cases:
# conf 2.066 and margin 3.862 (nc 2, shape (3, 16, 48)), ent 2.740 (nc 27, shape (3, 16, 48)); per case
# 0.06 ... 2.07, 0.13 ... 2.74 and 0.11 ... 3.86.  The kernel's own constants over the same cases:
# conf 0.07 ... 0.73, ent 0.08 ... 1.18, margin 0.05 ... 0.95.  DESIGN.md, "Route".
K_CONF_TORCH = 2.066
K_ENT_TORCH = 2.740
K_MARGIN_TORCH = 3.862
K_CONF, K_ENT, K_MARGIN = 4 * K_CONF_TORCH, 4 * K_ENT_TORCH, 4 * K_MARGIN_TORCH
K_OF = {"ent": K_ENT, "conf": K_CONF, "margin": K_MARGIN}
COLUMNS = ("ent", "conf", "margin")                   # the columns of ``scores``


@pytest.fixture(scope="module")
def dev():
    return HC.device("routing")


def order_slack(v):
    """What an fp64 summation of the values ``v`` in any order may differ from their exact sum by."""
    return v.numel() * 2.0 ** -53 * v.abs().sum().item()


# ------------------------------------------------------------------------------------- the stem
@functools.lru_cache(maxsize=None)
def stem_reference(shape):
    """fp64 activation NHWC [N,H,W,16] and its per-element bound (0 on the pool channels); shared."""
    images, w, b = R.stem_case(shape)
    act, S = R.stem64(images, w, b)
    tol = torch.cat([gamma(27) * S, torch.zeros_like(act[:, 13:])], 1)
    return nhwc(act), nhwc(tol)


def run_stem(dev, shape, images=None, act=True, nonfinite=False):
    from mdil_ss_amd.route import stem_moments
    x, w, b = R.stem_case(shape)
    x = x if images is None else images
    nonf = torch.zeros(x.shape[0], dtype=torch.int64, device=dev) if nonfinite else None
    moments, a = stem_moments(x.to(dev), w.to(dev), b.to(dev), act=act, nonfinite=nonf)
    torch.cuda.synchronize()
    return {"moments": moments.cpu(), "act": None if a is None else a.cpu(), "nonfinite": None if nonf is None else nonf.cpu()}


@functools.lru_cache(maxsize=None)
def stem_full(dev, shape):
    return run_stem(dev, shape)


@pytest.mark.parametrize("shape", R.STEM_SHAPES + (R.STRIDE_SHAPE,))
def test_stem_activation(dev, shape):
    images, _, _ = R.stem_case(shape)
    ref, tol = stem_reference(shape)
    act = stem_full(dev, shape)["act"]
    assert act.dtype == torch.float32 and tuple(act.shape) == tuple(ref.shape)
    assert torch.equal(as_bytes(act[..., 13:]), as_bytes(nhwc(F.max_pool2d(images, 2))))     # bit-equal
    err = (act[..., :13].double() - ref[..., :13]).abs()
    print(f"stem {shape}: worst conv error / bound {(err / tol[..., :13]).max().item():.3f}")
    assert (err <= tol[..., :13]).all()


def check_moments(moments, act, ref, tol, channels=range(16)):
    """Both checks of the header for every image and the ``channels``."""
    assert moments.dtype == torch.float64 and tuple(moments.shape) == (ref.shape[0], 16, 2)
    worst = 0.0
    for n in range(ref.shape[0]):
        for c in channels:
            a64, t, a = ref[n, :, :, c].reshape(-1), tol[n, :, :, c].reshape(-1), act[n, :, :, c].reshape(-1).double()
            for j, (v64, bound, own) in enumerate(((a64, t, a), (a64 * a64, 2 * a64.abs() * t + t * t, a * a))):
                got = moments[n, c, j].item()
                limit = bound.sum().item() + order_slack(v64)
                assert abs(got - math.fsum(v64.tolist())) <= limit, (n, c, j)
                assert abs(got - math.fsum(own.tolist())) <= order_slack(own), (n, c, j)      # the reduction alone
                worst = max(worst, abs(got - math.fsum(v64.tolist())) / limit)
    return worst


@pytest.mark.parametrize("shape", R.STEM_SHAPES)
def test_stem_moments(dev, shape):
    ref, tol = stem_reference(shape)
    out = stem_full(dev, shape)
    print(f"stem {shape}: worst |moment - fp64| / bound {check_moments(out['moments'], out['act'], ref, tol):.3f}")


def test_stem_moments_where_the_loop_strides(dev):
    """(1,514,514): 66,049 positions, 256 work-groups that each make a second trip for some lanes.  Three
    channels (a conv channel, the last conv channel, a pool channel) keep the exact host sums cheap."""
    ref, tol = stem_reference(R.STRIDE_SHAPE)
    out = stem_full(dev, R.STRIDE_SHAPE)
    check_moments(out["moments"], out["act"], ref, tol, channels=(0, 12, 15))
    for j, v in enumerate((out["act"].double(), out["act"].double() ** 2)):                    # every channel: torch's own
        slack = 2 * v[0].numel() // 16 * 2.0 ** -53 * v.abs().sum((1, 2))                      # fp64 sum has the same bound
        assert ((out["moments"][:, :, j] - v.sum((1, 2))).abs() <= slack).all()


def test_stem_without_the_activation_gives_the_same_moments(dev):
    shape = (3, 32, 96)
    assert torch.equal(as_bytes(run_stem(dev, shape, act=False)["moments"]), as_bytes(stem_full(dev, shape)["moments"]))


def test_stem_counts_nonfinite_positions(dev):
    shape = (3, 32, 96)
    images = R.stem_case(shape)[0].clone()
    images[1, 2, 9, 11] = float("nan")                                  # odd row, odd column: four windows
    images[2, 0, 0, 0] = float("inf")
    out = run_stem(dev, shape, images=images, nonfinite=True)
    act64 = R.stem64(images, *R.stem_case(shape)[1:])[0]
    want = (~torch.isfinite(act64)).any(1).sum((1, 2))
    assert want.tolist() == [0, 4, 1] and out["nonfinite"].tolist() == want.tolist()
    clean = stem_full(dev, shape)
    assert torch.equal(as_bytes(out["moments"][0]), as_bytes(clean["moments"][0]))
    assert torch.isnan(out["moments"][1]).any() and not torch.isfinite(out["moments"][2, :, 0]).all()
    assert torch.isnan(out["act"][1, 4, 5, 15]) and torch.isnan(out["act"][1, 5, 6, :13]).all()   # the pool keeps a NaN


# ------------------------------------------------------------------------------------- the head
@functools.lru_cache(maxsize=None)
def head_reference(nc, shape):
    """fp64 conf, ent, margin [N,2H,2W] of a case and their per-pixel scales; shared, never modified."""
    x, w, b = HC.head_inputs(nc, shape)
    logits, S = HC.head64(x, w, b)
    conf, ent, margin = R.head_stats64(logits)
    scale = U * (1 + S.max(1)[0])
    return dict(conf=conf, ent=ent, margin=margin, tol_conf=scale, tol_ent=scale * (1 + ent), tol_margin=scale)


def run_head(dev, nc, shape, x=None, **kw):
    from mdil_ss_amd.route import route_head
    xx, w, b = HC.head_inputs(nc, shape)
    xx = xx if x is None else x
    kw.setdefault("maps", True)
    out = route_head(nhwc(xx).to(dev), w.to(dev), b.to(dev), **kw)
    torch.cuda.synchronize()
    return HC.host(out)


@functools.lru_cache(maxsize=None)
def head_full(dev, nc, shape):
    return run_head(dev, nc, shape)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nc", CLASSES)
def test_head_labels_are_predict_heads(dev, nc, shape):
    out = head_full(dev, nc, shape)
    assert out["label"].dtype == torch.uint8
    assert torch.equal(out["label"], HC.predict_labels(dev, *HC.head_inputs(nc, shape)))


def constant(got, want, tol):
    return ((got.double() - want).abs() / tol).max().item()


def torch_route(dev, nc, shape):
    """The dense fp32 route on the device: stored fp32 logits, log_softmax, the formulas -> host maps."""
    x, w, b = HC.head_inputs(nc, shape)
    logits = F.conv_transpose2d(x.to(dev), w.to(dev), b.to(dev), stride=2)
    conf, ent, margin = R.head_stats64(logits)
    return dict(conf=conf.cpu(), ent=ent.cpu(), margin=margin.cpu())


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nc", CLASSES)
def test_head_maps_match_fp64(dev, nc, shape):
    ref = head_reference(nc, shape)
    out = head_full(dev, nc, shape)
    theirs = torch_route(dev, nc, shape)
    for k in COLUMNS:
        assert out[k].dtype == torch.float32 and tuple(out[k].shape) == tuple(ref[k].shape) and torch.isfinite(out[k]).all()
    assert (out["conf"] > 0).all() and (out["conf"] <= 1).all() and (out["margin"] >= 0).all() and (out["margin"] <= 1).all()
    mine = {k: constant(out[k], ref[k], ref["tol_" + k]) for k in COLUMNS}
    torchs = {k: constant(theirs[k], ref[k], ref["tol_" + k]) for k in COLUMNS}
    print(f"nc {nc} shape {shape}: kernel conf {mine['conf']:.3f} ent {mine['ent']:.3f} margin {mine['margin']:.3f}; dense "
          f"fp32 torch route conf {torchs['conf']:.3f} ent {torchs['ent']:.3f} margin {torchs['margin']:.3f}")
    for k in COLUMNS:
        assert mine[k] <= K_OF[k], k


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nc", CLASSES)
def test_head_sums(dev, nc, shape):
    """Per image: within the summed per-pixel bounds of the fp64 sums, and within fp64 order error of
    the kernel's own maps summed exactly."""
    ref = head_reference(nc, shape)
    out = head_full(dev, nc, shape)
    scores = out["scores"]
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (shape[0], 3)
    worst = 0.0
    for n in range(shape[0]):
        for j, k in enumerate(COLUMNS):
            v64, own = ref[k][n].reshape(-1), out[k][n].reshape(-1).double()
            got = scores[n, j].item()
            assert abs(got - math.fsum(own.tolist())) <= order_slack(own), (n, k)
            bound = K_OF[k] * ref["tol_" + k][n].sum().item() + order_slack(v64)
            assert abs(got - math.fsum(v64.tolist())) <= bound, (n, k)
            worst = max(worst, abs(got - math.fsum(v64.tolist())) / ref["tol_" + k][n].sum().item())
    print(f"nc {nc} shape {shape}: worst |sum - fp64| / sum of per-pixel scales {worst:.3f}")


def test_head_nonfinite_pixels_are_counted_and_enter_no_sum(dev):
    nc, shape = 20, (2, 12, 20)
    x = HC.head_inputs(nc, shape)[0].clone()
    x[1, 9, 5, 7] = float("nan")                                       # every logit of its four output pixels
    nonf = torch.zeros(2, dtype=torch.int64, device=dev)
    out = run_head(dev, nc, shape, x=x, nonfinite=nonf)
    clean = head_full(dev, nc, shape)
    hit = torch.zeros(2, 24, 40, dtype=torch.bool)
    hit[1, 10:12, 14:16] = True
    assert nonf.cpu().tolist() == [0, 4]
    assert (out["label"][hit] == 0).all() and torch.equal(out["label"][~hit], clean["label"][~hit])
    assert torch.isnan(out["conf"][hit]).all()
    assert torch.equal(as_bytes(out["scores"][0]), as_bytes(clean["scores"][0]))
    for j, k in enumerate(COLUMNS):
        own = out[k][1][~hit[1]].double()
        assert abs(out["scores"][1, j].item() - math.fsum(own.tolist())) <= order_slack(own)


# -------------------------------------------------------------------------- batch independence
def test_stem_batch_independence_two_calls_and_a_side_stream(dev):
    """Image n's 32 numbers from the batch call equal, as bytes, those of a call on that image alone
    and of a call on the batch in reverse order; two calls agree; a side stream agrees."""
    for shape in ((3, 32, 96), (2, 34, 62)):
        images = R.stem_case(shape)[0]
        first = stem_full(dev, shape)["moments"]
        for n in range(shape[0]):
            alone = run_stem(dev, shape, images=images[n:n + 1].contiguous(), act=False)["moments"]
            assert torch.equal(as_bytes(alone[0]), as_bytes(first[n])), (shape, n)
        flipped = run_stem(dev, shape, images=images.flip(0).contiguous(), act=False)["moments"]
        assert torch.equal(as_bytes(flipped.flip(0)), as_bytes(first))
        assert torch.equal(as_bytes(run_stem(dev, shape)["moments"]), as_bytes(first))
        assert torch.equal(as_bytes(HC.side_stream(lambda: run_stem(dev, shape))["moments"]), as_bytes(first))


def test_head_batch_independence_two_calls_and_a_side_stream(dev):
    nc, shape = 27, (3, 16, 48)
    x = HC.head_inputs(nc, shape)[0]
    first = head_full(dev, nc, shape)
    for n in range(shape[0]):
        alone = run_head(dev, nc, shape, x=x[n:n + 1].contiguous(), maps=False)["scores"]
        assert torch.equal(as_bytes(alone[0]), as_bytes(first["scores"][n])), n
    flipped = run_head(dev, nc, shape, x=x.flip(0).contiguous(), maps=False)["scores"]
    assert torch.equal(as_bytes(flipped.flip(0)), as_bytes(first["scores"]))
    for out in (run_head(dev, nc, shape), HC.side_stream(lambda: run_head(dev, nc, shape))):
        for k in first:
            assert torch.equal(as_bytes(out[k]), as_bytes(first[k])), k


# ---------------------------------------------------------------------------------- guard bands
@pytest.mark.parametrize("shape", ((1, 2, 2), (2, 34, 62)))
def test_stem_writes_only_what_it_was_given(dev, shape):
    """One 0xA5-filled arena [guard | moments | guard | act | guard | nonfinite | guard]."""
    from mdil_ss_amd import _route_lib
    from mdil_ss_amd.route import stem_workspace_bytes
    lib = _route_lib.load()
    N, Hi, Wi = shape
    base = stem_full(dev, shape)
    x, w, b = (t.to(dev) for t in R.stem_case(shape))
    sizes = {"moments": N * 32 * 8, "act": N * (Hi // 2) * (Wi // 2) * 64, "nonfinite": N * 8}
    ws = torch.empty(stem_workspace_bytes(*shape) // 8, dtype=torch.float64, device=dev)
    combos = [c for r in (1, 2, 3) for c in itertools.combinations(sizes, r)]
    assert len(combos) == 7                                             # every combination the library accepts
    for given in combos:
        arena = HC.Arena(dev, sizes)
        p = lambda k: arena.ptr(k) if k in given else None               # noqa: E731
        rc = lib.mdil_route_stem(x.data_ptr(), w.data_ptr(), b.data_ptr(), N, Hi, Wi, p("moments"), p("act"),
                                 p("nonfinite"), ws.data_ptr(), ws.numel() * 8, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.mdil_route_last_error()
        torch.cuda.synchronize()
        arena.read()
        arena.assert_untouched([k for k in given if k != "nonfinite"], given)   # nothing is non-finite: nothing is added
        for k in given:
            if k != "nonfinite":
                assert torch.equal(arena.cut(k), as_bytes(base[k]).reshape(-1)), (k, given)


def call_head(lib, dev, arena, given, x, w, b, shape, nc, ws):
    N, H, W = shape
    p = lambda k: arena.ptr(k) if k in given else None               # noqa: E731
    rc = lib.mdil_route_head(x.data_ptr(), w.data_ptr(), b.data_ptr(), N, H, W, nc, p("label"), p("conf"), p("ent"),
                             p("margin"), p("scores"), p("nonfinite"), ws.data_ptr(), ws.numel() * 8,
                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mdil_route_last_error()
    torch.cuda.synchronize()
    arena.read()


def head_arena(dev, shape, nc):
    from mdil_ss_amd.route import head_workspace_bytes
    N, H, W = shape
    npx = N * 4 * H * W
    sizes = {"label": npx, "conf": 4 * npx, "ent": 4 * npx, "margin": 4 * npx, "scores": N * 24, "nonfinite": N * 8}
    return sizes, torch.empty(head_workspace_bytes(N, H, W, nc) // 8, dtype=torch.float64, device=dev)


@pytest.mark.parametrize("shape", ((1, 1, 1), (1, 9, 7), (3, 16, 48)))
def test_head_writes_only_what_it_was_given(dev, shape):
    """One 0xA5-filled arena [guard | label | guard | conf | guard | ent | guard | margin | guard | scores | guard |
    nonfinite | guard] and all 63 combinations of the six optional outputs.  No pixel is non-finite here,
    so a ``nonfinite`` that was given is added nothing and keeps its bytes, like one that was not."""
    from mdil_ss_amd import _route_lib
    lib = _route_lib.load()
    nc = 27
    base = head_full(dev, nc, shape)
    x, w, b = HC.head_inputs(nc, shape)
    x, w, b = nhwc(x).to(dev), w.to(dev), b.to(dev)
    sizes, ws = head_arena(dev, shape, nc)
    combos = [c for r in range(1, 7) for c in itertools.combinations(sizes, r)]
    assert len(combos) == 63
    for given in combos:
        arena = HC.Arena(dev, sizes)
        call_head(lib, dev, arena, given, x, w, b, shape, nc, ws)
        written = [k for k in given if k != "nonfinite"]
        arena.assert_untouched(written, given)
        for k in written:
            assert torch.equal(arena.cut(k), as_bytes(base[k]).reshape(-1)), (k, given)


@pytest.mark.parametrize("given", (("nonfinite",), ("nonfinite", "label"), ("nonfinite", "conf", "margin"),
                                   ("nonfinite", "scores"), ("nonfinite", "label", "ent", "scores")))
def test_head_counts_nonfinite_pixels_with_and_without_scores(dev, given):
    """NaN pixels with ``nonfinite`` given and ``scores`` omitted (no workspace is written, nothing but the
    counter and the maps asked for is stored), and with ``scores`` for comparison: the counter gains the
    four pixels of image 1 on top of what it held, image 0's keeps its bytes."""
    from mdil_ss_amd import _route_lib
    lib = _route_lib.load()
    nc, shape = 20, (2, 12, 20)
    xs, w, b = HC.head_inputs(nc, shape)
    xs = xs.clone()
    xs[1, 9, 5, 7] = float("nan")
    x, w, b = nhwc(xs).to(dev), w.to(dev), b.to(dev)
    sizes, ws = head_arena(dev, shape, nc)
    ws.fill_(-7.0)
    arena = HC.Arena(dev, sizes)
    call_head(lib, dev, arena, given, x, w, b, shape, nc, ws)
    arena.assert_untouched(given, given)
    filled = int.from_bytes(bytes([0xA5] * 8), "little", signed=True)
    assert arena.cut("nonfinite").view(torch.int64).tolist() == [filled, filled + 4]
    if "scores" not in given:
        assert (ws.cpu() == -7.0).all()                                 # no sums: the workspace is not touched
    want = run_head(dev, nc, shape, x=xs)
    for k in given:
        if k != "nonfinite":
            got, ref = arena.cut(k), as_bytes(want[k]).reshape(-1)
            same = got == ref
            if k in ("conf", "ent", "margin"):                          # a NaN's payload may differ: compare as floats there
                gf, rf = got.view(torch.float32), ref.view(torch.float32)
                assert torch.equal(torch.isnan(gf), torch.isnan(rf)) and torch.equal(gf[~torch.isnan(gf)], rf[~torch.isnan(rf)])
            else:
                assert same.all(), k


# -------------------------------------------------------------------------------------- routing
def test_stats_route_on_the_photometric_domains(dev):
    """The seed-0 model of three tasks (its stem is ``HC.tiny_model``'s) with the reference's statistics
    in its ``bn_ini`` buffers: ``Router(by="stats").choose`` equals the reference's choices exactly.
    tests/test_route_cpu.py asserts that the reference routes all 36 images right with a gap >= 0.1."""
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    from mdil_ss_amd.route import Router
    c = R.photometric_case()
    assert torch.equal(c["choice"], c["true"]) and float(c["gap"].min()) >= R.MIN_GAP
    torch.manual_seed(0)
    model = Net([20, 20, 20], 3, 2).to(dev).eval()
    for t, bn in enumerate(model.encoder.initial_block.bn_ini):
        bn.running_mean.copy_(c["mean"][t])
        bn.running_var.copy_(c["var"][t])
    router = Router(model, "stats")
    images = c["images"].to(dev)
    assert router.choose(images) == c["choice"].tolist()
    scores = router.scores(images).cpu()
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (36, 3)
    print(f"stats route: worst relative score error {((scores - c['scores']).abs() / c['scores']).max().item():.2e}, "
          f"worst relative gap {float(R.gaps(scores).min()):.4f}")
    # a subset of the tasks, in another order: positions map back to task ids
    assert Router(model, "stats", [2, 0]).choose(torch.cat([images[:12], images[24:]])) == [0] * 12 + [2] * 12


@pytest.fixture(scope="module")
def tiny(dev):
    return HC.tiny_model(dev)


def expected_labels(model, images, tasks, whole_batch):
    """``predict``'s label maps of the routed tasks: a head route forwards the whole batch through every
    task, the statistics route only the images sent to a task, and the forward is compared like for like."""
    from mdil_ss_amd.predict import predict
    label = torch.empty(images.shape[0], images.shape[2], images.shape[3], dtype=torch.uint8, device=images.device)
    for t in set(tasks):
        idx = torch.tensor([i for i, v in enumerate(tasks) if v == t], device=images.device)
        label[idx] = predict(model, images, t)[0][idx] if whole_batch else predict(model, images[idx], t)[0]
    return label


@pytest.mark.parametrize("by", ("entropy", "confidence", "margin"))
def test_head_routes_choose_the_reference_argmin(dev, tiny, by):
    """Untrained heads: no accuracy is asserted.  Each chosen task is the argmin of the fp64 reference
    scores on the same features; an image whose reference gap is within the two scores' summed
    tolerances is excluded, and at most 1 of the 12 may be."""
    from mdil_ss_amd.dataset import ProceduralSeg
    from mdil_ss_amd.route import HEAD_COLUMN, Router, head_scores
    ds = ProceduralSeg(12, 32, 64, 20, seed=12, domain=0)
    images = torch.stack([ds[i][0] for i in range(12)]).to(dev)
    name = COLUMNS[HEAD_COLUMN[by]]
    ref, tol = [], []
    for t in (0, 1):
        with torch.no_grad():
            feat = tiny.features(images, t).contiguous().cpu()
        w, b = (p.detach().cpu() for p in tiny.head_params(t))
        logits, S = HC.head64(feat.permute(0, 3, 1, 2), w, b)
        maps = dict(zip(("conf", "ent", "margin"), R.head_stats64(logits)))
        scale = U * (1 + S.max(1)[0]) * ((1 + maps["ent"]) if name == "ent" else 1.0)
        sums = torch.zeros(12, 3, dtype=torch.float64)
        sums[:, HEAD_COLUMN[by]] = maps[name].sum((1, 2))
        ref.append(head_scores(sums, 32 * 64, 20, by))
        tol.append(K_OF[name] * scale.sum((1, 2)) / (32 * 64) / (math.log(20) if by == "entropy" else 1.0))
    ref, tol = torch.stack(ref, 1), torch.stack(tol, 1)
    excluded = (ref[:, 0] - ref[:, 1]).abs() <= tol.sum(1)
    print(f"{by}: {int(excluded.sum())} of 12 images excluded; reference scores {ref.tolist()}")
    assert int(excluded.sum()) <= 1
    router = Router(tiny, by)
    chosen = torch.tensor(router.choose(images))
    assert torch.equal(chosen[~excluded], ref.argmin(1)[~excluded])
    got = router.scores(images).cpu()
    assert ((got - ref).abs() <= tol + 1e-12).all()
    tasks, label = router.predict(images)
    assert tasks == chosen.tolist() and label.dtype == torch.uint8 and tuple(label.shape) == (12, 32, 64)
    assert torch.equal(label, expected_labels(tiny, images, tasks, whole_batch=True))


def test_a_head_with_nonfinite_pixels_loses_the_route(dev, tiny):
    """A NaN in head 1's bias makes every softmax sum of that head non-finite: its sums are empty (0 over
    the image, the lowest entropy there is), yet it scores inf and every image goes to task 0; likewise
    for head 0.  ``route`` reports the count."""
    from mdil_ss_amd.dataset import ProceduralSeg
    from mdil_ss_amd.route import Router
    ds = ProceduralSeg(3, 32, 64, 20, seed=12, domain=0)
    images = torch.stack([ds[i][0] for i in range(3)]).to(dev)
    for broken in (1, 0):
        bias = tiny.head_params(broken)[1]
        kept = bias.detach().clone()
        try:
            with torch.no_grad():
                bias[3] = float("nan")
            for by in ("entropy", "confidence", "margin"):
                router = Router(tiny, by)
                scores = router.scores(images).cpu()
                assert torch.isinf(scores[:, broken]).all() and torch.isfinite(scores[:, 1 - broken]).all()
                r = router.route(images)
                assert r["tasks"] == [1 - broken] * 3 and r["nonfinite"] == 3 * 32 * 64
        finally:
            with torch.no_grad():
                bias.copy_(kept)


def test_stats_route_predicts_with_the_chosen_heads_only(dev, tiny):
    from mdil_ss_amd.dataset import ProceduralSeg
    from mdil_ss_amd.route import Router
    ds = ProceduralSeg(4, 32, 64, 20, seed=12, domain=0)
    images = torch.stack([ds[i][0] for i in range(4)]).to(dev)
    router = Router(tiny, "stats")
    calls = []
    inner = tiny.features
    tiny.features = lambda x, t: (calls.append((t, x.shape[0])), inner(x, t))[1]
    try:
        tasks, label = router.predict(images)
    finally:
        del tiny.features
    assert sorted(t for t, _ in calls) == sorted(set(tasks)) and sum(n for _, n in calls) == 4
    assert torch.equal(label, expected_labels(tiny, images, tasks, whole_batch=False))


# ----------------------------------------------------------------------------------------- CLI
def test_cli_end_to_end(dev, tiny, tmp_path):
    """--synthetic 4 at 32 x 64, in-process: the PNGs, every field of the JSON, and an mIoU with head
    T that is ``predict``'s labels scored by the same rule."""
    from argparse import Namespace
    from PIL import Image
    from mdil_ss_amd import _report_common as rc
    from mdil_ss_amd import route as P
    from mdil_ss_amd.fullres import iou_rule
    from mdil_ss_amd.predict import predict
    ckpt = tmp_path / "model.pth.tar"
    HC.save_checkpoint(tiny, ckpt)
    base = ["--state", str(ckpt), "--num-classes", "20", "20", "--synthetic", "4", "--task", "1", "--height", "32",
            "--width", "64"]
    data = Namespace(synthetic=4, height=32, width=64, batch_size=4, task=1)
    (_, images, target), = rc.batches(data, 20, dev)
    label = predict(tiny, images, 1)[0].cpu()
    matrix, bad, _ = HC.expected_counts(target.cpu(), label, 20, 19)
    d = matrix.double()
    want = float(iou_rule(20, 19, d.diagonal(), d.sum(0), d.sum(1))[0])
    for by in ("stats", "entropy"):
        out = tmp_path / by
        report = P.main(P.build_parser().parse_args(base + ["--by", by, "--score", "--out", str(out), "--colour", "--json",
                                                            str(tmp_path / f"{by}.json")]))
        a = json.load(open(tmp_path / f"{by}.json"))
        assert json.loads(json.dumps(report)) == a
        assert (a["dataset"], a["by"], a["tasks"], a["images"], a["task"], a["nonfinite"]) == ("synthetic", by, [0, 1], 4, 1, 0)
        assert [r["image"] for r in a["routes"]] == [f"synthetic_{i:04d}" for i in range(4)]
        for r in a["routes"]:
            assert sorted(r["scores"]) == ["0", "1"] and all(math.isfinite(v) for v in r["scores"].values())
            assert r["task"] == int(min(r["scores"], key=lambda k: (r["scores"][k], int(k))))
        sent = [sum(1 for r in a["routes"] if r["task"] == t) for t in (0, 1)]
        assert a["sent"] == {"0": sent[0], "1": sent[1]} and a["routing_accuracy"] == sent[1] / 4
        assert a["mIoU_head"] == want and a["confusion_head"] == matrix.tolist() and bad == 0
        assert a["misrouted_unscored"] == 0 and a["pixels_routed"] == a["pixels_head"] == int(matrix.sum())
        assert len(a["iou_classes_head"]) == len(a["iou_classes_routed"]) == 19 and 0.0 <= a["mIoU_routed"] <= 1.0
        names = sorted(os.listdir(out))
        assert names == sorted(f"synthetic_{i:04d}_{k}.png" for i in range(4) for k in ("label", "colour"))
        assert sorted(a["written"]) == sorted(str(out / n) for n in names)
        labels = expected_labels(tiny, images, [r["task"] for r in a["routes"]], whole_batch=by != "stats").cpu()
        for i in range(4):
            with Image.open(out / f"synthetic_{i:04d}_label.png") as im:
                assert im.mode == "L" and im.size == (64, 32)
                assert torch.equal(torch.from_numpy(np.asarray(im).copy()), labels[i])
