"""GPU: the refinement kernel (mdil_ss_amd/ext/refine_head.hip) and the entry points over it
(mdil_ss_amd/refine.py), against tests/refine_reference.py evaluated in float64.

What is compared with what.  The yardstick of a case is the distance of the SAME reference evaluated
in float32 from its float64 evaluation, ``max |Q_32 - Q_64|``, computed here from the reference alone
(2e-8 to 1.5e-6 over these cases on a CPU).  The device's Q must lie within ``MARGIN`` times that
of Q_64: it sums the window in another order and takes the colour factor from the hardware exp2.
Labels must equal the fp64 argmax wherever the fp64 top-2 gap exceeds twice that bound; the
exclusion is a condition on the reference, checked first (at most 0.2 % of a case's pixels, none in
a case below 100 pixels).  Everything else is asserted exactly: plain prediction is
``predict_head``'s label bit for bit, a pixel's bytes depend neither on the batch nor on the stream,
counters are the bincounts of the call's own labels.

Measured on an MI355X: the ratio of (1) is 0.44 to 3.914 over the 120 cases.  The worst
is the 2 x 2 grid of 20 classes at weights x 8 under a dilated window, where no neighbour lies inside the image: the
device's 1.2e-7 there is two ulps of a probability near 1 against a yardstick of 3.1e-8.  Every case with a
neighbour inside the image is at or below 1.58, so the margin stays at the 4 the check starts from."""
import glob
import json

import numpy as np
import pytest
import torch

from tests import head_cases as HC
from tests import refine_reference as R
from tests.head_cases import nhwc

pytestmark = pytest.mark.gpu

TILE_H, TILE_W = 8, 32                          # refine_head.hip: kTileH, kTileW (one sub-grid tile per work-group)
WINDOWS = ((1, 1), (3, 2), (5, 1), (5, 4))      # (radius, dilation)
CLASSES = (2, 20, 32)
SCALES = (1.0, 8.0)                             # 8: the trained regime, logits 8 times as far apart
RAGGED = (1, 35, 131)                           # logit grid 70 x 262: see test_the_ragged_shape_is_ragged
SHAPES = HC.SHAPES + (RAGGED,)
BIG = (3, 16, 48)
MARGIN = 4.0                                    # another summation order plus a hardware exp against libm
MAX_EXCLUDED = 2e-3


@pytest.fixture(scope="module")
def dev():
    return HC.device("refinement")


def params(window=None, **kw):
    from mdil_ss_amd.refine import RefineParams
    if window is not None:
        kw.update(radius=window[0], dilation=window[1])
    return RefineParams(**kw)


def inputs(nc, shape, scale=1.0):
    x, w, b = HC.head_inputs(nc, shape)
    return x, (w * scale if scale != 1.0 else w), b


def on_device(dev, nc, shape, scale=1.0):
    x, w, b = inputs(nc, shape, scale)
    return nhwc(x).to(dev), w.to(dev), b.to(dev), R.image_for(shape).to(dev)


def run(dev, nc, shape, scale, p, **kw):
    """One refine_head call -> (label, confidence, Q) on the host."""
    from mdil_ss_amd.refine import refine_head
    out = refine_head(*on_device(dev, nc, shape, scale), p, want_confidence=True, want_q=True, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in out)


def test_the_ragged_shape_is_ragged():
    """Its logit grid is a multiple of the tile in neither axis and every sub-grid of every dilation
    tested spans at least three tiles each way."""
    Hl, Wl = 2 * RAGGED[1], 2 * RAGGED[2]
    assert Hl % TILE_H and Wl % TILE_W
    for _, d in WINDOWS:
        assert (Hl - (d - 1) + d - 1) // d > 2 * TILE_H and (Wl - (d - 1) + d - 1) // d > 2 * TILE_W
        assert ((Hl + d - 1) // d) % TILE_H and ((Wl + d - 1) // d) % TILE_W


# ------------------------------------------------------------------------------------ (1), (2)
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("nc", CLASSES)
def test_q_and_labels_against_fp64(dev, nc, scale, shape, window):
    p = params(window)
    x, w, b = inputs(nc, shape, scale)
    img = R.image_for(shape)
    q64 = R.mean_field(R.head_logits(x, w, b, torch.float64), img, p, torch.float64)
    q32 = R.mean_field(R.head_logits(x, w, b, torch.float32), img, p, torch.float32)
    yard = float((q32.double() - q64).abs().max())
    bound = MARGIN * yard
    what = f"nc {nc} scale {scale} shape {shape} window {window}"
    # (2)'s exclusion first: a condition on the reference alone
    top = q64.topk(2, 1)[0]
    excluded = (top[:, 0] - top[:, 1]) <= 2 * bound
    pixels = excluded.numel()
    print(f"{what}: excluded {int(excluded.sum())} of {pixels} pixels")
    assert int(excluded.sum()) <= (0 if pixels < 100 else int(MAX_EXCLUDED * pixels)), what
    label, conf, q = run(dev, nc, shape, scale, p)
    err = float((q.double() - q64.permute(0, 2, 3, 1)).abs().max())
    print(f"{what}: max |Q_gpu - Q_64| {err:.3e}, max |Q_32 - Q_64| {yard:.3e}, ratio {err / yard:.3f}")
    assert yard > 0 and err <= bound, what
    assert torch.equal(conf, q.max(3)[0])
    assert label.dtype == torch.uint8 and tuple(label.shape) == (shape[0], 2 * shape[1], 2 * shape[2])
    wrong = (label.long() != q64.max(1)[1]) & ~excluded
    assert not wrong.any(), f"{what}: {int(wrong.sum())} labels differ from the fp64 argmax"


# ------------------------------------------------------------------------------------------ (3)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nc", CLASSES)
def test_plain_prediction_is_predict_heads_label(dev, nc, shape):
    from mdil_ss_amd.predict import predict_head
    for scale in SCALES:
        xd, wd, bd, _ = on_device(dev, nc, shape, scale)
        want, _, want_conf = predict_head(xd, wd, bd, None, True)
        label, conf, _ = run(dev, nc, shape, scale, params(iterations=0))
        assert torch.equal(label, want.cpu()) and torch.equal(conf, want_conf.cpu())
        for window in ((5, 2), (3, 1)):
            label, _, _ = run(dev, nc, shape, scale, params(window, iterations=3, w_appearance=0.0, w_smooth=0.0))
            assert torch.equal(label, want.cpu()), (scale, window)


# ------------------------------------------------------------------------------------------ (4)
@pytest.mark.parametrize("window", ((3, 2), (5, 4)))
@pytest.mark.parametrize("nc", (20, 27))
def test_batch_run_and_stream_independence(dev, nc, window):
    from mdil_ss_amd.refine import refine_head
    p = params(window)
    xd, wd, bd, img = on_device(dev, nc, BIG)
    whole = run(dev, nc, BIG, 1.0, p)
    again = run(dev, nc, BIG, 1.0, p)
    side = HC.side_stream(lambda: refine_head(xd, wd, bd, img, p, want_confidence=True, want_q=True))
    for a, b, c in zip(whole, again, side):
        assert torch.equal(HC.as_bytes(a), HC.as_bytes(b)) and torch.equal(HC.as_bytes(a), HC.as_bytes(c.cpu()))
    for n in range(BIG[0]):
        alone = refine_head(xd[n:n + 1].contiguous(), wd, bd, img[n:n + 1].contiguous(), p, want_confidence=True,
                            want_q=True)
        for a, b in zip(whole, alone):
            assert torch.equal(HC.as_bytes(a[n:n + 1]), HC.as_bytes(b.cpu())), n


# ------------------------------------------------------------------------------------------ (5)
OUTPUTS = ("label", "confidence", "q", "confusion", "bad_targets", "changed")


def _raw(dev, nc, shape, p, given, short=0):
    """mdil_refine_head through the raw ABI into a sentinel arena; the workspace is exactly
    workspace_bytes (minus ``short``) between guard bands.  -> (rc, arena, target on the host, the library)."""
    from mdil_ss_amd import _refine_lib
    lib = _refine_lib.load()
    xd, wd, bd, img = on_device(dev, nc, shape)
    N, H, W = shape
    npx = N * 4 * H * W
    need = lib.mdil_refine_workspace_bytes(N, H, W, nc, p.iterations)
    assert need == (0 if p.iterations == 0 else (1 if p.iterations == 1 else 2) * npx * nc * 4)
    arena = HC.Arena(dev, {"workspace": max(need - short, 1), "label": npx, "confidence": 4 * npx, "q": 4 * npx * nc,
                           "confusion": 2 * nc * nc * 8, "bad_targets": 8, "changed": 8})
    target = HC.make_target(nc, (N, 2 * H, 2 * W), nc - 1, seed=nc + H)
    td = target.to(dev)
    ptr = {k: (arena.ptr(k) if k in given else None) for k in OUTPUTS}
    rc = lib.mdil_refine_head(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), img.data_ptr(), N, H, W, nc, p.iterations,
                              p.radius, p.dilation, p.w_appearance, p.w_smooth, p.theta_alpha, p.theta_beta,
                              p.theta_gamma, arena.ptr("workspace") if need else None, need - short, ptr["label"],
                              ptr["confidence"], ptr["q"], td.data_ptr() if "confusion" in given else None, nc - 1,
                              ptr["confusion"], ptr["bad_targets"], ptr["changed"],
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    arena.read()
    return rc, arena, target, lib


@pytest.mark.parametrize("iterations", (0, 1, 2, 5))
@pytest.mark.parametrize("shape", ((1, 9, 7), BIG))
def test_optional_outputs_workspace_and_guard_bands(dev, shape, iterations):
    """Each optional output absent in turn, then all of them: what was not given keeps its sentinel
    bytes, and so do the guard bands round a workspace of exactly ``workspace_bytes``.  The counters
    are ADDED to: they start from the sentinel 0xA5A5A5A5A5A5A5A5."""
    nc = 20
    p = params((3, 2), iterations=iterations)
    label, conf, q = run(dev, nc, shape, 1.0, p)
    plain = run(dev, nc, shape, 1.0, params(iterations=0))[0]
    sentinel = torch.tensor([0xA5] * 8, dtype=torch.uint8).view(torch.int64)
    everything = OUTPUTS
    for given in [("label",)] + [tuple(k for k in everything if k != drop) for drop in everything[1:]] + [everything]:
        if ("confusion" in given) != ("bad_targets" in given):
            given = tuple(k for k in given if k not in ("confusion", "bad_targets"))    # they come together
        rc, arena, target, lib = _raw(dev, nc, shape, p, given)
        assert rc == 0, lib.mdil_refine_last_error()
        matrix0, n_bad, _ = HC.expected_counts(target, plain, nc, nc - 1)
        n_changed = int((label != plain).sum())
        written = [k for k in given if k in ("label", "confidence", "q", "confusion")]
        if iterations:
            written.append("workspace")
        if "bad_targets" in given and n_bad:
            written.append("bad_targets")
        if "changed" in given and n_changed:
            written.append("changed")
        arena.assert_untouched(written, given)
        assert torch.equal(arena.cut("label"), label.reshape(-1))
        if "confidence" in given:
            assert torch.equal(arena.cut("confidence"), HC.as_bytes(conf).reshape(-1))
        if "q" in given:
            assert torch.equal(arena.cut("q"), HC.as_bytes(q).reshape(-1))
        if "confusion" in given:
            got = arena.cut("confusion").view(torch.int64).reshape(2, nc, nc) - sentinel
            assert torch.equal(got[0], matrix0)
            assert torch.equal(got[1], HC.expected_counts(target, label, nc, nc - 1)[0])
            assert int((arena.cut("bad_targets").view(torch.int64) - sentinel).item()) == n_bad
        if "changed" in given:
            assert int((arena.cut("changed").view(torch.int64) - sentinel).item()) == n_changed
    if iterations:
        rc, arena, _, lib = _raw(dev, nc, shape, p, everything, short=1)
        assert rc == -1 and b"need a workspace of" in lib.mdil_refine_last_error()
        arena.assert_untouched((), "a refused call writes nothing")


# ------------------------------------------------------------------------------------------ (6)
@pytest.mark.parametrize("window", ((1, 1), (5, 2)))
@pytest.mark.parametrize("nc, scale", ((2, 8.0), (20, 1.0), (32, 1.0)))
def test_counters(dev, nc, scale, window):
    p = params(window)
    N, H, W = BIG
    target = HC.make_target(nc, (N, 2 * H, 2 * W), nc - 1, seed=nc + H)
    confusion = torch.zeros(2, nc, nc, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    changed = torch.zeros(1, dtype=torch.int64, device=dev)
    kw = dict(target=target.to(dev), ignore_index=nc - 1, confusion=confusion, bad_targets=bad, changed=changed)
    plain = run(dev, nc, BIG, scale, params(iterations=0))[0]
    label = run(dev, nc, BIG, scale, p, **kw)[0]
    m0, n_bad, counted = HC.expected_counts(target, plain, nc, nc - 1)
    m1 = HC.expected_counts(target, label, nc, nc - 1)[0]
    n_changed = int((label != plain).sum())
    print(f"nc {nc} window {window}: {n_changed} of {label.numel()} labels changed")
    assert n_bad > 0 and n_changed > 0 and int(m0.sum()) == int(m1.sum()) == counted
    for times in (1, 2):
        if times == 2:
            assert torch.equal(run(dev, nc, BIG, scale, p, **kw)[0], label)       # accumulates, does not overwrite
        assert torch.equal(confusion.cpu(), times * torch.stack((m0, m1)))
        assert int(bad.item()) == times * n_bad and int(changed.item()) == times * n_changed
    # `changed` works without a target
    alone = torch.zeros(1, dtype=torch.int64, device=dev)
    run(dev, nc, BIG, scale, p, changed=alone)
    assert int(alone.item()) == n_changed


# ------------------------------------------------------------------------------------------ (7)
def restore_case():
    """Four flat colour regions (the quadrants of a 64 x 128 grid), the true class's logit 1 above the
    others, and a 4 x 4 lattice of isolated pixels (5.1 %; none within 2 pixels of the image's edge or
    of a region's border) whose lead went to a wrong class.  Features and weights that put any logit
    map through the head: channel 4 c + (a*2+b) is class c's logit at parity (a, b)."""
    Hl, Wl, nc, lead = 64, 128, 4, 1.0
    truth = torch.zeros(1, Hl, Wl, dtype=torch.long)
    truth[:, :Hl // 2, Wl // 2:], truth[:, Hl // 2:, :Wl // 2], truth[:, Hl // 2:, Wl // 2:] = 1, 2, 3
    colours = torch.tensor([[0.1, 0.2, 0.9], [0.9, 0.1, 0.2], [0.2, 0.9, 0.1], [0.8, 0.8, 0.7]])
    image = colours[truth].permute(0, 3, 1, 2).contiguous()
    ys, xs = torch.meshgrid(torch.arange(Hl), torch.arange(Wl), indexing="ij")

    def far(v, n):
        return (v >= 2) & (v < n - 2) & ((v - n // 2 >= 2) | (n // 2 - 1 - v >= 2))

    flip = (ys % 4 == 2) & (xs % 4 == 1) & far(ys, Hl) & far(xs, Wl)
    noisy = truth.clone()
    noisy[0][flip] = (truth[0][flip] + 1 + (ys[flip] + xs[flip]) % 3) % nc
    logits = torch.zeros(1, nc, Hl, Wl).scatter_(1, noisy.unsqueeze(1), lead)
    # logits [1,c,2h+a,2w+b] -> features [1,16,h,w] with channel 4c + 2a + b
    x = logits.reshape(1, nc, Hl // 2, 2, Wl // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(1, 16, Hl // 2, Wl // 2)
    w = torch.zeros(16, nc, 2, 2)
    for c in range(nc):
        for a in range(2):
            for b in range(2):
                w[4 * c + 2 * a + b, c, a, b] = 1.0
    return truth, noisy, flip, image, logits, x.contiguous(), w, torch.zeros(nc)


def test_refinement_restores_a_known_answer(dev):
    from mdil_ss_amd.refine import refine_head
    truth, noisy, flip, image, logits, x, w, b = restore_case()
    p = params()
    assert torch.equal(R.head_logits(x, w, b, torch.float64), logits.double())
    assert 0.045 < float(flip.double().mean()) < 0.055
    # the reference first: it restores every pixel, moves no border, and decides nothing narrowly
    q64 = R.mean_field(logits, image, p)
    top = q64.topk(2, 1)[0]
    assert torch.equal(q64.max(1)[1], truth) and float((top[:, 0] - top[:, 1]).min()) > 0.1
    changed = torch.zeros(1, dtype=torch.int64, device=dev)
    label, _, _ = refine_head(nhwc(x).to(dev), w.to(dev), b.to(dev), image.to(dev), p, changed=changed)
    plain, _, _ = refine_head(nhwc(x).to(dev), w.to(dev), b.to(dev), image.to(dev), params(iterations=0))
    assert torch.equal(plain.cpu().long(), noisy)
    assert torch.equal(label.cpu().long(), truth)
    assert int(changed.item()) == int(flip.sum())


# ------------------------------------------------------------------------------------------ (8)
@pytest.fixture(scope="module")
def tiny_model(dev):
    return HC.tiny_model(dev)


@pytest.fixture(scope="module")
def checkpoint(tiny_model, tmp_path_factory):
    path = tmp_path_factory.mktemp("refine") / "checkpoint.pth.tar"
    HC.save_checkpoint(tiny_model, path)
    return str(path)


def read_png(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == "L", (path, im.mode)
        return torch.from_numpy(np.array(im))


def test_cli_synthetic_end_to_end(dev, tiny_model, checkpoint, tmp_path):
    from mdil_ss_amd import refine as RF
    from mdil_ss_amd.dataset import ProceduralSeg
    from mdil_ss_amd.fullres import iou_rule
    out, report_file = tmp_path / "maps", tmp_path / "report.json"
    report = RF.main(RF.build_parser().parse_args(
        ["--state", checkpoint, "--num-classes", "20", "20", "--task", "1", "--synthetic", "3", "--height", "64",
         "--width", "128", "--batch-size", "2", "--radius", "3", "--out", str(out), "--confidence", "--score",
         "--json", str(report_file)]))
    files = sorted(glob.glob(str(out / "*_label.png")))
    assert len(files) == 3 and len(glob.glob(str(out / "*_conf.png"))) == 3 and len(report["written"]) == 6
    ds = ProceduralSeg(3, 64, 128, 20, seed=13, domain=1)
    images = torch.stack([ds[i][0] for i in range(3)]).to(dev)
    target = torch.stack([ds[i][1][0] for i in range(3)]).to(torch.uint8)
    p = RF.RefineParams(radius=3)
    labels = torch.cat([RF.refine(tiny_model, images[i:i + 2], 1, p)[0].cpu() for i in (0, 2)])
    plain = torch.cat([RF.refine(tiny_model, images[i:i + 2], 1, RF.RefineParams(iterations=0))[0].cpu() for i in (0, 2)])
    for i in range(3):
        got = read_png(out / f"synthetic_{i:04d}_label.png")
        assert tuple(got.shape) == (64, 128) and torch.equal(got, labels[i])
    with open(report_file) as f:
        saved = json.load(f)
    assert saved["pixels"] == 3 * 64 * 128 and saved["images"] == 3 and saved["params"] == p._asdict()
    assert saved["changed"] == int((labels != plain).sum()) and saved["changed_share"] == saved["changed"] / saved["pixels"]
    assert saved["bad_targets"] == HC.expected_counts(target, plain, 20, 19)[1]
    for name, lab in (("plain", plain), ("refined", labels)):
        m = torch.tensor(saved[f"confusion_{name}"])
        assert torch.equal(m, HC.expected_counts(target, lab, 20, 19)[0])
        miou, per_class = iou_rule(20, 19, m.double().diagonal(), m.double().sum(0), m.double().sum(1))
        assert saved[f"mIoU_{name}"] == float(miou) and saved[f"iou_classes_{name}"] == [float(v) for v in per_class]
