"""GPU: the fused output_conv + bilinear resize + argmax + confusion kernel
(mdil_ss_amd/ext/fullres_head.hip) and the entry points over it (mdil_ss_amd/fullres.py), against an
fp64 reference on the CPU:

    L  = F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2)
    Lu = F.interpolate(L, size, mode="bilinear", align_corners=False)
    Su = the same two steps on absolute values

Which pixels may differ.  The kernel's header counts k = 68 roundings on the longest path from the
inputs to a compared logit (two weight quotients, their product, the scaling of the feature, a
64-term FMA chain), so the near-tie rule of tests/head_cases.py applies to Lu and Su with k = 68.  A
pixel whose fp64 top-2 margin is within that bound is excluded, every other pixel must match the fp64
argmax exactly, and at most max(1, floor(0.001 * pixels)) pixels of a case may be excluded -- none in
a case of fewer than 100."""
import functools
import glob
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import head_cases as HC
from tests.head_cases import CLASSES, expected_counts, make_target, nhwc, random_luts

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 68                                     # the kernel header's count; checked against its text below
SIZES = {
    (1, 1, 1): ((1, 1), (2, 2), (5, 7)),
    (1, 9, 7): ((18, 14), (36, 28), (25, 31), (11, 9)),             # identity, 2x, odd, down
    (2, 12, 20): ((24, 40), (48, 80), (45, 77)),
    (3, 16, 48): ((64, 192), (45, 80), (90, 135)),
}
CASES = [(shape, size) for shape, sizes in SIZES.items() for size in sizes]
SOME = [((1, 1, 1), (5, 7)), ((1, 9, 7), (25, 31)), ((2, 12, 20), (48, 80)), ((3, 16, 48), (90, 135))]


@pytest.fixture(scope="module")
def dev():
    return HC.device("full-resolution")


def reference(x, w, b, size):
    """-> (label i64 [N,Ho,Wo], excluded bool) from fp64 logits resized in fp64."""
    L, S = HC.head64(x, w, b)
    Lu = F.interpolate(L, size, mode="bilinear", align_corners=False)
    Su = F.interpolate(S, size, mode="bilinear", align_corners=False)
    return Lu.max(1)[1], HC.near_tie(Lu, Su, K)


@functools.lru_cache(maxsize=None)
def case(nc, shape, size):
    """Inputs and their reference, computed once and shared (never modified)."""
    x, w, b = HC.head_inputs(nc, shape)
    return (x, w, b) + reference(x, w, b, size)


def run(dev, x, w, b, size, **kw):
    from mdil_ss_amd.fullres import fullres_head
    kw = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    out = fullres_head(nhwc(x).to(dev), w.to(dev), b.to(dev), size, **kw)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu() for t in out)


def test_header_states_the_rounding_count():
    src = open(os.path.join(REPO, "mdil_ss_amd", "ext", "fullres_head.hip")).read()
    assert [int(v) for v in re.findall(r"k = (\d+) roundings", src)] == [K] and K <= 96


@pytest.mark.parametrize("shape, size", CASES)
@pytest.mark.parametrize("nc", CLASSES)
def test_labels_match_fp64_argmax(dev, nc, shape, size):
    x, w, b, ref, excluded = case(nc, shape, size)
    label, colour = run(dev, x, w, b, size)
    assert colour is None
    HC.check_labels(label, ref, excluded, f"nc {nc} shape {shape} -> {size}", HC.count_cap)


def test_ties_go_to_the_lowest_class(dev):
    """Classes 3 and 11 with bit-identical weights and bias tie exactly at every pixel of a resized
    map too; with the largest bias they are also the winners almost everywhere."""
    x, w, b = HC.head_inputs(20, (2, 12, 20))
    w, b = w.clone(), b.clone()
    b[3] = b.max() + 1.0
    w[:, 11], b[11] = w[:, 3], b[3]
    label = run(dev, x, w, b, (45, 77))[0]
    assert not (label == 11).any()
    assert (label == 3).double().mean() > 0.5
    w[:, 11] = 0                      # without the twin class the same labels must come out
    b[11] = -1e30
    assert torch.equal(run(dev, x, w, b, (45, 77))[0], label)


def test_nan_logits_give_the_first_nan_class(dev):
    """(45, 77) from 24 x 40 logits has no source coordinate that is a whole number, so every
    neighbour has a weight above zero and the footprint of a NaN is the fp64 reference's."""
    x, w, b = HC.head_inputs(20, (2, 12, 20))
    size = (45, 77)
    clean = run(dev, x, w, b, size)[0]
    xn = x.clone()
    xn[1, 5, 7, 9] = float("nan")
    Lu = F.interpolate(F.conv_transpose2d(xn.double(), w.double(), b.double(), stride=2), size, mode="bilinear",
                       align_corners=False)
    hit = torch.isnan(Lu).any(1)
    assert 0 < int(hit.sum()) < 100 and not hit[0].any()
    label = run(dev, xn, w, b, size)[0]
    assert (label[hit] == 0).all()                      # every class is NaN there: the first one
    assert torch.equal(label[~hit], clean[~hit])
    # NaN logits at classes 7 and 12 only (their bias): the first of them wins everywhere
    bn = b.clone()
    bn[7] = bn[12] = float("nan")
    assert (run(dev, x, w, bn, size)[0] == 7).all()


@pytest.mark.parametrize("shape, size", SOME)
@pytest.mark.parametrize("nc", CLASSES)
def test_id_map_and_palette_are_applied_after_the_argmax(dev, nc, shape, size):
    x, w, b = HC.head_inputs(nc, shape)
    ids, pal = random_luts(nc)
    plain = run(dev, x, w, b, size)[0]
    label, colour = run(dev, x, w, b, size, id_map=ids, palette=pal)
    assert colour.dtype == torch.uint8 and tuple(colour.shape) == tuple(plain.shape) + (3,)
    assert torch.equal(label, ids[plain.long()])
    assert torch.equal(colour, pal[plain.long()])
    only_colour = run(dev, x, w, b, size, palette=pal)
    assert torch.equal(only_colour[0], plain) and torch.equal(only_colour[1], colour)


def check_confusion(dev, x, w, b, nc, size, ignore):
    from mdil_ss_amd.fullres import fullres_head
    args = (nhwc(x).to(dev), w.to(dev), b.to(dev), size)
    return HC.check_confusion(lambda **kw: fullres_head(*args, **kw), dev, nc, x.shape[0], size, ignore)


@pytest.mark.parametrize("ignore", ("last", 255))
@pytest.mark.parametrize("shape, size", SOME + [((1, 9, 7), (36, 28))])
@pytest.mark.parametrize("nc", CLASSES)
def test_confusion_counts_the_kernels_own_labels(dev, nc, shape, size, ignore):
    x, w, b = HC.head_inputs(nc, shape)
    label = check_confusion(dev, x, w, b, nc, size, nc - 1 if ignore == "last" else 255)
    assert torch.equal(label, run(dev, x, w, b, size)[0])


def test_confusion_meter(dev):
    from mdil_ss_amd.fullres import ConfusionMeter
    nc, shape, size = 20, (2, 12, 20), (45, 77)
    x, w, b = HC.head_inputs(nc, shape)
    args = (nhwc(x).to(dev), w.to(dev), b.to(dev))
    target = make_target(nc, (2,) + size, nc - 1, seed=5)
    clean = target.clone()
    clean[clean >= nc] = nc - 1
    meter = ConfusionMeter(nc, nc - 1)
    label = meter.add(*args, target=clean.to(dev))[0].cpu()
    matrix, n_bad, _ = expected_counts(clean, label, nc, nc - 1)
    assert n_bad == 0 and torch.equal(meter.matrix(), matrix) and meter.matrix().dtype == torch.int64
    mean, per_class = meter.iou()
    tp = matrix.diagonal().double()
    want = (tp / (matrix.sum(0) + matrix.sum(1) - tp + 1e-15))[:nc - 1]
    assert torch.equal(per_class, want) and mean.item() == want.mean().item()
    meter.add(*args, target=target.to(dev))
    n_bad = int((target >= nc).sum())
    with pytest.raises(RuntimeError, match=f"{n_bad} target pixels are outside"):
        meter.matrix()


@pytest.mark.parametrize("size", ((25, 31), (48, 80)))
def test_null_outputs_and_guard_bands_stay_untouched(dev, size):
    """One 0xA5-filled arena [guard | label | guard | colour | guard] and pre-filled confusion /
    bad_targets: nothing outside the requested maps changes; with target = NULL the two counters
    keep their bytes although their pointers are passed."""
    from mdil_ss_amd import _fullres_lib
    lib = _fullres_lib.load()
    nc, shape = 27, (1, 9, 7) if size == (25, 31) else (2, 12, 20)
    x, w, b = HC.head_inputs(nc, shape)
    ids, pal = random_luts(nc)
    plain = run(dev, x, w, b, size)[0].reshape(-1)
    N, _, H, W = x.shape
    npx = N * size[0] * size[1]
    xd, wd, bd, idd, pd = nhwc(x).to(dev), w.to(dev), b.to(dev), ids.to(dev), pal.to(dev)
    target = make_target(nc, (N,) + size, nc - 1, seed=1).to(dev)
    for with_colour, with_target in ((False, False), (True, False), (True, True)):
        arena = HC.Arena(dev, {"label": npx, "colour": 3 * npx})
        conf = torch.full((nc, nc), 7, dtype=torch.int64, device=dev)
        bad = torch.full((1,), 5, dtype=torch.int64, device=dev)
        rc = lib.mdil_fullres_head(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), N, H, W, nc, size[0], size[1],
                                   idd.data_ptr(), pd.data_ptr(), target.data_ptr() if with_target else None, nc - 1,
                                   arena.ptr("label"), arena.ptr("colour") if with_colour else None, conf.data_ptr(),
                                   bad.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.mdil_fullres_last_error()
        torch.cuda.synchronize()
        arena.read()
        arena.assert_untouched(("label", "colour") if with_colour else ("label",), (with_colour, with_target))
        assert torch.equal(arena.cut("label"), ids[plain.long()])
        if with_colour:
            assert torch.equal(arena.cut("colour").reshape(-1, 3), pal[plain.long()])
        if with_target:
            matrix, n_bad, _ = expected_counts(target.cpu(), plain, nc, nc - 1)
            assert torch.equal(conf.cpu(), matrix + 7) and int(bad.item()) == n_bad + 5
        else:
            assert (conf.cpu() == 7).all() and int(bad.item()) == 5


def test_grid_stride_loop_past_the_grid_bound(dev):
    """The grid is bounded at 2048 work-groups of 256 lanes, a lane owning four pixels of a row:
    1025 rows of ceil(2051 / 4) = 513 items are 525,825 items, 1,537 of which go round the loop a
    second time, with odd sizes on both axes.  Two classes keep the fp64 reference cheap."""
    nc, shape, size = 2, (1, 200, 300), (1025, 2051)
    assert size[0] * ((size[1] + 3) // 4) > 2048 * 256
    x, w, b, ref, excluded = case(nc, shape, size)
    label = check_confusion(dev, x, w, b, nc, size, 255)
    HC.check_labels(label, ref, excluded, f"nc {nc} shape {shape} -> {size}", HC.count_cap)


def test_side_stream_gives_the_same_bytes(dev):
    from mdil_ss_amd.fullres import fullres_head
    nc, size = 27, (90, 135)
    x, w, b = HC.head_inputs(nc, (3, 16, 48))
    ids, pal = random_luts(nc)
    args = (nhwc(x).to(dev), w.to(dev), b.to(dev), size)
    kw = dict(id_map=ids.to(dev), palette=pal.to(dev))
    first = fullres_head(*args, **kw)
    torch.cuda.synchronize()
    second = HC.side_stream(lambda: fullres_head(*args, **kw))
    for a, c in zip(first, second):
        assert torch.equal(a.cpu(), c.cpu())


@pytest.fixture(scope="module")
def tiny_model(dev):
    return HC.tiny_model(dev)


def test_agrees_with_the_shipped_forward(dev, tiny_model):
    """predict_fullres() against the unfused route on the device (stored fp32 logits, torch's
    bilinear resize, torch's argmax): equal except inside the bound above, taken from the fp64
    evaluation of the same features; both routes are within gamma_k * Su of it."""
    from mdil_ss_amd.fullres import predict_fullres
    from oracle import fixtures as fx
    size = (128, 256)
    images, _ = fx.make_batch(2, 64, 128, 20, seed=100)
    images = images.to(dev)
    with torch.no_grad():
        logits = tiny_model(images, 0).float()
        want = F.interpolate(logits, size, mode="bilinear", align_corners=False).max(1)[1].cpu()
        feat = tiny_model.features(images, 0)
    label, colour = predict_fullres(tiny_model, images, 0, size)
    torch.cuda.synchronize()
    assert colour is None and tuple(label.shape) == (2,) + size
    w, b = (t.detach().cpu() for t in tiny_model.head_params(0))
    _, excluded = reference(feat.cpu().permute(0, 3, 1, 2), w, b, size)
    HC.check_labels(label.cpu(), want, excluded, "shipped path", HC.count_cap)


def test_cli_end_to_end(dev, tiny_model, tmp_path):
    """--synthetic 3 at a native size of 96 x 200 through a 64 x 128 network, in-process: PNGs of
    the native size and the right mode that hold what predict_fullres() returns, and the reported
    mIoU and matrix equal those counted here from those labels and the native labels."""
    from PIL import Image
    from mdil_ss_amd import fullres as FR
    from mdil_ss_amd.dataset import ProceduralSeg
    from mdil_ss_amd.predict import default_palette
    ckpt, out, report_file = tmp_path / "checkpoint.pth.tar", tmp_path / "maps", tmp_path / "report.json"
    HC.save_checkpoint(tiny_model, ckpt)
    report = FR.main(FR.build_parser().parse_args(
        ["--state", str(ckpt), "--num-classes", "20", "20", "--task", "1", "--synthetic", "3", "--native-height", "96",
         "--native-width", "200", "--height", "64", "--width", "128", "--score", "--json", str(report_file),
         "--out", str(out), "--colour"]))
    files = sorted(glob.glob(str(out / "*.png")))
    assert len(files) == 6 and sorted(report["written"]) == files
    ds = ProceduralSeg(3, 96, 200, 20, seed=13, domain=1)
    samples = [FR.synthetic_sample(ds, i, 64, 128) for i in range(3)]
    images = torch.from_numpy(np.stack([im for im, _ in samples])).to(dev).permute(0, 3, 1, 2).float().div(255.0)
    native = torch.stack([ds[i][1][0] for i in range(3)])
    assert all(torch.equal(torch.from_numpy(lab).long(), native[i]) for i, (_, lab) in enumerate(samples))
    pal = default_palette(20)
    label, colour = (t.cpu() for t in FR.predict_fullres(tiny_model, images, 1, (96, 200), palette=pal.to(dev)))
    for i in range(3):
        maps = {}
        for kind, mode in (("label", "L"), ("colour", "RGB")):
            with Image.open(os.path.join(out, f"synthetic_{i:04d}_{kind}.png")) as im:
                assert im.size == (200, 96) and im.mode == mode, (kind, im.size, im.mode)
                maps[kind] = torch.from_numpy(np.array(im))
        assert torch.equal(maps["label"], label[i])
        assert torch.equal(maps["colour"], colour[i]) and torch.equal(maps["colour"], pal[label[i].long()])
    matrix, n_bad, n_counted = expected_counts(native, label, 20, 19)
    assert n_bad == 0 and report["confusion"] == matrix.tolist() and report["pixels"] == n_counted
    tp = matrix.diagonal().double()
    iou = (tp / (matrix.sum(0) + matrix.sum(1) - tp + 1e-15))[:19]
    assert report["mIoU"] == iou.mean().item() and report["iou_classes"] == iou.tolist()
    assert json.load(open(report_file))["confusion"] == matrix.tolist()
