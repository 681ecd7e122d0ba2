"""GPU: the fused multi-view kernel (mdil_ss_amd/ext/ensemble_head.hip) and the entry points over it
(mdil_ss_amd/ensemble.py) against the fp64 reference of tests/ensemble_reference.py, which also says
which pixels may differ and why (the kernel header's ``k`` roundings per resized logit and
``softmax: cs u``): a pixel whose fp64 top-2 margin is within its two classes' bounds is excluded,
every other pixel must equal the fp64 argmax, and at most max(1, pixels // 1000) pixels of a case
may be excluded -- none in a case of fewer than 100."""
import glob
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ensemble_reference as R
from tests import head_cases as HC
from tests.head_cases import U, expected_counts, make_target, nhwc, random_luts

pytestmark = pytest.mark.gpu

NCASES = range(len(R.CASES))


@pytest.fixture(scope="module")
def dev():
    return HC.device("ensemble")


def run(dev, xs, flips, w, b, size, mode, **kw):
    from mdil_ss_amd.ensemble import ensemble_head
    kw = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    views = [(nhwc(x).to(dev), bool(f)) for x, f in zip(xs, flips)]
    out = ensemble_head(views, w.to(dev), b.to(dev), size, mode=mode, **kw)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu() for t in out)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("index", NCASES)
@pytest.mark.parametrize("nc", R.CLASSES)
def test_labels_match_fp64_argmax(dev, nc, index, mode):
    xs, w, b, flips, size, _, ref, excluded, _ = R.case(nc, index, mode)
    label, colour, conf = run(dev, xs, flips, w, b, size, mode)
    assert colour is None and conf is None
    HC.check_labels(label, ref, excluded, f"nc {nc} case {index} {mode}", HC.count_cap)


def check_confusion(dev, xs, flips, w, b, nc, size, mode, ignore):
    from mdil_ss_amd.ensemble import ensemble_head
    args = ([(nhwc(x).to(dev), bool(f)) for x, f in zip(xs, flips)], w.to(dev), b.to(dev), size)
    head = lambda **kw: ensemble_head(*args, mode=mode, **kw)  # noqa: E731
    return HC.check_confusion(head, dev, nc, xs[0].shape[0], size, ignore)


@pytest.mark.parametrize("mode", R.MODES)
def test_grid_stride_loop_past_the_grid_bound(dev, mode):
    """The grid is bounded at 8192 work-groups of 64 lanes, a lane owning two pixels of a row: 1025
    rows of ceil(2051 / 2) = 1026 items are 1,051,650 items, so every lane goes round the loop a
    second time and some a third, with odd sizes on both axes."""
    xs, w, b, flips, size, _, ref, excluded, _ = R.case(R.BIG_NC, -1, mode)
    assert size[0] * ((size[1] + 1) // 2) > 2 * 8192 * 64
    label = check_confusion(dev, xs, flips, w, b, R.BIG_NC, size, mode, 255)
    HC.check_labels(label, ref, excluded, f"bounded-grid case {mode}", HC.count_cap)


@pytest.mark.parametrize("index", (0, 2, 4, 6))
@pytest.mark.parametrize("nc", R.CLASSES)
def test_one_plain_view_in_logit_mode_is_fullres_head(dev, nc, index):
    """One unmirrored view in logit mode runs fullres_head's operations in fullres_head's order (the
    kernel's header says so): the same bytes, not only the same labels outside the exclusion."""
    from mdil_ss_amd.fullres import fullres_head
    xs, w, b = R.case_inputs(nc, index)
    size = R.CASES[index][2]
    ids, pal = random_luts(nc)
    label, colour, _ = run(dev, xs[:1], [0], w, b, size, "logit", id_map=ids, palette=pal)
    want = fullres_head(nhwc(xs[0]).to(dev), w.to(dev), b.to(dev), size, id_map=ids.to(dev), palette=pal.to(dev))
    assert torch.equal(label, want[0].cpu()) and torch.equal(colour, want[1].cpu())


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("index", (1, 2, 4, 5, 7))
def test_a_mirrored_view_is_the_flipped_view(dev, index, mode):
    """l'[y, j] = l[y, 2W - 1 - j]: logit column 2w + b of the mirrored view is column
    2 (W - 1 - w) + (1 - b) of the plain one, so flagging a view mirrored is the same as flipping its
    FEATURES along W and swapping the two kernel columns (flipping the features alone would leave
    every 2 x 2 block of logits unmirrored inside).  w is shared by the views of a call, so all of
    them are flagged here.  The kernel runs the same arithmetic on the same numbers in the same
    order in both cases (its header says so): torch.equal, labels and confidence."""
    nc = 20
    xs, w, b = R.case_inputs(nc, index)
    size = R.CASES[index][2]
    flagged = run(dev, xs, [1] * len(xs), w, b, size, mode, confidence=True)
    flipped = run(dev, [x.flip(3) for x in xs], [0] * len(xs), w.flip(3).contiguous(), b, size, mode, confidence=True)
    assert torch.equal(flagged[0], flipped[0]) and torch.equal(flagged[2], flipped[2])
    if index >= 2:                                       # and the flag does something
        assert not torch.equal(run(dev, xs, [0] * len(xs), w, b, size, mode)[0], flagged[0])
    # against the reference, which flips the LOGITS
    k, cs = R.header_constants()
    _, ref, excluded, _ = R.reference(xs, w, b, [1] * len(xs), size, mode, k, cs)
    wrong = (flagged[0].long() != ref) & ~excluded
    assert not wrong.any()


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("index", (3, 4, 6))
def test_view_order_changes_labels_only_inside_the_exclusion(dev, index, mode):
    nc = 27
    xs, w, b, flips, size, _, ref, excluded, _ = R.case(nc, index, mode)
    first = run(dev, xs, flips, w, b, size, mode)[0]
    perm = torch.randperm(len(xs), generator=torch.Generator().manual_seed(index)).tolist()
    perm = perm if perm != list(range(len(xs))) else perm[::-1]
    second = run(dev, [xs[i] for i in perm], [flips[i] for i in perm], w, b, size, mode)[0]
    assert not ((first != second) & ~excluded).any()
    HC.check_labels(second, ref, excluded, f"nc {nc} case {index} {mode} permuted {perm}", HC.count_cap)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("index", NCASES)
@pytest.mark.parametrize("nc", (2, 20, 32))
def test_confidence(dev, nc, index, mode):
    """prob: S_max / nviews, within B_winner / nviews + 4 u (the division and the conversion of the
    reference) of the fp64 value.  logit: the winner's softmax of S / nviews; every S_c / nviews is
    within B_max / nviews, which moves the probability by at most 2 p (1 - p) B_max / nviews to
    first order, and the softmax arithmetic adds cs u."""
    xs, w, b, flips, size, S, ref, excluded, B = R.case(nc, index, mode)
    nv = len(xs)
    k, cs = R.header_constants()
    label, _, conf = run(dev, xs, flips, w, b, size, mode, confidence=True)
    assert conf.dtype == torch.float32 and tuple(conf.shape) == tuple(ref.shape)
    assert torch.equal(label, run(dev, xs, flips, w, b, size, mode)[0])
    assert (conf > 0).all() and (conf <= 1).all()
    if mode == "prob":
        want = S.max(1)[0] / nv
        bound = B.gather(1, ref[:, None])[:, 0] / nv + 4 * U
    else:
        want = (S / nv).softmax(1).max(1)[0]
        bound = 2 * want * (1 - want) * (B.max(1)[0] / nv) + cs * U
    err = (conf.double() - want).abs()
    keep = ~excluded
    print(f"nc {nc} case {index} {mode}: worst error / bound {float((err / bound)[keep].max()) if keep.any() else 0:.3f}")
    assert (err <= bound)[keep].all()


@pytest.mark.parametrize("mode", R.MODES)
def test_ties_go_to_the_lowest_class(dev, mode):
    """Classes 3 and 11 with bit-identical weights and bias tie exactly in every view, so in the sum
    too; with the largest bias they are also the winners almost everywhere."""
    xs, w, b = R.case_inputs(20, 4)
    flips, size = R.CASES[4][1], R.CASES[4][2]
    w, b = w.clone(), b.clone()
    b[3] = b.max() + 8.0
    w[:, 11], b[11] = w[:, 3], b[3]
    label = run(dev, xs, flips, w, b, size, mode)[0]
    assert not (label == 11).any()
    assert (label == 3).double().mean() > 0.5


def test_nan_rules(dev):
    """A NaN in one view of three.  Where it reaches a pixel, every class of that view is NaN there
    (the feature meets every class), so is every S_c, and the first class wins; elsewhere the
    labels are those of the clean inputs.  A NaN bias at classes 7 and 12: in logit mode the first
    NaN class wins everywhere; in prob mode the softmax makes every class NaN: class 0."""
    nc, index = 20, 5
    xs, w, b = R.case_inputs(nc, index)
    flips, size = R.CASES[index][1], R.CASES[index][2]
    xn = [x.clone() for x in xs]
    xn[1][1, 5, 4, 7] = float("nan")
    k, cs = R.header_constants()
    hit = torch.isnan(R.reference(xn, w, b, flips, size, "logit", k, cs)[0]).any(1)
    assert 0 < int(hit.sum()) < 400 and not hit[0].any()
    bn = b.clone()
    bn[7] = bn[12] = float("nan")
    for mode in R.MODES:
        clean = run(dev, xs, flips, w, b, size, mode)[0]
        label = run(dev, xn, flips, w, b, size, mode)[0]
        assert (label[hit] == 0).all(), mode
        assert torch.equal(label[~hit], clean[~hit]), mode
        assert (run(dev, xs, flips, w, bn, size, mode)[0] == (7 if mode == "logit" else 0)).all(), mode


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("index", (0, 2, 5, 6))
@pytest.mark.parametrize("nc", R.CLASSES)
def test_id_map_palette_and_confusion(dev, nc, index, mode):
    """id_map and palette are applied after the argmax; the matrix counts the kernel's own labels
    (the train ids), accumulates over two calls, and out-of-range targets go to bad_targets."""
    xs, w, b = R.case_inputs(nc, index)
    flips, size = R.CASES[index][1], R.CASES[index][2]
    ids, pal = random_luts(nc)
    plain = run(dev, xs, flips, w, b, size, mode)[0]
    label, colour, _ = run(dev, xs, flips, w, b, size, mode, id_map=ids, palette=pal)
    assert colour.dtype == torch.uint8 and tuple(colour.shape) == tuple(plain.shape) + (3,)
    assert torch.equal(label, ids[plain.long()]) and torch.equal(colour, pal[plain.long()])
    for ignore in (nc - 1, 255):
        assert torch.equal(check_confusion(dev, xs, flips, w, b, nc, size, mode, ignore), plain)


def test_ensemble_meter(dev):
    from mdil_ss_amd.ensemble import EnsembleMeter
    from mdil_ss_amd.fullres import ConfusionMeter
    nc, index = 20, 4
    xs, w, b = R.case_inputs(nc, index)
    flips, size = R.CASES[index][1], R.CASES[index][2]
    views = [(nhwc(x).to(dev), bool(f)) for x, f in zip(xs, flips)]
    target = make_target(nc, (2,) + size, nc - 1, seed=5)
    clean = target.clone()
    clean[clean >= nc] = nc - 1
    meter = EnsembleMeter(nc, nc - 1)
    assert isinstance(meter, ConfusionMeter) and EnsembleMeter.iou is ConfusionMeter.iou \
        and EnsembleMeter.matrix is ConfusionMeter.matrix
    label = meter.add(views, w.to(dev), b.to(dev), target=clean.to(dev), mode="prob")[0].cpu()
    assert torch.equal(label, run(dev, xs, flips, w, b, size, "prob")[0])
    matrix, n_bad, _ = expected_counts(clean, label, nc, nc - 1)
    assert n_bad == 0 and torch.equal(meter.matrix(), matrix)
    tp = matrix.diagonal().double()
    want = (tp / (matrix.sum(0) + matrix.sum(1) - tp + 1e-15))[:nc - 1]
    mean, per_class = meter.iou()
    assert torch.equal(per_class, want) and mean.item() == want.mean().item()
    meter.add(views, w.to(dev), b.to(dev), target=target.to(dev))
    with pytest.raises(RuntimeError, match=f"{int((target >= nc).sum())} target pixels are outside"):
        meter.matrix()


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("index", (2, 5))
def test_null_outputs_and_guard_bands_stay_untouched(dev, index, mode):
    """One 0xA5-filled arena [guard | label | guard | colour | guard | confidence | guard] and
    pre-filled confusion / bad_targets: nothing outside the requested maps changes; with
    target = NULL the two counters keep their bytes although their pointers are passed."""
    from mdil_ss_amd import _ensemble_lib
    lib = _ensemble_lib.load()
    nc = 27
    xs, w, b = R.case_inputs(nc, index)
    flips, size = R.CASES[index][1], R.CASES[index][2]
    ids, pal = random_luts(nc)
    plain, _, conf_ref = run(dev, xs, flips, w, b, size, mode, confidence=True)
    plain = plain.reshape(-1)
    N = xs[0].shape[0]
    npx = N * size[0] * size[1]
    feats = [nhwc(x).to(dev) for x in xs]
    table = _ensemble_lib.view_table([(f.data_ptr(), f.shape[1], f.shape[2], m) for f, m in zip(feats, flips)])
    wd, bd, idd, pd = w.to(dev), b.to(dev), ids.to(dev), pal.to(dev)
    target = make_target(nc, (N,) + size, nc - 1, seed=1).to(dev)
    for with_colour, with_conf, with_target in ((False, False, False), (True, False, False), (False, True, False),
                                                (True, True, True)):
        arena = HC.Arena(dev, {"label": npx, "colour": 3 * npx, "confidence": 4 * npx})
        conf = torch.full((nc, nc), 7, dtype=torch.int64, device=dev)
        bad = torch.full((1,), 5, dtype=torch.int64, device=dev)
        rc = lib.mdil_ensemble_head(table, len(feats), wd.data_ptr(), bd.data_ptr(), N, nc, size[0], size[1],
                                    _ensemble_lib.MODES[mode], idd.data_ptr(), pd.data_ptr(),
                                    target.data_ptr() if with_target else None, nc - 1, arena.ptr("label"),
                                    arena.ptr("colour") if with_colour else None,
                                    arena.ptr("confidence") if with_conf else None,
                                    conf.data_ptr(), bad.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.mdil_ensemble_last_error()
        torch.cuda.synchronize()
        arena.read()
        on = (("label", True), ("colour", with_colour), ("confidence", with_conf))
        arena.assert_untouched([k for k, given in on if given], (with_colour, with_conf, with_target))
        assert torch.equal(arena.cut("label"), ids[plain.long()])
        if with_colour:
            assert torch.equal(arena.cut("colour").reshape(-1, 3), pal[plain.long()])
        if with_conf:
            assert torch.equal(arena.cut("confidence").clone().view(torch.float32), conf_ref.reshape(-1))
        if with_target:
            matrix, n_bad, _ = expected_counts(target.cpu(), plain, nc, nc - 1)
            assert torch.equal(conf.cpu(), matrix + 7) and int(bad.item()) == n_bad + 5
        else:
            assert (conf.cpu() == 7).all() and int(bad.item()) == 5


@pytest.mark.parametrize("mode", R.MODES)
def test_side_stream_gives_the_same_bytes(dev, mode):
    from mdil_ss_amd.ensemble import ensemble_head
    nc, index = 27, 6
    xs, w, b = R.case_inputs(nc, index)
    flips, size = R.CASES[index][1], R.CASES[index][2]
    ids, pal = random_luts(nc)
    args = ([(nhwc(x).to(dev), bool(f)) for x, f in zip(xs, flips)], w.to(dev), b.to(dev), size)
    kw = dict(mode=mode, id_map=ids.to(dev), palette=pal.to(dev), confidence=True)
    first = ensemble_head(*args, **kw)
    torch.cuda.synchronize()
    second = HC.side_stream(lambda: ensemble_head(*args, **kw))
    for a, c in zip(first, second):
        assert torch.equal(a.cpu(), c.cpu())


@pytest.fixture(scope="module")
def tiny_model(dev):
    return HC.tiny_model(dev)


SCALES = (0.75, 1.0, 1.25)


def test_agrees_with_the_shipped_forward(dev, tiny_model):
    """predict_ensemble() against the unfused route on the device (the shipped forward's stored
    fp32 logits, flipped back, torch's bilinear resize, softmax, running sum, torch's argmax): equal
    except inside the exclusion, taken from the fp64 evaluation of the same features."""
    from mdil_ss_amd.ensemble import predict_ensemble
    from oracle import fixtures as fx
    size = (128, 256)
    images, _ = fx.make_batch(2, 64, 128, 20, seed=100)
    images = images.to(dev)
    views = [images if hw == (64, 128) else F.interpolate(images, hw, mode="bilinear", align_corners=False)
             for hw in ((48, 96), (64, 128), (80, 160))]
    total, feats, flips = 0, [], []
    with torch.no_grad():
        for v in views:
            for mirrored in (False, True):
                src = v.flip(3).contiguous() if mirrored else v
                logits = tiny_model(src, 0).float()
                logits = logits.flip(3) if mirrored else logits
                total = total + F.interpolate(logits, size, mode="bilinear", align_corners=False).softmax(1)
                feats.append(tiny_model.features(src, 0).cpu().permute(0, 3, 1, 2))
                flips.append(int(mirrored))
        want = total.max(1)[1].cpu()
    label, colour, conf = predict_ensemble(tiny_model, views, 0, size, scales=SCALES, flip=True)
    torch.cuda.synchronize()
    assert colour is None and conf is None and tuple(label.shape) == (2,) + size
    w, b = (t.detach().cpu() for t in tiny_model.head_params(0))
    k, cs = R.header_constants()
    _, ref, excluded, _ = R.reference(feats, w, b, flips, size, "prob", k, cs)
    # no cap on the exclusion here: a freshly initialised network's probabilities are close to uniform, so
    # far more of its pixels are fp32 near-ties (about 1 %) than of the seeded cases, whatever route computes them
    print(f"shipped path: excluded {int(excluded.sum())} of {excluded.numel()} pixels")
    label = label.cpu()
    assert not ((label.long() != ref) & ~excluded).any(), "differs from the fp64 argmax outside the exclusion"
    assert not ((label.long() != want) & ~excluded).any(), "differs from the unfused route outside the exclusion"


def test_cli_end_to_end(dev, tiny_model, tmp_path):
    """--synthetic 3 at a native size of 96 x 200 through a 64 x 128 network at scales 0.75 / 1 /
    1.25 with flips, in-process: 9 PNGs of the native size and the right mode that hold what
    predict_ensemble() returns for the views made the same way, and the reported mIoU and matrix
    equal those counted here from those labels and the native labels."""
    from PIL import Image
    from mdil_ss_amd import ensemble as E
    from mdil_ss_amd import fullres as FR
    from mdil_ss_amd.dataset import ProceduralSeg
    from mdil_ss_amd.predict import default_palette
    ckpt, out, report_file = tmp_path / "checkpoint.pth.tar", tmp_path / "maps", tmp_path / "report.json"
    HC.save_checkpoint(tiny_model, ckpt)
    report = E.main(E.build_parser().parse_args(
        ["--state", str(ckpt), "--num-classes", "20", "20", "--task", "1", "--synthetic", "3", "--native-height", "96",
         "--native-width", "200", "--height", "64", "--width", "128", "--scales", "0.75", "1", "1.25", "--flip",
         "--score", "--json", str(report_file), "--out", str(out), "--colour", "--confidence"]))
    files = sorted(glob.glob(str(out / "*.png")))
    assert len(files) == 9 and sorted(report["written"]) == files
    assert (report["scales"], report["flip"], report["mode"]) == ([0.75, 1.0, 1.25], True, "prob")
    assert all(k in report for k in ("dataset", "task", "images", "written", "mIoU", "iou_classes", "confusion",
                                     "pixels"))
    ds = ProceduralSeg(3, 96, 200, 20, seed=13, domain=1)
    native = torch.stack([ds[i][1][0] for i in range(3)])
    images = []
    for s in SCALES:
        h, w_ = E.scaled_size(64, s), E.scaled_size(128, s)
        assert (h, w_) == {0.75: (48, 96), 1.0: (64, 128), 1.25: (80, 160)}[s]
        u8 = np.stack([FR.synthetic_sample(ds, i, h, w_)[0] for i in range(3)])
        images.append(torch.from_numpy(u8).to(dev).permute(0, 3, 1, 2).float().div(255.0))
    pal = default_palette(20)
    label, colour, conf = (t.cpu() for t in E.predict_ensemble(tiny_model, images, 1, (96, 200), scales=SCALES,
                                                               flip=True, palette=pal.to(dev), confidence=True))
    conf8 = conf.mul(255.0).round().to(torch.uint8)
    for i in range(3):
        maps = {}
        for kind, mode in (("label", "L"), ("colour", "RGB"), ("conf", "L")):
            with Image.open(os.path.join(out, f"synthetic_{i:04d}_{kind}.png")) as im:
                assert im.size == (200, 96) and im.mode == mode, (kind, im.size, im.mode)
                maps[kind] = torch.from_numpy(np.array(im))
        assert torch.equal(maps["label"], label[i])
        assert torch.equal(maps["colour"], colour[i]) and torch.equal(maps["colour"], pal[label[i].long()])
        assert torch.equal(maps["conf"], conf8[i])
    matrix, n_bad, n_counted = expected_counts(native, label, 20, 19)
    assert n_bad == 0 and report["confusion"] == matrix.tolist() and report["pixels"] == n_counted
    tp = matrix.diagonal().double()
    iou = (tp / (matrix.sum(0) + matrix.sum(1) - tp + 1e-15))[:19]
    assert report["mIoU"] == iou.mean().item() and report["iou_classes"] == iou.tolist()
    assert json.load(open(report_file))["confusion"] == matrix.tolist()
