"""GPU: the boundary kernels (mdil_ss_amd/ext/boundary.hip) and the entry points over them
(mdil_ss_amd/boundary.py) against the numpy reference of tests/boundary_reference.py.  The kernel is
integer only, so every comparison is exact equality: both distance maps and all six counters.  The
cases sit where a tiled two-pass kernel can go wrong: maps smaller than the band, widths that are no
multiple of four pixels, rows longer than one wavefront's chunk of 256, a cap above the height,
several images in one call, one-pixel stripes, labels outside the classes."""
import functools
import glob
import json
import os

import numpy as np
import pytest
import torch

from tests import boundary_reference as R
from tests import head_cases as HC

pytestmark = pytest.mark.gpu

ALL8 = (1, 2, 4, 8, 16, 32, 64, 128)


@pytest.fixture(scope="module")
def dev():
    return HC.device("boundary")


def perturbed(target, n_labels, seed, shift=2, share=0.01):
    """A prediction: the target moved ``shift`` pixels right and down, ``share`` of the pixels redrawn."""
    rng = np.random.default_rng(seed)
    pred = np.roll(target, (shift, shift), axis=(-2, -1))
    flip = rng.random(target.shape) < share
    pred[flip] = rng.integers(0, n_labels, int(flip.sum()), dtype=np.uint8)
    return np.ascontiguousarray(pred)


@functools.lru_cache(maxsize=None)
def procedural(nc):
    from mdil_ss_amd.dataset import ProceduralSeg
    ds = ProceduralSeg(2, 96, 200, nc, seed=2, domain=1)
    target = np.stack([ds[i][1][0].numpy().astype(np.uint8) for i in range(2)])
    return perturbed(target, nc, seed=nc), target


def stripes():
    t = np.zeros((1, 21, 45), dtype=np.uint8)
    t[0, :, 17] = 3                                         # one pixel wide, top to bottom
    t[0, 9, :] = 5                                          # one pixel high, left to right (cuts the other)
    p = np.zeros_like(t)
    p[0, :, 18] = 3
    p[0, 10, 4:40] = 5
    return p, t


def out_of_range(nc):
    t = R.blocky((2, 33, 47), nc + 3, seed=3)               # labels nc, nc + 1, nc + 2 are outside the classes
    p = R.blocky((2, 33, 47), nc + 2, seed=4, block=7)
    t[0, 5:9, 5:30] = 255
    p[1, 20:25, :] = 200
    return p, t


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (pred, target u8 [N,H,W], nc, widths, ignore_index, expected distances and counters);
    computed once, shared and never modified."""
    if name == "one pixel":
        p, t, nc, widths, ign = np.zeros((1, 1, 1), np.uint8), np.ones((1, 1, 1), np.uint8), 2, (1,), -1
    elif name == "smaller than the band":
        t = R.blocky((1, 5, 3), 2, seed=5, block=2)
        p, nc, widths, ign = perturbed(t, 2, 5, shift=1, share=0.1), 2, (8,), -1
    elif name == "odd width, two images":
        t = R.blocky((2, 37, 130), 20, seed=6, block=11)
        p, nc, widths, ign = perturbed(t, 20, 6), 20, (1, 3, 7), 19
    elif name == "cap above the height":
        t = R.blocky((1, 70, 257), 5, seed=7, block=60)
        p, nc, widths, ign = perturbed(t, 5, 7), 5, ALL8, 4
    elif name == "one label everywhere":
        t = np.full((3, 64, 64), 6, dtype=np.uint8)
        p, nc, widths, ign = t.copy(), 8, (2, 20), -1
    elif name in ("procedural 20", "procedural 27"):
        nc = int(name.split()[1])
        (p, t), widths, ign = procedural(nc), (2, 5, 12), 19 if nc == 20 else -1
    elif name == "published width":
        t = R.blocky((1, 300, 520), 7, seed=8, block=97)
        p, nc, widths, ign = perturbed(t, 7, 8, shift=3), 7, (46,), 6
    elif name == "two classes":
        t = R.blocky((1, 40, 72), 2, seed=9, block=13)
        p, nc, widths, ign = perturbed(t, 2, 9), 2, (1, 4), -1
    elif name == "32 classes":
        t = R.blocky((1, 40, 72), 32, seed=10, block=6)
        p, nc, widths, ign = perturbed(t, 32, 10, share=0.05), 32, ALL8, 31
    elif name == "stripes":
        (p, t), nc, widths, ign = stripes(), 8, (1, 2, 6), -1
    elif name == "labels outside the classes":
        (p, t), nc, widths, ign = out_of_range(6), 6, (2, 4), 255
    elif name == "past the grid bounds":
        # the row pass strides beyond 8192 work-groups of 4 rows (2 x 16500 rows), the column pass
        # beyond 2048 work-groups of 256 lanes of 4 pixels (16500 x 34 items)
        t = R.blocky((1, 16500, 136), 9, seed=12, block=23)
        p, nc, widths, ign = perturbed(t, 9, 12, share=0.002), 9, (1, 3), 8
        assert 2 * 16500 > 8192 * 4 and 16500 * 34 > 2048 * 256
    else:
        raise KeyError(name)
    cap = widths[-1]
    dp, dt = R.distances(p, cap), R.distances(t, cap)
    if p.size <= 2000:                                      # the definition itself where it is cheap
        assert np.array_equal(dp, R.distances(p, cap, R.distance_brute))
        assert np.array_equal(dt, R.distances(t, cap, R.distance_brute))
    return p, t, nc, widths, ign, dp, dt, R.counters(p, t, dp, dt, nc, widths, ign)


CASES = ["one pixel", "smaller than the band", "odd width, two images", "cap above the height",
         "one label everywhere", "procedural 20", "procedural 27", "published width", "two classes", "32 classes",
         "stripes", "labels outside the classes", "past the grid bounds"]


def run(dev, p, t, nc, widths, ign, dist=True, counters=None, **kw):
    from mdil_ss_amd import boundary as B
    counters = B.new_counters(nc, len(widths) + 1, dev) if counters is None else counters
    dp, dt = B.boundary_count(torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev), nc, widths, ignore_index=ign,
                              counters=counters, dist=dist, **kw)
    torch.cuda.synchronize()
    return (None if dp is None else dp.cpu().numpy(), None if dt is None else dt.cpu().numpy(),
            {k: v.cpu().numpy() for k, v in counters.items()})


def check_counters(got, want, times=1):
    assert sorted(got) == sorted(R.COUNTERS)
    for k in R.COUNTERS:
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], times * want[k]), k


@pytest.mark.parametrize("name", CASES)
def test_distances_and_counters_are_exact(dev, name):
    p, t, nc, widths, ign, dp, dt, want = case(name)
    got_p, got_t, got = run(dev, p, t, nc, widths, ign)
    assert got_p.dtype == np.uint8 and got_p.shape == p.shape
    assert np.array_equal(got_p, dp), f"dist_pred differs at {int((got_p != dp).sum())} of {dp.size} pixels"
    assert np.array_equal(got_t, dt), f"dist_target differs at {int((got_t != dt).sum())} of {dt.size} pixels"
    check_counters(got, want)
    counted = int(((t != ign) & (t < nc) & (p < nc)).sum())
    assert got["confusion"].sum() == got["target_hist"].sum() == got["pred_hist"].sum() == counted


def test_the_cases_reach_what_they_are_for():
    """Properties of the inputs, so that a case cannot quietly stop testing its point."""
    p, t, nc, widths, ign, dp, dt, want = case("labels outside the classes")
    assert want["bad_targets"][0] > 0 and want["bad_preds"][0] > 0 and (t == ign).any()
    assert ((t >= nc) & (t != ign) & (p >= nc)).any()          # both bad: a bad target, nothing else
    assert want["confusion"].sum() + want["bad_targets"][0] + want["bad_preds"][0] + (t == ign).sum() == t.size
    assert case("cap above the height")[6].max() < 129 and case("published width")[6].max() == 47
    assert (case("one label everywhere")[6][:, 32, 32] == 21).all()
    _, t, _, _, _, _, dt, _ = case("stripes")
    assert (dt[t == 3] == 1).all() and (dt[t == 5] == 1).all()
    assert (case("procedural 20")[1] == 19).any()               # the ignore class is there to be ignored
    p, t = case("odd width, two images")[:2]
    assert not np.array_equal(t[0], t[1]) and t.shape[2] % 4 != 0


@pytest.mark.parametrize("name", ["odd width, two images", "procedural 20"])
def test_counters_accumulate_and_dist_is_optional(dev, name):
    from mdil_ss_amd import boundary as B
    p, t, nc, widths, ign, dp, dt, want = case(name)
    counters = B.new_counters(nc, len(widths) + 1, dev)
    ws = torch.empty(B.workspace_bytes(*p.shape) + 64, dtype=torch.uint8, device=dev)
    a = run(dev, p, t, nc, widths, ign, dist=False, counters=counters, workspace=ws)
    assert a[0] is None and a[1] is None
    check_counters(a[2], want)                                # without the distance maps: the same counts
    b = run(dev, p, t, nc, widths, ign, dist=True, counters=counters, workspace=ws)
    assert np.array_equal(b[0], dp) and np.array_equal(b[1], dt)
    check_counters(b[2], want, times=2)                       # added to, never cleared


def test_images_of_a_batch_never_see_each_other(dev):
    """Each image alone gives the distances it has inside the batch, and the counts add up."""
    p, t, nc, widths, ign, dp, dt, want = case("odd width, two images")
    total = None
    for n in range(p.shape[0]):
        got_p, got_t, got = run(dev, p[n:n + 1].copy(), t[n:n + 1].copy(), nc, widths, ign)
        assert np.array_equal(got_p[0], dp[n]) and np.array_equal(got_t[0], dt[n])
        total = got if total is None else {k: total[k] + got[k] for k in got}
    check_counters(total, want)


def test_side_stream_gives_the_same(dev):
    p, t, nc, widths, ign, dp, dt, want = case("procedural 27")
    got_p, got_t, got = HC.side_stream(lambda: run(dev, p, t, nc, widths, ign))
    assert np.array_equal(got_p, dp) and np.array_equal(got_t, dt)
    check_counters(got, want)


def test_guard_bands_and_the_workspace_bound(dev):
    """Distance maps inside a 0xA5-filled arena and a workspace of exactly the promised size with a
    guard behind it: nothing outside what the header names is written."""
    from mdil_ss_amd import _boundary_lib
    from mdil_ss_amd import boundary as B
    lib = _boundary_lib.load()
    p, t, nc, widths, ign, dp, dt, want = case("odd width, two images")
    N, H, W = p.shape
    npx = p.size
    need = lib.mdil_boundary_workspace_bytes(N, H, W)
    arena = HC.Arena(dev, {"dist_pred": npx, "dist_target": npx, "workspace": need})
    counters = B.new_counters(nc, len(widths) + 1, dev)
    pd, td = torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev)
    import ctypes as C
    rc = lib.mdil_boundary_count(pd.data_ptr(), td.data_ptr(), N, H, W, nc, (C.c_int * len(widths))(*widths),
                                 len(widths), ign, arena.ptr("workspace"), need, arena.ptr("dist_pred"),
                                 arena.ptr("dist_target"),
                                 *(counters[k].data_ptr() for k in B.COUNTERS),
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mdil_boundary_last_error()
    torch.cuda.synchronize()
    arena.read()
    arena.assert_untouched(("dist_pred", "dist_target", "workspace"))
    assert (arena.cut("workspace")[2 * npx:] == 0xA5).all()    # used: the capped run distances of both maps
    assert np.array_equal(arena.cut("dist_pred").numpy().reshape(p.shape), dp)
    assert np.array_equal(arena.cut("dist_target").numpy().reshape(p.shape), dt)
    check_counters({k: v.cpu().numpy() for k, v in counters.items()}, want)


@pytest.fixture(scope="module")
def tiny_model(dev):
    return HC.tiny_model(dev)


def test_every_bin_together_is_the_confusion_matrix_of_fullres(dev):
    """The same features and target through BoundaryMeter and through the shipped ConfusionMeter:
    confusion.sum(0) is its matrix bit for bit, and the scores over every bin are its scores."""
    from mdil_ss_amd import boundary as B
    from mdil_ss_amd import fullres as F
    nc, size = 20, (45, 77)
    g = torch.Generator().manual_seed(3)
    x = torch.relu(torch.randn(2, 12, 20, 16, generator=g)).to(dev)
    w, b = (torch.randn(16, nc, 2, 2, generator=g) * 0.3).to(dev), (torch.randn(nc, generator=g) * 0.2).to(dev)
    target = torch.from_numpy(R.blocky((2,) + size, nc, seed=11, block=9)).to(dev)
    shipped = F.ConfusionMeter(nc, nc - 1)
    label = shipped.add(x, w, b, target=target)[0]
    meter = B.BoundaryMeter(nc, nc - 1, widths=[1, 3, 9])
    pred, dist_p, dist_t = meter.add(x, w, b, target=target, dist=True)
    assert torch.equal(pred, label) and dist_p.shape == dist_t.shape == label.shape
    counters = meter.counters()
    assert torch.equal(counters["confusion"].sum(0), shipped.matrix())
    rep = meter.report()
    mean, per_class = shipped.iou()
    assert rep["mIoU"] == mean.item() and rep["iou_classes"] == per_class.tolist()
    # and the counters are the reference's on the kernel's own label map
    p, t = pred.cpu().numpy(), target.cpu().numpy()
    dp, dt = R.distances(p, 9), R.distances(t, 9)
    assert np.array_equal(dist_p.cpu().numpy(), dp) and np.array_equal(dist_t.cpu().numpy(), dt)
    check_counters({k: v.numpy() for k, v in counters.items()}, R.counters(p, t, dp, dt, nc, [1, 3, 9], nc - 1))


def test_meter_ratio_mode_and_bad_labels(dev):
    from mdil_ss_amd import boundary as B
    p, t, nc, widths, ign, dp, dt, want = case("procedural 20")
    meter = B.BoundaryMeter(nc, ign, ratio=0.03)              # 96 x 200: round(0.03 * 221.8) = 7
    pd, td = torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev)
    meter.add(pd, td)
    meter.add(pd[:, :40, :64].contiguous(), td[:, :40, :64].contiguous())      # round(0.03 * 75.5) = 2
    rep = meter.report()
    assert rep["widths_used"] == [2, 7] and rep["widths"] == [None] and len(rep["boundary_iou"]) == 1
    d7 = R.counters(p, t, R.distances(p, 7), R.distances(t, 7), nc, [7], ign)
    ps, ts = np.ascontiguousarray(p[:, :40, :64]), np.ascontiguousarray(t[:, :40, :64])
    d2 = R.counters(ps, ts, R.distances(ps, 2), R.distances(ts, 2), nc, [2], ign)
    check_counters({k: v.numpy() for k, v in meter.counters().items()}, {k: d7[k] + d2[k] for k in d7})
    bad = td.clone()
    bad[0, 0, :5] = 77
    meter.add(pd, bad)
    with pytest.raises(RuntimeError, match="5 target pixels are outside"):
        meter.report()
    meter = B.BoundaryMeter(nc, ign, widths=[3])
    worse = pd.clone()
    worse[1, 3, :9] = 99
    meter.add(worse, td)
    n_bad = int((td[1, 3, :9] != ign).sum())
    with pytest.raises(RuntimeError, match=f"{n_bad} predicted pixels are outside"):
        meter.report()


def test_cli_end_to_end(dev, tiny_model, tmp_path):
    """--synthetic 3 at a native size of 96 x 200 through a 64 x 128 network, in-process: once from
    the checkpoint with --score --json --out, once with --pred on the label PNGs that a
    ``fullres --out`` run wrote.  Both reports hold the same counters, those of the reference on the
    label maps of ``predict_fullres``; the band PNGs have the native size and only the three colours."""
    from PIL import Image
    from mdil_ss_amd import boundary as B
    from mdil_ss_amd import fullres as FR
    from mdil_ss_amd.dataset import ProceduralSeg
    ckpt, maps, bands = tmp_path / "checkpoint.pth.tar", tmp_path / "maps", tmp_path / "bands"
    first, second = tmp_path / "first.json", tmp_path / "second.json"
    HC.save_checkpoint(tiny_model, ckpt)
    data = ["--num-classes", "20", "20", "--task", "1", "--synthetic", "3", "--native-height", "96",
            "--native-width", "200", "--height", "64", "--width", "128"]
    a = B.main(B.build_parser().parse_args(data + ["--state", str(ckpt), "--widths", "1", "3", "8", "--score", "--json",
                                                   str(first), "--out", str(bands)]))
    FR.main(FR.build_parser().parse_args(data + ["--state", str(ckpt), "--out", str(maps)]))
    b = B.main(B.build_parser().parse_args(data + ["--pred", str(maps), "--widths", "1", "3", "8", "--score", "--json",
                                                   str(second)]))
    ja, jb = json.load(open(first)), json.load(open(second))
    assert ja["counters"] == jb["counters"] == a["counters"] == b["counters"]
    for k in ("boundary_iou", "trimap_iou", "interior_iou", "mIoU", "iou_classes", "pixels", "widths"):
        assert ja[k] == jb[k] == a[k], k
    assert jb["written"] == [] and ja["images"] == 3

    ds = ProceduralSeg(3, 96, 200, 20, seed=13, domain=1)
    samples = [FR.synthetic_sample(ds, i, 64, 128) for i in range(3)]
    images = torch.from_numpy(np.stack([im for im, _ in samples])).to(dev).permute(0, 3, 1, 2).float().div(255.0)
    t = np.stack([lab for _, lab in samples])
    p = FR.predict_fullres(tiny_model, images, 1, (96, 200))[0].cpu().numpy()
    dp, dt = R.distances(p, 8), R.distances(t, 8)
    want = R.counters(p, t, dp, dt, 20, [1, 3, 8], 19)
    assert a["counters"] == {k: want[k].tolist() for k in R.COUNTERS}
    assert a["pixels"] == int(want["confusion"].sum()) > 0

    files = sorted(glob.glob(str(bands / "*.png")))
    assert len(files) == 3 and sorted(a["written"]) == files
    for i, f in enumerate(files):
        assert os.path.basename(f) == f"synthetic_{i:04d}_boundary.png"
        with Image.open(f) as im:
            assert im.size == (200, 96) and im.mode == "RGB"
            img = np.array(im)
        band = dt[i] <= 8
        assert (img[~band] == B.GREY).all()
        assert (img[band & (p[i] == t[i])] == B.RIGHT).all() and (img[band & (p[i] != t[i])] == B.WRONG).all()

    # a label PNG of another size than its label is refused
    Image.fromarray(np.zeros((96, 100), dtype=np.uint8)).save(maps / "synthetic_0001_label.png")
    with pytest.raises(RuntimeError, match="synthetic_0001_label.png is 96 x 100, its label 96 x 200"):
        B.main(B.build_parser().parse_args(data + ["--pred", str(maps), "--score"]))
