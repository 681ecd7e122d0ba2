"""GPU: the moments kernel (mdil_ss_amd/ext/similarity.hip) and the entry points over it
(mdil_ss_amd/similarity.py) against the fp64 checker tests/similarity_reference.py.

Exactness.  With integer features and pivots, |x - p| <= 8, every product (<= 64) and every partial
sum of a chain of at most 1024 rows (<= 65,536) is an integer below 2^24: fp32 holds each exactly,
the fp64 reduction too, so the state must equal the checker's bit for bit.

Rounding.  One fp32 fma chain of K terms is within K 2^-24 sum |a_k b_k| of the exact sum (one
rounding per step, relative 2^-24 each, first order); the chains are at most MDIL_SIM_CHAIN rows
long and the fp64 sum of the partials adds 2^-53 per step; the two extra units cover the second
order."""
import functools
import json
import math

import numpy as np
import pytest
import torch

from tests import head_cases as HC
from tests import similarity_reference as R

pytestmark = pytest.mark.gpu

ROWS = (1, 2, 65, 1027, 4099)
CHANNELS = ((1, 0), (16, 16), (20, 27), (128, 128), (33, 128))
CLASSES = (1, 20, 32)
BLOCKS = ("sx", "sy", "gxx", "gyy", "gxy")


@pytest.fixture(scope="module")
def dev():
    return HC.device("similarity")


def bound():
    from mdil_ss_amd import _similarity_lib
    return (_similarity_lib.CHAIN + 2) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def case(rows, cx, cy, nc, kind):
    """-> (x, y or None, labels u8 with some values >= nc, pivot_x, pivot_y or None) as numpy; never modified.
    ``kind`` "int": integers with |x - p| <= 8; "gauss": unit Gaussians around a mean of 3."""
    g = np.random.default_rng(1000 * rows + 10 * cx + cy + nc + (0 if kind == "int" else 500000))
    out = []
    for c in (cx, cy):
        if not c:
            out.append((None, None))
        elif kind == "int":
            p = g.integers(-20, 21, c)
            out.append(((p + g.integers(-8, 9, (rows, c))).astype(np.float32), p.astype(np.float32)))
        else:
            v = (3.0 + g.standard_normal((rows, c))).astype(np.float32)
            out.append((v, v[0].copy()))
    labels = g.integers(0, nc + 2, rows).astype(np.uint8)
    return out[0][0], out[1][0], labels, out[0][1], out[1][1]


def run(dev, x, y, labels, nc, px, py, splits=()):
    """The state after one ``add`` (or one per part, split at the rows ``splits``), on the host."""
    from mdil_ss_amd.similarity import MomentMeter
    meter = MomentMeter(x.shape[1], 0 if y is None else y.shape[1], nc, dev, pivot_x=px, pivot_y=py)
    tx = torch.from_numpy(x).to(dev)
    ty = None if y is None else torch.from_numpy(y).to(dev)
    tl = None if labels is None else torch.from_numpy(labels).to(dev)
    edges = (0,) + tuple(splits) + (len(x),)
    for a, b in zip(edges[:-1], edges[1:]):
        meter.add(tx[a:b], None if ty is None else ty[a:b], None if tl is None else tl[a:b])
    torch.cuda.synchronize()
    return meter.state.cpu().numpy(), meter


def label_modes(nc):
    return (True, False) if nc == 1 else (True,)


# ---------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("nc", CLASSES)
@pytest.mark.parametrize("cx,cy", CHANNELS)
def test_integer_data_gives_the_checkers_bits(dev, cx, cy, nc):
    for rows in ROWS:
        x, y, labels, px, py = case(rows, cx, cy, nc, "int")
        for with_labels in label_modes(nc):
            lab = labels if with_labels else None
            want = R.moments(x, y, lab, nc, px, py)
            got, meter = run(dev, x, y, lab, nc, px, py)
            assert got.dtype == np.float64 and got.shape == R.pack(want).shape
            m = meter.moments()
            assert m["skipped"] == want["skipped"] == (int((labels >= nc).sum()) if with_labels else 0), rows
            assert np.array_equal(m["n"], want["n"]), (rows, with_labels)
            for k in BLOCKS:
                assert np.array_equal(m[k], want[k]), (rows, with_labels, k, np.argwhere(m[k] != want[k])[:4])
            assert np.array_equal(got, R.pack(want)), (rows, with_labels)
    assert any(int((case(r, cx, cy, nc, "int")[2] >= nc).sum()) > 0 for r in ROWS)


# ------------------------------------------------------------------------------------ rounding
@pytest.mark.parametrize("nc", CLASSES)
@pytest.mark.parametrize("cx,cy", CHANNELS)
def test_gaussian_data_stays_within_one_chains_rounding(dev, cx, cy, nc):
    worst = 0.0
    for rows in ROWS:
        x, y, labels, px, py = case(rows, cx, cy, nc, "gauss")
        want, mag = R.moments(x, y, labels, nc, px, py), R.absolute_moments(x, y, labels, nc, px, py)
        _, meter = run(dev, x, y, labels, nc, px, py)
        m = meter.moments()
        assert np.array_equal(m["n"], want["n"]) and m["skipped"] == want["skipped"]
        for k in BLOCKS:
            err, tol = np.abs(m[k] - want[k]), bound() * mag[k]
            if err.size:
                worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
            assert (err <= tol).all(), (rows, k, float(err.max()))
    print(f"cx {cx} cy {cy} nc {nc}: largest error / bound {worst:.4f}")


# ----------------------------------------------------------- accumulation and determinism
def test_two_halves_accumulate_and_equal_calls_give_equal_bits(dev):
    cx, cy, nc, rows = 33, 128, 20, 4099
    x, y, labels, px, py = case(rows, cx, cy, nc, "gauss")
    want, mag = R.moments(x, y, labels, nc, px, py), R.absolute_moments(x, y, labels, nc, px, py)
    whole, meter = run(dev, x, y, labels, nc, px, py)
    again, _ = run(dev, x, y, labels, nc, px, py)
    assert np.array_equal(whole.view(np.int64), again.view(np.int64))
    halves, hm = run(dev, x, y, labels, nc, px, py, splits=(2048,))       # row 2048 of x: 16-byte aligned
    m = hm.moments()
    assert np.array_equal(m["n"], want["n"]) and m["skipped"] == want["skipped"] and hm.rows == rows
    for k in BLOCKS:
        assert (np.abs(m[k] - want[k]) <= bound() * mag[k]).all(), k
    for mm in (meter.moments(), m):
        for k in ("gxx", "gyy"):
            assert np.array_equal(mm[k].view(np.int64), mm[k].T.copy().view(np.int64)), k
    # reset clears the sums and keeps the pivots
    hm.reset()
    hm.add(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(labels).to(dev))
    torch.cuda.synchronize()
    assert np.array_equal(hm.state.cpu().numpy().view(np.int64), whole.view(np.int64))


def test_integer_halves_add_up_exactly_and_the_default_pivot_is_the_first_rows_mean(dev):
    from mdil_ss_amd.similarity import MomentMeter, PIVOT_ROWS
    x, y, labels, px, py = case(4099, 16, 16, 20, "int")
    want = R.pack(R.moments(x, y, labels, 20, px, py))
    got, _ = run(dev, x, y, labels, 20, px, py, splits=(1028, 3000))
    assert np.array_equal(got, want)
    meter = MomentMeter(16, 16, 20, dev)
    meter.add(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(labels).to(dev))
    m = meter.moments()
    assert np.array_equal(m["pivot_x"], x[:PIVOT_ROWS].astype(np.float64).mean(0).astype(np.float32))
    ref = R.moments(x, y, labels, 20, m["pivot_x"], m["pivot_y"])
    mag = R.absolute_moments(x, y, labels, 20, m["pivot_x"], m["pivot_y"])
    for k in BLOCKS:
        assert (np.abs(m[k] - ref[k]) <= bound() * mag[k]).all(), k


def test_device_refusals(dev):
    from mdil_ss_amd.similarity import MomentMeter
    meter = MomentMeter(16, 16, 20, dev)
    x = torch.zeros(8, 16, device=dev)
    lab = torch.zeros(8, dtype=torch.uint8, device=dev)
    msg = "must be a contiguous {} device tensor.*no CPU fallback in the similarity path"
    with pytest.raises(RuntimeError, match="y " + msg.format("float32")):
        meter.add(x, x.double(), lab)
    with pytest.raises(RuntimeError, match="labels " + msg.format("uint8")):
        meter.add(x, x, lab.long())
    with pytest.raises(RuntimeError, match="labels " + msg.format("uint8")):
        meter.add(x, x, lab.cpu())
    with pytest.raises(RuntimeError, match=r"y must be float32 \[rows,16\]"):
        meter.add(x, torch.zeros(8, 17, device=dev), lab)
    with pytest.raises(RuntimeError, match="x has 8 rows and y 4"):
        meter.add(x, x[:4], lab)
    with pytest.raises(RuntimeError, match="labels are needed with nc 20"):
        meter.add(x, x)
    with pytest.raises(RuntimeError, match="y must be given exactly when cy > 0"):
        meter.add(x, None, lab)
    with pytest.raises(RuntimeError, match=r"labels must be uint8 \[8\]"):
        meter.add(x, x, lab[:4])


# ---------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def models(dev):
    return HC.teacher_student(dev)


@pytest.fixture(scope="module")
def batch(dev):
    from oracle import fixtures as fx
    images, labels = fx.make_batch(2, 64, 128, 20, seed=100)
    return images.to(dev), labels[:, 0].to(torch.uint8).to(dev)


@pytest.mark.parametrize("layer", ("encoder", "penultimate", "logits"))
def test_compare_and_population_match_the_checker_on_the_models_features(dev, models, batch, layer):
    from mdil_ss_amd import latent as L
    from mdil_ss_amd import similarity as S
    teacher, student = models
    images, labels = batch
    nc = 19                                                 # class 19, the ignore class, is skipped
    fa, fb = L.latents(teacher, images, 0, layer), L.latents(student, images, 0, layer)
    lab = L.resize_labels(labels, fa.shape[1], fa.shape[2]).reshape(-1).cpu().numpy()
    xa, lk = R.kept(fa.reshape(-1, fa.shape[3]).cpu().numpy(), lab, nc)
    xb, _ = R.kept(fb.reshape(-1, fb.shape[3]).cpu().numpy(), lab, nc)
    m = S.compare(teacher, student, images, 0, layer, labels=labels, classes=nc).moments()
    assert m["n"].sum() == len(xa) and m["skipped"] == (lab >= nc).sum() > 0
    cka, want = S.linear_cka(m), R.linear_cka(xa, xb)
    sep = S.separability(m)
    print(f"{layer}: CKA {cka:.8f} (checker {want:.8f}), separability {sep['x']:.6f} -> {sep['y']:.6f}")
    assert abs(cka - want) <= 1e-5 * want
    assert abs(sep["x"] - R.separability(xa, lk)) <= 1e-5 * R.separability(xa, lk)
    assert abs(sep["y"] - R.separability(xb, lk)) <= 1e-5 * R.separability(xb, lk)
    classes, shift, rel = R.class_shift(xa, xb, lk)
    got = S.class_shift(m)
    scale = math.sqrt(np.trace(R.mean_cov(xa)[1]))
    assert got["classes"] == classes
    assert np.abs(np.array(got["shift"]) - shift).max() <= 1e-5 * scale
    assert np.abs(np.array(got["relative"]) - rel).max() <= 1e-5 * max(rel.max(), 1.0)
    pa = S.population(teacher, images, 0, layer, labels=labels, classes=nc).moments()
    pb = S.population(student, images, 0, layer, labels=labels, classes=nc).moments()
    traces = np.trace(R.mean_cov(xa)[1]) + np.trace(R.mean_cov(xb)[1])
    fd, want_fd = S.frechet(pa, pb), R.frechet(xa, xb)
    print(f"{layer}: Frechet {fd:.8g} (checker {want_fd:.8g}), traces {traces:.6g}")
    assert abs(fd - want_fd) <= 1e-5 * traces
    # a checkpoint against itself
    same = S.compare(student, student, images, 0, layer, labels=labels, classes=nc).moments()
    assert S.linear_cka(same) >= 1 - 1e-6
    assert max(S.class_shift(same)["shift"]) <= 1e-5 * math.sqrt(np.trace(R.mean_cov(xb)[1]))
    assert abs(S.frechet(pb, pb)) <= 1e-5 * 2 * np.trace(R.mean_cov(xb)[1])


# ----------------------------------------------------------------------------------------- CLI
def _finite(v):
    if isinstance(v, dict):
        return all(_finite(w) for w in v.values())
    if isinstance(v, list):
        return all(_finite(w) for w in v)
    return v is None or isinstance(v, (str, bool)) or math.isfinite(v)


def test_cli_end_to_end_in_both_modes(dev, models, tmp_path):
    from mdil_ss_amd import similarity as S
    teacher, student = models
    for model, name in ((teacher, "before.pth.tar"), (student, "after.pth.tar")):
        HC.save_checkpoint(model, tmp_path / name)
    size = ["--synthetic", "2", "--height", "64", "--width", "128"]
    ckpt = ["--before", str(tmp_path / "before.pth.tar"), "--before-num-classes", "20", "--after",
            str(tmp_path / "after.pth.tar"), "--after-num-classes", "20", "20", "--task", "0"] + size
    dom = ["--state", str(tmp_path / "after.pth.tar"), "--num-classes", "20", "20", "--task-a", "0", "--task-b", "1"] + size
    files = {}
    for mode, argv in (("checkpoints", ckpt), ("domains", dom)):
        for turn in ("first", "second"):
            path = tmp_path / f"{mode}_{turn}.json"
            report = S.main(S.build_parser().parse_args(argv + ["--json", str(path)]))
            files[mode, turn] = open(path, "rb").read()
            assert json.loads(files[mode, turn]) == json.loads(json.dumps(report))
        assert files[mode, "first"] == files[mode, "second"], mode
    saved = json.loads(files["checkpoints", "first"])
    assert (saved["mode"], saved["dataset"], saved["task"], saved["images"], saved["classes"]) == \
        ("checkpoints", "synthetic", 0, 2, 19)
    assert list(saved["layers"]) == ["encoder", "penultimate", "logits"] and _finite(saved)
    for layer, channels, rows in (("encoder", 128, 2 * 8 * 16), ("penultimate", 16, 2 * 32 * 64), ("logits", 20, 2 * 64 * 128)):
        e = saved["layers"][layer]
        assert sorted(e) == ["channels", "cka", "class_shift", "matrices", "rows", "rows_per_class", "separability_after",
                             "separability_before", "skipped"]
        assert e["channels"] == [channels, channels] and e["rows"] + e["skipped"] == rows
        assert 0 < e["cka"] <= 1 + 1e-9 and e["separability_before"] > 0 and e["separability_after"] > 0
        assert sorted(e["class_shift"]) == ["classes", "relative", "shift"] and len(e["class_shift"]["shift"]) > 0
        assert sorted(e["matrices"]) == ["cxx", "cxy", "cyy", "mean_x", "mean_y", "n"]
        assert np.array(e["matrices"]["cxy"]).shape == (channels, channels)
    saved = json.loads(files["domains", "first"])
    assert (saved["mode"], saved["task_a"], saved["task_b"], saved["images_a"], saved["images_b"]) == ("domains", 0, 1, 2, 2)
    assert list(saved["layers"]) == ["encoder", "penultimate", "logits"] and _finite(saved)
    for layer, channels in (("encoder", 128), ("penultimate", 16), ("logits", 20)):
        e = saved["layers"][layer]
        assert sorted(e) == ["centroid_distance", "channels", "frechet", "matrices", "rows_a", "rows_b", "trace_a", "trace_b"]
        assert e["frechet"] > 0 and e["trace_a"] > 0 and e["trace_b"] > 0 and e["channels"] == [channels, channels]
        assert sorted(e["centroid_distance"]) == ["classes", "relative", "shift"]
        assert np.array(e["matrices"]["cov_a"]).shape == (channels, channels)
