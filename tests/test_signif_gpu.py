"""GPU: the significance add-on against its numpy reference (tests/signif_reference.py).  Every
integer output -- the per-image counts, the replicate sums, the masks of empty classes -- must equal
the reference exactly (``torch.equal``).  The fp64 scores are held to |kernel - reference| <= 1e-12:
an IoU lies in [0, 1] and an mIoU is at most 32 correctly rounded divides and adds of 2.2e-16 each,
so the bound leaves two orders of magnitude; the tests print whether the scores were bit-equal, and
the integer sums they are computed from are compared exactly beside them."""
import itertools
import json

import numpy as np
import pytest
import torch

from tests import head_cases as hc
from tests import signif_reference as R

pytestmark = pytest.mark.gpu

BOUND = 1e-12
SEEDS = (0, (1 << 63) + 5)


@pytest.fixture(scope="module")
def dev():
    return hc.device("significance")


@pytest.fixture(scope="module")
def S(dev):
    from mdil_ss_amd import significance
    return significance


# --------------------------------------------------------------------------------------- count
def make_pred(nc, target, seed):
    """u8 predictions: the target where it is a class on about half the pixels, any class elsewhere,
    and a few 255 and nc (outside the classes)."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(0, nc, target.shape, generator=g, dtype=torch.uint8)
    r = torch.rand(target.shape, generator=g)
    keep = (r < 0.5) & (target < nc)
    p[keep] = target[keep]
    p[(r >= 0.90) & (r < 0.93)] = 255
    p[(r >= 0.93) & (r < 0.95)] = nc
    return p


def table_of(preds, target, nc, ignore):
    """-> (int64 [N,G,3,nc], bad targets, unpredicted) of the reference for the predictors ``preds``."""
    each = [R.counts(p.numpy(), target.numpy(), nc, ignore) for p in preds]
    return np.stack([e[0] for e in each], axis=1), sum(e[1] for e in each), sum(e[2] for e in each)


COUNT_SHAPES = ((1, 1, 1), (1, 1, 333), (2, 37, 131), (3, 96, 200), (2, 6, 10))     # the last: whole dwords only


@pytest.mark.parametrize("shape", COUNT_SHAPES, ids=str)
@pytest.mark.parametrize("nc", hc.CLASSES)
def test_count_matches_the_reference(dev, S, nc, shape):
    N = shape[0]
    for ignore in (-1, nc - 1, 255):
        target = hc.make_target(nc, shape, ignore if ignore >= 0 else 255, seed=nc + shape[2])
        preds = [make_pred(nc, target, seed=7 * nc + g) for g in range(2)]
        want, bad, unpredicted = table_of(preds, target, nc, ignore)
        assert shape[1] * shape[2] < 400 or (bad > 0 and unpredicted > 0)
        # into the rows 3 .. 3 + N - 1 of a larger table that holds something already
        M, first = N + 5, 3
        start = torch.arange(M * 2 * 3 * nc, dtype=torch.int64).reshape(M, 2, 3, nc)
        counts = start.to(dev)
        stray = None
        for g in range(2):
            stray = S.image_counts(preds[g].to(dev), target.to(dev), nc, ignore_index=ignore, counts=counts,
                                   first_image=first, group=g, stray=stray)
        expect = start.clone()
        expect[first:first + N] += torch.from_numpy(want)
        assert torch.equal(counts.cpu(), expect), (nc, shape, ignore)
        assert stray.cpu().tolist() == [bad, unpredicted]
        # a second call adds up; one group only
        S.image_counts(preds[1].to(dev), target.to(dev), nc, ignore_index=ignore, counts=counts, first_image=first,
                       group=1, stray=stray)
        expect[first:first + N, 1] += torch.from_numpy(want[:, 1])
        assert torch.equal(counts.cpu(), expect)
        one = R.counts(preds[1].numpy(), target.numpy(), nc, ignore)
        assert stray.cpu().tolist() == [bad + one[1], unpredicted + one[2]]


def test_count_one_label_everywhere_and_maps_of_strays(dev, S):
    nc, shape = 20, (2, 96, 200)
    full = torch.full(shape, 3, dtype=torch.uint8)
    cases = {"one label": (full, full), "all wrong": (torch.full(shape, 4, dtype=torch.uint8), full),
             "all unpredicted": (torch.full(shape, 255, dtype=torch.uint8), full),
             "all bad targets": (full, torch.full(shape, 200, dtype=torch.uint8)),
             "all ignored": (full, torch.full(shape, 19, dtype=torch.uint8))}
    for name, (p, t) in cases.items():
        want, bad, unpredicted = R.counts(p.numpy(), t.numpy(), nc, 19)
        counts = S.new_counts(2, 1, nc, dev)
        stray = S.image_counts(p.to(dev), t.to(dev), nc, ignore_index=19, counts=counts, first_image=0)
        assert torch.equal(counts.cpu()[:, 0], torch.from_numpy(want)), name
        assert stray.cpu().tolist() == [bad, unpredicted], name
    assert want.sum() == 0 and R.counts(full.numpy(), full.numpy(), nc, 19)[0][0, :, 3].tolist() == [96 * 200] * 3


def test_count_takes_maps_that_are_only_4_byte_aligned(dev, S):
    nc, shape = 20, (2, 16, 32)
    target = hc.make_target(nc, shape, 19, seed=3)
    pred = make_pred(nc, target, seed=4)
    arena = torch.zeros(2 * 1024 + 64, dtype=torch.uint8, device=dev)
    p, t = arena[4:4 + 1024].view(shape), arena[1040:1040 + 1024].view(shape)
    assert p.data_ptr() % 16 == 4
    p.copy_(pred.to(dev))
    t.copy_(target.to(dev))
    counts = S.new_counts(2, 1, nc, dev)
    S.image_counts(p, t, nc, ignore_index=19, counts=counts, first_image=0)
    assert torch.equal(counts.cpu()[:, 0], torch.from_numpy(R.counts(pred.numpy(), target.numpy(), nc, 19)[0]))


@pytest.mark.parametrize("nc", hc.CLASSES)
def test_count_sums_to_the_confusion_matrix_of_the_fused_head(dev, S, nc):
    from mdil_ss_amd import fullres as FR
    x, w, b = hc.head_inputs(nc, (3, 16, 48))
    target = hc.make_target(nc, (3, 40, 100), nc - 1, seed=nc)
    target[target >= nc] = 0                              # the meter refuses targets outside the classes
    meter = FR.ConfusionMeter(nc, nc - 1)
    label, _ = meter.add(hc.nhwc(x).to(dev), w.to(dev), b.to(dev), target=target.to(dev))
    counts = S.new_counts(3, 1, nc, dev)
    stray = S.image_counts(label, target.to(dev), nc, ignore_index=nc - 1, counts=counts, first_image=0)
    matrix, total = meter.matrix(), counts.sum(0).cpu()[0]
    assert torch.equal(total[0], matrix.diagonal()) and torch.equal(total[1], matrix.sum(0))
    assert torch.equal(total[2], matrix.sum(1)) and stray.cpu().tolist() == [0, 0]
    miou = S.score_counts(total.numpy(), nc, nc - 1)[0]
    assert abs(float(meter.iou(matrix)[0]) - float(miou)) < 1e-14


def test_count_on_a_side_stream(dev, S):
    nc, shape = 27, (3, 96, 200)
    target = hc.make_target(nc, shape, 26, seed=1)
    pred = make_pred(nc, target, seed=2)
    p, t = pred.to(dev), target.to(dev)
    counts = S.new_counts(3, 1, nc, dev)
    torch.cuda.synchronize()
    hc.side_stream(lambda: S.image_counts(p, t, nc, ignore_index=26, counts=counts, first_image=0))
    assert torch.equal(counts.cpu()[:, 0], torch.from_numpy(R.counts(pred.numpy(), target.numpy(), nc, 26)[0]))


# ------------------------------------------------------------------------------------ resample
def random_table(M, G, nc, seed, top=1 << 20):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, top, size=(M, G, 3, nc))
    t[:, :, 0] = np.minimum(t[:, :, 0], np.minimum(t[:, :, 1], t[:, :, 2]))       # tp within both margins
    return t.astype(np.int64)


def reference(table, nc, ignore, mode, B, seed, first=0, step=128):
    """``R.replicates`` in slices of ``step`` replicates (the gather of all of them at once is large)."""
    parts = [R.replicates(table, nc, ignore, mode, min(step, B - s), seed, first + s) for s in range(0, B, step)]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def check_replicates(S, dev, table, nc, ignore, mode, B, seed, first=0, what=""):
    want = reference(table, nc, ignore, mode, B, seed, first)
    counts = torch.from_numpy(table).to(dev)
    got = S.resample(counts, nc, ignore, mode, B, seed, first, sums=True)
    host = {k: v.cpu() for k, v in got.items()}
    assert torch.equal(host["sums"], torch.from_numpy(want["sums"])), what
    assert torch.equal(host["empty"], torch.from_numpy(want["empty"])), what
    errs = {k: float((host[k] - torch.from_numpy(want[k])).abs().max()) for k in ("miou", "iou")}
    same = all(torch.equal(host[k], torch.from_numpy(want[k])) for k in ("miou", "iou"))
    print(f"{what}: max |kernel - reference| mIoU {errs['miou']:.1e}, IoU {errs['iou']:.1e}; bit-equal: {same}")
    assert errs["miou"] <= BOUND and errs["iou"] <= BOUND, what
    assert float(host["iou"].min()) >= 0.0 and float(host["iou"].max()) <= 1.0
    # without the sums (and without the other optional outputs) the scores are the same bytes
    bare = S.resample(counts, nc, ignore, mode, B, seed, first, iou=False, empty=False)
    assert set(bare) == {"miou"} and torch.equal(bare["miou"].cpu(), host["miou"]), what
    return counts, host


IMAGES, REPLICATES = (1, 2, 37, 64, 65, 300), (1, 63, 65, 1000)
MODES = (R.BOOTSTRAP, R.JACKKNIFE, R.SWAP)
# every (M, B) with every mode; the class count, the groups and the seed go round so that every
# (nc, G, mode) meets: the swap needs two groups
RESAMPLE_CASES = []
for n, ((M, B), mode) in enumerate(itertools.product(itertools.product(IMAGES, REPLICATES), MODES)):
    pair = n // 3
    RESAMPLE_CASES.append((M, B, mode, hc.CLASSES[pair % 4], 2 if mode == R.SWAP else 1 + (pair // 4) % 2,
                           SEEDS[(pair // 2) % 2]))


def test_the_cases_meet_every_combination():
    assert {(nc, G, mode) for _, _, mode, nc, G, _ in RESAMPLE_CASES} == \
        {(nc, G, mode) for nc in hc.CLASSES for G in (1, 2) for mode in MODES if G == 2 or mode != R.SWAP}
    assert {(M, B, mode) for M, B, mode, *_ in RESAMPLE_CASES} == set(itertools.product(IMAGES, REPLICATES, MODES))
    assert {seed for *_, seed in RESAMPLE_CASES} == set(SEEDS)


@pytest.mark.parametrize("M, B, mode, nc, G, seed", RESAMPLE_CASES,
                         ids=[f"M{M}-B{B}-{mode}-nc{nc}-G{G}-s{seed & 7}"
                              for M, B, mode, nc, G, seed in RESAMPLE_CASES])
def test_resample_matches_the_reference(dev, S, M, B, mode, nc, G, seed):
    if mode == R.JACKKNIFE:
        B = min(B, M)                                      # the jackknife has M replicates
    ignore = (nc - 1, 255, -1)[(M + B) % 3]
    table = random_table(M, G, nc, seed=M * 1000 + B)
    what = f"{mode} M={M} B={B} nc={nc} G={G} ignore={ignore}"
    counts, host = check_replicates(S, dev, table, nc, ignore, mode, B, seed, what=what)
    if B >= 2:
        # the same replicates from two calls split at an odd replicate
        cut = B // 2 if (B // 2) % 2 else B // 2 + 1
        if cut < B:
            a = S.resample(counts, nc, ignore, mode, cut, seed, 0, sums=True)
            b = S.resample(counts, nc, ignore, mode, B - cut, seed, cut, sums=True)
            for k in ("sums", "miou", "iou", "empty"):
                assert torch.equal(torch.cat([a[k], b[k]]).cpu(), host[k]), (what, k)


# The bootstrap reads one group's slice from LDS where M * 3 nc <= 32768 entries and the table from the
# L2 above that; in LDS a lane adds a second column where 3 nc > 64 (nc >= 22); from the L2 it adds
# one, two or three columns (G * 3 nc up to 64, 128, 192).
@pytest.mark.parametrize("nc, G, M", ((32, 2, 341), (32, 2, 342), (27, 1, 404), (27, 1, 405), (20, 2, 546), (20, 2, 547),
                                      (20, 1, 547), (21, 1, 65), (22, 2, 65)))
def test_bootstrap_on_both_sides_of_its_thresholds(dev, S, nc, G, M):
    table = random_table(M, G, nc, seed=M + nc)
    table[M - 1] = (1 << 31) - 1                          # the last row of the slice, the largest entries
    what = f"bootstrap M={M} nc={nc} G={G}: {M * 3 * nc} entries per group"
    counts, host = check_replicates(S, dev, table, nc, nc - 1, R.BOOTSTRAP, 67, SEEDS[1], what=what)
    a = S.resample(counts, nc, nc - 1, "bootstrap", 33, SEEDS[1], 0, sums=True)
    b = S.resample(counts, nc, nc - 1, "bootstrap", 34, SEEDS[1], 33, sums=True)
    for k in ("sums", "miou", "iou", "empty"):
        assert torch.equal(torch.cat([a[k], b[k]]).cpu(), host[k]), (what, k)


@pytest.mark.parametrize("mode, G, B", ((R.BOOTSTRAP, 2, 2100), (R.BOOTSTRAP, 1, 4200), (R.SWAP, 2, 66000),
                                        (R.JACKKNIFE, 2, 2100)))
def test_resample_strides_past_the_grid_bound(dev, S, mode, G, B):
    """More replicates than one pass of the capped grids takes: 256 / G work-groups of 16 wavefronts
    from LDS, 16384 work-groups of 4 from the L2, 512 of 4 for the jackknife."""
    M, nc = {R.BOOTSTRAP: (37, 20), R.SWAP: (3, 2), R.JACKKNIFE: (B, 2)}[mode]
    table = random_table(M, G, nc, seed=B)
    check_replicates(S, dev, table, nc, -1, mode, B, 1, what=f"{mode} B={B} G={G}")


@pytest.mark.parametrize("mode", MODES)
def test_resample_with_the_largest_entries(dev, S, mode):
    """Every entry 2^31 - 1: 300 of them overflow an i32 accumulator many times over."""
    M, nc, G = 300, 32, 2
    table = np.full((M, G, 3, nc), (1 << 31) - 1, dtype=np.int64)
    table[::7, 1, :, 5] = 0
    _, host = check_replicates(S, dev, table, nc, -1, mode, 70, SEEDS[1], what=f"{mode}, entries 2^31 - 1")
    assert int(host["sums"].max()) >= 299 * ((1 << 31) - 1)
    with pytest.raises(RuntimeError, match=r"entries of counts must be in \[0, 2\^31\)"):
        S.resample(torch.from_numpy(table + 1).to(dev), nc, -1, mode, 4, 0)
    with pytest.raises(RuntimeError, match=r"entries of counts must be in \[0, 2\^31\)"):
        S.resample(torch.from_numpy(table - (1 << 31)).to(dev), nc, -1, mode, 4, 0)


@pytest.mark.parametrize("mode", (R.BOOTSTRAP, R.SWAP))
def test_resample_at_the_last_replicates(dev, S, mode):
    M, nc, B = 65, 20, 70
    table = random_table(M, 2, nc, seed=11)
    first = (1 << 32) - B
    check_replicates(S, dev, table, nc, 19, mode, B, SEEDS[1], first=first, what=f"{mode}, replicates up to 2^32 - 1")
    with pytest.raises(RuntimeError, match=r"outside \[0, 2\^32\)"):
        S.resample(torch.from_numpy(table).to(dev), nc, 19, mode, B, 0, first + 1)


def test_jackknife_rows_are_the_total_minus_the_image(dev, S):
    M, nc = 300, 27
    table = random_table(M, 2, nc, seed=12)
    counts = torch.from_numpy(table).to(dev)
    got = S.resample(counts, nc, 26, "jackknife", M, 0, sums=True)
    assert torch.equal(got["sums"], counts.sum(0, keepdim=True) - counts)
    part = S.resample(counts, nc, 26, "jackknife", 37, 0, 263, sums=True)
    assert torch.equal(part["sums"], got["sums"][263:]) and torch.equal(part["miou"], got["miou"][263:])
    with pytest.raises(RuntimeError, match="the jackknife of 300 images has 300 replicates"):
        S.resample(counts, nc, 26, "jackknife", 38, 0, 263)
    with pytest.raises(RuntimeError, match="needs a table of two groups"):
        S.resample(counts[:, :1].contiguous(), nc, 26, "swap", 4, 0)


def test_empty_masks_where_classes_live_in_one_image(dev, S):
    M, nc = 6, 20
    table = random_table(M, 2, nc, seed=13) + 1
    table[1:, :, :, 4] = 0                                # class 4 lives in image 0 only
    table[:5, 0, :, 17] = 0                               # class 17 of predictor A in image 5 only
    table[:, 1, :, 9] = 0                                 # class 9 of predictor B nowhere
    for mode in MODES:
        _, host = check_replicates(S, dev, table, nc, 19, mode, 6 if mode == R.JACKKNIFE else 200, 0,
                                   what=f"{mode} masks")
        e = host["empty"]
        assert not ((e >> 3) & 1).any()
        assert mode == R.SWAP or ((e[:, 1] >> 9) & 1).all()       # exchanged, B takes A's class 9
        gone = ((e[:, 0] >> 4) & 1).sum().item()
        assert gone == 1 if mode == R.JACKKNIFE else 0 <= gone < e.shape[0] if mode == R.SWAP else 30 < gone < 110
    _, host = check_replicates(S, dev, table, nc, 19, R.BOOTSTRAP, 200, 0, what="bootstrap masks")
    without = ((host["empty"][:, 0] >> 4) & 1).bool()
    assert (host["iou"][without][:, 0, 4] == 0).all() and (host["iou"][~without][:, 0, 4] > 0).all()


def test_resample_on_a_side_stream(dev, S):
    table = random_table(300, 2, 20, seed=14)
    counts = torch.from_numpy(table).to(dev)
    torch.cuda.synchronize()
    got = hc.side_stream(lambda: S.resample(counts, 20, 19, "bootstrap", 500, 3, sums=True, check_entries=False))
    assert torch.equal(got["sums"].cpu(), torch.from_numpy(reference(table, 20, 19, R.BOOTSTRAP, 500, 3)["sums"]))


# ---------------------------------------------------------------------------- through the module
def assert_reports_agree(got, want, path="report"):
    if isinstance(want, dict):
        assert isinstance(got, dict) and sorted(got) == sorted(want), path
        for k in want:
            assert_reports_agree(got[k], want[k], f"{path}.{k}")
    elif isinstance(want, (list, tuple)):
        assert isinstance(got, (list, tuple)) and len(got) == len(want), path
        for i, (g, w) in enumerate(zip(got, want)):
            assert_reports_agree(g, w, f"{path}[{i}]")
    elif isinstance(want, float):
        assert isinstance(got, float) and abs(got - want) <= BOUND, (path, got, want)
    else:
        assert got == want and type(got) is type(want), (path, got, want)


def images_and_target(dev, nc, n=5, size=(40, 72)):
    g = torch.Generator().manual_seed(21)
    images = torch.rand(n, 3, 32, 64, generator=g)
    target = torch.randint(0, nc, (n,) + size, generator=g, dtype=torch.uint8)
    return images.to(dev), target


def test_meter_on_a_model(dev, S):
    model = hc.tiny_model(dev)
    images, target = images_and_target(dev, 20)
    meter = S.SignificanceMeter(20, 19)
    stems = [f"img{i}" for i in range(5)]
    a, = meter.add(model, images[:2], 1, target=target[:2].to(dev), stems=stems[:2])
    b, = meter.add(model, images[2:], 1, target=target[2:].to(dev), stems=stems[2:])
    assert a.dtype == torch.uint8 and tuple(b.shape) == (3, 40, 72) and meter.images == 5
    got = meter.report(replicates=300, seed=5, level=0.9, influence=3)
    want = R.report([torch.cat([a, b]).cpu().numpy()], target.numpy(), 20, 19, stems, 300, 5, 0.9, 3)
    assert_reports_agree(got, want)
    assert got["images"] == 5 and len(got["predictors"]) == 1 and len(got["predictors"][0]["iou_classes"]) == 19
    assert [e["stem"] for e in got["predictors"][0]["influence"]] == [stems[e["image"]] for e in
                                                                       got["predictors"][0]["influence"]]
    # label maps instead of a model: the same report
    again = S.SignificanceMeter(20, 19)
    again.add(torch.cat([a, b]), target.to(dev), stems=stems)
    assert_reports_agree(again.report(replicates=300, seed=5, level=0.9, influence=3), want)
    bad = S.SignificanceMeter(20, 19)
    bad.add(torch.cat([a, b]), torch.full_like(target, 77).to(dev))
    with pytest.raises(RuntimeError, match="target pixels are outside"):
        bad.report(replicates=10)


def test_paired_meter_on_a_teacher_and_a_student(dev, S):
    teacher, student = hc.teacher_student(dev)
    images, target = images_and_target(dev, 20)
    meter = S.SignificanceMeter(20, 19, paired=True)
    a, b = meter.add((teacher, images, 0), (student, images, 0), target=target.to(dev))
    assert not torch.equal(a, b)
    got = meter.report(replicates=300, seed=2)
    stems = [f"image_{i:06d}" for i in range(5)]
    want = R.report([a.cpu().numpy(), b.cpu().numpy()], target.numpy(), 20, 19, stems, 300, 2)
    assert_reports_agree(got, want)
    d = got["delta"]
    assert abs(d["value"] - (got["predictors"][1]["mIoU"]["value"] - got["predictors"][0]["mIoU"]["value"])) < 1e-15
    assert 0 < d["p_boot"] <= 1 and 0 < d["p_swap"] <= 1 and len(d["classes"]) == 19
    # a predictor against itself, features and head parameters instead of a model
    feat = student.features(images, 0).contiguous()
    w, bias = (t.detach() for t in student.head_params(0))
    same = S.SignificanceMeter(20, 19, paired=True)
    x, y = same.add((feat, w, bias), b, target=target.to(dev))
    assert torch.equal(x, y)
    d = same.report(replicates=100)["delta"]
    assert d["value"] == 0.0 and d["se"] == 0.0 and d["p_boot"] == 1.0 and d["p_swap"] == 1.0


def test_command_line_on_synthetic_images(dev, S, tmp_path):
    from mdil_ss_amd import fullres as FR
    teacher, student = hc.teacher_student(dev)
    hc.save_checkpoint(teacher, tmp_path / "before.pth.tar")
    hc.save_checkpoint(student, tmp_path / "after.pth.tar")
    data = ["--task", "0", "--synthetic", "5", "--native-height", "48", "--native-width", "96", "--height", "32",
            "--width", "64", "--batch-size", "2"]
    settings = ["--replicates", "200", "--seed", "3", "--influence", "2"]
    before = ["--state", str(tmp_path / "before.pth.tar"), "--num-classes", "20"]
    after = ["--state", str(tmp_path / "after.pth.tar"), "--num-classes", "20", "20"]

    def run(argv, name):
        rep = S.main(S.build_parser().parse_args(argv + data + settings + ["--json", str(tmp_path / name)]))
        with open(tmp_path / name) as f:
            assert_reports_agree(json.load(f), rep)          # what was written is what was returned
        return rep
    one, two = run(before, "a.json"), run(after, "b.json")
    for rep in (one, two):
        assert (rep["dataset"], rep["task"], rep["images"], rep["replicates"], rep["seed"], rep["paired"]) == \
            ("synthetic", 0, 5, 200, 3, False)
        m = rep["predictors"][0]["mIoU"]
        assert 0 <= m["percentile"][0] <= m["percentile"][1] <= 1 and len(rep["predictors"][0]["influence"]) == 2
        assert rep["predictors"][0]["influence"][0]["stem"].startswith("synthetic_")
    pair = run(["--before", before[1], "--before-num-classes", "20", "--after", after[1], "--after-num-classes", "20",
                "20"], "pair.json")
    assert pair["paired"] and [p["mIoU"]["value"] for p in pair["predictors"]] == \
        [one["predictors"][0]["mIoU"]["value"], two["predictors"][0]["mIoU"]["value"]]
    assert pair["delta"]["value"] == two["predictors"][0]["mIoU"]["value"] - one["predictors"][0]["mIoU"]["value"]
    assert pair["predictors"][0]["mIoU"] == one["predictors"][0]["mIoU"]        # the same draws for the same seed
    # the label maps fullres writes for the two checkpoints, read back: the same pair
    for name, state in (("maps_a", before), ("maps_b", after)):
        FR.main(FR.build_parser().parse_args(state + data + ["--out", str(tmp_path / name)]))
    maps = run(["--pred", str(tmp_path / "maps_a"), "--pred-b", str(tmp_path / "maps_b"), "--num-classes", "20"],
               "maps.json")
    assert_reports_agree(maps, pair)
    single = run(["--pred", str(tmp_path / "maps_b"), "--num-classes", "20", "20"], "single.json")
    assert_reports_agree(single, two)
