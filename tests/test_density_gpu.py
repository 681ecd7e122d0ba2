"""GPU: the density kernels (mdil_ss_amd/ext/density_head.hip) and the entry points over them
(mdil_ss_amd/density.py), against tests/density_reference.py and the shared cases of tests/head_cases.py.

What is compared with what.  ``density_head`` walks ``predict_head``'s chain, so its label is asserted bit
for bit.  Both scores are held to their fp64 definition (evaluated from the fp32 model buffer and
fl32(x - pivot)): a code must lie between the keys of u64 - tol and u64 + tol, tol per row the larger of
the first-order rounding bound of the definition (density_reference.scores64) and 4 x the worst distance
of a plain float32 torch evaluation from fp64 on the same case.  The test prints how far the kernel's
codes lie from the fp64 score as a multiple of that float32 distance.  ``nearest`` must be the fp64
argmin wherever the two smallest fp64 distances differ by more than 2 tol_maha; that mask may hold at
most 1e-3 of a case's rows, which is asserted first, on the reference alone.  Everything after the codes
is integer arithmetic and is asserted exactly, on the kernel's own maps."""
import functools
import glob
import json

import numpy as np
import pytest
import torch

from tests import density_reference as R
from tests import head_cases as HC
from tests import openset_reference as OR
from tests.head_cases import CLASSES, SHAPES, nhwc

pytestmark = pytest.mark.gpu

MAX_EXCLUDED = 1e-3
BIG = (3, 16, 48)
BIG_ROWS = BIG[0] * BIG[1] * BIG[2]
HEAD_WG, HEAD_BLOCKS = 256, 768                 # density_head.hip: kHeadWG, kHeadMaxBlocks
ROWS_TRIP, ROWS_BLOCKS = 64, 512                # kRowsPerTrip, kRowsMaxBlocks
SOURCES = ("clustered", "relu")
ROW_C, ROW_N, ROW_K = (16, 48, 128), (1, 63, 64, 65, 4671), (1, 2, 20, 32)
SENTINEL = torch.tensor([0xA5] * 8, dtype=torch.uint8).view(torch.int64)


@pytest.fixture(scope="module")
def dev():
    return HC.device("density")


def new_hist(dev):
    return torch.zeros(2, 2, 65536, dtype=torch.int64, device=dev)


def zeros(dev, n):
    return torch.zeros(n, dtype=torch.int64, device=dev)


# ------------------------------------------------------------------------------------ the cases
def relu_labels(x, classes):
    """Structured labels for post-ReLU features [rows, 16], so that the class means differ: the strongest
    channel, and for more than 16 classes also whether the row's sum is above the median."""
    strongest = x.argmax(1)
    high = (x.sum(1) > x.sum(1).median()).long()
    return ((strongest + 16 * high) % classes).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def head_model(nc, source):
    """A model of nc - 1 class means for 16 channels and the BIG case's rows it was fitted to."""
    classes = nc - 1
    if source == "clustered":
        x, lab, _ = R.clustered(16, classes, BIG_ROWS, seed=100 + nc)
    else:
        x = nhwc(HC.head_inputs(nc, BIG)[0]).reshape(-1, 16)
        lab = relu_labels(x, classes)
    pivot = x[:64].double().mean(0).float().numpy()
    return R.fit(x, lab, classes, min_rows=2, pivot=pivot), x


def head_features(nc, shape, source):
    """NHWC features [N,H,W,16] of a case: the first rows of the model's own population."""
    N, H, W = shape
    if source == "relu":
        return nhwc(HC.head_inputs(nc, shape)[0])
    return head_model(nc, source)[1][:N * H * W].reshape(N, H, W, 16).contiguous()


@functools.lru_cache(maxsize=None)
def head_reference(nc, shape, source):
    """fp64 scores of the feature pixels and the float32 torch evaluation's worst distance per kind.  Computed
    once, never modified."""
    model = head_model(nc, source)[0]
    x = head_features(nc, shape, source).reshape(-1, 16)
    ref = R.scores64(x, model)
    m32, r32 = R.scores32(x, model)
    ref["d32"] = [float((m32.double() - ref["maha"]).abs().max()), float((r32.double() - ref["rmaha"]).abs().max())]
    return ref


def expand(t, shape):
    """One value per feature pixel -> its four output pixels."""
    N, H, W = shape
    return t.reshape(N, H, W).repeat_interleave(2, 1).repeat_interleave(2, 2)


@functools.lru_cache(maxsize=None)
def head_run(nc, shape, source):
    """density_head once per map kind (the first call also fills every output as group 0) and predict_head."""
    from mdil_ss_amd import density as D
    from mdil_ss_amd import openset as OS
    from mdil_ss_amd.predict import predict_head
    dev = torch.device("cuda", 0)
    _, w, b = HC.head_inputs(nc, shape)
    xd, wd, bd = head_features(nc, shape, source).to(dev), w.to(dev), b.to(dev)
    dm = D.DeviceModel(head_model(nc, source)[0], dev)
    hist, nonf, agree = new_hist(dev), zeros(dev, 1), zeros(dev, 2)
    label, nearest, c0 = D.density_head(xd, wd, bd, dm, map_kind=0, hist=hist, nonfinite=nonf, agree=agree, want_nearest=True)
    c1 = D.density_head(xd, wd, bd, dm, map_kind="rmaha", want_label=False)[2]
    plabel = predict_head(xd, wd, bd, None, False)[0]
    torch.cuda.synchronize()
    return dict(label=label.cpu(), nearest=nearest.cpu(), codes=torch.stack([OS.code_values(c.cpu()) for c in (c0, c1)]),
                hist=hist.cpu(), nonfinite=int(nonf.item()), agree=agree.tolist(), plabel=plabel.cpu(), dcodes=(c0, c1),
                dlabel=label, args=(xd, wd, bd, dm))


def check_codes(what, codes, ref, keep=None):
    """(b): codes [2, rows] of the feature rows against the fp64 scores."""
    from mdil_ss_amd import openset as OS
    for k, name in enumerate(R.KINDS):
        u64, d32 = ref[name], ref["d32"][k]
        tol = torch.clamp(ref["tol_" + name], min=4.0 * d32)
        lo, hi = OR.key16((u64 - tol).float().numpy()), OR.key16((u64 + tol).float().numpy())
        code = codes[k].reshape(-1)
        floor, nxt = OS.code_floor(code).double(), OS.code_floor(code + 1).double()
        away = torch.maximum(floor - u64, u64 - nxt).clamp(min=0).max().item()
        print(f"{what} {name}: bound {float(ref['tol_' + name].max()):.3e}, float32 torch {d32:.3e}; the kernel's codes are "
              f"at least {away:.3e} away = {away / max(d32, 1e-300):.2f} x float32 torch")
        ok = (code >= lo) & (code <= hi)
        assert bool((ok if keep is None else ok[keep]).all()), (what, name)


def check_nearest(what, nearest, ref):
    """(c): the fp64 argmin outside the near ties; the share of near ties is a condition on the reference alone."""
    tie = ref["gap"] <= 2 * ref["tol_maha"]
    HC.share(MAX_EXCLUDED)(tie, what)
    assert bool((nearest.reshape(-1).long() == ref["nearest"])[~tie].all()), what


# ---------------------------------------------------------------------- (a) - (c) the head form
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nc", CLASSES)
def test_head_label_codes_and_nearest(dev, nc, shape, source):
    from mdil_ss_amd import openset as OS
    run, ref = head_run(nc, shape, source), head_reference(nc, shape, source)
    what = f"nc {nc} shape {shape} {source}"
    N, H, W = shape
    npix = 4 * N * H * W
    assert run["label"].dtype == torch.uint8 and tuple(run["label"].shape) == (N, 2 * H, 2 * W)
    assert torch.equal(run["label"], run["plabel"])                                        # (a)
    small = run["codes"][:, :, ::2, ::2]
    check_codes(what, small.reshape(2, -1), ref)                                           # (b)
    check_nearest(what, run["nearest"][:, ::2, ::2], ref)                                  # (c)
    # (d) the 2 x 2 replication and the counters, on the kernel's own maps
    for k in range(2):
        assert torch.equal(run["codes"][k], expand(small[k], shape))
        assert torch.equal(run["hist"][k], OR.hist_of(run["codes"][k], torch.zeros_like(run["codes"][k])))
        assert int(run["hist"][k].sum()) == npix
    assert torch.equal(run["nearest"], expand(run["nearest"][:, ::2, ::2], shape))
    assert run["nonfinite"] == 0
    assert int(run["codes"].min()) >= OS.FINITE_CODES[0] and int(run["codes"].max()) <= OS.FINITE_CODES[1]
    assert run["agree"] == [npix, int((run["nearest"] == run["label"]).sum())]
    assert set(run["nearest"].unique().tolist()) <= set(head_model(nc, source)[0]["cls"].tolist())


# ------------------------------------------------------------------------------ (d) integers
def lut_case(nc):
    from mdil_ss_amd import openset as OS
    unknown = [c for c in range(nc) if c % 3 == 1] + [nc]
    ignore = [c for c in range(nc) if c % 5 == 2 and c % 3 != 1]
    return OS.group_lut(unknown, ignore)


@pytest.mark.parametrize("shape", ((1, 9, 7), BIG))
@pytest.mark.parametrize("nc", (2, 27))
def test_head_histograms_split_by_group_and_agree_counts(dev, nc, shape):
    from mdil_ss_amd import density as D
    run = head_run(nc, shape, "clustered")
    codes, lut = run["codes"], lut_case(nc)
    target = HC.make_target(nc, tuple(run["label"].shape), nc - 1, seed=nc + shape[1])
    groups = lut[target.long()].long()
    assert all(int((groups == g).sum()) > 0 for g in (0, 1)) and (nc == 2 or int((groups == 2).sum()) > 0)
    hist, agree = new_hist(dev), zeros(dev, 2)
    D.density_head(*run["args"], target=target.to(dev), lut=lut.to(dev), hist=hist, agree=agree, want_label=False)
    for k in range(2):
        assert torch.equal(hist[k].cpu(), OR.hist_of(codes[k], groups)), R.KINDS[k]
        assert int(hist[k].sum()) == int((groups < 2).sum())
    known = groups == 0
    assert agree.tolist() == [int(known.sum()), int((run["nearest"] == run["label"])[known].sum())]
    for g in (0, 1, 2):
        hist, agree = new_hist(dev), zeros(dev, 2)
        D.density_head(*run["args"], const_group=g, hist=hist, agree=agree, want_label=False)
        for k in range(2):
            assert torch.equal(hist[k].cpu(), OR.hist_of(codes[k], torch.full_like(codes[k], g)))
        assert int(hist.sum()) == (0 if g == 2 else 2 * codes[0].numel())
        assert int(agree[0]) == (codes[0].numel() if g == 0 else 0)
    for kind in (0, 1):                                             # one kind: the other row keeps what it held
        hist = torch.full((2, 2, 65536), 7, dtype=torch.int64, device=dev)
        D.density_head(*run["args"], target=target.to(dev), lut=lut.to(dev), kinds=[R.KINDS[kind]], hist=hist,
                       want_label=False)
        got = hist.cpu() - 7
        assert torch.equal(got[kind], OR.hist_of(codes[kind], groups)) and int(got.sum()) == int(got[kind].sum())


def test_head_counters_accumulate_and_runs_repeat(dev):
    from mdil_ss_amd import density as D
    run = head_run(27, BIG, "clustered")
    hist, nonf, agree = new_hist(dev), zeros(dev, 1), zeros(dev, 2)
    for n in (1, 2):
        label, nearest, code = D.density_head(*run["args"], map_kind="rmaha", hist=hist, nonfinite=nonf, agree=agree,
                                              want_label=(n == 1), want_nearest=(n == 2))
        assert (label is None) == (n == 2) and (nearest is None) == (n == 1)
        assert torch.equal(hist.cpu(), n * run["hist"]) and int(nonf.item()) == 0
        assert agree.tolist() == [n * v for v in run["agree"]]
        assert torch.equal(HC.as_bytes(code.cpu()), HC.as_bytes(run["dcodes"][1].cpu()))
    assert torch.equal(nearest.cpu(), run["nearest"])


def _raw_head(dev, nc, shape, given):
    from mdil_ss_amd import _density_lib
    lib = _density_lib.load()
    xd, wd, bd, dm = head_run(nc, shape, "clustered")["args"]
    N, H, W = shape
    npx = N * 4 * H * W
    arena = HC.Arena(dev, {"label": npx, "nearest": npx, "code": 2 * npx, "hist": 2 * 2 * 65536 * 8, "nonfinite": 8,
                           "agree": 16})
    p = {k: (arena.ptr(k) if k in given else None) for k in arena.sizes}
    rc = lib.mdil_density_head(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), N, H, W, nc, dm.buffer.data_ptr(),
                               dm.cls.data_ptr(), dm.K, None, None, 0, 3, 1 if "code" in given else -1, p["label"],
                               p["nearest"], p["code"], p["hist"], p["nonfinite"], p["agree"],
                               torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mdil_density_last_error()
    torch.cuda.synchronize()
    arena.read()
    return arena


@pytest.mark.parametrize("shape", ((1, 1, 1), (1, 9, 7), BIG))
def test_head_null_outputs_and_guard_bands_stay_untouched(dev, shape):
    """Each output alone, then all of them: what was not given keeps its sentinel bytes, and so do the
    guard bands.  The counters are ADDED to: they start from the sentinel 0xA5A5A5A5A5A5A5A5."""
    nc = 27
    run = head_run(nc, shape, "clustered")
    names = ("label", "nearest", "code", "hist", "nonfinite", "agree")
    for given in tuple((n,) for n in names) + (names,):
        arena = _raw_head(dev, nc, shape, given)
        arena.assert_untouched([k for k in given if k != "nonfinite"], given)      # no NaN: nonfinite is never touched
        if "label" in given:
            assert torch.equal(arena.cut("label"), run["label"].reshape(-1))
        if "nearest" in given:
            assert torch.equal(arena.cut("nearest"), run["nearest"].reshape(-1))
        if "code" in given:
            assert torch.equal(arena.cut("code").view(torch.int16).long() & 0xffff, run["codes"][1].reshape(-1))
        if "hist" in given:
            assert torch.equal(arena.cut("hist").view(torch.int64).reshape(2, 2, 65536) - SENTINEL, run["hist"])
        if "agree" in given:
            assert (arena.cut("agree").view(torch.int64) - SENTINEL).tolist() == run["agree"]


def test_head_grid_stride_loop_past_the_grid_bound(dev):
    """The grid is bounded at 768 work-groups of 256 feature pixels; 1 x 385 x 511 = 196,735 of them sends
    127 pixels (one whole wave and a ragged one) round the loop a second time, into a work-group's table
    that already holds counts.  Two classes (one mean); every check of the small cases."""
    from mdil_ss_amd import density as D
    nc, shape = 2, (1, 385, 511)
    rows = shape[1] * shape[2]
    assert HEAD_WG * HEAD_BLOCKS < rows < 2 * HEAD_WG * HEAD_BLOCKS and (rows - HEAD_WG * HEAD_BLOCKS) % 64 == 63
    model = head_model(nc, "clustered")[0]
    x = R.clustered(16, 1, rows, seed=5)[0]
    _, w, b = HC.head_inputs(nc, BIG)
    xd, wd, bd = x.reshape(1, shape[1], shape[2], 16).to(dev), w.to(dev), b.to(dev)
    from mdil_ss_amd import openset as OS
    from mdil_ss_amd.predict import predict_head
    lut = OS.group_lut([1], [2])
    target = HC.make_target(3, (1, 2 * shape[1], 2 * shape[2]), 2, seed=7)
    groups = lut[target.long()].long()
    hist, nonf, agree = new_hist(dev), zeros(dev, 1), zeros(dev, 2)
    label, nearest, c0 = D.density_head(xd, wd, bd, model, target=target.to(dev), lut=lut.to(dev), map_kind=0, hist=hist,
                                        nonfinite=nonf, agree=agree, want_nearest=True)
    c1 = D.density_head(xd, wd, bd, model, map_kind=1, want_label=False)[2]
    assert torch.equal(label, predict_head(xd, wd, bd, None, False)[0])
    codes = torch.stack([OS.code_values(c.cpu()) for c in (c0, c1)])
    ref = R.scores64(x, model)
    m32, r32 = R.scores32(x, model)
    ref["d32"] = [float((m32.double() - ref["maha"]).abs().max()), float((r32.double() - ref["rmaha"]).abs().max())]
    small = codes[:, :, ::2, ::2]
    check_codes("past the grid bound", small.reshape(2, -1), ref)
    assert bool((nearest == 0).all()) and int(nonf.item()) == 0
    for k in range(2):
        assert torch.equal(codes[k], expand(small[k], shape))
        assert torch.equal(hist[k].cpu(), OR.hist_of(codes[k], groups)), R.KINDS[k]
    known = groups == 0
    assert agree.tolist() == [int(known.sum()), int((label.cpu() == 0)[known].sum())]


def test_head_side_stream_gives_the_same_bytes(dev):
    from mdil_ss_amd import density as D
    from mdil_ss_amd import openset as OS
    nc = 27
    run = head_run(nc, BIG, "clustered")
    lut = lut_case(nc).to(dev)
    target = HC.make_target(nc, tuple(run["label"].shape), nc - 1, seed=3).to(dev)
    cdf = (torch.arange(65536) // 256).to(torch.uint8).to(dev)

    def everything():
        hist, agree = new_hist(dev), zeros(dev, 2)
        label, nearest, code = D.density_head(*run["args"], target=target, lut=lut, map_kind=0, hist=hist, agree=agree,
                                              want_nearest=True)
        counters = OS.new_apply_counters(nc, dev)
        thr = int(OS.code_values(code).median().item())
        out, score = OS.openset_apply(label, code, nc, thr, None, 255, cdf, target, lut, counters)
        return [label, nearest, code, hist, agree, out, score] + [counters[k] for k in OS.APPLY_COUNTERS]

    first = everything()
    torch.cuda.synchronize()
    second = HC.side_stream(everything)
    for a, c in zip(first, second):
        assert torch.equal(HC.as_bytes(a.cpu()), HC.as_bytes(c.cpu()))
    assert torch.equal(first[0].cpu(), run["label"])


def test_head_nan_feature_is_counted_and_enters_no_histogram(dev):
    from mdil_ss_amd import density as D
    from mdil_ss_amd import openset as OS
    nc, shape = 20, (2, 12, 20)
    clean = head_run(nc, shape, "clustered")
    xd, wd, bd, dm = clean["args"]
    xn = xd.clone()
    xn[1, 9, 5, 7] = float("nan")                                   # one feature pixel: its four output pixels
    hit = torch.zeros_like(clean["codes"][0], dtype=torch.bool)
    hit[1, 18:20, 10:12] = True
    for k in range(2):
        hist, nonf, agree = new_hist(dev), zeros(dev, 1), zeros(dev, 2)
        label, nearest, code = D.density_head(xn, wd, bd, dm, map_kind=k, hist=hist, nonfinite=nonf, agree=agree,
                                              want_nearest=True)
        code, nearest = OS.code_values(code.cpu()), nearest.cpu()
        assert int(nonf.item()) == 4 and bool((code[hit] == D.NONFINITE_CODE).all())
        assert bool((nearest[hit] == D.NO_CLASS).all()) and torch.equal(nearest[~hit], clean["nearest"][~hit])
        assert torch.equal(code[~hit], clean["codes"][k][~hit])
        for j in range(2):
            assert int(hist[j].sum()) == code.numel() - 4 and int(hist[j, :, D.NONFINITE_CODE].sum()) == 0
        assert torch.equal(hist[k].cpu(), OR.hist_of(code, hit.long() * 2))
        assert agree.tolist() == [code.numel(), int((nearest == label.cpu()).sum())]


# ------------------------------------------------------------------------------- (e) the rows form
@functools.lru_cache(maxsize=None)
def rows_model(C, K):
    x, lab, far = R.clustered(C, K, max(ROW_N), seed=7 * C + K)
    pivot = x[:64].double().mean(0).float().numpy()
    return R.fit(x, lab, K, min_rows=2, pivot=pivot), x, far


@functools.lru_cache(maxsize=None)
def rows_reference(C, K, n):
    model, x, _ = rows_model(C, K)
    ref = R.scores64(x[:n], model)
    m32, r32 = R.scores32(x[:n], model)
    ref["d32"] = [float((m32.double() - ref["maha"]).abs().max()), float((r32.double() - ref["rmaha"]).abs().max())]
    return ref


def rows_groups(n, seed):
    return torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


@pytest.mark.parametrize("K", ROW_K)
@pytest.mark.parametrize("n", ROW_N)
@pytest.mark.parametrize("C", ROW_C)
def test_rows_codes_nearest_and_histograms(dev, C, n, K):
    from mdil_ss_amd import density as D
    from mdil_ss_amd import openset as OS
    model, x, _ = rows_model(C, K)
    assert len(model["cls"]) == K
    ref = rows_reference(C, K, n)
    dm = D.DeviceModel(model, dev)
    xd = x[:n].contiguous().to(dev)
    what = f"C {C} rows {n} K {K}"
    group = rows_groups(n, C + n + K)
    hist, nonf = new_hist(dev), zeros(dev, 1)
    nearest, c0 = D.density_rows(xd, dm, group.to(dev), map_kind=0, hist=hist, nonfinite=nonf)
    none, c1 = D.density_rows(xd, dm, map_kind=1, want_nearest=False)
    assert none is None and nearest.dtype == torch.uint8 and tuple(nearest.shape) == (n,) and c0.dtype == torch.uint16
    codes = torch.stack([OS.code_values(c.cpu()) for c in (c0, c1)])
    check_codes(what, codes, ref)                                                          # (b)
    check_nearest(what, nearest.cpu(), ref)                                                # (c)
    assert int(nonf.item()) == 0
    for k in range(2):                                                                     # (d)
        assert torch.equal(hist[k].cpu(), OR.hist_of(codes[k], group.long())), R.KINDS[k]
    for g in (0, 1, 2):
        h = new_hist(dev)
        D.density_rows(xd, dm, const_group=g, kinds=["rmaha"], hist=h, want_nearest=False)
        assert int(h[0].sum()) == 0
        assert torch.equal(h[1].cpu(), OR.hist_of(codes[1], torch.full_like(codes[1], g)))
    D.density_rows(xd, dm, group.to(dev), hist=hist, nonfinite=nonf, want_nearest=False)       # accumulates
    for k in range(2):
        assert torch.equal(hist[k].cpu(), 2 * OR.hist_of(codes[k], group.long()))


def test_rows_grid_stride_loop_past_the_grid_bound(dev):
    """512 work-groups of 64 rows; 32,895 rows send 127 of them (a whole trip and one with 63 rows) round the
    loop a second time."""
    from mdil_ss_amd import density as D
    from mdil_ss_amd import openset as OS
    C, K, n = 16, 2, ROWS_TRIP * ROWS_BLOCKS + 127
    assert (n - ROWS_TRIP * ROWS_BLOCKS) % 64 == 63
    model = rows_model(C, K)[0]
    x = R.clustered(C, K, n, seed=11)[0]
    ref = R.scores64(x, model)
    m32, r32 = R.scores32(x, model)
    ref["d32"] = [float((m32.double() - ref["maha"]).abs().max()), float((r32.double() - ref["rmaha"]).abs().max())]
    xd, group = x.to(dev), rows_groups(n, 5)
    hist, nonf = new_hist(dev), zeros(dev, 1)
    nearest, c0 = D.density_rows(xd, model, group.to(dev), map_kind=0, hist=hist, nonfinite=nonf)
    c1 = D.density_rows(xd, model, map_kind=1, want_nearest=False)[1]
    codes = torch.stack([OS.code_values(c.cpu()) for c in (c0, c1)])
    check_codes("rows past the grid bound", codes, ref)
    check_nearest("rows past the grid bound", nearest.cpu(), ref)
    assert int(nonf.item()) == 0
    for k in range(2):
        assert torch.equal(hist[k].cpu(), OR.hist_of(codes[k], group.long())), R.KINDS[k]


@pytest.mark.parametrize("C, n", ((16, 65), (128, 4671)))
def test_rows_null_outputs_guard_bands_side_stream_and_nan(dev, C, n):
    from mdil_ss_amd import _density_lib
    from mdil_ss_amd import density as D
    from mdil_ss_amd import openset as OS
    lib = _density_lib.load()
    K = 20
    model, x, _ = rows_model(C, K)
    dm = D.DeviceModel(model, dev)
    xd = x[:n].contiguous().to(dev)
    hist = new_hist(dev)
    nearest, c1 = D.density_rows(xd, dm, map_kind=1, hist=hist)
    torch.cuda.synchronize()
    names = ("nearest", "code", "hist", "nonfinite")
    for given in tuple((k,) for k in names) + (names,):
        arena = HC.Arena(dev, {"nearest": n, "code": 2 * n, "hist": 2 * 2 * 65536 * 8, "nonfinite": 8})
        p = {k: (arena.ptr(k) if k in given else None) for k in names}
        rc = lib.mdil_density_rows(xd.data_ptr(), n, C, dm.buffer.data_ptr(), dm.cls.data_ptr(), dm.K, None, 0, 3,
                                   1 if "code" in given else -1, p["nearest"], p["code"], p["hist"], p["nonfinite"],
                                   torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.mdil_density_last_error()
        torch.cuda.synchronize()
        arena.read()
        arena.assert_untouched([k for k in given if k != "nonfinite"], given)
        if "nearest" in given:
            assert torch.equal(arena.cut("nearest"), nearest.cpu())
        if "code" in given:
            assert torch.equal(arena.cut("code"), HC.as_bytes(c1.cpu()).reshape(-1))
        if "hist" in given:
            assert torch.equal(arena.cut("hist").view(torch.int64).reshape(2, 2, 65536) - SENTINEL, hist.cpu())
    side = HC.side_stream(lambda: D.density_rows(xd, dm, map_kind=1))
    assert torch.equal(side[0].cpu(), nearest.cpu()) and torch.equal(HC.as_bytes(side[1].cpu()), HC.as_bytes(c1.cpu()))
    xn = xd.clone()
    xn[n // 2, C - 3] = float("nan")
    h, nonf = new_hist(dev), zeros(dev, 1)
    near_n, code_n = D.density_rows(xn, dm, map_kind=0, hist=h, nonfinite=nonf)
    code_n, clean = OS.code_values(code_n.cpu()), OS.code_values(D.density_rows(xd, dm, map_kind=0)[1].cpu())
    hit = torch.zeros(n, dtype=torch.bool)
    hit[n // 2] = True
    assert int(nonf.item()) == 1 and int(code_n[n // 2]) == D.NONFINITE_CODE and int(near_n[n // 2]) == D.NO_CLASS
    assert torch.equal(code_n[~hit], clean[~hit]) and torch.equal(near_n.cpu()[~hit], nearest.cpu()[~hit])
    assert torch.equal(h[0].cpu(), OR.hist_of(code_n, hit.long() * 2)) and int(h[1].sum()) == n - 1


# ------------------------------------------------------------- (f) crowded and spread histograms
@pytest.mark.parametrize("shape", ((1, 9, 7), BIG))
def test_crowded_and_spread_bins(dev, shape):
    """All rows equal: one bin per kind holds every pixel, whatever the groups.  The far rows alone (uniform
    in +-6): at least 200 occupied bins, the input the table is built for."""
    from mdil_ss_amd import density as D
    from mdil_ss_amd import openset as OS
    nc = 20
    N, H, W = shape
    npix = 4 * N * H * W
    model = head_model(nc, "clustered")[0]
    dm = D.DeviceModel(model, dev)
    _, w, b = HC.head_inputs(nc, shape)
    wd, bd = w.to(dev), b.to(dev)
    one = head_model(nc, "clustered")[1][:1]
    same = one.expand(N * H * W, 16).reshape(N, H, W, 16).contiguous().to(dev)
    lut = OS.group_lut([1], [2]).to(dev)
    for pattern in ("none", "by lane", "by pixel", "thirds"):
        target = torch.zeros(N, 2 * H, 2 * W, dtype=torch.uint8)
        if pattern == "by lane":
            target[:, :, 2::4] = 1
            target[:, :, 3::4] = 1
        elif pattern == "by pixel":
            target[:, :, 1::2] = 1
        elif pattern == "thirds":
            target.reshape(-1)[1::3] = 1
            target.reshape(-1)[2::3] = 2
        hist = new_hist(dev)
        codes = [OS.code_values(D.density_head(same, wd, bd, dm, target=target.to(dev), lut=lut, map_kind=k,
                                               hist=hist if k == 0 else None, want_label=False)[2].cpu()) for k in range(2)]
        for k in range(2):
            c = int(codes[k].reshape(-1)[0])
            assert bool((codes[k] == c).all())
            for g in (0, 1):
                assert int(hist[k, g, c]) == int((target == g).sum()), (pattern, k, g)
            assert int(hist[k].sum()) == int((target < 2).sum()) and int((hist[k].sum(0) > 0).sum()) == 1
    far = (torch.rand(N * H * W, 16, generator=torch.Generator().manual_seed(H)) * 12.0 - 6.0)
    hist = new_hist(dev)
    fd = far.reshape(N, H, W, 16).contiguous().to(dev)
    codes = [OS.code_values(D.density_head(fd, wd, bd, dm, map_kind=k, hist=hist if k == 0 else None,
                                           want_label=False)[2].cpu()) for k in range(2)]
    rows_hist = new_hist(dev)
    rcodes = OS.code_values(D.density_rows(far.to(dev), dm, map_kind=0, hist=rows_hist, want_nearest=False)[1].cpu())
    # (the two forms sum a row's 16 squares in different orders: their codes need not be equal)
    assert torch.equal(rows_hist[0].cpu(), OR.hist_of(rcodes, torch.zeros_like(rcodes)))
    assert int(rows_hist[1].sum()) == N * H * W and (shape != BIG or int((rows_hist[1, 0] > 0).sum()) >= 200)
    for k in range(2):
        assert torch.equal(hist[k].cpu(), OR.hist_of(codes[k], torch.zeros_like(codes[k])))
        occupied = int((hist[k, 0] > 0).sum())
        print(f"shape {shape} {R.KINDS[k]}: {occupied} occupied bins over {npix} pixels")
        if shape == BIG:
            assert occupied >= 200


# ----------------------------------------------------------------------------- (g) end to end
@pytest.fixture(scope="module")
def tiny_model(dev):
    return HC.tiny_model(dev)


@pytest.fixture(scope="module")
def checkpoint(tiny_model, tmp_path_factory):
    path = tmp_path_factory.mktemp("density") / "checkpoint.pth.tar"
    HC.save_checkpoint(tiny_model, path)
    return str(path)


CLI = ["--num-classes", "20", "20", "--task", "1", "--synthetic", "4", "--height", "64", "--width", "128",
       "--batch-size", "3"]


def synthetic(dev, n, task):
    from mdil_ss_amd.dataset import ProceduralSeg
    ds = ProceduralSeg(n, 64, 128, 20, seed=12 + task, domain=task)
    return (torch.stack([ds[i][0] for i in range(n)]).to(dev),
            torch.stack([ds[i][1][0] for i in range(n)]).to(torch.uint8))


def saved_table(kind_report):
    table = torch.zeros(2, 65536, dtype=torch.int64)
    for g, name in enumerate(("known", "unknown")):
        for b, n in kind_report["hist"][name]:
            table[g, b] = n
    return table


def check_report_metrics(kinds, names, hist):
    """Every figure of the report against the reference's Fractions of the given histograms."""
    for k, name in enumerate(names):
        got, want = kinds[name], OR.metrics(hist[k])
        assert torch.equal(saved_table(got), hist[k]), name
        for key in ("auroc", "fpr_at_tpr", "tie_mass"):
            assert got[key] == float(want[key]), (name, key)
        assert abs(got["aupr"] - float(want["aupr"])) <= 4 * 2.0 ** -53
        assert (got["threshold_code"], got["P"], got["N"]) == (want["threshold_code"], want["P"], want["N"])
        assert got["occupied_bins"] == int((hist[k].sum(0) > 0).sum())


@pytest.fixture(scope="module")
def fitted(dev, checkpoint, tmp_path_factory):
    """``--fit`` on the procedural set, both layers -> {layer: (path, report)}."""
    from mdil_ss_amd import density as D
    root = tmp_path_factory.mktemp("density_models")
    out = {}
    for layer in ("penultimate", "encoder"):
        path = str(root / f"{layer}.npz")
        report = D.main(D.build_parser().parse_args(["--state", checkpoint] + CLI + ["--fit", path, "--layer", layer,
                                                                                    "--min-rows", "8"]))
        out[layer] = (path, report)
    return out


def test_cli_fit_matches_the_fit_from_rows(dev, tiny_model, fitted):
    from mdil_ss_amd import density as D
    from mdil_ss_amd import latent
    images, target = synthetic(dev, 4, 1)
    for layer, C in (("penultimate", 16), ("encoder", 128)):
        path, report = fitted[layer]
        model = D.load_model(path, layer=layer, nc=20, C=C, task=1)
        feat = latent.latents(tiny_model, images, 1, layer)
        lab = latent.resize_labels(target, feat.shape[1], feat.shape[2])
        want = R.fit(feat.reshape(-1, C).cpu(), lab.reshape(-1), 19, min_rows=8, pivot=model["pivot"])
        assert report["rows"] == want["rows"] == model["rows"] and report["ridge_note"] == "untuned"
        assert model["cls"].tolist() == want["cls"].tolist() == report["classes"]
        assert model["counts"].tolist() == want["counts"].tolist()
        # the moments come from the fp32 MFMA (exact products, fp32 chains of at most 1,024 rows, then fp64)
        for key in ("means", "cov_within", "cov_total"):
            err = float(np.abs(model[key] - want[key]).max()) / float(np.abs(want[key]).max())
            print(f"{layer} {key}: relative distance from the fp64 fit {err:.2e}")
            assert err <= 1e-4, (layer, key)


def test_cli_score_report(dev, tiny_model, checkpoint, fitted, tmp_path):
    from mdil_ss_amd import density as D
    from mdil_ss_amd import openset as OS
    report_file = tmp_path / "report.json"
    D.main(D.build_parser().parse_args(["--state", checkpoint] + CLI + ["--model", fitted["penultimate"][0], "--score",
                                                                       "--with-logit-scores", "--json", str(report_file)]))
    with open(report_file) as f:
        saved = json.load(f)
    images, target = synthetic(dev, 4, 1)
    model = D.load_model(fitted["penultimate"][0])
    lut = OS.group_lut([19])
    meter, logit = D.DensityMeter(20, model, D.KINDS, lut), OS.OpenSetMeter(20, OS.KINDS, lut)
    labels, nearests = [], []
    for i in (0, 3):
        label, nearest, _ = meter.add(tiny_model, images[i:i + 3], 1, target=target[i:i + 3].to(dev), want_label=True,
                                      want_nearest=True)
        logit.add(tiny_model, images[i:i + 3], 1, target=target[i:i + 3].to(dev))
        labels.append(label.cpu())
        nearests.append(nearest.cpu())
    label, nearest = torch.cat(labels), torch.cat(nearests)
    unknown = int((target == 19).sum())
    assert 0 < unknown < target.numel()
    assert saved["images"] == 4 and saved["pixels"] == target.numel() and saved["nonfinite"] == 0
    assert saved["unknown_ids"] == [19] and sorted(saved["kinds"]) == sorted(R.KINDS) and saved["layer"] == "penultimate"
    assert sorted(saved["logit_kinds"]) == sorted(OR.KINDS) and saved["ridge_note"] == "untuned"
    check_report_metrics(saved["kinds"], R.KINDS, meter.hist())
    check_report_metrics(saved["logit_kinds"], OR.KINDS, logit.hist())
    for name in R.KINDS:
        assert (saved["kinds"][name]["P"], saved["kinds"][name]["N"]) == (unknown, target.numel() - unknown)
    known = target != 19
    assert saved["known_pixels"] == int(known.sum()) and saved["nearest_agrees"] == int((nearest == label)[known].sum())
    assert saved["nearest_agreement"] == saved["nearest_agrees"] / saved["known_pixels"]
    from mdil_ss_amd.fullres import iou_rule
    for name, pred in (("head", label), ("nearest", nearest)):
        m = HC.expected_counts(target, pred, 20, 19)[0].double()
        assert saved["mIoU"][name]["mIoU"] == float(iou_rule(20, 19, m.diagonal(), m.sum(0), m.sum(1))[0])


def test_cli_score_encoder_layer_and_foreign_domain(dev, tiny_model, checkpoint, fitted, tmp_path):
    from mdil_ss_amd import density as D
    from mdil_ss_amd import openset as OS
    report_file = tmp_path / "encoder.json"
    D.main(D.build_parser().parse_args(["--state", checkpoint] + CLI + [
        "--model", fitted["encoder"][0], "--score", "--json", str(report_file), "--foreign-synthetic", "2",
        "--foreign-task", "0"]))
    with open(report_file) as f:
        saved = json.load(f)
    images, target = synthetic(dev, 4, 1)
    foreign, _ = synthetic(dev, 2, 0)
    meter = D.DensityMeter(20, D.load_model(fitted["encoder"][0]), D.KINDS, OS.group_lut([], [19]), layer="encoder")
    for i in (0, 3):
        meter.add(tiny_model, images[i:i + 3], 1, target=target[i:i + 3].to(dev))
    meter.add(tiny_model, foreign, 1, const_group=OS.UNKNOWN)
    assert saved["layer"] == "encoder" and saved["grid_size"] == [8, 16] and "encoder's own grid" in saved["grid"]
    assert saved["foreign_images"] == 2 and saved["pixels"] == 6 * 8 * 16 and saved["mIoU"] is None
    check_report_metrics(saved["kinds"], R.KINDS, meter.hist())
    for name in R.KINDS:
        assert saved["kinds"][name]["P"] == 2 * 8 * 16


def test_cli_fit_threshold_then_reject_maps(dev, tiny_model, checkpoint, fitted, tmp_path):
    from mdil_ss_amd import boundary as B
    from mdil_ss_amd import density as D
    from mdil_ss_amd import openset as OS
    model_file = fitted["penultimate"][0]
    fit_file, out = tmp_path / "thresholds.json", tmp_path / "maps"
    thr_report = D.main(D.build_parser().parse_args(["--state", checkpoint] + CLI + ["--model", model_file, "--fit-threshold",
                                                                                    str(fit_file), "--known-fpr", "0.05"]))
    images, target = synthetic(dev, 4, 1)
    known = target != 19
    for name in R.KINDS:
        k = thr_report["kinds"][name]
        assert k["known_pixels"] == int(known.sum()) and k["rejected_known"] <= 0.05 * k["known_pixels"]
    report = D.main(D.build_parser().parse_args(["--state", checkpoint] + CLI + [
        "--model", model_file, "--threshold", str(fit_file), "--kind", "rmaha", "--out", str(out), "--unknown-id", "254",
        "--colour", "--nearest"]))
    assert len(glob.glob(str(out / "*_label.png"))) == 4 and len(report["written"]) == 16
    thr = thr_report["kinds"]["rmaha"]["threshold_code"]
    cdf = OS.cdf_from_starts(thr_report["kinds"]["rmaha"]["cdf_starts"])
    meter = D.DensityMeter(20, D.load_model(model_file), ["rmaha"])
    seen, rejected = torch.zeros(20, dtype=torch.int64), torch.zeros(20, dtype=torch.int64)
    from PIL import Image
    for i in range(4):
        got = torch.from_numpy(B.read_label_png(str(out), f"synthetic_{i:04d}", (64, 128)))
        label, nearest, code = meter.add(tiny_model, images[i:i + 1], 1, const_group=OS.IGNORED, map_kind="rmaha",
                                         want_label=True, want_nearest=True)
        want = OR.apply_rule(label.cpu()[0], OS.code_values(code.cpu())[0], 20, thr, None, 254, cdf)
        assert torch.equal(got.reshape(-1), want["out"])
        with Image.open(out / f"synthetic_{i:04d}_unknown.png") as im:
            assert im.mode == "L" and im.size == (128, 64)
            assert torch.equal(torch.from_numpy(np.array(im)).reshape(-1), want["score"])
        with Image.open(out / f"synthetic_{i:04d}_nearest.png") as im:
            assert torch.equal(torch.from_numpy(np.array(im)), nearest.cpu()[0])
        seen += want["seen"]
        rejected += want["rejected"]
    assert report["seen"] == seen.tolist() and report["rejected"] == rejected.tolist()
    assert int(rejected.sum()) > 0
