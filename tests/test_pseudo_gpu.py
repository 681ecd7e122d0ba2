"""GPU: the pseudo-label kernels (mdil_ss_amd/ext/pseudo_head.hip) and the entry points over them
(mdil_ss_amd/pseudo.py), against tests/pseudo_reference.py and the fp64 head of tests/head_cases.py.

What is compared with what.  ``pseudo_head`` promises ``predict_head``'s chain of operations, so its
label and its confidence (before the quantisation) are ``predict_head``'s bits: both are asserted
bit for bit.  Independently the label is held to the fp64 argmax outside fp32 near-ties (k = 17, at
most 0.1 % of a case, as tests/test_predict_gpu.py), and q to the quantised fp64 softmax maximum
within one quantum: the measured relative error bound of the confidence there (2 x 6.967e-7) is
0.091 of a quantum at q = 65536, so truncation can move q by at most one.  Everything after the
quantisation is integer arithmetic and is asserted exactly, on the kernel's own maps."""
import functools
import glob
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import head_cases as HC
from tests import pseudo_reference as R
from tests.head_cases import CLASSES, SHAPES, nhwc

pytestmark = pytest.mark.gpu

K = 17
MAX_EXCLUDED = 1e-3
BIG = (3, 16, 48)
SCALE = 8.0                                     # the trained regime: logits 8 times as far apart
NPIX = (1, 3, 5, 1001, 1024)                    # 8 pixels per load: odd tails, a ragged and a whole size
HEAD_WG, HEAD_BLOCKS = 1024, 256                # pseudo_head.hip: kHeadWG, kHeadMaxBlocks
MAP_WG, MAP_BLOCKS, PER_ITEM = 256, 512, 8      # kMapWG, kMapMaxBlocks, kPerItem


@pytest.fixture(scope="module")
def dev():
    return HC.device("pseudo-label")


def inputs(nc, shape, scale=1.0):
    x, w, b = HC.head_inputs(nc, shape)
    return x, (w * scale if scale != 1.0 else w), b


@functools.lru_cache(maxsize=None)
def reference(nc, shape, scale=1.0):
    """fp64: label, q64 of the softmax maximum, near-tie mask.  Computed once, never modified."""
    x, w, b = inputs(nc, shape, scale)
    logits, S = HC.head64(x, w, b)
    return logits.max(1)[1], R.quantise(F.softmax(logits, 1).max(1)[0]), HC.near_tie(logits, S, K)


@functools.lru_cache(maxsize=None)
def device_run(nc, shape, scale=1.0):
    """One pseudo_head call into fresh counters and predict_head on the same inputs -> host tensors
    (label u8, q i64, hist, nonfinite, predict's label, predict's confidence) and the device maps."""
    from mdil_ss_amd import pseudo as P
    from mdil_ss_amd.predict import predict_head
    dev = torch.device("cuda", 0)
    x, w, b = inputs(nc, shape, scale)
    xd, wd, bd = nhwc(x).to(dev), w.to(dev), b.to(dev)
    hist = torch.zeros(nc, 256, dtype=torch.int64, device=dev)
    nonf = torch.zeros(1, dtype=torch.int64, device=dev)
    label, qconf = P.pseudo_head(xd, wd, bd, hist, nonf)
    plabel, _, pconf = predict_head(xd, wd, bd, None, True)
    torch.cuda.synchronize()
    return dict(label=label.cpu(), q=P.q_values(qconf.cpu()), hist=hist.cpu(), nonfinite=int(nonf.item()),
                plabel=plabel.cpu(), pconf=pconf.cpu(), dlabel=label, dqconf=qconf, args=(xd, wd, bd))


def check_head(nc, shape, scale, run):
    """The integer contracts and the bit identity with predict_head."""
    assert run["label"].dtype == torch.uint8 and tuple(run["label"].shape) == (shape[0], 2 * shape[1], 2 * shape[2])
    assert torch.equal(run["label"], run["plabel"])
    assert torch.equal(run["q"], R.quantise(run["pconf"]))
    assert run["nonfinite"] == 0 and int(run["q"].min()) >= 1 and int(run["q"].max()) <= 65535
    assert torch.equal(run["hist"], R.hist_level1(run["label"], run["q"], nc))
    assert int(run["hist"].sum()) == run["label"].numel()


# ------------------------------------------------------------------------------------ (1), (2)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nc", CLASSES)
def test_head_matches_predict_head_and_the_fp64_reference(dev, nc, shape):
    run = device_run(nc, shape)
    ref_label, q64, excluded = reference(nc, shape)
    check_head(nc, shape, 1.0, run)
    HC.check_labels(run["label"], ref_label, excluded, f"nc {nc} shape {shape}", HC.share(MAX_EXCLUDED))
    diff = (run["q"] - q64).abs()[~excluded]
    print(f"nc {nc} shape {shape}: |q - q64| max {int(diff.max())}, differing {int((diff > 0).sum())} of {diff.numel()}")
    assert int(diff.max()) <= 1


def test_histogram_accumulates(dev):
    from mdil_ss_amd import pseudo as P
    nc = 27
    run = device_run(nc, BIG)
    hist = torch.zeros(nc, 256, dtype=torch.int64, device=dev)
    for n in (1, 2):
        label, qconf = P.pseudo_head(*run["args"], hist, None, want_label=(n == 1), want_qconf=(n == 2))
        assert (label is None) == (n == 2) and (qconf is None) == (n == 1)
        assert torch.equal(hist.cpu(), n * run["hist"])
    assert torch.equal(P.q_values(qconf.cpu()), run["q"])


def _raw_head(dev, nc, shape, given):
    from mdil_ss_amd import _pseudo_lib
    lib = _pseudo_lib.load()
    xd, wd, bd = device_run(nc, shape)["args"]
    N, H, W = shape
    npx = N * 4 * H * W
    arena = HC.Arena(dev, {"label": npx, "qconf": 2 * npx, "hist": nc * 256 * 8, "nonfinite": 8})
    rc = lib.mdil_pseudo_head(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), N, H, W, nc,
                              *(arena.ptr(k) if k in given else None for k in ("label", "qconf", "hist", "nonfinite")),
                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mdil_pseudo_last_error()
    torch.cuda.synchronize()
    arena.read()
    return arena


@pytest.mark.parametrize("shape", ((1, 1, 1), (1, 9, 7), BIG))
def test_head_null_outputs_and_guard_bands_stay_untouched(dev, shape):
    """Each map alone, then all of them: what was not given keeps its sentinel bytes, and so do the
    guard bands.  The counters are ADDED to: they start from the sentinel 0xA5A5A5A5A5A5A5A5."""
    nc = 27
    run = device_run(nc, shape)
    sentinel = torch.tensor([0xA5] * 8, dtype=torch.uint8).view(torch.int64)
    for given in (("label",), ("qconf",), ("hist",), ("label", "qconf", "hist", "nonfinite")):
        arena = _raw_head(dev, nc, shape, given)
        written = [k for k in given if k != "nonfinite"]           # no NaN: nonfinite is never touched
        arena.assert_untouched(written, given)
        if "label" in given:
            assert torch.equal(arena.cut("label"), run["label"].reshape(-1))
        if "qconf" in given:
            assert torch.equal(arena.cut("qconf").view(torch.int16).long() & 0xffff, run["q"].reshape(-1))
        if "hist" in given:
            assert torch.equal(arena.cut("hist").view(torch.int64).reshape(nc, 256) - sentinel, run["hist"])


def test_nan_confidences_are_counted_and_quantised_to_zero(dev):
    from mdil_ss_amd import pseudo as P
    nc = 20
    x, w, b = inputs(nc, (2, 12, 20))
    xn = x.clone()
    xn[1, 5, 7, 9] = float("nan")                                   # one feature: its four output pixels
    hist = torch.zeros(nc, 256, dtype=torch.int64, device=dev)
    nonf = torch.zeros(1, dtype=torch.int64, device=dev)
    label, qconf = P.pseudo_head(nhwc(xn).to(dev), w.to(dev), b.to(dev), hist, nonf)
    q = P.q_values(qconf.cpu())
    clean = device_run(nc, (2, 12, 20))
    hit = torch.zeros_like(q, dtype=torch.bool)
    hit[1, 14:16, 18:20] = True
    assert int(nonf.item()) == 4 and (q[hit] == 0).all() and (label.cpu()[hit] == 0).all()
    assert torch.equal(q[~hit], clean["q"][~hit]) and torch.equal(label.cpu()[~hit], clean["label"][~hit])
    assert torch.equal(hist.cpu(), R.hist_level1(label.cpu(), q, nc)) and int(hist.sum()) == q.numel()


# ------------------------------------------------------------------------------------------ (3)
@pytest.mark.parametrize("nc", (2, 20))
def test_trained_regime_crowds_the_top_bin(dev, nc):
    """Weights times 8: the fp64 reference puts 20 % of the nc-2 pixels at q = 65535 (8 to 26 % per
    class) and up to 6.6 % of a class at nc 20.  Only the integer contracts and the bit identity with
    predict_head are asserted here; at nc 2 a portion of 0.05 must give the threshold 65535 and keep
    the whole tied run, which is more than k_c."""
    from mdil_ss_amd import pseudo as P
    run = device_run(nc, BIG, SCALE)
    check_head(nc, BIG, SCALE, run)
    top = (run["q"] == 65535)
    print(f"nc {nc}: {top.double().mean().item():.2%} of the pixels at q = 65535; fp64: "
          f"{(reference(nc, BIG, SCALE)[1] == 65535).double().mean().item():.2%}")
    if nc != 2:
        return
    thr = thresholds_on_device(run, nc, 0.05)
    assert thr == [65535, 65535] == R.sort_thresholds(run["label"], run["q"], nc, 0.05)[0]
    counters = P.new_apply_counters(nc, dev)
    P.pseudo_apply(run["dlabel"], run["dqconf"], nc, thr, counters={k: counters[k] for k in ("seen", "kept")},
                   want_out=False)
    for c in range(nc):
        seen, kept = int(counters["seen"][c].item()), int(counters["kept"][c].item())
        assert kept == int((top & (run["label"] == c)).sum()) > math.floor(0.05 * seen)


# ------------------------------------------------------------------------------------------ (4)
def refine_on_device(dev, label, q, nc, sel, hist2=None, bad=None):
    from mdil_ss_amd import pseudo as P
    hist2 = torch.zeros(nc, 256, dtype=torch.int64, device=dev) if hist2 is None else hist2
    bad = torch.zeros(1, dtype=torch.int64, device=dev) if bad is None else bad
    P.pseudo_refine(label, q, nc, sel, hist2, bad)
    return hist2, bad


def busiest_bytes(run, nc, skip):
    """Per class the high byte that holds most of its pixels; -1 for the class ``skip``."""
    return [-1 if c == skip else int(run["hist"][c].argmax()) for c in range(nc)]


@pytest.mark.parametrize("npix", NPIX + (None,))
@pytest.mark.parametrize("nc, scale", ((2, SCALE), (20, 1.0), (32, 1.0)))
def test_refine_counts_the_low_byte(dev, nc, scale, npix):
    run = device_run(nc, BIG, scale)
    n = run["label"].numel() if npix is None else npix
    dl, dq = run["dlabel"].reshape(-1)[:n], run["dqconf"].reshape(-1)[:n]
    hl, hq = run["label"].reshape(-1)[:n], run["q"].reshape(-1)[:n]
    sel = busiest_bytes(run, nc, skip=1)
    want, _ = R.hist_level2(hl, hq, nc, sel)
    hist2, bad = refine_on_device(dev, dl, dq, nc, sel)
    assert torch.equal(hist2.cpu(), want) and int(bad.item()) == 0
    assert int(want[1].sum()) == 0 and (npix is not None or int(want.sum()) > 0)
    refine_on_device(dev, dl, dq, nc, torch.tensor(sel, dtype=torch.int32, device=dev), hist2, bad)   # accumulates
    assert torch.equal(hist2.cpu(), 2 * want) and int(bad.item()) == 0


def test_refine_counts_bad_labels_and_nothing_else_for_them(dev):
    nc = 20
    run = device_run(nc, BIG)
    label = run["label"].clone().reshape(-1)
    g = torch.Generator().manual_seed(3)
    spoil = torch.rand(label.numel(), generator=g) < 0.02
    label[spoil] = torch.randint(nc, 256, (int(spoil.sum()),), generator=g, dtype=torch.uint8)
    sel = busiest_bytes(run, nc, skip=None)
    want, n_bad = R.hist_level2(label, run["q"].reshape(-1), nc, sel)
    assert n_bad == int(spoil.sum()) > 0
    hist2, bad = refine_on_device(dev, label.to(dev), run["dqconf"].reshape(-1), nc, sel)
    assert torch.equal(hist2.cpu(), want) and int(bad.item()) == n_bad


# ------------------------------------------------------------------------------------------ (5)
def thresholds_on_device(run, nc, portion, floor=0.0):
    from mdil_ss_amd import pseudo as P
    dev = run["dlabel"].device
    return P.thresholds(run["hist"], lambda sel: refine_on_device(dev, run["dlabel"], run["dqconf"], nc, sel)[0].cpu(),
                        portion, floor)


@pytest.mark.parametrize("nc, scale", [(nc, 1.0) for nc in CLASSES] + [(2, SCALE), (20, SCALE)])
def test_thresholds_end_to_end_match_the_sort(dev, nc, scale):
    run = device_run(nc, BIG, scale)
    per_class = [(0.0, 0.05, 0.2, 0.5, 1.0)[c % 5] for c in range(nc)]
    for portion, floor in ((0.0, 0.0), (0.05, 0.0), (0.2, 0.0), (0.5, 0.0), (1.0, 0.0), (per_class, 0.0), (0.2, 0.7),
                           (per_class, 0.31)):
        want, k = R.sort_thresholds(run["label"], run["q"], nc, portion, floor)
        thr = thresholds_on_device(run, nc, portion, floor)
        assert thr == want, (portion, floor)
        for c in range(nc):
            if floor == 0.0:
                assert int(((run["label"] == c) & (run["q"] >= thr[c])).sum()) >= k[c]


# ------------------------------------------------------------------------------------------ (6)
def apply_case(run, nc, n):
    """Host inputs of an apply over the first ``n`` pixels: thr (half of every class, class 1 wholly
    kept, class 0 not at all), id_map with a duplicate and a 255, targets with ignore and bad values."""
    hl, hq = run["label"].reshape(-1)[:n], run["q"].reshape(-1)[:n]
    thr = R.sort_thresholds(run["label"], run["q"], nc, 0.5)[0]
    thr[0], thr[1] = 65536, 0
    ids = HC.random_luts(nc)[0]
    target = HC.make_target(nc, (n,), nc - 1, seed=nc + n)
    return hl, hq, thr, ids, target


@pytest.mark.parametrize("npix", NPIX + (None,))
@pytest.mark.parametrize("nc, scale", ((2, SCALE), (20, 1.0), (32, 1.0)))
def test_apply_maps_and_counters(dev, nc, scale, npix):
    from mdil_ss_amd import pseudo as P
    run = device_run(nc, BIG, scale)
    n = run["label"].numel() if npix is None else npix
    hl, hq, thr, ids, target = apply_case(run, nc, n)
    dl, dq = run["dlabel"].reshape(-1)[:n], run["dqconf"].reshape(-1)[:n]
    want = R.apply_rule(hl, hq, nc, thr, ids, 254, target, nc - 1)
    keep = hq >= torch.tensor(thr)[hl.long()]                      # the reference, said with head_cases' own words
    assert torch.equal(HC.expected_counts(target[keep], hl[keep], nc, nc - 1)[0], want["confusion"])
    assert HC.expected_counts(target, hl, nc, nc - 1)[1] == want["bad_targets"]
    counters = P.new_apply_counters(nc, dev)
    for times in (1, 2):
        out = P.pseudo_apply(dl, dq, nc, thr, ids.to(dev), 254, target.to(dev), nc - 1, counters)
        assert out.dtype == torch.uint8 and torch.equal(out.cpu(), want["out"])
        for k in ("seen", "kept", "confusion"):
            assert torch.equal(counters[k].cpu(), times * want[k]), k
        assert int(counters["bad_targets"].item()) == times * want["bad_targets"]
        assert int(counters["bad_labels"].item()) == 0
    if npix is None:
        assert want["bad_targets"] > 0 and int(want["kept"].sum()) > 0 and int(want["kept"][0]) == 0
        assert torch.equal(want["kept"][1], want["seen"][1]) and int(want["confusion"].sum()) > 0
    # no id_map, no target, a subset of the counters: the identity map, nothing else touched
    some = {"kept": torch.zeros(nc, dtype=torch.int64, device=dev)}
    plain = R.apply_rule(hl, hq, nc, thr)
    assert torch.equal(P.pseudo_apply(dl, dq, nc, thr, counters=some).cpu(), plain["out"])
    assert torch.equal(some["kept"].cpu(), plain["kept"])


def test_apply_counts_bad_labels(dev):
    from mdil_ss_amd import pseudo as P
    nc = 20
    run = device_run(nc, BIG)
    hl, hq, thr, ids, target = apply_case(run, nc, run["label"].numel())
    label = hl.clone()
    g = torch.Generator().manual_seed(5)
    spoil = torch.rand(label.numel(), generator=g) < 0.02
    label[spoil] = torch.randint(nc, 256, (int(spoil.sum()),), generator=g, dtype=torch.uint8)
    want = R.apply_rule(label, hq, nc, thr, ids, 77, target, nc - 1)
    counters = P.new_apply_counters(nc, dev)
    out = P.pseudo_apply(label.to(dev), run["dqconf"].reshape(-1), nc, thr, ids.to(dev), 77, target.to(dev), nc - 1,
                         counters)
    assert torch.equal(out.cpu(), want["out"]) and (out.cpu()[spoil] == 77).all()
    for k in ("seen", "kept", "confusion"):
        assert torch.equal(counters[k].cpu(), want[k]), k
    assert int(counters["bad_labels"].item()) == want["bad_labels"] == int(spoil.sum())
    assert int(counters["bad_targets"].item()) == want["bad_targets"]


@pytest.mark.parametrize("npix", (5, 1001, 1024))
def test_map_kernels_null_outputs_and_guard_bands_stay_untouched(dev, npix):
    """refine and apply through the C entry points on a sentinel arena: with everything given only
    the given maps change; with ``out`` alone the counters keep their sentinel bytes."""
    from mdil_ss_amd import _pseudo_lib
    lib = _pseudo_lib.load()
    nc = 20
    run = device_run(nc, BIG)
    hl, hq, thr, ids, target = apply_case(run, nc, npix)
    dl, dq = run["dlabel"].reshape(-1), run["dqconf"].reshape(-1)
    sel = busiest_bytes(run, nc, skip=1)
    tables = dict(sel=torch.tensor(sel, dtype=torch.int32).to(dev), thr=torch.tensor(thr, dtype=torch.int32).to(dev),
                  ids=ids.to(dev), target=target.to(dev))
    stream = torch.cuda.current_stream().cuda_stream
    sentinel = torch.tensor([0xA5] * 8, dtype=torch.uint8).view(torch.int64)
    sizes = {"out": npix, "seen": nc * 8, "kept": nc * 8, "confusion": nc * nc * 8, "bad_targets": 8, "bad_labels": 8,
             "hist2": nc * 256 * 8, "bad_refine": 8}
    want = R.apply_rule(hl, hq, nc, thr, ids, 255, target, nc - 1)
    for given in (("out",), ("seen", "kept"), tuple(sizes)):
        arena = HC.Arena(dev, sizes)
        p = {k: (arena.ptr(k) if k in given else None) for k in sizes}
        with_target = "confusion" in given
        rc = lib.mdil_pseudo_apply(dl.data_ptr(), dq.data_ptr(), npix, nc, tables["thr"].data_ptr(),
                                   tables["ids"].data_ptr(), 255, tables["target"].data_ptr() if with_target else None,
                                   nc - 1, p["out"], p["seen"], p["kept"], p["confusion"], p["bad_targets"],
                                   p["bad_labels"], stream)
        assert rc == 0, lib.mdil_pseudo_last_error()
        if "hist2" in given:
            rc = lib.mdil_pseudo_refine(dl.data_ptr(), dq.data_ptr(), npix, nc, tables["sel"].data_ptr(), p["hist2"],
                                        p["bad_refine"], stream)
            assert rc == 0, lib.mdil_pseudo_last_error()
        torch.cuda.synchronize()
        arena.read()
        changed = [k for k in given if k == "out" or k in ("seen", "kept", "confusion", "hist2")]
        if with_target and want["bad_targets"]:
            changed.append("bad_targets")
        arena.assert_untouched(changed, given)
        if "out" in given:
            assert torch.equal(arena.cut("out"), want["out"])
        for k in ("seen", "kept", "confusion"):
            if k in given:
                assert torch.equal(arena.cut(k).view(torch.int64) - sentinel, want[k].reshape(-1)), k
        if "hist2" in given:
            assert torch.equal(arena.cut("hist2").view(torch.int64).reshape(nc, 256) - sentinel,
                               R.hist_level2(hl, hq, nc, sel)[0])


# ------------------------------------------------------------------------------------------ (7)
def test_head_grid_stride_loop_past_the_grid_bound(dev):
    """The grid is bounded at 256 work-groups of 1024 feature pixels; 1 x 513 x 513 = 263,169 of them
    is the smallest odd-sized square that sends pixels (1,025 of them, an odd remainder that fills one
    work-group and one lane of the next) round the loop a second time.  Two classes keep the fp64
    reference cheap."""
    nc, shape = 2, (1, 513, 513)
    assert HEAD_WG * HEAD_BLOCKS < shape[1] * shape[2] < 2 * HEAD_WG * HEAD_BLOCKS
    assert (shape[1] * shape[2] - HEAD_WG * HEAD_BLOCKS) % 2 == 1
    run = device_run(nc, shape)
    ref_label, q64, excluded = reference(nc, shape)
    check_head(nc, shape, 1.0, run)
    HC.check_labels(run["label"], ref_label, excluded, f"nc {nc} shape {shape}", HC.share(MAX_EXCLUDED))
    assert int((run["q"] - q64).abs()[~excluded].max()) <= 1


@functools.lru_cache(maxsize=None)
def big_maps(nc):
    """Random stored maps of 512 x 256 x 8 + 2,053 pixels: the map kernels' grid is bounded at 512
    work-groups of 256 items of 8 pixels, so 2,053 pixels (256 whole items and an odd tail of 5) go
    round the loop a second time."""
    n = MAP_WG * MAP_BLOCKS * PER_ITEM + 2053
    g = torch.Generator().manual_seed(nc)
    label = torch.randint(0, nc, (n,), generator=g, dtype=torch.uint8)
    q = torch.randint(0, 65536, (n,), generator=g)
    q[torch.rand(n, generator=g) < 0.25] = 65535
    return label, q


def test_refine_grid_stride_loop_past_the_grid_bound(dev):
    nc = 27
    label, q = big_maps(nc)
    assert label.numel() > MAP_WG * MAP_BLOCKS * PER_ITEM and (label.numel() - MAP_WG * MAP_BLOCKS * PER_ITEM) % 8 == 5
    sel = [255 if c % 2 else 17 + c for c in range(nc)]
    want, _ = R.hist_level2(label, q, nc, sel)
    hist2, bad = refine_on_device(dev, label.to(dev), q.to(torch.uint16).to(dev), nc, sel)
    assert torch.equal(hist2.cpu(), want) and int(bad.item()) == 0 and int(want.sum()) > 100000


def test_apply_grid_stride_loop_past_the_grid_bound(dev):
    from mdil_ss_amd import pseudo as P
    nc = 27
    label, q = big_maps(nc)
    thr = [(c * 2521) % 65537 for c in range(nc)]
    ids = HC.random_luts(nc)[0]
    target = HC.make_target(nc, (label.numel(),), nc - 1, seed=9)
    want = R.apply_rule(label, q, nc, thr, ids, 255, target, nc - 1)
    counters = P.new_apply_counters(nc, dev)
    out = P.pseudo_apply(label.to(dev), q.to(torch.uint16).to(dev), nc, thr, ids.to(dev), 255, target.to(dev), nc - 1,
                         counters)
    assert torch.equal(out.cpu(), want["out"])
    for k in ("seen", "kept", "confusion"):
        assert torch.equal(counters[k].cpu(), want[k]), k
    assert int(counters["bad_targets"].item()) == want["bad_targets"] > 0


# ------------------------------------------------------------------------------------------ (8)
def test_side_stream_gives_the_same_bytes(dev):
    from mdil_ss_amd import pseudo as P
    nc = 27
    run = device_run(nc, BIG)
    hl, hq, thr, ids, target = apply_case(run, nc, run["label"].numel())
    sel = busiest_bytes(run, nc, skip=None)
    tables = (ids.to(dev), target.to(dev).reshape(run["dlabel"].shape))

    def everything():
        hist = torch.zeros(nc, 256, dtype=torch.int64, device=dev)
        label, qconf = P.pseudo_head(*run["args"], hist, None)
        hist2, _ = refine_on_device(dev, label, qconf, nc, sel)
        counters = P.new_apply_counters(nc, dev)
        out = P.pseudo_apply(label, qconf, nc, thr, tables[0], 255, tables[1], nc - 1, counters)
        return [label, qconf, hist, hist2, out] + [counters[k] for k in P.APPLY_COUNTERS]

    first = everything()
    torch.cuda.synchronize()
    second = HC.side_stream(everything)
    for a, c in zip(first, second):
        assert torch.equal(HC.as_bytes(a.cpu()), HC.as_bytes(c.cpu()))
    assert torch.equal(first[0].cpu(), run["label"])


# ------------------------------------------------------------------------------------------ (9)
def test_labeller_in_two_batches_equals_one_call(dev):
    from mdil_ss_amd import pseudo as P
    nc = 20
    run = device_run(nc, BIG)
    xd, wd, bd = run["args"]
    meter = P.PseudoLabeller(nc)
    meter.add(xd[:1].contiguous(), wd, bd)
    meter.add(xd[1:].contiguous(), wd, bd)
    assert torch.equal(meter.hist(), run["hist"]) and meter.nonfinite() == 0 and meter.stored == 3 * run["q"].numel()
    portion = [0.1 + 0.04 * c for c in range(nc)]
    thr = meter.thresholds(portion, 0.2)
    assert thr == R.sort_thresholds(run["label"], run["q"], nc, portion, 0.2)[0]
    ids, _ = HC.random_luts(nc)
    target = HC.make_target(nc, tuple(run["label"].shape), nc - 1, seed=4)
    target[target >= nc] = nc - 1                                   # the meter refuses bad targets: see below
    want = R.apply_rule(run["label"], run["q"], nc, thr, ids, 255, target, nc - 1)
    outs = list(meter.apply(thr, ids, 255, [target[:1].to(dev), target[1:].to(dev)], nc - 1))
    assert [tuple(o.shape) for o in outs] == [(1, 32, 96), (2, 32, 96)]
    assert torch.equal(torch.cat([o.cpu() for o in outs]), want["out"])
    for k in ("seen", "kept", "confusion"):
        assert torch.equal(meter.counters[k], want[k]), k
    assert P.precision(meter.counters["confusion"]) == \
        (want["confusion"].diagonal().double() / want["confusion"].sum(0).clamp(min=1).double()).tolist()
    # without targets: the same maps, no confusion
    assert torch.equal(torch.cat([o.cpu() for o in meter.apply(thr, ids)]), want["out"])
    assert int(meter.counters["confusion"].sum()) == 0 and torch.equal(meter.counters["kept"], want["kept"])
    bad = HC.make_target(nc, tuple(run["label"].shape), nc - 1, seed=4)
    with pytest.raises(RuntimeError, match="target pixels are outside"):
        list(meter.apply(thr, ids, 255, [bad[:1].to(dev), bad[1:].to(dev)], nc - 1))
    with pytest.raises(RuntimeError, match="1 targets for 2 chunks"):
        list(meter.apply(thr, ids, 255, [target.to(dev)], nc - 1))


def test_labeller_refuses_to_outgrow_its_store(dev):
    from mdil_ss_amd import pseudo as P
    nc = 20
    xd, wd, bd = device_run(nc, BIG)["args"]
    one = 3 * 4 * 16 * 48                                           # bytes of one image's maps
    meter = P.PseudoLabeller(nc, store_gb=2.5 * one / 1e9)
    meter.add(xd[:2].contiguous(), wd, bd)
    with pytest.raises(RuntimeError, match="above store_gb"):
        meter.add(xd[2:].contiguous(), wd, bd)
    assert len(meter.chunks) == 1 and int(meter.hist().sum()) == 2 * 4 * 16 * 48    # the refusal stored nothing


# ----------------------------------------------------------------------------------------- (10)
@pytest.fixture(scope="module")
def tiny_model(dev):
    return HC.tiny_model(dev)


@pytest.fixture(scope="module")
def checkpoint(tiny_model, tmp_path_factory):
    path = tmp_path_factory.mktemp("pseudo") / "checkpoint.pth.tar"
    HC.save_checkpoint(tiny_model, path)
    return str(path)


def read_png(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == "L", (path, im.mode)
        return torch.from_numpy(np.array(im))


def expected_maps(model, images, task, nc, portion, batch):
    """What the command line must write for ``images`` fed in batches of ``batch``: apply()'s maps
    with the last class and the dropped pixels as 255."""
    from mdil_ss_amd import pseudo as P
    meter = P.PseudoLabeller(nc)
    for i in range(0, images.shape[0], batch):
        meter.add(model, images[i:i + batch], task)
    thr = meter.thresholds(portion)
    ids = torch.arange(nc, dtype=torch.uint8)
    ids[nc - 1] = 255
    maps = torch.cat([o.cpu() for o in meter.apply(thr, ids, 255)])
    return maps, thr, meter.counters


def test_cli_synthetic_end_to_end(dev, tiny_model, checkpoint, tmp_path):
    from mdil_ss_amd import pseudo as P
    from mdil_ss_amd.dataset import ProceduralSeg
    out, report_file = tmp_path / "maps", tmp_path / "report.json"
    report = P.main(P.build_parser().parse_args(
        ["--state", checkpoint, "--num-classes", "20", "20", "--task", "1", "--synthetic", "5", "--height", "64",
         "--width", "128", "--batch-size", "3", "--portion", "0.3", "--out", str(out), "--json", str(report_file)]))
    files = sorted(glob.glob(str(out / "*.png")))
    assert len(files) == 5 and sorted(report["written"]) == files
    ds = ProceduralSeg(5, 64, 128, 20, seed=13, domain=1)
    images = torch.stack([ds[i][0] for i in range(5)]).to(dev)
    maps, thr, counters = expected_maps(tiny_model, images, 1, 20, 0.3, 3)
    for i in range(5):
        got = read_png(out / f"synthetic_{i:04d}_pseudo.png")
        assert tuple(got.shape) == (64, 128) and torch.equal(got, maps[i])
    with open(report_file) as f:
        saved = json.load(f)
    assert saved["seen"] == counters["seen"].tolist() and saved["kept"] == counters["kept"].tolist()
    assert saved["thr"] == thr and sum(saved["seen"]) == 5 * 64 * 128 and saved["nonfinite"] == 0
    assert saved["thr_probability"] == [t / 65536 for t in thr] and len(saved["k"]) == 20
    assert saved["kept_share"] == sum(saved["kept"]) / sum(saved["seen"])
    # labelled: the kept pixels' confusion next to every pixel's
    all_pixels = torch.tensor(saved["confusion_all"])
    target = torch.stack([ds[i][1][0] for i in range(5)])
    counted = int((target != 19).sum())
    assert int(all_pixels.sum()) == counted and int(torch.tensor(saved["confusion_kept"]).sum()) <= counted
    assert len(saved["precision_kept"]) == len(saved["precision_all"]) == 20


def _write_images(folder, names, seed):
    from PIL import Image
    g = np.random.default_rng(seed)
    paths = []
    for n in names:
        path = os.path.join(folder, n)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        Image.fromarray(g.integers(0, 256, (40, 72, 3), dtype=np.uint8)).save(path)
        paths.append(path)
    return paths


def _expected_for_files(dev, tiny_model, paths, portion):
    from mdil_ss_amd import _head_common as hc
    from mdil_ss_amd import predict as PR
    images = hc.image_batch([PR._load_resized(p, 64, 128) for p in paths], dev)
    return expected_maps(tiny_model, images, 1, 20, portion, 3)[0]


def test_cli_writes_a_bdd_tree_the_loader_opens(dev, tiny_model, checkpoint, tmp_path):
    from mdil_ss_amd import dataset as D
    from mdil_ss_amd import pseudo as P
    pics = tmp_path / "unlabelled" / "images" / "train"
    names = [f"{s}.png" for s in ("b1c66a42", "0a0a0b1a", "7d2f7975", "3f4e5d6c", "fe1f55fa")]
    paths = _write_images(str(pics), names, seed=1)
    root = tmp_path / "bdd"
    P.main(P.build_parser().parse_args(
        ["--state", checkpoint, "--num-classes", "20", "20", "--task", "1", "--images", str(pics), "--height", "64",
         "--width", "128", "--batch-size", "3", "--out-root", str(root), "--layout", "BDD", "--subset", "train"]))
    ds = D.BDD100k(str(root), subset="train")
    assert len(ds) == 5 and len(ds.filenamesGt) == 5
    maps = _expected_for_files(dev, tiny_model, sorted(paths), 0.2)
    for i, (img, lab) in enumerate(zip(ds.filenames, ds.filenamesGt)):
        stem = os.path.splitext(os.path.basename(img))[0]
        assert os.path.basename(lab) == f"{stem}_train_id.png"
        assert os.path.realpath(img) == os.path.realpath(sorted(paths)[i])
        assert torch.equal(read_png(lab), maps[i])
        image, label = ds[i]
        assert image.size == (72, 40) and np.array_equal(np.array(label), maps[i].numpy())
    assert (maps == 255).any() and (maps != 255).any() and not (maps == 19).any()


def test_cli_writes_a_cityscapes_tree_the_loader_opens(dev, tiny_model, checkpoint, tmp_path):
    from mdil_ss_amd import dataset as D
    from mdil_ss_amd import pseudo as P
    pics = tmp_path / "frames"
    names = ["aachen/aachen_000000_000019_leftImg8bit.png", "aachen/aachen_000001_000019_leftImg8bit.png",
             "bochum/bochum_000000_000313_leftImg8bit.png", "ulm_000000_000019_leftImg8bit.png",
             "ulm_000001_000019_leftImg8bit.png"]
    paths = _write_images(str(pics), names, seed=2)
    root = tmp_path / "cs"
    P.main(P.build_parser().parse_args(
        ["--state", checkpoint, "--num-classes", "20", "20", "--task", "1", "--images", str(pics), "--height", "64",
         "--width", "128", "--batch-size", "3", "--out-root", str(root), "--layout", "cityscapes", "--subset", "train",
         "--keep-void", "--portion", "0.5"]))
    ds = D.cityscapes(str(root), subset="train")
    assert len(ds) == 5 and len(ds.filenamesGt) == 5
    order = sorted(paths)
    images_sorted = [os.path.realpath(f) for f in ds.filenames]
    assert images_sorted == [os.path.realpath(p) for p in order]
    from mdil_ss_amd import _head_common as hc
    from mdil_ss_amd import predict as PR
    meter = P.PseudoLabeller(20)
    batch = hc.image_batch([PR._load_resized(p, 64, 128) for p in order], dev)
    for i in (0, 3):
        meter.add(tiny_model, batch[i:i + 3], 1)
    maps = torch.cat([o.cpu() for o in meter.apply(meter.thresholds(0.5), None, 255)])
    for i, (img, lab) in enumerate(zip(ds.filenames, ds.filenamesGt)):
        stem = os.path.basename(img)[:-len("_leftImg8bit.png")]
        assert os.path.basename(lab) == f"{stem}_gtFine_labelTrainIds.png"
        assert os.path.relpath(os.path.dirname(lab), ds.labels_root) == os.path.relpath(os.path.dirname(img), ds.images_root)
        assert torch.equal(read_png(lab), maps[i])
