"""GPU: the sliding-region acquisition add-on (include/mdil_ripu.h) against tests/ripu_reference.py.  Every
comparison is exact (``torch.equal``): the library computes in integers.

  (1) ripu_score   every criterion, with and without ``taken``, over the shapes, radii and widths below, on noise,
                   one label, balanced labels at q = 65535, labels >= nc and acquire_head's own maps
  (2) ripu_select  the same shapes, r in {0, 1, 3, 32}: budgets that stop midway, max_picks, overlapping regions,
                   a constant and an all-zero key map, the rows of ``picks`` past the count
  (3) ripu_apply   widths {1, 3, 5, 1001, 1024}, every counter
  (4) all three    NULL outputs and guard bands, refusals, a side stream, counters added twice
  (5) the command line on --synthetic 4"""
import functools
import glob
import json
import os

import pytest
import torch

from tests import annotate_cases as AC
from tests import head_cases as HC
from tests import ripu_reference as R
from tests.annotate_cases import IGNORE, N_IMAGES, SENTINEL, SIZE, check_counters, checkpoint, read_tree, synthetic_targets

pytestmark = pytest.mark.gpu

# ripu.hip: a job of ripu_score is 32 output rows (kScoreRows) of a strip of 256 - 2k columns: 254 (k = 1), 250 (k = 3),
# 192 (k = 32).  EDGES crosses the row segment at 32 and two strip borders of every radius (192 and 384; 250 and 500;
# 254 and 508), with a last strip of a few columns.
EDGES = (1, 40, 520)
SHAPES = ((1, 1, 1), (2, 9, 7), (1, 5, 300), (2, 70, 134), EDGES)
RADII = (1, 3, 32)
WIDTHS = (2, 20, 32)
# ripu_select: chunks of 64 pixels up to 4096 of them, 128 beyond: the first size with chunks of 128
WIDE = (1, 513, 512)


@pytest.fixture(scope="module")
def dev():
    return HC.device("ripu")


def stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def maps(shape, nc, family="noise"):
    """(label u8, q int64, target u8, taken u8) on the host; never modified."""
    g = torch.Generator().manual_seed(shape[1] * 1000 + shape[2] + nc)
    N, H, W = shape
    if family == "noise":
        label = torch.randint(0, nc, shape, generator=g, dtype=torch.uint8)
        q = torch.randint(0, 65536, shape, generator=g)
    elif family == "blobs":                                        # large regions: many pure windows, ties and zero keys
        yy, xx = torch.arange(H)[:, None], torch.arange(W)[None]
        label = (((yy // 7) + (xx // 11)) % nc).to(torch.uint8).expand(shape).contiguous()
        q = torch.randint(0, 4, shape, generator=g) * 20000
    elif family == "one":
        label = torch.full(shape, nc - 1, dtype=torch.uint8)
        q = torch.randint(0, 65536, shape, generator=g)
    elif family == "balanced":                                     # the largest products
        yy, xx = torch.arange(H)[:, None], torch.arange(W)[None]
        label = ((yy * 5 + xx * 3) % nc).to(torch.uint8).expand(shape).contiguous()
        q = torch.full(shape, 65535)
    else:                                                          # "beyond": labels >= nc present
        label = torch.randint(0, nc + 3, shape, generator=g, dtype=torch.uint8)
        label[torch.rand(shape, generator=g) < 0.05] = 255
        q = torch.randint(0, 65536, shape, generator=g)
    target = HC.make_target(nc, shape, IGNORE, seed=nc + H)
    taken = (torch.rand(shape, generator=g) < 0.15).to(torch.uint8) * torch.randint(1, 256, shape, generator=g, dtype=torch.uint8)
    return label, q, target, taken


def to_q(q, dev):
    """A q map (int64 on the host) as the library reads it: uint16 on the device."""
    return torch.from_numpy(q.numpy().astype("uint16")).to(dev)


def to_key(key, dev):
    return torch.from_numpy(key.numpy().astype("uint32")).to(dev)


def score_all(dev, shape, k, nc, family):
    """Every criterion with and without ``taken`` against the reference."""
    from mdil_ss_amd import ripu as P
    label, q, target, taken = maps(shape, nc, family)
    dl, dq, dt, dk = label.to(dev), to_q(q, dev), target.to(dev), taken.to(dev)
    for by in R.CRITERIA:
        for tk, dtk in ((None, None), (taken, dk)):
            got = P.ripu_score(dl, k, nc, by, dq, dt, IGNORE, dtk, seed=11, image0=5)
            want = R.keys_fast(label, k, nc, by, q, target, IGNORE, tk, seed=11, image0=5)
            assert got.dtype == torch.uint32 and torch.equal(P.key_values(got.cpu()), want), (shape, k, nc, family, by, tk is None)
    assert torch.equal(dk.cpu(), taken) and torch.equal(dl.cpu(), label)


# ---------------------------------------------------------------------------------- (1) score
@pytest.mark.parametrize("k", RADII)
@pytest.mark.parametrize("shape", SHAPES)
def test_score_on_noise(dev, shape, k):
    """k = 32 on 9 x 7 and on 1 x 1 is the window larger than the image."""
    for nc in WIDTHS:
        score_all(dev, shape, k, nc, "noise")


@pytest.mark.parametrize("family", ("blobs", "one", "balanced", "beyond"))
@pytest.mark.parametrize("shape, k, nc", (((2, 9, 7), 1, 2), ((2, 9, 7), 32, 20), ((1, 5, 300), 3, 32), ((2, 70, 134), 32, 32),
                                          ((2, 70, 134), 3, 20), (EDGES, 32, 20), (EDGES, 1, 32)))
def test_score_input_families(dev, shape, k, nc, family):
    score_all(dev, shape, k, nc, family)
    if family == "one":
        from mdil_ss_amd import ripu as P
        label, q, _, _ = maps(shape, nc, family)
        for by in ("impurity", "ripu"):
            assert int(P.key_values(P.ripu_score(label.to(dev), k, nc, by, to_q(q, dev))).sum()) == 0


def test_score_reference_forms_agree_on_a_device_case(dev):
    """The per-pixel Python-integer form of the reference on one small case, beside the tensor form used above."""
    from mdil_ss_amd import ripu as P
    label, q, target, taken = maps((2, 9, 7), 20, "noise")
    for by in R.CRITERIA:
        got = P.ripu_score(label.to(dev), 3, 20, by, to_q(q, dev), target.to(dev), IGNORE, taken.to(dev), seed=2 ** 63 + 5)
        assert torch.equal(P.key_values(got.cpu()), R.keys(label, 3, 20, by, q, target, IGNORE, taken, seed=2 ** 63 + 5)), by


@functools.lru_cache(maxsize=None)
def head_maps():
    """acquire_head's own label and q maps of the tiny model on 2 procedural images of 64 x 128."""
    from mdil_ss_amd import acquire as A
    from mdil_ss_amd.dataset import ProceduralSeg
    dev = torch.device("cuda", 0)
    model = HC.tiny_model(dev)
    ds = ProceduralSeg(2, 64, 128, 20, seed=13, domain=1)
    images = torch.stack([ds[i][0] for i in range(2)]).to(dev)
    target = torch.stack([ds[i][1][0] for i in range(2)]).to(torch.uint8)
    with torch.no_grad():
        feat = model.features(images, 1).contiguous()
    w, b = (t.detach() for t in model.head_params(1))
    label, qmap = A.acquire_head(feat, w, b, (2, 2), "entropy", want_label=True, want_qmap=True)
    torch.cuda.synchronize()
    return label, qmap, label.cpu(), A.q_values(qmap.cpu()), target


@pytest.mark.parametrize("k", RADII)
def test_score_on_acquire_heads_own_maps(dev, k):
    from mdil_ss_amd import ripu as P
    dl, dq, label, q, target = head_maps()
    assert tuple(label.shape) == (2, 64, 128) and int(q.max()) > 0
    for by in R.CRITERIA:
        got = P.ripu_score(dl, k, 20, by, dq, target.to(dev), 19)
        assert torch.equal(P.key_values(got.cpu()), R.keys_fast(label, k, 20, by, q, target, 19)), by


# --------------------------------------------------------------------------------- (2) select
FILL = 0x5A5A5A5A5A5A5A5A


def check_select(dev, key, taken, r, budget, P_max):
    """key int64 [N,H,W] and taken u8 on the host -> the device's picks against the reference's; -> counts."""
    from mdil_ss_amd import ripu as P
    N = key.shape[0]
    dkey = to_key(key, dev)
    dtaken = taken.to(dev)
    picks = torch.full((N, P_max, 4), FILL, dtype=torch.int64, device=dev)
    got = P.ripu_select(dkey, dtaken, r, budget, P_max, picks)
    torch.cuda.synchronize()
    after, want, shown, stop = R.select(key, taken, r, budget, P_max)
    what = (tuple(key.shape), r, budget, P_max)
    assert got["count"].tolist() == [len(p) for p in want], what
    assert got["shown"].tolist() == shown and got["stop"].tolist() == stop, what
    host = picks.cpu()
    for n in range(N):
        assert host[n, :len(want[n])].tolist() == [list(p) for p in want[n]], what
        assert bool((host[n, len(want[n]):] == FILL).all()), what              # rows past the count keep their fill
    assert torch.equal(dtaken.cpu(), after), what
    assert torch.equal(dkey.cpu().view(torch.int32), to_key(key, "cpu").view(torch.int32))
    return got["count"].tolist(), stop


@functools.lru_cache(maxsize=None)
def select_keys(shape):
    """Real keys with many ties and zeros (ripu on blobs) and hashed keys; a taken map with marks."""
    label, q, target, taken = maps(shape, 20, "blobs")
    return R.keys_fast(label, 3, 20, "ripu", q), R.keys(label, 1, 20, "random", seed=3), taken


@pytest.mark.parametrize("r", (0, 1, 3, 32))
@pytest.mark.parametrize("shape", SHAPES)
def test_select_matches_the_greedy_loop(dev, shape, r):
    tied, hashed, taken = select_keys(shape)
    HW = shape[1] * shape[2]
    free = torch.zeros(shape, dtype=torch.uint8)
    area = min(HW, (2 * r + 1) ** 2)
    stops = set()
    # budgets that stop midway (a few regions, with overlaps: fresh < the region), one that max_picks cuts, one no pick fits
    for key, tk, budget, P_max in ((tied, taken, 3 * area + 2, 64), (hashed, free, max(1, HW // 3), 64), (hashed, taken, HW, 5),
                                   (tied, free, 0, 4), (hashed, taken, 2 * area, 1)):
        _, stop = check_select(dev, key, tk, r, min(budget, 40 if r == 0 else budget), P_max)
        stops.update(stop)
    if HW > 1:
        assert R.STOP_BUDGET in stops


def test_select_overlap_budget_and_pick_limits(dev):
    tied, hashed, taken = select_keys((2, 70, 134))
    count, stop = check_select(dev, hashed, torch.zeros_like(taken), 3, 2000, 4096)
    assert all(c > 40 for c in count) and stop == [R.STOP_BUDGET] * 2          # overlapping 7 x 7 regions: fresh < 49 somewhere
    count, stop = check_select(dev, hashed, taken, 3, 70 * 134, 20)
    assert count == [20, 20] and stop == [R.STOP_PICKS] * 2                    # max_picks reached
    count, stop = check_select(dev, tied, taken, 32, 70 * 134, 4096)           # everything with a key goes: stops on a zero key
    assert stop == [R.STOP_EMPTY] * 2
    count, stop = check_select(dev, hashed, torch.zeros_like(taken), 0, 300, 65536)   # pixel mode, the largest pick table
    assert count == [300, 300]


@pytest.mark.parametrize("shape", ((2, 9, 7), EDGES))
def test_select_constant_and_zero_key_maps(dev, shape):
    _, _, taken = select_keys(shape)
    const = torch.full(shape, 77, dtype=torch.int64)
    n_free = int((taken[0] == 0).sum())
    count, _ = check_select(dev, const, taken, 0, shape[1] * shape[2], min(n_free, 50))   # raster order, taken pixels skipped
    from mdil_ss_amd import ripu as P
    picks = torch.zeros(shape[0], 50, 4, dtype=torch.int64, device=dev)
    dt = taken.to(dev)
    P.ripu_select(to_key(const, dev), dt, 0, 10 ** 6, 50, picks)
    first = [(int(i) // shape[2], int(i) % shape[2]) for i in (taken[0].reshape(-1) == 0).nonzero().reshape(-1)[:50]]
    got = picks.cpu()[0, :len(first), :2].tolist()
    assert got == [list(p) for p in first]
    zero = torch.zeros(shape, dtype=torch.int64)
    count, stop = check_select(dev, zero, taken, 3, 10 ** 6, 16)               # count 0, taken untouched (checked inside)
    assert count == [0] * shape[0] and stop == [R.STOP_EMPTY] * shape[0]
    count, stop = check_select(dev, const, torch.full(shape, 9, dtype=torch.uint8), 3, 10 ** 6, 16)
    assert count == [0] * shape[0]


def test_select_with_chunks_of_128_pixels(dev):
    """WIDE: the first image size whose chunks hold 128 pixels; regions that straddle chunk and row borders."""
    g = torch.Generator().manual_seed(4)
    key = torch.randint(0, 2 ** 32, WIDE, generator=g)
    key[0, :40, :60] = 2 ** 32 - 1                                             # a tied block: raster order across chunks
    taken = torch.zeros(WIDE, dtype=torch.uint8)
    taken[0, 3, 5] = 128
    check_select(dev, key, taken, 32, 40 * 60 + 65 * 65 * 6, 64)
    check_select(dev, key, taken, 0, 70, 4096)


# ---------------------------------------------------------------------------------- (3) apply
@pytest.mark.parametrize("Wl", AC.APPLY_WIDTHS)
@pytest.mark.parametrize("Hl", AC.APPLY_HEIGHTS)
def test_apply_maps_and_counters(dev, Hl, Wl):
    from mdil_ss_amd import ripu as P
    nc, N = AC.APPLY_NC, AC.APPLY_N
    sel, target, previous, fill, label = AC.apply_maps(N, Hl, Wl, nc, AC.apply_seed(Hl, Wl))
    ds, dt, dp, df, dl = (t.to(dev) for t in (sel, target, previous, fill, label))
    want = R.apply_ref(sel, nc, target, previous, fill, label, IGNORE, 250)
    counters = P.new_apply_counters(nc, dev)
    for times in (1, 2):                                                       # the counters are ADDED to
        out, mask = P.ripu_apply(ds, nc, dt, dp, df, dl, IGNORE, 250, counters, want_out=True, want_mask=True)
        assert torch.equal(out.cpu(), want["out"]) and torch.equal(mask.cpu(), want["mask"])
        check_counters(counters, want, times)
    assert want["shown"] > 0 or Wl * Hl < 4
    # fewer inputs: no previous; no target (drop_id in the chosen pixels); nothing but the mask
    for kw in (dict(target=dt, fill=df), dict(previous=dp), dict()):
        ref = R.apply_ref(sel, nc, target if "target" in kw else None, previous if "previous" in kw else None,
                          fill if "fill" in kw else None, None, IGNORE, 250)
        names = ("shown", "kept", "filled") + (("annotated", "bad_targets") if "target" in kw else ())
        c = P.new_apply_counters(nc, dev, names)
        out, mask = P.ripu_apply(ds, nc, ignore_index=IGNORE, drop_id=250, counters=c, want_mask=True, **kw)
        assert torch.equal(out.cpu(), ref["out"]) and torch.equal(mask.cpu(), ref["mask"])
        check_counters(c, ref, 1)


# ----------------------------------------------------------- (4) NULL outputs, guard bands, refusals
def test_score_and_select_guard_bands_refusals_and_side_stream(dev):
    from mdil_ss_amd import _ripu_lib
    from mdil_ss_amd import ripu as P
    lib = _ripu_lib.load()
    shape, nc, k, r, P_max = (2, 70, 134), 20, 3, 3, 32
    N, Hl, Wl = shape
    npix = N * Hl * Wl
    label, q, target, taken = maps(shape, nc, "noise")
    dl, dq, dt, dk = label.to(dev), to_q(q, dev), target.to(dev), taken.to(dev)
    tlog = P.tlog_table(k).to(dev)
    want = R.keys_fast(label, k, nc, "ripu", q, taken=taken)
    arena = HC.Arena(dev, {"key": npix * 4})

    def score(key, **kw):
        a = dict(nc=nc, k=k, by=2, qmap=dq.data_ptr(), tlog=tlog.data_ptr())
        a.update(kw)
        return lib.mdil_ripu_score(dl.data_ptr(), a["qmap"], dt.data_ptr(), IGNORE, dk.data_ptr(), a["tlog"], N, Hl, Wl, a["nc"],
                                   a["k"], a["by"], 0, 0, key, stream())

    for kw, text in ((dict(nc=33), b"nc=33"), (dict(k=0), b"k=0"), (dict(k=33), b"k=33"), (dict(by=5), b"by=5"),
                     (dict(qmap=None), b"needs a qmap"), (dict(tlog=None), b"needs the tlog")):
        assert score(arena.ptr("key"), **kw) == -1 and text in lib.mdil_ripu_last_error(), text
    assert score(arena.ptr("key") + 4) == -1 and score(None) == -1
    torch.cuda.synchronize()
    arena.read()
    arena.assert_untouched([])                                                # refusals leave everything untouched
    assert score(arena.ptr("key")) == 0, lib.mdil_ripu_last_error()
    torch.cuda.synchronize()
    arena.read()
    arena.assert_untouched(["key"])
    assert torch.equal(arena.cut("key").view(torch.int32).to(torch.int64) & 0xffffffff, want.reshape(-1))
    side = HC.side_stream(lambda: P.ripu_score(dl, k, nc, "ripu", dq, taken=dk))
    assert torch.equal(P.key_values(side.cpu()), want)

    # select: each output may be NULL; the guard bands and what was not given stay untouched
    dkey = to_key(want, dev)
    after, picks, shown, stop = R.select(want, taken, r, 500, P_max)
    sizes = {"picks": N * P_max * 32, "count": N * 8, "shown": N * 8, "stop": N * 8}

    def select(p, tk, **kw):
        a = dict(r=r, P=P_max, budget=500)
        a.update(kw)
        return lib.mdil_ripu_select(dkey.data_ptr(), tk, N, Hl, Wl, a["r"], a["budget"], a["P"], p["picks"], p["count"],
                                    p["shown"], p["stop"], stream())

    for given in [(k_,) for k_ in sizes] + [(), tuple(sizes)]:
        arena = HC.Arena(dev, sizes)
        p = {k_: (arena.ptr(k_) if k_ in given else None) for k_ in sizes}
        tk = taken.to(dev)
        assert select(p, tk.data_ptr()) == 0, lib.mdil_ripu_last_error()
        torch.cuda.synchronize()
        arena.read()
        assert torch.equal(tk.cpu(), after), given
        if "count" in given:
            assert arena.cut("count").view(torch.int64).tolist() == [len(v) for v in picks]
        if "shown" in given:
            assert arena.cut("shown").view(torch.int64).tolist() == shown
        if "stop" in given:
            assert arena.cut("stop").view(torch.int64).tolist() == stop
        if "picks" in given:
            rows = arena.cut("picks").view(torch.int64).reshape(N, P_max, 4)
            for n in range(N):
                assert rows[n, :len(picks[n])].tolist() == [list(v) for v in picks[n]]
                assert bool((rows[n, len(picks[n]):] == SENTINEL).all())
        arena.assert_untouched([k_ for k_ in given])
    arena = HC.Arena(dev, sizes)
    every = {k_: arena.ptr(k_) for k_ in sizes}
    tk = taken.to(dev)
    for kw, text in ((dict(r=-1), b"r=-1"), (dict(r=33), b"r=33"), (dict(P=0), b"max_picks=0"), (dict(budget=-5), b"budget_pixels")):
        assert select(every, tk.data_ptr(), **kw) == -1 and text in lib.mdil_ripu_last_error(), text
    assert select(dict(every, picks=every["picks"] + 4), tk.data_ptr()) == -1 and select(every, None) == -1
    torch.cuda.synchronize()
    arena.read()
    arena.assert_untouched([])
    assert torch.equal(tk.cpu(), taken)

    def on_side():
        t2 = taken.to(dev)
        return t2, P.ripu_select(dkey, t2, r, 500, P_max)
    t2, got = HC.side_stream(on_side)
    assert torch.equal(t2.cpu(), after) and got["shown"].tolist() == shown and got["count"].tolist() == [len(v) for v in picks]


@pytest.mark.parametrize("Wl", (5, 1001, 1024))
def test_apply_null_outputs_refusals_and_guard_bands(dev, Wl):
    from mdil_ss_amd import _ripu_lib
    from mdil_ss_amd import ripu as P
    lib = _ripu_lib.load()
    nc, N, Hl = 20, 2, 5
    sel, target, previous, fill, label = AC.apply_maps(N, Hl, Wl, nc, AC.apply_seed(Hl, Wl))
    want = R.apply_ref(sel, nc, target, previous, fill, label, IGNORE, 250)
    ds, dt, dp, df, dl = (t.to(dev) for t in (sel, target, previous, fill, label))
    npix = N * Hl * Wl
    sizes = {"out": npix, "mask": npix, "shown": 8, "annotated": nc * 8, "kept": nc * 8, "filled": nc * 8, "bad_targets": 8,
             "wrong_shown": 8, "wrong_all": 8}

    def call(p, nc_arg=nc, drop=250, tgt=True, lab=True):
        return lib.mdil_ripu_apply(ds.data_ptr(), dt.data_ptr() if tgt else None, dp.data_ptr(), df.data_ptr(),
                                   dl.data_ptr() if lab else None, N, Hl, Wl, nc_arg, IGNORE, drop, p["out"], p["mask"],
                                   p["shown"], p["annotated"], p["kept"], p["filled"], p["bad_targets"], p["wrong_shown"],
                                   p["wrong_all"], stream())

    combos = [(k,) for k in sizes] + [("out", "mask"), tuple(k for k in sizes if k not in ("out", "mask")), tuple(sizes)]
    for given in combos:
        arena = HC.Arena(dev, sizes)
        p = {k: (arena.ptr(k) if k in given else None) for k in sizes}
        assert call(p) == 0, lib.mdil_ripu_last_error()
        torch.cuda.synchronize()
        arena.read()
        AC.check_arena(arena, given, want, ("shown", "bad_targets", "wrong_shown", "wrong_all"))
    assert want["wrong_shown"] > 0 and want["wrong_all"] > want["wrong_shown"]
    assert want["bad_targets"] > 0 or npix < 100                              # 50 pixels hold no chosen target out of range
    arena = HC.Arena(dev, sizes)
    every = {k: arena.ptr(k) for k in sizes}
    for p, kw, text in ((dict.fromkeys(sizes), {}, b"nothing to write"), (every, dict(nc_arg=33), b"nc=33"),
                        (every, dict(drop=256), b"drop_id=256"), (every, dict(tgt=False), b"need a target"),
                        (every, dict(lab=False), b"need a target and a label"),
                        (dict(every, out=every["out"] + 4), {}, b"alignment")):
        assert call(p, **kw) == -1 and text in lib.mdil_ripu_last_error(), text
    torch.cuda.synchronize()
    arena.read()
    arena.assert_untouched([])
    side = HC.side_stream(lambda: P.ripu_apply(ds, nc, dt, dp, df, dl, IGNORE, 250, want_mask=True))
    assert torch.equal(side[0].cpu(), want["out"]) and torch.equal(side[1].cpu(), want["mask"])


# ----------------------------------------------------------------------------- (5) end to end
RADIUS = 4
CLI = AC.CLI_BASE + ["--subset", "val", "--radius", str(RADIUS)]
REPORT_KEYS = ("dataset", "kind", "by", "radius", "select_radius", "budget", "budget_is", "budget_pixels_per_image", "images",
               "total_pixels", "shown", "shown_share", "picks", "picks_per_image_mean", "picks_per_image_max", "stops",
               "nonfinite", "criteria", "error_recall", "error_recall_chosen", "wrong_pixels", "annotated", "annotated_pixels",
               "given", "annotated_share_per_class", "kept", "filled", "written")


run_cli = functools.partial(AC.run_cli, "ripu", CLI)


def selected_mask(selection):
    """The union of the picked regions, and the sum of their fresh pixels."""
    r = selection["select_radius"]
    mask, fresh = torch.zeros((N_IMAGES,) + SIZE, dtype=torch.bool), 0
    for stem, picks in selection["picks"].items():
        for y, x, _, f in picks:
            mask[int(stem[-4:]), max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] = True
            fresh += f
    return mask, fresh


@pytest.mark.parametrize("layout, by, select_radius", (("BDD", "ripu", None), ("cityscapes", "oracle", 0)))
def test_cli_report_selection_and_label_tree(dev, checkpoint, tmp_path, layout, by, select_radius):
    import numpy as np
    from PIL import Image
    budget = 0.1 if select_radius is None else 0.005
    report_file, root, out = tmp_path / "report.json", tmp_path / "round1", tmp_path / "maps"
    extra = ["--budget", budget, "--by", by, "--json", report_file, "--out-root", root, "--layout", layout, "--out", out]
    run_cli(checkpoint, extra + ([] if select_radius is None else ["--select-radius", select_radius]))
    with open(report_file) as f:
        saved = json.load(f)
    assert all(k in saved for k in REPORT_KEYS), [k for k in REPORT_KEYS if k not in saved]
    per_image = int(budget * SIZE[0] * SIZE[1])
    r = RADIUS if select_radius is None else select_radius
    assert saved["total_pixels"] == N_IMAGES * SIZE[0] * SIZE[1] and saved["nonfinite"] == 0 and "per image" in saved["budget_is"]
    assert (saved["radius"], saved["select_radius"], saved["budget_pixels_per_image"]) == (RADIUS, r, per_image)
    assert 0 < saved["shown"] <= N_IMAGES * per_image and sum(saved["stops"].values()) == N_IMAGES
    assert set(saved["criteria"]) == set(saved["error_recall"]) == set(R.CRITERIA)
    assert saved["error_recall_chosen"] == saved["error_recall"][by] == saved["criteria"][by]["error_recall"]
    for v in saved["criteria"].values():
        assert 0 <= v["shown"] <= N_IMAGES * per_image and sum(v["stops"].values()) == N_IMAGES
        assert v["error_recall"] == (v["wrong_shown"] / saved["wrong_pixels"] if saved["wrong_pixels"] else 0.0)
    with open(root / "selection.json") as f:
        selection = json.load(f)
    with open(out / "selection.json") as f:
        assert json.load(f) == selection
    chosen, fresh = selected_mask(selection)
    assert int(chosen.sum()) == fresh == saved["shown"] and sum(len(v) for v in selection["picks"].values()) == saved["picks"]
    for picks in selection["picks"].values():                                  # greedy: the keys never rise within an image
        keys = [p[2] for p in picks]
        assert keys == sorted(keys, reverse=True)
    target = synthetic_targets()
    want = torch.where(chosen & (target != 19), target, torch.tensor(255, dtype=torch.uint8))
    assert torch.equal(read_tree(root, layout), want)                          # opened by the trainers' dataset class
    assert saved["annotated"] == torch.bincount(target[chosen & (target != 19)].long(), minlength=20).tolist()
    assert saved["given"] == torch.bincount(target[target != 19].long(), minlength=20).tolist()
    assert len(glob.glob(str(out / "*_select.png"))) == len(glob.glob(str(out / "*_score.png"))) == N_IMAGES
    for i in range(N_IMAGES):
        with Image.open(out / f"synthetic_{i:04d}_select.png") as im:
            assert torch.equal(torch.from_numpy(np.array(im)) == 255, chosen[i])
        with Image.open(out / f"synthetic_{i:04d}_score.png") as im:
            assert np.array(im).shape == SIZE
    if by == "oracle":                                                         # pixel mode on the oracle of an untrained head
        assert saved["criteria"]["oracle"]["wrong_shown"] > 0


def test_cli_same_seed_same_bytes_and_previous_rounds(dev, checkpoint, tmp_path):
    budget = 0.1
    roots = [tmp_path / n for n in ("a", "b", "round2")]
    for root in roots[:2]:
        run_cli(checkpoint, ["--budget", budget, "--by", "random", "--seed", 3, "--out-root", root, "--layout", "BDD",
                             "--json", root / "report.json"])
    AC.assert_same_files(roots[0], roots[1], 2 * N_IMAGES + 2)
    with open(roots[0] / "selection.json") as f:
        first = json.load(f)
    other = run_cli(checkpoint, ["--budget", budget, "--by", "random", "--seed", 4, "--json", tmp_path / "other.json"])
    with_seed_4 = other["picks"]
    assert with_seed_4 > 0 and other["criteria"]["random"]["shown"] == other["shown"]
    # round 2: the regions of round 1 are not picked or shown again, its labels are kept
    rep = run_cli(checkpoint, ["--budget", budget, "--by", "uncertainty", "--previous", roots[0] / "selection.json",
                               "--previous-root", roots[0], "--out-root", roots[2], "--layout", "BDD", "--json",
                               tmp_path / "r2.json"])
    with open(roots[2] / "selection.json") as f:
        second = json.load(f)
    (one, _), (two, fresh) = selected_mask(first), selected_mask(second)
    new = two & ~one
    assert int(new.sum()) == fresh == rep["shown"] > 0
    for stem, picks in second["picks"].items():
        for y, x, _, _ in picks:
            assert not bool(one[int(stem[-4:]), y, x])                        # no centre inside round 1's regions
    target = synthetic_targets()
    want = torch.where((one | two) & (target != 19), target, torch.tensor(255, dtype=torch.uint8))
    assert torch.equal(read_tree(roots[2], "BDD"), want)
    assert sum(rep["kept"]) == int((one & (target != 19)).sum())
    # with round 1's tree as fill instead: the same tree, counted as filled
    rep3 = run_cli(checkpoint, ["--budget", budget, "--by", "uncertainty", "--previous", roots[0] / "selection.json",
                                "--fill-root", roots[0], "--out-root", tmp_path / "round3", "--layout", "BDD"])
    assert torch.equal(read_tree(tmp_path / "round3", "BDD"), want) and rep3["filled"] == rep["kept"]


def test_cli_on_unlabelled_images(dev, checkpoint, tmp_path):
    root = tmp_path / "tree"
    run_cli(checkpoint, ["--budget", 0.1, "--by", "ripu", "--out-root", root, "--layout", "BDD"])   # writes the images
    plain = AC.run_cli("ripu", AC.images_base(root / "images" / "val"), checkpoint, [
        "--radius", RADIUS, "--budget", "0.1", "--by", "ripu", "--out", tmp_path / "plain", "--json", tmp_path / "plain.json"])
    assert "error_recall" not in plain and "annotated" not in plain and plain["images"] == N_IMAGES
    assert 0 < plain["shown"] <= 0.1 * plain["total_pixels"]
    with open(tmp_path / "plain" / "selection.json") as f:
        selection = json.load(f)
    chosen, fresh = selected_mask(selection)
    assert fresh == plain["shown"] == int(chosen.sum())
    AC.assert_select_maps(tmp_path / "plain", selection["picks"], chosen)
    assert all(os.path.isfile(tmp_path / "plain" / f"{stem}_score.png") for stem in selection["picks"])
