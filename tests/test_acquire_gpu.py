"""GPU: the acquisition kernels (mdil_ss_amd/ext/acquire_head.hip) and the entry points over them
(mdil_ss_amd/acquire.py), against tests/acquire_reference.py and the fp64 head of tests/head_cases.py.

What is compared with what.  ``acquire_head`` promises ``route_head``'s chain of operations, so its label
is ``predict_head``'s: asserted bit for bit.  Independently every 16-bit q is held to the fp64 definition of
its uncertainty u: q must lie in [q_of(u64 - t), q_of(u64 + t)], t per case the larger of the logit bound
2 gamma_17 max S + 16 u (a logit within gamma_17 S moves each of the three scores by at most twice that;
16 u for the exp2, the sums, the reciprocal, the logarithm and the products) and 4 x the worst absolute
distance of a plain float32 torch evaluation of the same score from fp64 on the same case; no pixel is
excluded.  The test prints how far the kernel's q lie from the fp64 score as a multiple of that float32
distance.  Everything after q is integer arithmetic and is asserted exactly, on the kernel's own maps."""
import functools
import glob
import json

import pytest
import torch
import torch.nn.functional as F

from tests import acquire_reference as R
from tests import annotate_cases as AC
from tests import head_cases as HC
from tests.annotate_cases import IGNORE, N_IMAGES, SENTINEL, SIZE, checkpoint, read_tree, synthetic_targets
from tests.head_cases import CLASSES, SHAPES, nhwc

pytestmark = pytest.mark.gpu

K = 17
BIG = (3, 16, 48)
SCALE = 8.0                                     # the trained regime: logits 8 times as far apart
TILE = (4, 6)                                   # the tile of the shared runs: ragged on every shape but (3, 16, 48)
HEAD_WG, HEAD_BLOCKS = 256, 768                 # acquire_head.hip: kHeadWG, kHeadMaxBlocks
TILE_CASES = (((2, 2), (2, 12, 20)), ((2, 2), BIG), ((4, 6), (1, 9, 7)), ((4, 6), (2, 12, 20)), ((6, 4), (1, 9, 7)),
              ((6, 4), (2, 12, 20)), ((8, 8), BIG), ((256, 256), BIG), ((256, 256), (1, 1, 1)), ((2, 256), (2, 12, 20)))


@pytest.fixture(scope="module")
def dev():
    return HC.device("acquisition")


def inputs(nc, shape, scale=1.0):
    x, w, b = HC.head_inputs(nc, shape)
    return x, (w * scale if scale != 1.0 else w), b


def case_target(nc, shape):
    return HC.make_target(nc, (shape[0], 2 * shape[1], 2 * shape[2]), IGNORE, seed=nc + shape[1])


def head(dev, xd, wd, bd, tile, kind="entropy", target=None, tiles=None, counters=None, maps=True):
    """One call -> host (label, q as int64, tiles, counters)."""
    from mdil_ss_amd import acquire as A
    nc, (N, H, W) = wd.shape[1], xd.shape[:3]
    if tiles is None:
        tiles = A.new_tiles(N, (2 * H, 2 * W), tile, nc, dev)
    if counters is None:
        counters = {k: torch.zeros(1, dtype=torch.int64, device=dev) for k in
                    (A.HEAD_COUNTERS if target is not None else ("nonfinite",))}
    label, qmap = A.acquire_head(xd, wd, bd, tile, kind, target, IGNORE if target is not None else -1, tiles, counters,
                                 want_label=maps, want_qmap=maps)
    torch.cuda.synchronize()
    return (label.cpu() if maps else None, A.q_values(qmap.cpu()) if maps else None, tiles.cpu(),
            {k: int(v.item()) for k, v in counters.items()})


@functools.lru_cache(maxsize=None)
def device_run(nc, shape, scale=1.0):
    """Case (nc, shape) with its target and TILE: the maps and table of every kind, and predict_head's label."""
    dev = torch.device("cuda", 0)
    x, w, b = inputs(nc, shape, scale)
    xd, wd, bd = nhwc(x).to(dev), w.to(dev), b.to(dev)
    target = case_target(nc, shape)
    run = {"args": (xd, wd, bd), "target": target, "dtarget": target.to(dev), "plabel": HC.predict_labels(dev, x, w, b)}
    for kind in R.KINDS:
        run[kind] = head(dev, xd, wd, bd, TILE, kind, run["dtarget"])
    return run


@functools.lru_cache(maxsize=None)
def reference(nc, shape, scale=1.0):
    """Per kind the fp64 score, the float32 torch score's worst absolute distance from it, and the bound t.
    Computed once, never modified."""
    x, w, b = inputs(nc, shape, scale)
    logits, S = HC.head64(x, w, b)
    logits32 = F.conv_transpose2d(x, w, b, stride=2)
    out = {}
    for kind in R.KINDS:
        u64 = R.scores(logits, kind)
        d32 = float((R.scores(logits32, kind).double() - u64).abs().max())
        out[kind] = (u64, d32, max(4.0 * d32, 2 * HC.gamma(K) * float(S.max()) + 16 * HC.U))
    return out


def check_table(table, label, q, target, nc, tile, counters, finite=None, times=1, base=0):
    """The table is the bincounts of the kernel's own maps; its sums close."""
    want = R.tile_table(label, q, target, nc, IGNORE, tile, finite)
    got = table - base
    assert torch.equal(got, times * want), f"tile {tile}: {int((got != times * want).sum())} cells differ"
    pixels = label.numel()
    assert int(got[..., 0].sum()) + times * counters["nonfinite"] == times * pixels
    assert torch.equal(got[..., R.FIELDS:].sum(-1), got[..., 0])
    if target is not None:
        assert counters["bad_targets"] == int(((target.long() >= nc) & (target.long() != IGNORE)).sum())
        assert bool((got[..., 2] <= got[..., 3]).all()) and bool((got[..., 3] <= got[..., 0]).all())
    else:
        assert int(got[..., 2:4].abs().sum()) == 0


# ------------------------------------------------------------------------------------- (1) bits
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nc", CLASSES)
def test_label_is_predict_heads_label(dev, nc, shape):
    run = device_run(nc, shape)
    for kind in R.KINDS:
        label, q, table, counters = run[kind]
        assert label.dtype == torch.uint8 and tuple(label.shape) == (shape[0], 2 * shape[1], 2 * shape[2])
        assert torch.equal(label, run["plabel"]), kind
        assert counters["nonfinite"] == 0
        assert int(q.min()) >= 0 and int(q.max()) <= 65535


# ---------------------------------------------------------------------------------- (2) fp64
def check_q(nc, shape, scale):
    run, ref = device_run(nc, shape, scale), reference(nc, shape, scale)
    for kind in R.KINDS:
        u64, d32, t = ref[kind]
        q = run[kind][1]
        what = f"nc {nc} shape {shape} scale {scale} {kind}"
        floor = q.double() / 65536.0
        ceil = torch.where(q == 65535, torch.full_like(floor, float("inf")), (q.double() + 1) / 65536.0)
        away = float(torch.maximum(floor - u64, u64 - ceil).clamp(min=0).max())
        print(f"{what}: t {t:.3e} (float32 torch {d32:.3e}); the kernel's q are at most {away:.3e} away = "
              f"{away / max(d32, 1e-300):.2f} x float32 torch; {int((q != R.q_of(u64)).sum())} of {q.numel()} q differ from "
              "the fp64 q")
        assert bool(((q >= R.q_of(u64 - t)) & (q <= R.q_of(u64 + t))).all()), what


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nc", CLASSES)
def test_q_match_the_fp64_scores(dev, nc, shape):
    check_q(nc, shape, 1.0)


@pytest.mark.parametrize("nc", CLASSES)
def test_q_in_the_trained_regime(dev, nc):
    check_q(nc, BIG, SCALE)
    run = device_run(nc, BIG, SCALE)
    assert torch.equal(run["entropy"][0], run["plabel"])


# ------------------------------------------------------------------------------ (3) integers
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nc", CLASSES)
def test_tables_of_the_shared_runs(dev, nc, shape):
    run = device_run(nc, shape)
    for kind in R.KINDS:
        label, q, table, counters = run[kind]
        check_table(table, label, q, run["target"], nc, TILE, counters)


@pytest.mark.parametrize("tile, shape", TILE_CASES)
@pytest.mark.parametrize("nc", (2, 20, 27))
def test_tables_on_the_kernels_own_maps(dev, nc, tile, shape):
    from mdil_ss_amd import acquire as A
    run = device_run(nc, shape)
    xd, wd, bd = run["args"]
    for kind, target in (("entropy", run["dtarget"]), ("margin", None)):
        host_target = run["target"] if target is not None else None
        label, q, table, counters = head(dev, xd, wd, bd, tile, kind, target)
        assert torch.equal(label, run[kind][0]) and torch.equal(q, run[kind][1])       # the tile moves no map
        check_table(table, label, q, host_target, nc, tile, counters)
        # a second call into the same table (which held 7s): twice the counts
        N, H, W = shape
        held = A.new_tiles(N, (2 * H, 2 * W), tile, nc, dev) + 7
        for times in (1, 2):
            _, _, again, c2 = head(dev, xd, wd, bd, tile, kind, target, tiles=held, maps=False)
            check_table(again, label, q, host_target, nc, tile, c2, times=times, base=7)


# ------------------------------------------------------------------------------ (4) degenerate
@pytest.mark.parametrize("shape", ((1, 9, 7), (2, 12, 20), BIG))
def test_crowded_and_noisy_tables(dev, shape):
    """All-zero features: one label and one q, every add of a tile on one address.  Per-pixel noise: neighbouring
    lanes share neither label nor q, the merge inside the wave finds nothing."""
    nc = 20
    N, H, W = shape
    _, w, b = inputs(nc, shape)
    target = case_target(nc, shape)
    g = torch.Generator().manual_seed(3)
    noise = torch.randn(N, 16, H, W, generator=g) * 4.0
    for name, x in (("zero", torch.zeros(N, 16, H, W)), ("noise", noise)):
        xd, wd, bd = nhwc(x).to(dev), w.to(dev), b.to(dev)
        for tile in ((2, 2), (4, 6), (32, 32), (256, 256)):
            label, q, table, counters = head(dev, xd, wd, bd, tile, "entropy", target.to(dev))
            check_table(table, label, q, target, nc, tile, counters)
            assert counters["nonfinite"] == 0
            if name == "zero":
                # parities differ only through the weights' own (a, b): at most four labels and four q
                assert len(set(label.reshape(-1).tolist())) <= 4 and len(set(q.reshape(-1).tolist())) <= 4
            else:
                assert len(set(label.reshape(-1).tolist())) > nc // 2


def test_an_infinite_feature_is_counted_and_enters_no_tile(dev):
    nc, shape = 20, (2, 12, 20)
    x, w, b = inputs(nc, shape)
    xi = x.clone()
    xi[1, 9, 5, 7] = float("inf")                                   # one feature: its four output pixels
    clean = device_run(nc, shape)
    hit = torch.zeros(clean["target"].shape, dtype=torch.bool)
    hit[1, 10:12, 14:16] = True
    target = clean["target"].clone()
    target[1, 10:12, 14:16] = torch.tensor([[3, IGNORE], [nc, 5]], dtype=torch.uint8)
    xd, wd, bd = nhwc(xi).to(dev), w.to(dev), b.to(dev)
    for kind in R.KINDS:
        label, q, table, counters = head(dev, xd, wd, bd, TILE, kind, target.to(dev))
        assert counters["nonfinite"] == 4 and bool((q[hit] == 0).all())
        assert torch.equal(q[~hit], clean[kind][1][~hit]) and torch.equal(label[~hit], clean[kind][0][~hit])
        check_table(table, label, q, target, nc, TILE, counters, finite=~hit)
        assert int(table[..., 0].sum()) == target.numel() - 4


# ------------------------------------------------------------------------------ (5) strided
def test_grid_stride_loop_past_the_grid_bound(dev):
    """The grid is bounded at 768 work-groups of 256 feature pixels; 400 x 520 = 208,000 of them send 11,392
    round the loop a second time, into work-groups whose LDS table already holds other tiles."""
    nc, shape, tile = 20, (1, 400, 520), (32, 32)
    assert shape[1] * shape[2] > HEAD_WG * HEAD_BLOCKS
    x, w, b = HC.draw(nc, shape, 5)
    target = HC.make_target(nc, (1, 800, 1040), IGNORE, seed=9)
    label, q, table, counters = head(dev, nhwc(x).to(dev), w.to(dev), b.to(dev), tile, "entropy", target.to(dev))
    assert tuple(table.shape) == (1, 25, 33, 24)
    check_table(table, label, q, target, nc, tile, counters)


# ------------------------------------------------------------- (6) nothing else is written
HEAD_OUTPUTS = ("label", "qmap", "tiles", "nonfinite", "bad_targets")


def raw_head(lib, run, shape, nc, tile, p, target=True, kind=1, nc_arg=None, inv=None):
    from mdil_ss_amd import acquire as A
    xd, wd, bd = run["args"]
    N, H, W = shape
    return lib.mdil_acquire_head(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), N, H, W, nc if nc_arg is None else nc_arg,
                                 tile[0], tile[1], kind, A.inv_log_nc(nc) if inv is None else inv,
                                 run["dtarget"].data_ptr() if target else None, IGNORE, p["label"], p["qmap"], p["tiles"],
                                 p["nonfinite"], p["bad_targets"], torch.cuda.current_stream().cuda_stream)


def head_arena(dev, nc, shape, tile):
    N, H, W = shape
    npx = N * 4 * H * W
    Ty, Tx = R.grid((2 * H, 2 * W), tile)
    return HC.Arena(dev, {"label": npx, "qmap": 2 * npx, "tiles": N * Ty * Tx * (4 + nc) * 8, "nonfinite": 8, "bad_targets": 8})


@pytest.mark.parametrize("shape", ((1, 1, 1), (1, 9, 7), BIG))
def test_head_null_outputs_and_guard_bands_stay_untouched(dev, shape):
    """What was not given keeps its sentinel bytes, and so do the guard bands.  The counters are ADDED to:
    they start from the sentinel 0xA5A5A5A5A5A5A5A5."""
    from mdil_ss_amd import _acquire_lib
    lib = _acquire_lib.load()
    nc = 27
    run = device_run(nc, shape)
    label, q, table, counters = run["entropy"]
    combos = [tuple(k for i, k in enumerate(HEAD_OUTPUTS) if m >> i & 1) for m in range(1, 32)]
    for given in combos:
        arena = head_arena(dev, nc, shape, TILE)
        p = {k: (arena.ptr(k) if k in given else None) for k in HEAD_OUTPUTS}
        assert raw_head(lib, run, shape, nc, TILE, p) == 0, lib.mdil_acquire_last_error()
        torch.cuda.synchronize()
        arena.read()
        written = [k for k in given if k != "nonfinite" and (k != "bad_targets" or counters["bad_targets"])]
        arena.assert_untouched(written, given)
        if "label" in given:
            assert torch.equal(arena.cut("label"), label.reshape(-1)), given
        if "qmap" in given:
            assert torch.equal(arena.cut("qmap").view(torch.int16).long() & 0xffff, q.reshape(-1)), given
        if "tiles" in given:
            assert torch.equal(arena.cut("tiles").view(torch.int64) - SENTINEL, table.reshape(-1)), given
        if "bad_targets" in given and counters["bad_targets"]:
            assert int(arena.cut("bad_targets").view(torch.int64) - SENTINEL) == counters["bad_targets"]
    # without a target the fields 2 and 3 of the table keep what they held
    arena = head_arena(dev, nc, shape, TILE)
    p = dict.fromkeys(HEAD_OUTPUTS)
    p["tiles"] = arena.ptr("tiles")
    assert raw_head(lib, run, shape, nc, TILE, p, target=False) == 0
    torch.cuda.synchronize()
    arena.read()
    got = (arena.cut("tiles").view(torch.int64) - SENTINEL).reshape(table.shape)
    assert int(got[..., 2:4].abs().sum()) == 0 and torch.equal(got[..., :2], table[..., :2])
    assert torch.equal(got[..., 4:], table[..., 4:])


def test_head_refusals_leave_everything_untouched(dev):
    from mdil_ss_amd import _acquire_lib
    lib = _acquire_lib.load()
    nc, shape = 27, (1, 9, 7)
    run = device_run(nc, shape)
    arena = head_arena(dev, nc, shape, TILE)
    every = {k: arena.ptr(k) for k in HEAD_OUTPUTS}
    none = dict.fromkeys(HEAD_OUTPUTS)
    refused = [
        (every, dict(target=False), TILE, b"needs a target"),
        (none, dict(), TILE, b"nothing to write"),
        (every, dict(), (3, 6), b"tile 3 x 6"), (every, dict(), (4, 7), b"tile 4 x 7"), (every, dict(), (4, 258), b"tile 4 x 258"),
        (every, dict(), (0, 6), b"tile 0 x 6"),
        (every, dict(kind=3), TILE, b"kind=3"), (every, dict(kind=-1), TILE, b"kind=-1"),
        (every, dict(inv=float("nan")), TILE, b"inv_log_nc"),
        (every, dict(nc_arg=33), TILE, b"nc=33"), (every, dict(nc_arg=1), TILE, b"nc=1"),
        (dict(every, qmap=every["qmap"] + 2), dict(), TILE, b"alignment"),
        (dict(every, label=every["label"] + 1), dict(), TILE, b"alignment"),
        (dict(every, tiles=every["tiles"] + 4), dict(), TILE, b"alignment"),
    ]
    for p, kw, tile, text in refused:
        assert raw_head(lib, run, shape, nc, tile, p, **kw) == -1, (kw, text)
        assert text in lib.mdil_acquire_last_error(), (text, lib.mdil_acquire_last_error())
    torch.cuda.synchronize()
    arena.read()
    arena.assert_untouched([])


def test_side_stream_gives_the_same_bytes(dev):
    from mdil_ss_amd import acquire as A
    nc = 27
    run = device_run(nc, BIG)
    xd, wd, bd = run["args"]
    size = (2 * BIG[1], 2 * BIG[2])
    sel = (torch.arange(BIG[0] * 8 * 16).reshape(BIG[0], 8, 16) % 3 == 0).to(torch.uint8).to(dev)

    def everything():
        tiles = A.new_tiles(BIG[0], size, TILE, nc, dev)
        c = {k: torch.zeros(1, dtype=torch.int64, device=dev) for k in A.HEAD_COUNTERS}
        label, qmap = A.acquire_head(xd, wd, bd, TILE, "margin", run["dtarget"], IGNORE, tiles, c, True, True)
        a = A.new_apply_counters(nc, dev)
        out, mask = A.acquire_apply(sel, size, TILE, nc, run["dtarget"], label, None, IGNORE, 250, a, want_mask=True)
        return [label, qmap, tiles, out, mask] + list(c.values()) + list(a.values())

    first = everything()
    torch.cuda.synchronize()
    second = HC.side_stream(everything)
    for a, c in zip(first, second):
        assert torch.equal(HC.as_bytes(a.cpu()), HC.as_bytes(c.cpu()))
    assert torch.equal(first[0].cpu(), run["margin"][0])


# ---------------------------------------------------------------------------------- (7) apply
@pytest.mark.parametrize("Wl", AC.APPLY_WIDTHS)
@pytest.mark.parametrize("Hl", AC.APPLY_HEIGHTS)
def test_apply_maps_and_counters(dev, Hl, Wl):
    from mdil_ss_amd import acquire as A
    nc, N = AC.APPLY_NC, AC.APPLY_N
    _, target, previous, fill, _ = AC.apply_maps(N, Hl, Wl, nc, AC.apply_seed(Hl, Wl))
    dmaps = [t.to(dev) for t in (target, previous, fill)]
    for tile in AC.APPLY_TILES:
        Ty, Tx = R.grid((Hl, Wl), tile)
        sel = AC.tile_selection(N, (Ty, Tx), AC.apply_seed(Hl, Wl))
        dsel = sel.to(dev)
        for use in range(8):
            host = [m if use >> i & 1 else None for i, m in enumerate((target, previous, fill))]
            devm = [m if use >> i & 1 else None for i, m in enumerate(dmaps)]
            want = R.apply_ref(sel, (Hl, Wl), tile, nc, *host, IGNORE, 250)
            names = A.APPLY_COUNTERS if host[0] is not None else ("shown", "kept", "filled")
            counters = A.new_apply_counters(nc, dev, names)
            for times in (1, 2):
                out, mask = A.acquire_apply(dsel, (Hl, Wl), tile, nc, *devm, IGNORE, 250, counters, want_mask=True)
                what = (tile, use, times)
                assert out.dtype == torch.uint8 and torch.equal(out.cpu(), want["out"]), what
                assert mask.dtype == torch.uint8 and torch.equal(mask.cpu(), want["mask"]), what
                AC.check_counters(counters, want, times)
    every = torch.ones(N, Ty, Tx, dtype=torch.uint8, device=dev)
    out, _ = A.acquire_apply(every, (Hl, Wl), tile, nc, dmaps[0], dmaps[1], dmaps[2], IGNORE, 250)
    assert torch.equal(out.cpu(), target)                             # every tile chosen: the target itself
    out, mask = A.acquire_apply(every * 0, (Hl, Wl), tile, nc, dmaps[0], None, None, IGNORE, 250, want_mask=True)
    assert bool((out == 250).all()) and not bool(mask.any())


@pytest.mark.parametrize("Wl", (5, 1001, 1024))
def test_apply_null_outputs_refusals_and_guard_bands(dev, Wl):
    from mdil_ss_amd import _acquire_lib
    lib = _acquire_lib.load()
    nc, N, Hl, tile = 20, 2, 5, (4, 6)
    _, target, previous, fill, _ = AC.apply_maps(N, Hl, Wl, nc, AC.apply_seed(Hl, Wl))
    Ty, Tx = R.grid((Hl, Wl), tile)
    sel = (torch.arange(N * Ty * Tx).reshape(N, Ty, Tx) % 2).to(torch.uint8)
    want = R.apply_ref(sel, (Hl, Wl), tile, nc, target, previous, fill, IGNORE, 250)
    dt, dp, df, ds = (t.to(dev) for t in (target, previous, fill, sel))
    npix = N * Hl * Wl
    sizes = {"out": npix, "mask": npix, "shown": 8, "annotated": nc * 8, "kept": nc * 8, "filled": nc * 8, "bad_targets": 8}

    def call(p, th=tile[0], nc_arg=nc, drop=250, tgt=True):
        return lib.mdil_acquire_apply(ds.data_ptr(), dt.data_ptr() if tgt else None, dp.data_ptr(), df.data_ptr(), N, Hl, Wl,
                                      th, tile[1], nc_arg, IGNORE, drop, p["out"], p["mask"], p["shown"], p["annotated"],
                                      p["kept"], p["filled"], p["bad_targets"], torch.cuda.current_stream().cuda_stream)

    combos = [(k,) for k in sizes] + [("out", "mask"), ("shown", "annotated", "kept", "filled", "bad_targets"), tuple(sizes)]
    for given in combos:
        arena = HC.Arena(dev, sizes)
        p = {k: (arena.ptr(k) if k in given else None) for k in sizes}
        assert call(p) == 0, lib.mdil_acquire_last_error()
        torch.cuda.synchronize()
        arena.read()
        AC.check_arena(arena, given, want, ("shown", "bad_targets"))
    arena = HC.Arena(dev, sizes)
    every = {k: arena.ptr(k) for k in sizes}
    for p, kw, text in ((dict.fromkeys(sizes), {}, b"nothing to write"), (every, dict(th=3), b"tile 3 x 6"),
                        (every, dict(nc_arg=33), b"nc=33"), (every, dict(drop=256), b"drop_id=256"),
                        (every, dict(tgt=False), b"need a target"), (dict(every, out=every["out"] + 4), {}, b"alignment")):
        assert call(p, **kw) == -1 and text in lib.mdil_acquire_last_error(), text
    torch.cuda.synchronize()
    arena.read()
    arena.assert_untouched([])


# ----------------------------------------------------------------------------- (8) end to end
CLI_TILE = (16, 16)
CLI = AC.CLI_BASE + ["--subset", "val", "--tile", "16", "16"]
REPORT_KEYS = ("dataset", "kind", "by", "tile", "budget", "images", "total_pixels", "pixels_asked", "pixels_spent",
               "tiles", "tiles_selected", "images_touched", "tiles_per_image_mean", "tiles_per_image_max",
               "mean_uncertainty_selected", "mean_uncertainty_all", "mean_impurity_selected", "mean_impurity_all",
               "predicted_selected", "predicted_all", "nonfinite", "error_recall", "error_recall_chosen", "wrong_pixels",
               "shown", "annotated", "annotated_pixels", "given", "annotated_share_per_class", "kept", "filled", "written")


run_cli = functools.partial(AC.run_cli, "acquire", CLI)


def selected_mask(selection):
    mask = torch.zeros((N_IMAGES,) + SIZE, dtype=torch.bool)
    for stem, tiles in selection["tiles"].items():
        for y0, x0, y1, x1, _ in tiles:
            mask[int(stem[-4:]), y0:y1, x0:x1] = True
    return mask


@pytest.mark.parametrize("layout, by", (("BDD", "ripu"), ("cityscapes", "oracle")))
def test_cli_report_selection_and_label_tree(dev, checkpoint, tmp_path, layout, by):
    budget = 0.1
    report_file, root, out = tmp_path / "report.json", tmp_path / "round1", tmp_path / "maps"
    run_cli(checkpoint, ["--budget", budget, "--by", by, "--json", report_file, "--out-root", root, "--layout", layout,
                         "--out", out])
    with open(report_file) as f:
        saved = json.load(f)
    assert all(k in saved for k in REPORT_KEYS), [k for k in REPORT_KEYS if k not in saved]
    total, tile_px = N_IMAGES * SIZE[0] * SIZE[1], CLI_TILE[0] * CLI_TILE[1]
    assert saved["total_pixels"] == total and saved["tiles"] == N_IMAGES * 4 * 8 and saved["nonfinite"] == 0
    assert budget * total - tile_px < saved["shown"] <= budget * total
    assert saved["shown"] == saved["pixels_spent"] == saved["tiles_selected"] * tile_px
    assert set(saved["error_recall"]) == set(R.CRITERIA) and saved["error_recall_chosen"] == saved["error_recall"][by]
    # a tile size that divides the image: no criterion finds more errors in as many tiles than the oracle
    assert all(saved["error_recall"]["oracle"] >= v for v in saved["error_recall"].values())
    assert sum(saved["predicted_all"]) == total and sum(saved["predicted_selected"]) == saved["shown"]
    with open(root / "selection.json") as f:
        selection = json.load(f)
    with open(out / "selection.json") as f:
        assert json.load(f) == selection
    chosen = selected_mask(selection)
    assert int(chosen.sum()) == saved["shown"] and sum(len(v) for v in selection["tiles"].values()) == saved["tiles_selected"]
    target = synthetic_targets()
    want = torch.where(chosen & (target != 19), target, torch.tensor(255, dtype=torch.uint8))
    assert torch.equal(read_tree(root, layout), want)                  # opened by the trainers' dataset class
    assert saved["annotated"] == torch.bincount(target[chosen & (target != 19)].long(), minlength=20).tolist()
    assert saved["given"] == torch.bincount(target[target != 19].long(), minlength=20).tolist()
    # the maps of --out, for the images with a selected tile
    import numpy as np
    from PIL import Image
    assert len(glob.glob(str(out / "*_select.png"))) == saved["images_touched"] == len(selection["tiles"])
    AC.assert_select_maps(out, selection["tiles"], chosen)
    for stem in selection["tiles"]:
        with Image.open(out / f"{stem}_uncertainty.png") as im:
            assert np.array(im).shape == SIZE
    # the scores in selection.json are the criterion's, in rank order within an image
    for tiles in selection["tiles"].values():
        scores = [t[4] for t in tiles]
        assert scores == sorted(scores, reverse=True)


def test_cli_same_seed_same_bytes_and_previous_rounds(dev, checkpoint, tmp_path):
    budget = 0.1
    roots = [tmp_path / n for n in ("a", "b", "round2")]
    for root in roots[:2]:
        run_cli(checkpoint, ["--budget", budget, "--by", "random", "--seed", 3, "--out-root", root, "--layout", "BDD",
                             "--json", root / "report.json"])
    AC.assert_same_files(roots[0], roots[1], 2 * N_IMAGES + 2)
    other = run_cli(checkpoint, ["--budget", budget, "--by", "random", "--seed", 4, "--json", tmp_path / "other.json"])
    with open(roots[0] / "selection.json") as f:
        first = json.load(f)
    assert other["tiles_selected"] == sum(len(v) for v in first["tiles"].values())
    # round 2: the tiles of round 1 leave the ranking, its labels are kept
    rep = run_cli(checkpoint, ["--budget", budget, "--by", "uncertainty", "--previous", roots[0] / "selection.json",
                               "--previous-root", roots[0], "--out-root", roots[2], "--layout", "BDD", "--json",
                               tmp_path / "r2.json", "--max-per-image", 0.5])
    with open(roots[2] / "selection.json") as f:
        second = json.load(f)
    one, two = selected_mask(first), selected_mask(second)
    assert not bool((one & two).any()) and int(two.sum()) == rep["shown"] > 0
    target = synthetic_targets()
    want = torch.where((one | two) & (target != 19), target, torch.tensor(255, dtype=torch.uint8))
    assert torch.equal(read_tree(roots[2], "BDD"), want)
    assert sum(rep["kept"]) == int((one & ~two & (target != 19)).sum())
    # with round 1's tree as fill instead: the same tree, counted as filled
    rep3 = run_cli(checkpoint, ["--budget", budget, "--by", "uncertainty", "--previous", roots[0] / "selection.json",
                                "--fill-root", roots[0], "--out-root", tmp_path / "round3", "--layout", "BDD", "--max-per-image",
                                0.5])
    assert torch.equal(read_tree(tmp_path / "round3", "BDD"), want) and rep3["filled"] == rep["kept"]


def test_cli_on_unlabelled_images(dev, checkpoint, tmp_path):
    root = tmp_path / "tree"
    run_cli(checkpoint, ["--budget", 0.1, "--by", "ripu", "--out-root", root, "--layout", "BDD"])   # writes the images
    plain = AC.run_cli("acquire", AC.images_base(root / "images" / "val"), checkpoint, [
        "--tile", "16", "16", "--budget", "0.1", "--by", "ripu", "--out", tmp_path / "plain", "--json", tmp_path / "plain.json"])
    assert "error_recall" not in plain and "annotated" not in plain and plain["images"] == N_IMAGES
    assert 0 < plain["shown"] <= 0.1 * plain["total_pixels"] and plain["shown"] == plain["pixels_spent"]
    with open(tmp_path / "plain" / "selection.json") as f:
        selection = json.load(f)
    chosen = selected_mask(selection)
    AC.assert_select_maps(tmp_path / "plain", selection["tiles"], chosen)
