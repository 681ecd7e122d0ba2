"""GPU: the superpixel acquisition add-on (include/mdil_spx.h) against tests/spx_reference.py.  Every comparison
is exact (``torch.equal``): the library computes in integers after the colour quantisation.

  (1) spx_slic    id, centres and sums over the shapes, steps, compactnesses and iteration counts below, on noise, a
                  constant image, two-colour stripes, values on k / 255 +- 1 ulp, NaN and out-of-range values and the
                  hand-built image that empties a centre; a batch past the grid bound; the same bytes twice and on a
                  side stream; guard bands
  (2) spx_table   SLIC's ids, scattered ids and ids out of range; nc in {2, 20, 32}; widths {1, 3, 5, 1001, 1024}
  (3) spx_apply   the same, with and without answers, every counter
  (4) both        NULL outputs and guard bands, refusals, counters added twice, acquire_head's own maps, a map past
                  the grid bound
  (5) the command line on --synthetic 4"""
import functools
import glob
import json
import os

import numpy as np
import pytest
import torch

from tests import annotate_cases as AC
from tests import head_cases as HC
from tests import spx_reference as R
from tests.annotate_cases import IGNORE, N_IMAGES, SENTINEL, SIZE, check_counters, checkpoint, read_tree, synthetic_targets

pytestmark = pytest.mark.gpu

# spx.hip: a job of spx_assign is a block of whole cells of at most kBlockPx x kBlockPx = 64 x 64 pixels (16 x 16 cells
# at S = 4, 4 x 4 at 16, one at 64).  BLOCKS crosses two block borders down and three across at every step, with a last
# block of 3 rows and of 5 columns.  STRIDE holds 1030 jobs (one per image at S = 4), past kAssignMaxBlocks = 1024.
BLOCKS = (1, 131, 197)
STRIDE = (1030, 9, 7)
SHAPES = ((1, 1, 1), (2, 9, 7), (1, 5, 300), (2, 70, 134), BLOCKS)
STEPS = (4, 16, 64)
COMPACT = (1, 10, 64)
ROUNDS = (0, 1, 2, 10)
WIDTHS = (2, 20, 32)
# spx_table / spx_apply: 512 work-groups x 256 lanes x 8 pixels = 1,048,576 pixels per round of the loop
LARGE = (1, 1025, 1024)


@pytest.fixture(scope="module")
def dev():
    return HC.device("superpixel")


def stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def image(shape, family="noise"):
    """f32 [N,3,H,W] on the host; never modified."""
    N, H, W = shape
    g = torch.Generator().manual_seed(H * 1000 + W)
    if family == "noise":
        return torch.rand(N, 3, H, W, generator=g)
    if family == "constant":                                      # every D a tie or purely spatial
        return torch.full((N, 3, H, W), 0.3)
    if family == "stripes":                                        # two colours, diagonal, 2 pixels wide: centres get emptied at m = 1
        yy, xx = torch.arange(H)[:, None], torch.arange(W)[None]
        on = (((xx + yy) // 2) % 2).float()
        return torch.stack([on, 1.0 - on, on * 0.5], 0)[None].expand(N, -1, -1, -1).contiguous()
    if family == "ulp":                                            # exactly on k / 255 and (k + 0.5) / 255, one ulp either way
        k = torch.randint(0, 511, (N, 3, H, W), generator=g).float() / 510.0
        step = torch.randint(-1, 2, (N, 3, H, W), generator=g).numpy()
        v = k.numpy()
        v = np.where(step < 0, np.nextafter(v, np.float32(-1)), np.where(step > 0, np.nextafter(v, np.float32(2)), v))
        return torch.from_numpy(v.astype(np.float32))
    v = torch.rand(N, 3, H, W, generator=g) * 3.0 - 1.0             # "wild": out of range, NaN, infinities
    r = torch.rand(N, 3, H, W, generator=g)
    v[r < 0.1] = float("nan")
    v[(r >= 0.1) & (r < 0.13)] = float("inf")
    v[(r >= 0.13) & (r < 0.16)] = float("-inf")
    return v


@functools.lru_cache(maxsize=None)
def slic_ref(shape, family, S, m, T):
    return R.slic(image(shape, family), S, m, T)


def check_slic(dev, img, want, S, m, T, what):
    from mdil_ss_amd import superpixel as P
    ids, centres, sums = P.spx_slic(img.to(dev), S, m, T)
    assert ids.dtype == torch.int32 and centres.dtype == torch.int32 and sums.dtype == torch.int64
    assert torch.equal(ids.cpu().long(), want[0]), what
    assert torch.equal(centres.cpu().long(), want[1]), what
    assert torch.equal(sums.cpu(), want[2]), what
    return ids, centres, sums


# ----------------------------------------------------------------------------------- (1) slic
@pytest.mark.parametrize("S", STEPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_slic_on_noise(dev, shape, S):
    """S = 16 and 64 on 9 x 7 and 1 x 1: the image is smaller than a cell."""
    for m in COMPACT:
        for T in ROUNDS:
            check_slic(dev, image(shape), slic_ref(shape, "noise", S, m, T), S, m, T, (shape, S, m, T))


@pytest.mark.parametrize("family, m", (("constant", 1), ("constant", 64), ("stripes", 1), ("stripes", 10), ("ulp", 10), ("wild", 10)))
@pytest.mark.parametrize("shape", ((2, 9, 7), (2, 70, 134), BLOCKS))
def test_slic_input_families(dev, shape, family, m):
    emptied = 0
    for S in STEPS:
        for T in (0, 2, 10):
            want = slic_ref(shape, family, S, m, T)
            check_slic(dev, image(shape, family), want, S, m, T, (shape, family, S, m, T))
            emptied += int((want[2][..., 0] == 0).sum())
    if family == "stripes" and m == 1 and shape != (2, 9, 7):
        assert emptied > 0                                         # the case is what it says: some centre lost every pixel
    if family == "wild":
        codes = R.quantise(image(shape, family))
        assert int(codes.min()) == 0 and int(codes.max()) == 255


def test_slic_empties_a_centre_that_keeps_its_state(dev):
    img = R.emptied_image()
    for T in (0, 1, 2, 3):
        _, centres, sums = check_slic(dev, img, R.slic(img, 4, 1, T), 4, 1, T, T)
    assert sums[0, 1].tolist() == [0] * 6 and centres[0, 1].tolist() == [0, 88, 800, 800, 0]


def test_slic_past_the_grid_bound(dev):
    """STRIDE: more jobs than work-groups, so the loop over jobs strides; every image differs."""
    check_slic(dev, image(STRIDE), slic_ref(STRIDE, "noise", 4, 10, 1), 4, 10, 1, STRIDE)


def test_slic_same_bytes_side_stream_guard_bands_and_refusals(dev):
    from mdil_ss_amd import _spx_lib
    from mdil_ss_amd import superpixel as P
    lib = _spx_lib.load()
    shape, S, m, T = (2, 70, 134), 16, 10, 2
    N, H, W = shape
    Gy, Gx = R.grid(H, W, S)
    K = Gy * Gx
    img = image(shape).to(dev)
    want = slic_ref(shape, "noise", S, m, T)
    sizes = {"id": N * H * W * 4, "centres": N * K * 5 * 4, "sums": N * K * 6 * 8}
    arena = HC.Arena(dev, sizes)

    def call(**kw):
        a = dict(image=img.data_ptr(), S=S, m=m, T=T, id=arena.ptr("id"), centres=arena.ptr("centres"), sums=arena.ptr("sums"))
        a.update(kw)
        return lib.mdil_spx_slic(a["image"], N, H, W, a["S"], a["m"], a["T"], a["id"], a["centres"], a["sums"], stream())

    for kw, text in ((dict(S=3), b"step=3"), (dict(S=65), b"step=65"), (dict(m=0), b"compactness=0"), (dict(T=33), b"iterations=33"),
                     (dict(id=None), b"all required"), (dict(sums=None), b"all required"),
                     (dict(centres=arena.ptr("centres") + 4), b"alignment")):
        assert call(**kw) == -1 and text in lib.mdil_spx_last_error(), text
    torch.cuda.synchronize()
    arena.read()
    arena.assert_untouched([])                                     # refusals leave everything untouched
    for _ in range(2):                                             # the second call finds its own outputs in place
        assert call() == 0, lib.mdil_spx_last_error()
        torch.cuda.synchronize()
        arena.read()
        arena.assert_untouched(list(sizes))
        assert torch.equal(arena.cut("id").view(torch.int32).long().reshape(N, H, W), want[0])
        assert torch.equal(arena.cut("centres").view(torch.int32).long().reshape(N, K, 5), want[1])
        assert torch.equal(arena.cut("sums").view(torch.int64).reshape(N, K, 6), want[2])
    first = P.spx_slic(img, S, m, T)
    second = P.spx_slic(img, S, m, T)
    side = HC.side_stream(lambda: P.spx_slic(img, S, m, T))
    for a, b, c in zip(first, second, side):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(img.cpu(), image(shape))


# ------------------------------------------------------------------------- (2) table, (3) apply
@functools.lru_cache(maxsize=None)
def id_maps(shape, K, family):
    """int64 [N,H,W] on the host: SLIC's ids (local), scattered random ids, or scattered with ids out of range."""
    N, H, W = shape
    g = torch.Generator().manual_seed(H * 31 + W + K)
    if family == "slic":
        ids = R.slic(image(shape), 4, 10, 1)[0]
        assert int(ids.max()) < K
        return ids
    ids = torch.randint(0, K, shape, generator=g)
    if family == "beyond":
        r = torch.rand(shape, generator=g)
        ids[r < 0.05] = K
        ids[(r >= 0.05) & (r < 0.1)] = -1
        ids[(r >= 0.1) & (r < 0.12)] = 2 ** 31 - 1
        ids[(r >= 0.12) & (r < 0.14)] = -2 ** 31
    return ids


@functools.lru_cache(maxsize=None)
def region_maps(N, K, nc, seed):
    """(selected u8 [N,K]: 255 chosen, 128 and 1 marks, answer u8 [N,K]: classes, the ignore id and values >= nc)"""
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(N, K, generator=g)
    selected = torch.where(r < 0.35, 255, torch.where(r < 0.5, 128, torch.where(r < 0.55, 1, 0))).to(torch.uint8)
    answer = torch.randint(0, nc + 2, (N, K), generator=g, dtype=torch.uint8)
    answer[torch.rand(N, K, generator=g) < 0.1] = IGNORE
    return selected, answer


def to_q(q, dev):
    return torch.from_numpy(q.numpy().astype("uint16")).to(dev)


def table_case(dev, shape, K, nc, family, times=2):
    from mdil_ss_amd import superpixel as P
    N, H, W = shape
    _, target, _, _, label = AC.apply_maps(N, H, W, nc, AC.apply_seed(H, W))
    q = torch.randint(0, 65536, shape, generator=torch.Generator().manual_seed(H + W))
    ids = id_maps(shape, K, family)
    want = R.table_ref(label, q, ids, K, nc, target, IGNORE)
    dl, dq, dt, di = label.to(dev), to_q(q, dev), target.to(dev), ids.to(torch.int32).to(dev)
    table = tcount = None
    counters = hc_zero(dev, P.TABLE_COUNTERS)
    for t in range(1, times + 1):                                  # everything is ADDED to
        table, tcount = P.spx_table(dl, dq, di, K, nc, dt, IGNORE, table, tcount, counters)
        assert torch.equal(table.cpu(), t * want["table"]), (shape, K, nc, family, t)
        assert torch.equal(tcount.cpu(), t * want["tcount"]), (shape, K, nc, family, t)
        check_counters(counters, want, t)
    plain = R.table_ref(label, q, ids, K, nc)
    table, tcount = P.spx_table(dl, dq, di, K, nc)                 # no target: fields 2 and 3 stay 0, no tcount
    assert tcount is None and torch.equal(table.cpu(), plain["table"])
    return want


def hc_zero(dev, names):
    return {k: torch.zeros(1, dtype=torch.int64, device=dev) for k in names}


@pytest.mark.parametrize("Wl", AC.APPLY_WIDTHS)
@pytest.mark.parametrize("Hl", AC.APPLY_HEIGHTS)
def test_table_and_apply_over_the_widths(dev, Hl, Wl):
    """Widths 1001 and 1024 cross the packed / byte-wise border of an item; N = 2: an item may span two images."""
    for nc in WIDTHS:
        for family in ("scattered", "beyond"):
            want = table_case(dev, (AC.APPLY_N, Hl, Wl), 7, nc, family)
            assert want["bad_ids"] > 0 or family == "scattered" or Hl * Wl < 50
        apply_case(dev, (AC.APPLY_N, Hl, Wl), 7, nc, "beyond")


@pytest.mark.parametrize("nc", WIDTHS)
@pytest.mark.parametrize("shape", ((2, 9, 7), (2, 70, 134), BLOCKS))
def test_table_and_apply_on_slic_and_scattered_ids(dev, shape, nc):
    Gy, Gx = R.grid(shape[1], shape[2], 4)
    for family in ("slic", "scattered", "beyond"):
        table_case(dev, shape, Gy * Gx, nc, family)
        apply_case(dev, shape, Gy * Gx, nc, family)


def apply_case(dev, shape, K, nc, family):
    from mdil_ss_amd import superpixel as P
    N, H, W = shape
    _, target, previous, fill, label = AC.apply_maps(N, H, W, nc, AC.apply_seed(H, W))
    ids = id_maps(shape, K, family)
    selected, answer = region_maps(N, K, nc, H * 7 + W)
    di, ds, da = ids.to(torch.int32).to(dev), selected.to(dev), answer.to(dev)
    dt, dp, df, dl = (t.to(dev) for t in (target, previous, fill, label))
    for ans, dans in ((answer, da), (None, None)):
        want = R.apply_ref(ids, selected, nc, ans, target, previous, fill, label, IGNORE, 250)
        counters = P.new_apply_counters(nc, dev)
        for times in (1, 2):                                       # the counters are ADDED to
            out, mask = P.spx_apply(di, ds, nc, dans, dt, dp, df, dl, IGNORE, 250, counters, want_out=True, want_mask=True)
            assert torch.equal(out.cpu(), want["out"]) and torch.equal(mask.cpu(), want["mask"]), (shape, K, nc, family)
            check_counters(counters, want, times)
    # fewer inputs: an answer without a target; nothing but the selection
    for kw, names in ((dict(answer=da, fill=df), ("shown", "annotated", "kept", "filled", "bad_ids")), (dict(previous=dp), ("shown", "kept", "filled")), (dict(), ("shown",))):
        ref = R.apply_ref(ids, selected, nc, answer if "answer" in kw else None, None, previous if "previous" in kw else None,
                          fill if "fill" in kw else None, None, IGNORE, 250)
        c = P.new_apply_counters(nc, dev, names)
        out, mask = P.spx_apply(di, ds, nc, ignore_index=IGNORE, drop_id=250, counters=c, want_mask=True, **kw)
        assert torch.equal(out.cpu(), ref["out"]) and torch.equal(mask.cpu(), ref["mask"])
        check_counters(c, ref, 1)
    return want


def test_table_and_apply_past_the_grid_bound(dev):
    """LARGE: more items than one round of the loop holds; local ids (cells of 32 x 32) and scattered ones."""
    from mdil_ss_amd import superpixel as P
    N, H, W = LARGE
    nc, K = 20, 33 * 32
    g = torch.Generator().manual_seed(5)
    label = torch.randint(0, nc, LARGE, generator=g, dtype=torch.uint8)
    target = HC.make_target(nc, LARGE, IGNORE, 9)
    q = torch.randint(0, 65536, LARGE, generator=g)
    cells = ((torch.arange(H)[:, None] // 32) * 32 + torch.arange(W)[None] // 32)[None]
    selected, answer = region_maps(N, K, nc, 77)
    for ids in (cells, torch.randint(0, K, LARGE, generator=g)):
        di = ids.to(torch.int32).to(dev)
        want = R.table_ref(label, q, ids, K, nc, target, IGNORE)
        table, tcount = P.spx_table(label.to(dev), to_q(q, dev), di, K, nc, target.to(dev), IGNORE)
        assert torch.equal(table.cpu(), want["table"]) and torch.equal(tcount.cpu(), want["tcount"])
        ref = R.apply_ref(ids, selected, nc, answer, target, None, None, label, IGNORE, 250)
        counters = P.new_apply_counters(nc, dev)
        out, mask = P.spx_apply(di, selected.to(dev), nc, answer.to(dev), target.to(dev), label=label.to(dev), ignore_index=IGNORE,
                                drop_id=250, counters=counters, want_mask=True)
        assert torch.equal(out.cpu(), ref["out"]) and torch.equal(mask.cpu(), ref["mask"])
        check_counters(counters, ref, 1)


@functools.lru_cache(maxsize=None)
def head_maps():
    """acquire_head's own label and q maps of the tiny model on the 4 procedural images of the command-line tests."""
    from mdil_ss_amd import acquire as A
    from mdil_ss_amd.dataset import ProceduralSeg
    dev = torch.device("cuda", 0)
    model = HC.tiny_model(dev)
    ds = ProceduralSeg(N_IMAGES, SIZE[0], SIZE[1], 20, seed=13, domain=1)
    images = torch.stack([ds[i][0] for i in range(N_IMAGES)])
    with torch.no_grad():
        feat = model.features(images.to(dev), 1).contiguous()
    w, b = (t.detach() for t in model.head_params(1))
    label, qmap = A.acquire_head(feat, w, b, (2, 2), "entropy", want_label=True, want_qmap=True)
    torch.cuda.synchronize()
    return images, label, qmap, label.cpu(), A.q_values(qmap.cpu())


def test_table_on_acquire_heads_own_maps(dev):
    from mdil_ss_amd import superpixel as P
    images, dl, dq, label, q = head_maps()
    target = synthetic_targets()
    assert tuple(label.shape) == (N_IMAGES,) + SIZE and int(q.max()) > 0
    ids, centres, _ = P.spx_slic(images.to(dev), 16, 10, 3)
    want_ids = R.slic(images, 16, 10, 3)[0]
    assert torch.equal(ids.cpu().long(), want_ids)
    K = centres.shape[1]
    table, tcount = P.spx_table(dl, dq, ids, K, 20, target.to(dev), 19)
    want = R.table_ref(label, q, want_ids, K, 20, target, 19)
    assert torch.equal(table.cpu(), want["table"]) and torch.equal(tcount.cpu(), want["tcount"])
    assert int(table[..., 0].sum()) == N_IMAGES * SIZE[0] * SIZE[1]


# ----------------------------------------------------------- (4) NULL outputs, guard bands, refusals
def test_table_null_outputs_refusals_and_guard_bands(dev):
    from mdil_ss_amd import _spx_lib
    from mdil_ss_amd import superpixel as P
    lib = _spx_lib.load()
    shape, K, nc = (2, 5, 1001), 7, 20
    N, H, W = shape
    _, target, _, _, label = AC.apply_maps(N, H, W, nc, AC.apply_seed(H, W))
    q = torch.randint(0, 65536, shape, generator=torch.Generator().manual_seed(1))
    ids = id_maps(shape, K, "beyond")
    want = R.table_ref(label, q, ids, K, nc, target, IGNORE)
    dl, dq, dt, di = label.to(dev), to_q(q, dev), target.to(dev), ids.to(torch.int32).to(dev)
    sizes = {"table": N * K * (4 + nc) * 8, "tcount": N * K * nc * 8, "bad_targets": 8, "bad_ids": 8}

    def call(p, nc_arg=nc, K_arg=K, tgt=True):
        return lib.mdil_spx_table(dl.data_ptr(), dq.data_ptr(), dt.data_ptr() if tgt else None, IGNORE, di.data_ptr(), N, H, W,
                                  K_arg, nc_arg, p["table"], p["tcount"], p["bad_targets"], p["bad_ids"], stream())

    for given in [(k,) for k in sizes] + [("table", "tcount"), tuple(sizes)]:
        arena = HC.Arena(dev, sizes)
        p = {k: (arena.ptr(k) if k in given else None) for k in sizes}
        assert call(p) == 0, lib.mdil_spx_last_error()
        torch.cuda.synchronize()
        arena.read()
        arena.assert_untouched(list(given), given)
        for k in given:
            got = arena.cut(k).view(torch.int64) - SENTINEL
            w = want[k].reshape(-1) if isinstance(want[k], torch.Tensor) else torch.tensor([want[k]])
            assert torch.equal(got, w), (k, given)
    assert want["bad_targets"] > 0 and want["bad_ids"] > 0
    arena = HC.Arena(dev, sizes)
    every = {k: arena.ptr(k) for k in sizes}
    for p, kw, text in ((dict.fromkeys(sizes), {}, b"nothing to write"), (every, dict(nc_arg=33), b"nc=33"), (every, dict(K_arg=0), b"K=0"),
                        (every, dict(tgt=False), b"need a target"), (dict(every, table=every["table"] + 4), {}, b"alignment")):
        assert call(p, **kw) == -1 and text in lib.mdil_spx_last_error(), text
    torch.cuda.synchronize()
    arena.read()
    arena.assert_untouched([])
    side = HC.side_stream(lambda: P.spx_table(dl, dq, di, K, nc, dt, IGNORE))
    assert torch.equal(side[0].cpu(), want["table"]) and torch.equal(side[1].cpu(), want["tcount"])


@pytest.mark.parametrize("Wl", (5, 1001, 1024))
def test_apply_null_outputs_refusals_and_guard_bands(dev, Wl):
    from mdil_ss_amd import _spx_lib
    from mdil_ss_amd import superpixel as P
    lib = _spx_lib.load()
    nc, N, Hl, K = 20, 2, 5, 7
    _, target, previous, fill, label = AC.apply_maps(N, Hl, Wl, nc, AC.apply_seed(Hl, Wl))
    ids = id_maps((N, Hl, Wl), K, "beyond")
    selected, answer = region_maps(N, K, nc, Wl)
    want = R.apply_ref(ids, selected, nc, answer, target, previous, fill, label, IGNORE, 250)
    di, ds, da = ids.to(torch.int32).to(dev), selected.to(dev), answer.to(dev)
    dt, dp, df, dl = (t.to(dev) for t in (target, previous, fill, label))
    npix = N * Hl * Wl
    scalars = ("shown", "bad_targets", "wrong_shown", "wrong_all", "noisy", "bad_ids")
    sizes = {"out": npix, "mask": npix, "shown": 8, "annotated": nc * 8, "kept": nc * 8, "filled": nc * 8, "bad_targets": 8,
             "wrong_shown": 8, "wrong_all": 8, "noisy": 8, "bad_ids": 8}

    def call(p, nc_arg=nc, drop=250, tgt=True, lab=True, ans=True):
        return lib.mdil_spx_apply(di.data_ptr(), ds.data_ptr(), da.data_ptr() if ans else None, dt.data_ptr() if tgt else None,
                                  dp.data_ptr(), df.data_ptr(), dl.data_ptr() if lab else None, N, Hl, Wl, K, nc_arg, IGNORE, drop,
                                  *(p[k] for k in sizes), stream())

    combos = [(k,) for k in sizes] + [("out", "mask"), tuple(k for k in sizes if k not in ("out", "mask")), tuple(sizes)]
    for given in combos:
        arena = HC.Arena(dev, sizes)
        p = {k: (arena.ptr(k) if k in given else None) for k in sizes}
        assert call(p) == 0, lib.mdil_spx_last_error()
        torch.cuda.synchronize()
        arena.read()
        AC.check_arena(arena, given, want, scalars)
    assert want["wrong_shown"] > 0 and want["wrong_all"] > want["wrong_shown"] and want["noisy"] > 0 and want["bad_ids"] > 0
    arena = HC.Arena(dev, sizes)
    every = {k: arena.ptr(k) for k in sizes}
    for p, kw, text in ((dict.fromkeys(sizes), {}, b"nothing to write"), (every, dict(nc_arg=33), b"nc=33"),
                        (every, dict(drop=256), b"drop_id=256"), (every, dict(tgt=False), b"need a target"),
                        (every, dict(tgt=False, ans=False), b"annotated needs an answer or a target"),
                        (every, dict(lab=False), b"need a target and a label"),
                        (dict(every, out=every["out"] + 4), {}, b"alignment")):
        assert call(p, **kw) == -1 and text in lib.mdil_spx_last_error(), text
    torch.cuda.synchronize()
    arena.read()
    arena.assert_untouched([])
    side = HC.side_stream(lambda: P.spx_apply(di, ds, nc, da, dt, dp, df, dl, IGNORE, 250, want_mask=True))
    assert torch.equal(side[0].cpu(), want["out"]) and torch.equal(side[1].cpu(), want["mask"])


# ----------------------------------------------------------------------------- (5) end to end
STEP, ITER = 16, 3
CLI = AC.CLI_BASE + ["--subset", "val", "--step", str(STEP), "--iterations", str(ITER)]
REPORT_KEYS = ("dataset", "kind", "by", "answer", "step", "compactness", "iterations", "budget", "budget_is", "images", "total_pixels",
               "shown", "shown_share", "clicks", "superpixels", "superpixels_per_image", "empty_superpixels", "area_min",
               "area_median", "area_max", "nonfinite", "error_recall", "error_recall_chosen", "wrong_pixels", "achievable_accuracy",
               "noisy", "noisy_share", "noisy_applied", "annotated", "annotated_pixels", "given", "annotated_share_per_class",
               "kept", "filled", "written")

run_cli = functools.partial(AC.run_cli, "superpixel", CLI)


@functools.lru_cache(maxsize=None)
def composed():
    """What the command line must arrive at, from the reference: ids, table, tcount, answers of the 4 procedural images."""
    images, _, _, label, q = head_maps()
    ids = R.slic(images, STEP, 10, ITER)[0]
    Gy, Gx = R.grid(SIZE[0], SIZE[1], STEP)
    t = R.table_ref(label, q, ids, Gy * Gx, 20, synthetic_targets(), 19)
    return ids, t["table"], t["tcount"], Gy * Gx, Gx


def choose(by, budget, usable=None, seed=0):
    """acquire's own ranking on the reference's table -> the chosen (image, superpixel) pairs in rank order, pixels shown."""
    from mdil_ss_amd import acquire as A
    ids, table, tcount, K, Gx = composed()
    flat = table.reshape(-1, table.shape[-1])
    image_of, kidx = np.repeat(np.arange(N_IMAGES), K), np.tile(np.arange(K), N_IMAGES)
    scores = A.tile_scores(flat, by, image_of, kidx, seed, True).numpy()
    ok = flat[:, 0].numpy() > 0
    if usable is not None:
        ok &= usable
    order = A.rank_tiles(scores, image_of, kidx // Gx, kidx % Gx, ok)
    total = N_IMAGES * SIZE[0] * SIZE[1]
    chosen, spent = A.select_tiles(order, flat[:, 0].numpy(), image_of, [SIZE[0] * SIZE[1]] * N_IMAGES, budget * total)
    return [(int(image_of[i]), int(kidx[i])) for i in chosen], spent


def selection_pairs(selection):
    return [(int(stem[-4:]), row[0]) for stem, rows in selection["superpixels"].items() for row in rows]


def selected_map(pairs, K):
    sel = torch.zeros(N_IMAGES, K, dtype=torch.uint8)
    for i, k in pairs:
        sel[i, k] = 255
    return sel


@pytest.mark.parametrize("layout, by, answer", (("BDD", "ripu", "dominant"), ("cityscapes", "oracle", "exact")))
def test_cli_report_selection_and_label_tree(dev, checkpoint, tmp_path, layout, by, answer):
    from PIL import Image
    budget = 0.1
    report_file, root, out = tmp_path / "report.json", tmp_path / "round1", tmp_path / "maps"
    run_cli(checkpoint, ["--budget", budget, "--by", by, "--answer", answer, "--json", report_file, "--out-root", root, "--layout",
                         layout, "--out", out])
    with open(report_file) as f:
        saved = json.load(f)
    assert all(k in saved for k in REPORT_KEYS), [k for k in REPORT_KEYS if k not in saved]
    ids, table, tcount, K, Gx = composed()
    pairs, spent = choose(by, budget)
    with open(root / "selection.json") as f:
        selection = json.load(f)
    with open(out / "selection.json") as f:
        assert json.load(f) == selection
    assert (selection["step"], selection["compactness"], selection["iterations"], selection["size"], selection["answer"]) == \
        (STEP, 10, ITER, list(SIZE), answer)
    assert sorted(selection_pairs(selection)) == sorted(pairs) and len(pairs) > 0        # the report's selection is the reference's
    answers = R.dominant(tcount.reshape(-1, 20), 255).reshape(N_IMAGES, K)
    for stem, rows in selection["superpixels"].items():
        i = int(stem[-4:])
        for k, y, x, area, score, ans in rows:
            assert area == int(table[i, k, 0]) and 0 <= y < SIZE[0] and 0 <= x < SIZE[1]
            assert ans == (int(answers[i, k]) if answer == "dominant" else None)
    assert saved["clicks"] == len(pairs) and saved["shown"] == spent == saved["shown_applied"] <= budget * saved["total_pixels"]
    assert saved["superpixels_per_image"] == K and saved["superpixels"] == N_IMAGES * K and saved["nonfinite"] == 0
    areas = table[..., 0].reshape(-1)
    live = areas[areas > 0]
    assert (saved["empty_superpixels"], saved["area_min"], saved["area_max"]) == (int((areas == 0).sum()), int(live.min()), int(live.max()))
    assert saved["achievable_accuracy"] == R.achievable_accuracy(tcount)
    target = synthetic_targets()
    sel = selected_map(pairs, K)
    label = head_maps()[3]
    ref = R.apply_ref(ids, sel, 20, answers if answer == "dominant" else None, target, None, None, label, 19, 255)
    want = torch.where(ref["out"] == 19, torch.tensor(255, dtype=torch.uint8), ref["out"])
    assert torch.equal(read_tree(root, layout), want)                          # opened by the trainers' dataset class
    assert saved["annotated"] == ref["annotated"].tolist() and saved["noisy"] == saved["noisy_applied"] == ref["noisy"]
    assert saved["noisy_share"] == (ref["noisy"] / spent) and (ref["noisy"] > 0) == (answer == "dominant")
    assert saved["wrong_shown"] == ref["wrong_shown"] and saved["wrong_pixels"] == ref["wrong_all"]
    assert set(saved["error_recall"]) == {"uncertainty", "impurity", "ripu", "random", "oracle"}
    assert saved["error_recall_chosen"] == saved["error_recall"][by] == ref["wrong_shown"] / ref["wrong_all"]
    assert saved["given"] == torch.bincount(target[target != 19].long(), minlength=20).tolist()
    edges = R.edges(ids)
    for i in range(N_IMAGES):
        with Image.open(out / f"synthetic_{i:04d}_select.png") as im:
            assert torch.equal(torch.from_numpy(np.array(im)), ref["mask"][i])
        with Image.open(out / f"synthetic_{i:04d}_superpixels.png") as im:
            assert torch.equal(torch.from_numpy(np.array(im)), edges[i])
        with Image.open(out / f"synthetic_{i:04d}_uncertainty.png") as im:
            assert np.array(im).shape == SIZE


def test_cli_same_seed_same_bytes_and_previous_rounds(dev, checkpoint, tmp_path):
    budget = 0.1
    roots = [tmp_path / n for n in ("a", "b", "round2")]
    for root in roots[:2]:
        run_cli(checkpoint, ["--budget", budget, "--by", "random", "--seed", 3, "--out-root", root, "--layout", "BDD",
                             "--json", root / "report.json"])
    AC.assert_same_files(roots[0], roots[1], 2 * N_IMAGES + 2)
    with open(roots[0] / "selection.json") as f:
        first = json.load(f)
    ids, table, tcount, K, Gx = composed()
    one, _ = choose("random", budget, seed=3)
    assert sorted(selection_pairs(first)) == sorted(one)
    # round 2: the superpixels of round 1 leave the ranking, its labels are kept
    rep = run_cli(checkpoint, ["--budget", budget, "--by", "uncertainty", "--previous", roots[0] / "selection.json",
                               "--previous-root", roots[0], "--out-root", roots[2], "--layout", "BDD", "--json", tmp_path / "r2.json"])
    with open(roots[2] / "selection.json") as f:
        second = json.load(f)
    usable = np.ones(N_IMAGES * K, dtype=bool)
    for i, k in one:
        usable[i * K + k] = False
    two, spent = choose("uncertainty", budget, usable)
    assert sorted(selection_pairs(second)) == sorted(two) and not set(one) & set(two) and rep["shown"] == spent > 0
    target, answers = synthetic_targets(), R.dominant(tcount.reshape(-1, 20), 255).reshape(N_IMAGES, K)
    r1 = R.apply_ref(ids, selected_map(one, K), 20, answers, target, None, None, None, 19, 255)
    prev = torch.where(r1["out"] == 19, torch.tensor(255, dtype=torch.uint8), r1["out"])     # as the tree holds it
    r2 = R.apply_ref(ids, selected_map(two, K), 20, answers, target, prev, None, None, 19, 255)
    want = torch.where(r2["out"] == 19, torch.tensor(255, dtype=torch.uint8), r2["out"])
    assert torch.equal(read_tree(roots[0], "BDD"), prev) and torch.equal(read_tree(roots[2], "BDD"), want)
    assert rep["kept"] == r2["kept"].tolist() and sum(rep["kept"]) > 0
    # other SLIC parameters: the earlier selection names other regions and is refused
    with pytest.raises(RuntimeError, match="selected with"):
        AC.run_cli("superpixel", AC.CLI_BASE + ["--subset", "val", "--step", "8", "--iterations", str(ITER)], checkpoint,
                   ["--budget", budget, "--previous", roots[0] / "selection.json", "--json", tmp_path / "r3.json"])


def test_cli_vote_and_unlabelled_images(dev, checkpoint, tmp_path):
    from PIL import Image
    from mdil_ss_amd import fullres as FR
    root = tmp_path / "tree"
    run_cli(checkpoint, ["--budget", 0.1, "--by", "ripu", "--out-root", root, "--layout", "BDD"])      # writes the images
    rep = run_cli(checkpoint, ["--budget", 1, "--vote", "--out", tmp_path / "vote", "--json", tmp_path / "vote.json"])
    ids, table, tcount, K, Gx = composed()
    label, target = head_maps()[3], synthetic_targets()
    majority = R.dominant(table.reshape(-1, 24)[:, 4:], 255).reshape(N_IMAGES, K)
    voted = R.apply_ref(ids, torch.full((N_IMAGES, K), 255, dtype=torch.uint8), 20, majority)["out"]
    for i in range(N_IMAGES):
        with Image.open(tmp_path / "vote" / f"synthetic_{i:04d}_label.png") as im:
            assert torch.equal(torch.from_numpy(np.array(im)), voted[i])
    assert rep["pixels_changed"] == int((voted != label).sum()) > 0 and rep["images"] == N_IMAGES
    for name, pred in (("plain", label), ("voted", voted)):
        ok = target != 19
        m = torch.bincount(target[ok].long() * 20 + pred[ok].long(), minlength=400).reshape(20, 20).double()
        assert rep[f"miou_{name}"] == float(FR.iou_rule(20, 19, m.diagonal(), m.sum(0), m.sum(1))[0])
    # unlabelled: the images an earlier run wrote
    plain = AC.run_cli("superpixel", AC.images_base(root / "images" / "val"), checkpoint, [
        "--step", STEP, "--iterations", ITER, "--budget", "0.1", "--by", "ripu", "--out", tmp_path / "plain", "--json",
        tmp_path / "plain.json"])
    assert "error_recall" not in plain and "annotated" not in plain and "noisy" not in plain and plain["images"] == N_IMAGES
    assert 0 < plain["shown"] == plain["shown_applied"] <= 0.1 * plain["total_pixels"] and plain["clicks"] > 0
    with open(tmp_path / "plain" / "selection.json") as f:
        selection = json.load(f)
    assert sum(r[3] for rows in selection["superpixels"].values() for r in rows) == plain["shown"]
    assert all(r[5] is None for rows in selection["superpixels"].values() for r in rows)
    for stem in selection["superpixels"]:
        with Image.open(tmp_path / "plain" / f"{stem}_select.png") as im:
            assert int((torch.from_numpy(np.array(im)) == 255).sum()) == sum(r[3] for r in selection["superpixels"][stem])
        assert os.path.isfile(tmp_path / "plain" / f"{stem}_superpixels.png")
    assert len(glob.glob(str(tmp_path / "plain" / "*_uncertainty.png"))) == N_IMAGES
