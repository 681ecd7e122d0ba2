"""GPU: the open-set kernels (mdil_ss_amd/ext/openset_head.hip) and the entry points over them
(mdil_ss_amd/openset.py), against tests/openset_reference.py and the fp64 head of tests/head_cases.py.

What is compared with what.  ``openset_head`` promises ``route_head``'s chain of operations, so its
label is ``predict_head``'s and its entropy code is the key of ``route_head``'s entropy map: both are
asserted bit for bit.  Independently every score is held to its fp64 definition: the code must lie
between the keys of u64 - tol and u64 + tol, tol per kind and case the larger of gamma_17 * max S (the
logit bound of the head tests) and 4 x the worst deviation of a plain float32 torch evaluation
(conv_transpose2d, logsumexp, softmax) from fp64 on the same case.  The test prints, per kind, how far
the kernel's codes lie from the fp64 score as a multiple of that float32 distance (for the entropy,
whose float route_head stores, the float's own distance).  On an MI355X the tolerance was the logit
bound in every case; the float32 torch distance was 1.9e-8 to 9.5e-6; the kernel's codes lay at most
0.26 of it outside their fp64 score's bin, and its entropy float 0.35 to 1.43 of it away (at most
0.96 with the weights times 8).  Everything after
the code is integer arithmetic and is asserted exactly, on the kernel's own maps."""
import functools
import glob
import json

import pytest
import torch

from tests import head_cases as HC
from tests import openset_reference as R
from tests.head_cases import CLASSES, SHAPES, nhwc

pytestmark = pytest.mark.gpu

K = 17
MAX_EXCLUDED = 1e-3
BIG = (3, 16, 48)
SCALE = 8.0                                     # the trained regime: logits 8 times as far apart
NPIX = (1, 3, 5, 1001, 1024)                    # 8 pixels per load: odd tails, a ragged and a whole size
HEAD_WG, HEAD_BLOCKS = 256, 768                 # openset_head.hip: kHeadWG, kHeadMaxBlocks
SENTINEL = torch.tensor([0xA5] * 8, dtype=torch.uint8).view(torch.int64)


@pytest.fixture(scope="module")
def dev():
    return HC.device("open-set")


def inputs(nc, shape, scale=1.0):
    x, w, b = HC.head_inputs(nc, shape)
    return x, (w * scale if scale != 1.0 else w), b


@functools.lru_cache(maxsize=None)
def reference(nc, shape, scale=1.0):
    """fp64 scores [4,N,2H,2W], the float32 torch evaluation's worst distance from them per kind, the
    logit bound gamma_17 * max S, and the near-tie mask.  Computed once, never modified."""
    x, w, b = inputs(nc, shape, scale)
    logits, S = HC.head64(x, w, b)
    u64 = R.scores64(logits)
    d32 = (R.scores32(x, w, b).double() - u64).abs().reshape(4, -1).max(1)[0]
    return u64, d32, HC.gamma(K) * float(S.max()), HC.near_tie(logits, S, K)


def new_hist(dev):
    return torch.zeros(4, 2, 65536, dtype=torch.int64, device=dev)


@functools.lru_cache(maxsize=None)
def device_run(nc, shape, scale=1.0):
    """openset_head once per map kind (the first call also counts all four histograms as group 0),
    predict_head and route_head on the same inputs -> host tensors and the device maps."""
    from mdil_ss_amd import openset as O
    from mdil_ss_amd.predict import predict_head
    from mdil_ss_amd.route import route_head
    dev = torch.device("cuda", 0)
    x, w, b = inputs(nc, shape, scale)
    xd, wd, bd = nhwc(x).to(dev), w.to(dev), b.to(dev)
    hist, nonf = new_hist(dev), torch.zeros(1, dtype=torch.int64, device=dev)
    label, first = O.openset_head(xd, wd, bd, map_kind=0, hist=hist, nonfinite=nonf)
    dcodes = [first] + [O.openset_head(xd, wd, bd, map_kind=k, want_label=False)[1] for k in (1, 2, 3)]
    plabel = predict_head(xd, wd, bd, None, False)[0]
    ent = route_head(xd, wd, bd, label=False, maps=True, scores=False)["ent"]
    torch.cuda.synchronize()
    return dict(label=label.cpu(), codes=torch.stack([O.code_values(c.cpu()) for c in dcodes]), hist=hist.cpu(),
                nonfinite=int(nonf.item()), plabel=plabel.cpu(), ent=ent.cpu(), dlabel=label, dcodes=dcodes,
                args=(xd, wd, bd))


# ------------------------------------------------------------------------------------- (1) bits
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nc", CLASSES)
def test_label_is_predict_heads_and_entropy_is_route_heads(dev, nc, shape):
    from mdil_ss_amd import openset as O
    run = device_run(nc, shape)
    npix = 4 * shape[0] * shape[1] * shape[2]
    assert run["label"].dtype == torch.uint8 and tuple(run["label"].shape) == (shape[0], 2 * shape[1], 2 * shape[2])
    assert torch.equal(run["label"], run["plabel"])
    assert torch.equal(run["codes"][3], O.key16(run["ent"]))
    assert run["nonfinite"] == 0
    assert int(run["codes"].min()) >= O.FINITE_CODES[0] and int(run["codes"].max()) <= O.FINITE_CODES[1]
    for k in range(4):
        want = R.hist_of(run["codes"][k], torch.zeros_like(run["codes"][k]))
        assert torch.equal(run["hist"][k], want), R.KINDS[k]
        assert int(run["hist"][k].sum()) == npix


# ---------------------------------------------------------------------------------- (2) fp64
def check_scores(nc, shape, scale):
    run = device_run(nc, shape, scale)
    u64, d32, logit_bound, excluded = reference(nc, shape, scale)
    what = f"nc {nc} shape {shape} scale {scale}"
    HC.share(MAX_EXCLUDED)(excluded, what)                          # a condition on the fp64 reference alone
    from mdil_ss_amd import openset as O
    keep = ~excluded
    for k, name in enumerate(R.KINDS):
        tol = max(logit_bound, 4.0 * float(d32[k]))
        lo, hi = R.key16((u64[k] - tol).float().numpy()), R.key16((u64[k] + tol).float().numpy())
        code = run["codes"][k]
        # the kernel's own distance, from the bins its codes name: at least floor - u64, at most next floor - u64
        floor = O.code_floor(code).double()
        nxt = O.code_floor(code + 1).double()
        away = torch.maximum(floor - u64[k], u64[k] - nxt).clamp(min=0)[keep].max().item()
        print(f"{what} {name}: tol {tol:.3e} (logit bound {logit_bound:.3e}, float32 torch {float(d32[k]):.3e}); the "
              f"kernel's codes are at least {away:.3e} away = {away / max(float(d32[k]), 1e-300):.2f} x float32 torch")
        if name == "entropy":                                       # its float is route_head's, bit for bit
            own = (run["ent"].double() - u64[k]).abs()[keep].max().item()
            print(f"{what} entropy: the kernel's float is {own:.3e} away = {own / max(float(d32[k]), 1e-300):.2f} x "
                  "float32 torch")
        assert bool(((code >= lo) & (code <= hi))[keep].all()), (what, name)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nc", CLASSES)
def test_scores_match_the_fp64_definitions(dev, nc, shape):
    check_scores(nc, shape, 1.0)


@pytest.mark.parametrize("nc", CLASSES)
def test_scores_in_the_trained_regime(dev, nc):
    check_scores(nc, BIG, SCALE)
    run = device_run(nc, BIG, SCALE)
    assert torch.equal(run["label"], run["plabel"]) and run["nonfinite"] == 0
    from mdil_ss_amd import openset as O
    assert torch.equal(run["codes"][3], O.key16(run["ent"]))


# ------------------------------------------------------------------------------ (3) integers
def lut_case(nc):
    """A look-up table that sends some ids to 0, some to 1 and some to ignored, and a target over it."""
    from mdil_ss_amd import openset as O
    unknown = [c for c in range(nc) if c % 3 == 1] + [nc]
    ignore = [c for c in range(nc) if c % 5 == 2 and c % 3 != 1]
    return O.group_lut(unknown, ignore)


@pytest.mark.parametrize("shape", ((1, 9, 7), BIG))
@pytest.mark.parametrize("nc", (2, 27))
def test_histograms_split_by_group(dev, nc, shape):
    from mdil_ss_amd import openset as O
    run = device_run(nc, shape)
    codes = run["codes"]
    lut = lut_case(nc)
    target = HC.make_target(nc, tuple(run["label"].shape), nc - 1, seed=nc + shape[1])
    groups = lut[target.long()].long()
    assert all(int((groups == g).sum()) > 0 for g in (0, 1)) and (nc == 2 or int((groups == 2).sum()) > 0)
    hist = new_hist(dev)
    O.openset_head(*run["args"], target=target.to(dev), lut=lut.to(dev), hist=hist, want_label=False)
    for k in range(4):
        assert torch.equal(hist[k].cpu(), R.hist_of(codes[k], groups)), R.KINDS[k]
        assert int(hist[k].sum()) == int((groups < 2).sum())
    for g in (0, 1, 2):
        hist = new_hist(dev)
        O.openset_head(*run["args"], const_group=g, hist=hist, want_label=False)
        for k in range(4):
            assert torch.equal(hist[k].cpu(), R.hist_of(codes[k], torch.full_like(codes[k], g)))
        assert int(hist.sum()) == (0 if g == 2 else 4 * codes[0].numel())
    # one kind: the other rows keep what they held
    for kind in (0, 2):
        hist = torch.full((4, 2, 65536), 7, dtype=torch.int64, device=dev)
        O.openset_head(*run["args"], target=target.to(dev), lut=lut.to(dev), kinds=[R.KINDS[kind]], hist=hist,
                       want_label=False)
        got = hist.cpu() - 7
        assert torch.equal(got[kind], R.hist_of(codes[kind], groups))
        assert int(got.sum()) == int(got[kind].sum())


# ------------------------------------------------------------------------------- (4) crowding
def crowded_run(dev, nc, shape, x, target=None, lut=None):
    from mdil_ss_amd import openset as O
    _, w, b = inputs(nc, shape)
    w = w[:, :, :1, :1].expand(-1, -1, 2, 2).contiguous()           # one weight for the four parities
    hist = new_hist(dev)
    maps = [O.code_values(O.openset_head(nhwc(x).to(dev), w.to(dev), b.to(dev), target=target, lut=lut, map_kind=k,
                                         hist=hist if k == 0 else None, want_label=False)[1].cpu()) for k in range(4)]
    return hist.cpu(), torch.stack(maps)


@pytest.mark.parametrize("shape", ((1, 9, 7), (2, 12, 20), BIG))
def test_crowded_bins(dev, shape):
    """The inputs on which a merge inside the wave goes wrong: every lane in one bin, lanes that
    alternate between two bins, and one bin whose lanes alternate between the groups."""
    from mdil_ss_amd import openset as O
    nc = 20
    N, H, W = shape
    npix = 4 * N * H * W
    hist, codes = crowded_run(dev, nc, shape, torch.zeros(N, 16, H, W))
    for k in range(4):
        c = int(codes[k].reshape(-1)[0])
        assert bool((codes[k] == c).all()) and int(hist[k, 0, c]) == npix and int(hist[k].sum()) == npix
    x = torch.zeros(N, 16, H, W)
    x[:, :, :, 1::2] = 1.5                                          # neighbouring lanes differ
    hist, codes = crowded_run(dev, nc, shape, x)
    for k in range(4):
        assert torch.equal(hist[k], R.hist_of(codes[k], torch.zeros_like(codes[k])))
        assert 1 <= int((hist[k, 0] > 0).sum()) <= 2 and int(hist[k].sum()) == npix
    assert any(int((hist[k, 0] > 0).sum()) == 2 for k in range(4))
    lut = O.group_lut([1], [2]).to(dev)
    for pattern in ("by lane", "by pixel", "thirds"):
        target = torch.zeros(N, 2 * H, 2 * W, dtype=torch.uint8)
        if pattern == "by lane":
            target[:, :, 2::4] = 1
            target[:, :, 3::4] = 1
        elif pattern == "by pixel":
            target[:, :, 1::2] = 1
        else:
            target.reshape(-1)[1::3] = 1
            target.reshape(-1)[2::3] = 2
        hist, codes = crowded_run(dev, nc, shape, torch.zeros(N, 16, H, W), target.to(dev), lut)
        for k in range(4):
            c = int(codes[k].reshape(-1)[0])
            for g in (0, 1):
                assert int(hist[k, g, c]) == int((target == g).sum()), (pattern, k, g)
            assert int(hist[k].sum()) == int((target < 2).sum())


# --------------------------------------------------------------- (5) accumulation, side effects
def test_histogram_accumulates_and_runs_repeat(dev):
    from mdil_ss_amd import openset as O
    nc = 27
    run = device_run(nc, BIG)
    hist, nonf = new_hist(dev), torch.zeros(1, dtype=torch.int64, device=dev)
    for n in (1, 2):
        label, code = O.openset_head(*run["args"], map_kind="energy", hist=hist, nonfinite=nonf, want_label=(n == 1))
        assert (label is None) == (n == 2)
        assert torch.equal(hist.cpu(), n * run["hist"]) and int(nonf.item()) == 0
        assert torch.equal(HC.as_bytes(code.cpu()), HC.as_bytes(run["dcodes"][2].cpu()))


def _raw_head(dev, nc, shape, given):
    from mdil_ss_amd import _openset_lib
    lib = _openset_lib.load()
    xd, wd, bd = device_run(nc, shape)["args"]
    N, H, W = shape
    npx = N * 4 * H * W
    arena = HC.Arena(dev, {"label": npx, "code": 2 * npx, "hist": 4 * 2 * 65536 * 8, "nonfinite": 8})
    p = {k: (arena.ptr(k) if k in given else None) for k in ("label", "code", "hist", "nonfinite")}
    rc = lib.mdil_openset_head(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), N, H, W, nc, None, None, 0, 15,
                               1 if "code" in given else -1, p["label"], p["code"], p["hist"], p["nonfinite"],
                               torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mdil_openset_last_error()
    torch.cuda.synchronize()
    arena.read()
    return arena


@pytest.mark.parametrize("shape", ((1, 1, 1), (1, 9, 7), BIG))
def test_head_null_outputs_and_guard_bands_stay_untouched(dev, shape):
    """Each output alone, then all of them: what was not given keeps its sentinel bytes, and so do the
    guard bands.  The counters are ADDED to: they start from the sentinel 0xA5A5A5A5A5A5A5A5."""
    nc = 27
    run = device_run(nc, shape)
    for given in (("label",), ("code",), ("hist",), ("nonfinite",), ("label", "code", "hist", "nonfinite")):
        arena = _raw_head(dev, nc, shape, given)
        written = [k for k in given if k != "nonfinite"]            # no NaN: nonfinite is never touched
        arena.assert_untouched(written, given)
        if "label" in given:
            assert torch.equal(arena.cut("label"), run["label"].reshape(-1))
        if "code" in given:
            assert torch.equal(arena.cut("code").view(torch.int16).long() & 0xffff, run["codes"][1].reshape(-1))
        if "hist" in given:
            assert torch.equal(arena.cut("hist").view(torch.int64).reshape(4, 2, 65536) - SENTINEL, run["hist"])


def test_head_grid_stride_loop_past_the_grid_bound(dev):
    """The grid is bounded at 768 work-groups of 256 feature pixels; 1 x 385 x 511 = 196,735 of them sends
    127 pixels (one whole wave and a ragged one) round the loop a second time, into a work-group's
    table that already holds counts.  Two classes; the integer contracts and the bit identities only."""
    from mdil_ss_amd import openset as O
    nc, shape = 2, (1, 385, 511)
    assert HEAD_WG * HEAD_BLOCKS < shape[1] * shape[2] < 2 * HEAD_WG * HEAD_BLOCKS
    assert (shape[1] * shape[2] - HEAD_WG * HEAD_BLOCKS) % 64 == 63
    run = device_run(nc, shape)
    assert torch.equal(run["label"], run["plabel"]) and torch.equal(run["codes"][3], O.key16(run["ent"]))
    lut = O.group_lut([1], [2])
    target = HC.make_target(3, tuple(run["label"].shape), 2, seed=7)      # ids 0, 1, 2 and a few 3 / 200 (known)
    groups = lut[target.long()].long()
    hist = new_hist(dev)
    O.openset_head(*run["args"], target=target.to(dev), lut=lut.to(dev), hist=hist, want_label=False)
    for k in range(4):
        assert torch.equal(run["hist"][k], R.hist_of(run["codes"][k], torch.zeros_like(run["codes"][k])))
        assert torch.equal(hist[k].cpu(), R.hist_of(run["codes"][k], groups)), R.KINDS[k]


def test_side_stream_gives_the_same_bytes(dev):
    from mdil_ss_amd import openset as O
    nc = 27
    run = device_run(nc, BIG)
    lut = lut_case(nc).to(dev)
    target = HC.make_target(nc, tuple(run["label"].shape), nc - 1, seed=3).to(dev)
    cdf = (torch.arange(65536) // 256).to(torch.uint8).to(dev)

    def everything():
        hist = new_hist(dev)
        label, code = O.openset_head(*run["args"], target=target, lut=lut, map_kind=2, hist=hist)
        counters = O.new_apply_counters(nc, dev)
        thr = int(O.code_values(code).median().item())
        out, score = O.openset_apply(label, code, nc, thr, None, 255, cdf, target, lut, counters)
        return [label, code, hist, out, score] + [counters[k] for k in O.APPLY_COUNTERS]

    first = everything()
    torch.cuda.synchronize()
    second = HC.side_stream(everything)
    for a, c in zip(first, second):
        assert torch.equal(HC.as_bytes(a.cpu()), HC.as_bytes(c.cpu()))
    assert torch.equal(first[0].cpu(), run["label"])


# ------------------------------------------------------------------------------------ (6) NaN
def test_a_nan_feature_is_counted_and_enters_no_histogram(dev):
    from mdil_ss_amd import openset as O
    nc, shape = 20, (2, 12, 20)
    x, w, b = inputs(nc, shape)
    xn = x.clone()
    xn[1, 9, 5, 7] = float("nan")                                   # one feature: its four output pixels
    clean = device_run(nc, shape)
    hit = torch.zeros_like(clean["codes"][0], dtype=torch.bool)
    hit[1, 10:12, 14:16] = True
    for k in range(4):
        hist, nonf = new_hist(dev), torch.zeros(1, dtype=torch.int64, device=dev)
        _, code = O.openset_head(nhwc(xn).to(dev), w.to(dev), b.to(dev), map_kind=k, hist=hist, nonfinite=nonf,
                                 want_label=False)
        code = O.code_values(code.cpu())
        assert int(nonf.item()) == 4 and bool((code[hit] == O.NONFINITE_CODE).all())
        assert torch.equal(code[~hit], clean["codes"][k][~hit])
        for j in range(4):
            assert int(hist[j].sum()) == code.numel() - 4 and int(hist[j, :, O.NONFINITE_CODE].sum()) == 0
        assert torch.equal(hist[k].cpu(), R.hist_of(code, hit.long() * 2))


# ---------------------------------------------------------------------------------- (7) apply
@pytest.mark.parametrize("npix", NPIX + (None,))
@pytest.mark.parametrize("nc", (2, 20, 32))
def test_apply_maps_and_counters(dev, nc, npix):
    from mdil_ss_amd import openset as O
    run = device_run(nc, BIG)
    n = run["label"].numel() if npix is None else npix
    hl, hc_ = run["label"].reshape(-1)[:n].clone(), run["codes"][2].reshape(-1)[:n]
    if n > 100:                                                     # some labels outside the head
        hl[torch.rand(n, generator=torch.Generator().manual_seed(n)) < 0.02] = nc + 3
    dl, dc = hl.to(dev), run["dcodes"][2].reshape(-1)[:n]
    ids = HC.random_luts(nc)[0]
    lut = lut_case(nc)
    target = HC.make_target(nc, (n,), nc - 1, seed=nc + n)
    known = torch.bincount(run["codes"][2].reshape(-1), minlength=65536)
    cdf = O.cdf_lut(known)
    middle = int(run["codes"][2].reshape(-1).median())
    for thr in (0, middle, 65536):
        want = R.apply_rule(hl, hc_, nc, thr, ids, 254, cdf, target, lut)
        counters = O.new_apply_counters(nc, dev)
        for times in (1, 2):
            out, score = O.openset_apply(dl, dc, nc, thr, ids.to(dev), 254, cdf.to(dev), target.to(dev), lut.to(dev),
                                         counters)
            assert out.dtype == torch.uint8 and torch.equal(out.cpu(), want["out"])
            assert score.dtype == torch.uint8 and torch.equal(score.cpu(), want["score"])
            for k in ("seen", "rejected", "detect", "confusion"):
                assert torch.equal(counters[k].cpu(), times * want[k]), (k, thr)
            for k in ("bad_targets", "bad_labels"):
                assert int(counters[k].item()) == times * want[k], (k, thr)
        if thr == 0:
            assert torch.equal(want["rejected"], want["seen"]) and int(want["confusion"].sum()) == 0
        if thr == 65536:
            assert int(want["rejected"].sum()) == 0
    if npix is None:
        assert want["bad_labels"] > 0 and want["bad_targets"] > 0 and int(want["confusion"].sum()) > 0
        mid = R.apply_rule(hl, hc_, nc, middle, ids, 254, cdf, target, lut)
        assert 0 < int(mid["rejected"].sum()) < int(mid["seen"].sum()) and int(mid["detect"].min()) > 0
    # no id_map, no target, no score, a subset of the counters: the identity map, nothing else touched
    some = {"rejected": torch.zeros(nc, dtype=torch.int64, device=dev)}
    plain = R.apply_rule(hl, hc_, nc, middle, None, 255)
    out, score = O.openset_apply(dl, dc, nc, middle, counters=some)
    assert score is None and torch.equal(out.cpu(), plain["out"]) and torch.equal(some["rejected"].cpu(), plain["rejected"])


@pytest.mark.parametrize("npix", (5, 1001, 1024))
def test_apply_null_outputs_and_guard_bands_stay_untouched(dev, npix):
    from mdil_ss_amd import _openset_lib
    from mdil_ss_amd import openset as O
    lib = _openset_lib.load()
    nc = 20
    run = device_run(nc, BIG)
    dl, dc = run["dlabel"].reshape(-1), run["dcodes"][2].reshape(-1)
    hl, hc_ = run["label"].reshape(-1)[:npix], run["codes"][2].reshape(-1)[:npix]
    lut, target = lut_case(nc), HC.make_target(nc, (npix,), nc - 1, seed=npix)
    cdf = O.cdf_lut(torch.bincount(run["codes"][2].reshape(-1), minlength=65536))
    thr = int(run["codes"][2].reshape(-1).median())
    tables = dict(lut=lut.to(dev), target=target.to(dev), cdf=cdf.to(dev))
    sizes = {"out": npix, "score": npix, "seen": nc * 8, "rejected": nc * 8, "detect": 32, "confusion": nc * nc * 8,
             "bad_targets": 8, "bad_labels": 8}
    want = R.apply_rule(hl, hc_, nc, thr, None, 255, cdf, target, lut)
    for given in (("out",), ("score",), ("seen", "rejected"), tuple(sizes)):
        arena = HC.Arena(dev, sizes)
        p = {k: (arena.ptr(k) if k in given else None) for k in sizes}
        with_target = "confusion" in given
        rc = lib.mdil_openset_apply(dl.data_ptr(), dc.data_ptr(), npix, nc, thr, None, 255,
                                    tables["cdf"].data_ptr() if "score" in given else None,
                                    tables["target"].data_ptr() if with_target else None,
                                    tables["lut"].data_ptr() if with_target else None, p["out"], p["score"], p["seen"],
                                    p["rejected"], p["detect"], p["confusion"], p["bad_targets"], p["bad_labels"],
                                    torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.mdil_openset_last_error()
        torch.cuda.synchronize()
        arena.read()
        changed = [k for k in given if k in ("out", "score", "seen", "rejected", "detect", "confusion")]
        if with_target and want["bad_targets"]:
            changed.append("bad_targets")
        arena.assert_untouched(changed, given)
        for k in ("out", "score"):
            if k in given:
                assert torch.equal(arena.cut(k), want[k])
        for k in ("seen", "rejected", "detect", "confusion"):
            if k in given:
                assert torch.equal(arena.cut(k).view(torch.int64) - SENTINEL, want[k].reshape(-1)), k


# ----------------------------------------------------------------------------- (8) end to end
@pytest.fixture(scope="module")
def tiny_model(dev):
    return HC.tiny_model(dev)


@pytest.fixture(scope="module")
def checkpoint(tiny_model, tmp_path_factory):
    path = tmp_path_factory.mktemp("openset") / "checkpoint.pth.tar"
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


def check_report_metrics(kinds, hist):
    """Every figure of the report against the reference's Fractions of the given histograms."""
    for k, name in enumerate(R.KINDS):
        got, want = kinds[name], R.metrics(hist[k])
        assert torch.equal(saved_table(got), hist[k]), name
        for key in ("auroc", "fpr_at_tpr", "tie_mass"):
            assert got[key] == float(want[key]), (name, key)
        assert abs(got["aupr"] - float(want["aupr"])) <= 4 * 2.0 ** -53
        assert (got["threshold_code"], got["P"], got["N"]) == (want["threshold_code"], want["P"], want["N"])


def test_cli_score_report(dev, tiny_model, checkpoint, tmp_path):
    from mdil_ss_amd import openset as O
    report_file = tmp_path / "report.json"
    O.main(O.build_parser().parse_args(["--state", checkpoint] + CLI + ["--score", "--json", str(report_file)]))
    with open(report_file) as f:
        saved = json.load(f)
    images, target = synthetic(dev, 4, 1)
    meter = O.OpenSetMeter(20, O.KINDS, O.group_lut([19]))
    for i in (0, 3):
        meter.add(tiny_model, images[i:i + 3], 1, target=target[i:i + 3].to(dev))
    hist = meter.hist()
    unknown = int((target == 19).sum())
    assert 0 < unknown < target.numel()                            # the procedural labels hold the void class
    assert saved["images"] == 4 and saved["pixels"] == target.numel() and saved["nonfinite"] == 0
    assert saved["unknown_ids"] == [19] and sorted(saved["kinds"]) == sorted(R.KINDS)
    check_report_metrics(saved["kinds"], hist)
    for name in R.KINDS:
        assert (saved["kinds"][name]["P"], saved["kinds"][name]["N"]) == (unknown, target.numel() - unknown)


def test_cli_foreign_domain(dev, tiny_model, checkpoint, tmp_path):
    from mdil_ss_amd import openset as O
    report_file = tmp_path / "foreign.json"
    O.main(O.build_parser().parse_args(["--state", checkpoint] + CLI + ["--score", "--json", str(report_file),
                                                                       "--foreign-synthetic", "2", "--foreign-task", "0"]))
    with open(report_file) as f:
        saved = json.load(f)
    images, target = synthetic(dev, 4, 1)
    foreign, _ = synthetic(dev, 2, 0)
    meter = O.OpenSetMeter(20, O.KINDS, O.group_lut([], [19]))
    for i in (0, 3):
        meter.add(tiny_model, images[i:i + 3], 1, target=target[i:i + 3].to(dev))
    meter.add(tiny_model, foreign, 1, const_group=O.UNKNOWN)
    assert saved["foreign_images"] == 2 and saved["pixels"] == 6 * 64 * 128
    check_report_metrics(saved["kinds"], meter.hist())
    for name in R.KINDS:
        assert saved["kinds"][name]["P"] == 2 * 64 * 128 and saved["kinds"][name]["N"] == int((target != 19).sum())


def test_cli_fit_then_reject_maps(dev, tiny_model, checkpoint, tmp_path):
    from mdil_ss_amd import boundary as B
    from mdil_ss_amd import openset as O
    fit_file, out = tmp_path / "thresholds.json", tmp_path / "maps"
    fitted = O.main(O.build_parser().parse_args(["--state", checkpoint] + CLI + ["--fit", str(fit_file), "--known-fpr",
                                                                                  "0.05"]))
    images, target = synthetic(dev, 4, 1)
    known = target != 19
    for name in R.KINDS:
        k = fitted["kinds"][name]
        assert k["known_pixels"] == int(known.sum()) and k["rejected_known"] <= 0.05 * k["known_pixels"]
    report = O.main(O.build_parser().parse_args(["--state", checkpoint] + CLI + [
        "--threshold", str(fit_file), "--kind", "maxlogit", "--out", str(out), "--unknown-id", "254", "--colour"]))
    assert len(glob.glob(str(out / "*_label.png"))) == 4 and len(report["written"]) == 12
    thr = fitted["kinds"]["maxlogit"]["threshold_code"]         # the kind that spreads on an untrained head
    meter = O.OpenSetMeter(20, ["maxlogit"])
    plain, rejected = [], []
    for i in range(4):
        got = torch.from_numpy(B.read_label_png(str(out), f"synthetic_{i:04d}", (64, 128)))   # boundary's reader opens it
        label, code = meter.add(tiny_model, images[i:i + 1], 1, const_group=O.IGNORED, map_kind="maxlogit", want_label=True)
        rej = O.code_values(code.cpu())[0] >= thr
        want = torch.where(rej, torch.tensor(254, dtype=torch.uint8), label.cpu()[0])
        assert torch.equal(got, want)
        from PIL import Image
        with Image.open(out / f"synthetic_{i:04d}_unknown.png") as im:
            assert im.mode == "L" and im.size == (128, 64)
        rejected.append(rej)
        plain.append(label.cpu()[0])
    rejected = torch.stack(rejected)
    share = rejected[known].double().mean().item()
    print(f"rejected share of the known pixels of the fitted set: {share:.4f}")
    assert 0 < share <= 0.05 and int(rejected[known].sum()) == fitted["kinds"]["maxlogit"]["rejected_known"]
    assert report["rejected"] == torch.bincount(torch.stack(plain)[rejected].long(), minlength=20).tolist()
    assert report["seen"] == torch.bincount(torch.stack(plain).reshape(-1).long(), minlength=20).tolist()
