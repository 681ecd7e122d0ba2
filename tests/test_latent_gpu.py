"""GPU: the exact t-SNE of libmdil_tsne.so (mdil_ss_amd/ext/tsne.hip) and mdil_ss_amd/latent.py
against the fp64 checker tests/tsne_reference.py.  Every bound below comes from the number formats
or from the checker's own behaviour on the CPU, never from what the kernels give.

Sizes: N = 2, 65, 193, 1000 -- no multiple of 16 or 64; 65 and 193 are odd (the 4-byte-load walk
of the sweep), 1000 a multiple of 4 (the 16-byte walk) with 4 column tiles and 32 row strips;
d = 1, 16, 20, 128.  One case at N = 16,400, the size at which the search's row passes 64 KB of LDS
and the sweep's row strip passes the 1,024 row points staged at a time."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import head_cases as HC
from tests import tsne_reference as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    return HC.device("latent-space")


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "tsne_small.npz"))


def dense(cond, n):
    P = np.zeros((n, n))
    P[np.triu_indices(n, 1)] = cond
    return P + P.T


def up(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(dev).contiguous()


def fresh(Y0, dev):
    Y = up(Y0, dev)
    return Y, torch.zeros_like(Y), torch.ones_like(Y)


# ------------------------------------------------------------------------------------- sqdist
@pytest.mark.parametrize("N,d", [(2, 1), (65, 16), (193, 20), (1000, 128), (193, 1), (65, 128)])
def test_sqdist_against_fp64(dev, N, d):
    """Each entry is d rounded differences, squared and summed in fp32: the worst case is a relative
    (d + 2) * 2^-24.  The diagonal is exactly 0 and D equals its transpose bit for bit."""
    from mdil_ss_amd import latent as L
    X = (3.0 * np.random.RandomState(N + d).randn(N, d)).astype(np.float32)
    D = L.sqdist(up(X, dev)).cpu().numpy()
    ref = R.sqdist(X)
    err = np.abs(D - ref) / np.where(ref > 0, ref, 1.0)
    print(f"N {N} d {d}: worst relative error {err.max():.3e} (bound {(d + 2) * U:.3e})")
    assert D.dtype == np.float32 and D.shape == (N, N)
    assert err.max() <= (d + 2) * U
    assert (np.diag(D) == 0).all()
    assert np.array_equal(D.view(np.uint32), D.T.view(np.uint32))


# --------------------------------------------------------------------------------- affinities
@functools.lru_cache(maxsize=None)
def affinity_case(N):
    X, _ = R.clusters(N, seed=N)
    D64 = R.sqdist(X)
    return D64, D64.astype(np.float32)


@functools.lru_cache(maxsize=None)
def rounding_shift(N, perplexity):
    """What rounding the distances to fp32 does to the checker itself: its own search on the
    rounded distances, then at ITS betas (largest entropy shift over the rows,
    sum |P(rounded) - P(exact)|)."""
    D64, D32 = affinity_case(N)
    betas, C32 = R.binary_search(D32.astype(np.float64), perplexity)
    H32, _ = R.entropies(D32.astype(np.float64), betas)
    H64, _ = R.entropies(D64, betas)
    dP = np.abs(R.joint(C32) - R.joint(R.conditional(D64, betas))).sum()
    return float(np.abs(H64 - H32).max()), float(dP)


@pytest.mark.parametrize("perplexity", [5, 30, 100])
@pytest.mark.parametrize("N", [193, 1000])
def test_affinities_against_fp64(dev, N, perplexity):
    """The kernel gets the fp64 distances rounded to fp32 (nothing else perturbs its input).

    (a) Per row, the entropy recomputed in fp64 from the fp64 distances at the RETURNED beta lies
    within 1e-5 + a of log(perplexity), a = 4 x the checker's largest entropy shift under that
    rounding (4 x: another summation order).  Shifts measured on the CPU (N, perplexity):
    (193, 5) 5.7e-7, (193, 30) 4.8e-8, (193, 100) 6.1e-9, (1000, 5) 6.5e-7, (1000, 30) 1.4e-7,
    (1000, 100) 4.5e-8 -- so a is 2.5e-8 ... 2.6e-6; a search that counts j = i or normalises wrongly
    misses by about 1 / perplexity.
    (b) sum |P_gpu - P_ref|, P_ref from the fp64 distances at the returned betas, stays within
    4 x the checker's own sum |dP| under the rounding (7.7e-8 ... 1.8e-7 for the six cases, except
    9.8e-9 for (193, 100)) + 2 * 2^-24: C and P are each stored in fp32, one rounding each of entries
    that sum to 1."""
    from mdil_ss_amd import latent as L
    D64, D32 = affinity_case(N)
    shift, dP = rounding_shift(N, perplexity)
    P, betas = L.affinities(up(D32, dev), perplexity)
    P, betas = P.cpu().numpy(), betas.cpu().numpy()
    assert P.dtype == np.float32 and betas.dtype == np.float64 and betas.shape == (N,)
    H, _ = R.entropies(D64, betas)
    miss = np.abs(H - np.log(perplexity)).max()
    ref = R.joint(R.conditional(D64, betas))
    diff = np.abs(P.astype(np.float64) - ref).sum()
    print(f"N {N} perplexity {perplexity}: entropy miss {miss:.3e} (1e-5 + {4 * shift:.3e}); "
          f"sum|dP| {diff:.3e} (bound {4 * dP + 2 * U:.3e}); betas {betas.min():.3g} .. {betas.max():.3g}")
    assert miss <= 1e-5 + 4 * shift
    assert diff <= 4 * dP + 2 * U
    assert np.array_equal(P.view(np.uint32), P.T.view(np.uint32))
    assert (np.diag(P) == 0).all()
    assert abs(P.astype(np.float64).sum() - 1.0) <= 1e-5
    assert P[~np.eye(N, dtype=bool)].min() >= 2.2e-16


def test_affinities_refuse_a_perplexity_of_n(dev):
    from mdil_ss_amd import latent as L
    with pytest.raises(RuntimeError, match="perplexity 65 must be at least 1 and less than the 65 points"):
        L.affinities(torch.zeros(65, 65, device=dev), 65)


# ----------------------------------------------------------------------------------- gradient
@functools.lru_cache(maxsize=None)
def gradient_case(N):
    """-> (P as the kernel gets it, fp32; two probes Y, fp32)."""
    X, _ = R.clusters(N, seed=N + 1)
    P = R.joint(R.binary_search(R.sqdist(X), 30)[1]).astype(np.float32)
    rs = np.random.RandomState(N)
    return P, [(s * rs.randn(N, 2)).astype(np.float32) for s in (1e-4, 10.0)]


@functools.lru_cache(maxsize=None)
def gradient_reference(N, probe, exaggeration):
    P, Ys = gradient_case(N)
    return R.kl_and_grad(P.astype(np.float64), Ys[probe], exaggeration)


@pytest.mark.parametrize("exaggeration", [12.0, 1.0])
@pytest.mark.parametrize("probe", [0, 1])
@pytest.mark.parametrize("N", [193, 1000])
def test_gradient_and_kl_of_one_iteration(dev, N, probe, exaggeration):
    """One iteration from update = 0, gains = 1 with learning_rate 1: no component is "inc", so
    every gain becomes fl(0.8) and update = -(fl(0.8) * grad): grad is read back as
    -update / fl(0.8), one more rounding.  Each component stays within
    2 (N + 16) 2^-24 * sum_j |term_ij| of the fp64 value (a sum of N signed terms plus the Z
    reduction, worst case); KL agrees at 1e-4 relative."""
    from mdil_ss_amd import latent as L
    P, Ys = gradient_case(N)
    kl, grad, absterm = gradient_reference(N, probe, exaggeration)
    Y, update, gains = fresh(Ys[probe], dev)
    log = L.run(up(P, dev), Y, update, gains, 1, exaggeration=exaggeration, learning_rate=1.0, kl_every=1)
    g08 = np.float64(np.float32(0.8))
    assert np.array_equal(gains.cpu().numpy(), np.full((N, 2), np.float32(0.8)))
    got = -update.cpu().numpy().astype(np.float64) / g08
    assert np.array_equal(Y.cpu().numpy(), Ys[probe] + update.cpu().numpy())          # one fp32 addition
    bound = 2 * (N + 16) * U * absterm
    worst = (np.abs(got - grad) / bound).max()
    kl_gpu, gn_gpu = (float(v) for v in log.cpu().numpy()[0])
    print(f"N {N} probe {probe} e {exaggeration}: worst error / bound {worst:.3e}; KL {kl_gpu:.6f} (fp64 {kl:.6f}); "
          f"|grad| {gn_gpu:.4e} (fp64 {np.sqrt((grad ** 2).sum()):.4e})")
    assert worst <= 1.0
    assert abs(kl_gpu - kl) <= 1e-4 * abs(kl)
    assert abs(gn_gpu - np.sqrt((grad ** 2).sum())) <= 1e-4 * np.sqrt((grad ** 2).sum())


def test_sizes_past_the_staging_strip_and_the_64_kb_row(dev):
    """N = 16,400 is the one size here at which the code takes other paths: a row of distances is
    65.6 KB (above the default limit for dynamic LDS in the search), and a row strip of the sweep is
    1,094 rows (above the 1,024 row points staged in LDS at a time, so the staging loop goes round
    twice).  The reference is the same formulas in fp64 torch on the device, from the kernel's own
    fp32 D and P: the entropy at the returned betas then differs from the search's only by the order
    of fp64 sums (1e-10 allowed), the gradient bound is the one of the test above."""
    from mdil_ss_amd import latent as L
    N, e = 16400, 12.0
    g = torch.Generator(device=dev).manual_seed(7)
    X = torch.randn(N, 4, device=dev, generator=g)
    D = L.sqdist(X)
    assert torch.equal(D, D.T) and bool((D.diagonal() == 0).all())
    P, betas = L.affinities(D, 30)
    Dd = D.double()
    p = torch.exp(-Dd * betas[:, None]).fill_diagonal_(0.0)
    S = p.sum(1)
    H = torch.log(S) + betas * (Dd * p).sum(1) / S
    miss = float((H - np.log(30)).abs().max())
    del Dd, p, D
    assert miss <= 1e-5 + 1e-10
    assert torch.equal(P, P.T) and bool((P.diagonal() == 0).all())
    assert abs(float(P.double().sum()) - 1.0) <= 1e-5
    Y0 = torch.randn(N, 2, device=dev, generator=g)
    Y, update, gains = Y0.clone(), torch.zeros_like(Y0), torch.ones_like(Y0)
    log = L.run(P, Y, update, gains, 1, exaggeration=e, learning_rate=1.0, kl_every=1)
    Yd = Y0.double()
    dx, dy = Yd[:, None, 0] - Yd[None, :, 0], Yd[:, None, 1] - Yd[None, :, 1]
    n = (1.0 / (1.0 + dx * dx + dy * dy)).fill_diagonal_(0.0)
    Z = n.sum()
    Pe = e * P.double()
    w = (Pe - n / Z) * n
    grad = 4.0 * torch.stack(((w * dx).sum(1), (w * dy).sum(1)), 1)
    m = Pe * n + n * n / Z
    absterm = 4.0 * torch.stack(((m * dx.abs()).sum(1), (m * dy.abs()).sum(1)), 1)
    kl = float(torch.xlogy(Pe, Pe / (n / Z).fill_diagonal_(1.0)).sum())
    got = -update.double() / float(np.float32(0.8))
    worst = float(((got - grad).abs() / (2 * (N + 16) * U * absterm)).max())
    kl_gpu = float(log[0, 0])
    print(f"N {N}: entropy miss {miss:.3e}; worst gradient error / bound {worst:.3e}; KL {kl_gpu:.6f} (fp64 {kl:.6f})")
    assert worst <= 1.0
    assert abs(kl_gpu - kl) <= 1e-4 * abs(kl)


def test_two_points(dev):
    """N = 2: one column tile, one strip, one valid lane pair.  p_01 = p_10 = 1/2; the gradient is
    4 (p - q) n (y_0 - y_1) with q = 1/2, so it vanishes whatever Y is."""
    from mdil_ss_amd import latent as L
    X = np.array([[0.0], [2.0]], dtype=np.float32)
    D = L.sqdist(up(X, dev))
    assert D.cpu().tolist() == [[0.0, 4.0], [4.0, 0.0]]
    P, betas = L.affinities(D, 1.0)
    assert P.cpu().tolist() == [[0.0, 0.5], [0.5, 0.0]]
    Y, update, gains = fresh(np.array([[0.0, 0.0], [3.0, 4.0]], dtype=np.float32), dev)
    log = L.run(P, Y, update, gains, 1, exaggeration=1.0, learning_rate=1.0, kl_every=1).cpu().numpy()
    assert np.abs(update.cpu().numpy()).max() <= 8 * U * (4 * 0.5 / 26 * 4)       # a few roundings of either term
    assert abs(float(log[0, 0])) <= 16 * U * 3.3             # ... of log n = -3.26, log Z = -2.56, p log p


# ------------------------------------------------------------------------ descent on p150 / kl450
@functools.lru_cache(maxsize=None)
def p150():
    g = golden()
    return dense(g["p150_P"], 150).astype(np.float32), R.random_init(150, 0)


def test_run_is_deterministic(dev):
    from mdil_ss_amd import latent as L
    P, Y0 = p150()
    out = []
    for _ in range(2):
        Y, update, gains = fresh(Y0, dev)
        log = L.run(up(P, dev), Y, update, gains, 60, kl_every=10)
        out.append((Y.cpu().numpy(), log.cpu().numpy(), update.cpu().numpy(), gains.cpu().numpy()))
    assert out[0][1].shape == (6, 2) and np.isfinite(out[0][0]).all() and np.isfinite(out[0][1]).all()
    for a, b in zip(*out):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_split_calls_equal_one_call(dev):
    """300 iterations in one call against 200 + 100 (first_iter = 200): the exaggeration / momentum
    switch at 250 falls inside the second call."""
    from mdil_ss_amd import latent as L
    P, Y0 = p150()
    Pd = up(P, dev)
    Y, update, gains = fresh(Y0, dev)
    log = L.run(Pd, Y, update, gains, 300, kl_every=50)
    Y2, update2, gains2 = fresh(Y0, dev)
    log_a = L.run(Pd, Y2, update2, gains2, 200, kl_every=50)
    log_b = L.run(Pd, Y2, update2, gains2, 100, first_iter=200, kl_every=50)
    for a, b in ((Y, Y2), (update, update2), (gains, gains2), (log, torch.cat([log_a, log_b]))):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))
    # and the switch is where it is said to be: a run that never leaves the first phase differs
    Y3, update3, gains3 = fresh(Y0, dev)
    L.run(Pd, Y3, update3, gains3, 300, exaggeration_iters=400, kl_every=50)
    assert not np.array_equal(Y.cpu().numpy(), Y3.cpu().numpy())


# Short trajectory: the checker's own float32 run against its float64 run, 20 iterations on p150
# from the seed-0 init at learning rate N / exaggeration = 12.5 (Belkina et al.'s rule; at 200 and at
# 50 these 150 points oscillate from the first iterations and the checker's two precisions end 31 and
# 0.25 apart, so a comparison there checks nothing).  Measured on the CPU: largest |Y32 - Y64| =
# 3.008e-08 at a largest |Y| of 1.765e-02.
TRAJECTORY_LR = 12.5
TRAJECTORY_SELF_DEVIATION = 3.008e-08


def test_short_trajectory_against_fp64(dev):
    from mdil_ss_amd import latent as L
    P, Y0 = p150()
    ref, ref_log, _ = R.descend(P.astype(np.float64), Y0, 20, learning_rate=TRAJECTORY_LR, kl_every=10)
    Y, update, gains = fresh(Y0, dev)
    log = L.run(up(P, dev), Y, update, gains, 20, learning_rate=TRAJECTORY_LR, kl_every=10).cpu().numpy()
    dev_max = np.abs(Y.cpu().numpy() - ref).max()
    print(f"largest |Y - Y64| {dev_max:.3e} (bound {10 * TRAJECTORY_SELF_DEVIATION:.3e}), |Y| up to {np.abs(ref).max():.3e}")
    assert dev_max <= 10 * TRAJECTORY_SELF_DEVIATION
    for (kl, gn), (kl_ref, gn_ref) in zip(log, ref_log):
        assert abs(kl - kl_ref) <= 1e-4 * abs(kl_ref)


@functools.lru_cache(maxsize=None)
def kl450_reference():
    """The checker from the seed-0 init, once: (final KL, purity)."""
    g = golden()
    P = R.joint(R.binary_search(R.sqdist(g["kl450_X"]), 30)[1])
    Y, log, _ = R.descend(P, R.random_init(450, 0), 500)
    return log[-1][0], R.purity(Y, g["kl450_labels"])


def test_end_to_end_on_three_clusters(dev):
    """kl450, 500 iterations from the seed-0 init through sqdist, affinities and run: the final KL is
    at most the checker's from the same init times (1 + 2 x the relative spread of sklearn's four
    seeds, 2.1 %, so 4.2 %), the nearest-neighbour cluster purity at least 0.99 (checker: 1.000)."""
    from mdil_ss_amd import latent as L
    g = golden()
    sk = g["kl450_kl"]
    spread = (sk.max() - sk.min()) / sk.min()
    ref_kl, ref_purity = kl450_reference()
    assert ref_purity == 1.0
    Y, log = L.tsne(up(g["kl450_X"], dev), perplexity=30, iterations=500, seed=0)
    log = log.cpu().numpy()
    purity = R.purity(Y.cpu().numpy(), g["kl450_labels"])
    print(f"final KL {log[-1, 0]:.4f} (checker {ref_kl:.4f}, sklearn {sk}), purity {purity:.3f}")
    assert log.shape == (10, 2) and np.isfinite(log).all()
    assert log[-1, 0] <= ref_kl * (1 + 2 * spread)
    assert purity >= 0.99


# ------------------------------------------------------------------------------------ latents
@pytest.fixture(scope="module")
def tiny_model(dev):
    return HC.tiny_model(dev)


def test_latents_are_the_models_own_tensors(dev, tiny_model):
    from mdil_ss_amd import latent as L
    from mdil_ss_amd import ops
    from oracle import fixtures as fx
    images, _ = fx.make_batch(2, 64, 128, 20, seed=100)
    images = images.to(dev)
    before = {k: v.clone() for k, v in tiny_model.state_dict().items()}
    for task in (0, 1):
        with torch.no_grad():
            want_pen = tiny_model.features(images, task)
            want_logits = tiny_model(images, task).permute(0, 2, 3, 1)
            want_enc = tiny_model.encoder.run(ops.to_nhwc(images), task, False, None)
        pen = L.latents(tiny_model, images, task, "penultimate")
        logits = L.latents(tiny_model, images, task, "logits")
        enc = L.latents(tiny_model, images, task, "encoder")
        assert tuple(enc.shape) == (2, 8, 16, 128) and tuple(pen.shape) == (2, 32, 64, 16)
        assert tuple(logits.shape) == (2, 64, 128, 20)
        for got, want in ((pen, want_pen), (logits, want_logits), (enc, want_enc)):
            assert got.is_contiguous() and not got.requires_grad and torch.equal(got, want)
        assert enc.view(-1, 128).shape == (256, 128)
    assert not tiny_model.training
    after = tiny_model.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)


def test_cli_end_to_end(dev, tiny_model, tmp_path, capsys):
    from PIL import Image

    from mdil_ss_amd import latent as L
    ckpt = tmp_path / "model_best.pth.tar"
    HC.save_checkpoint(tiny_model, ckpt)
    base = ["--state", str(ckpt), "--num-classes", "20", "20", "--task", "0", "--synthetic", "1", "--height", "64",
            "--width", "128"]
    enc = base + ["--layer", "encoder", "--perplexity", "5", "--iterations", "60"]
    p = L.build_parser()
    files = []
    for name in ("a", "b"):
        out = L.main(p.parse_args(enc + ["--out", str(tmp_path / name)]))
        assert [os.path.basename(f) for f in out["written"]] == ["synthetic_0000_encoder_tsne.npz",
                                                                  "synthetic_0000_encoder_tsne.png"]
        files.append([open(f, "rb").read() for f in out["written"]])
    assert files[0] == files[1]
    assert "final KL divergence" in capsys.readouterr().out
    z = np.load(tmp_path / "a" / "synthetic_0000_encoder_tsne.npz")
    assert z["Y"].shape == (128, 2) and z["Y"].dtype == np.float32 and np.isfinite(z["Y"]).all()
    assert z["labels"].shape == (128,) and z["kl_log"].shape == (1, 2) and '"layer": "encoder"' in str(z["arguments"])
    assert Image.open(tmp_path / "a" / "synthetic_0000_encoder_tsne.png").size == (1024, 1024)
    out = L.main(p.parse_args(base + ["--layer", "penultimate", "--points", "500", "--iterations", "100", "--out",
                                      str(tmp_path / "c")]))
    z = np.load(out["written"][0])
    assert z["Y"].shape == (500, 2) and np.isfinite(z["Y"]).all() and z["labels"].shape == (500,)
    assert np.array_equal(z["index"], L.sample_points(32 * 64, 500, 2))
    with pytest.raises(SystemExit):
        p.parse_args(enc[:-4] + ["--perplexity", "200", "--out", str(tmp_path / "d")])
