"""CPU: the latent-space add-on (include/mdil_tsne.h, mdil_ss_amd/latent.py) -- the library exports
exactly what its header declares, the fp64 checker (tests/tsne_reference.py) against what
scikit-learn recorded in tests/golden/tsne_small.npz, the refusals, and the host-side functions."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import tsne_reference as R
from tests.helpers import declared_names, dynamic_exports

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "tsne_small.npz"))


def _dense(cond, n):
    P = np.zeros((n, n))
    P[np.triu_indices(n, 1)] = cond
    return P + P.T


# ------------------------------------------------------------------------------------------ ABI
def test_library_exports_exactly_the_declared_symbols():
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _tsne_lib
    lib = _tsne_lib.load()
    names = declared_names("mdil_tsne.h")
    assert names == ["mdil_tsne_affinities", "mdil_tsne_last_error", "mdil_tsne_run", "mdil_tsne_sqdist",
                     "mdil_tsne_version", "mdil_tsne_workspace_bytes"]
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/mdil_tsne.h but not exported"
    assert sorted(_tsne_lib.EXPORTS) == names
    assert dynamic_exports(_tsne_lib.LIB_PATH) == names
    assert lib.mdil_tsne_version() >= 100
    # the ctypes signatures carry as many arguments as the prototypes
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mdil_tsne.h")).read(), flags=re.S)
    for name, args in re.findall(r"\b(mdil_tsne_[a-z_]+)\s*\(([^)]*)\)\s*;", hdr):
        n_args = 0 if args.strip() == "void" else len(args.split(","))
        assert len(getattr(lib, name).argtypes) == n_args, name
    assert (_tsne_lib.MAX_POINTS, _tsne_lib.MAX_DIM) == (32768, 128)
    for macro, value in (("MDIL_TSNE_MAX_POINTS", 32768), ("MDIL_TSNE_MAX_DIM", 128)):
        assert re.search(rf"#define {macro} {value}\b", hdr)


def test_library_refuses_bad_arguments_without_a_device():
    """Argument checks come before any launch: sizes, perplexity, NULL pointers, alignment, overlap."""
    from mdil_ss_amd import _tsne_lib
    lib = _tsne_lib.load()
    err = lib.mdil_tsne_last_error
    assert lib.mdil_tsne_workspace_bytes(1) == -1 and lib.mdil_tsne_workspace_bytes(32769) == -1
    assert lib.mdil_tsne_workspace_bytes(8192) >= 32 * 8192 * 16
    for (X, N, d, D), text in (((4096, 32769, 4, 8192), b"N=32769"), ((4096, 1, 4, 8192), b"N=1 "),
                               ((4096, 10, 129, 8192), b"d=129"), ((4096, 10, 0, 8192), b"d=0"),
                               ((None, 10, 4, 8192), b"bad argument"), ((4096, 10, 4, None), b"bad argument")):
        assert lib.mdil_tsne_sqdist(X, N, d, D, None) == -1
        assert text in err(), (text, err())
    big = 1 << 40
    for (D, N, perp, beta, P, ws), text in (((4096, 10, 10.0, 8192, big, 16384), b"perplexity=10"),
                                            ((4096, 10, 0.5, 8192, big, 16384), b"perplexity=0.5"),
                                            ((4096, 10, float("nan"), 8192, big, 16384), b"perplexity"),
                                            ((4096, 40000, 5.0, 8192, big, 16384), b"N=40000"),
                                            ((4100, 10, 5.0, 8192, big, 16384), b"alignment"),
                                            ((4096, 10, 5.0, 8192, 4096 + 16, 16384), b"overlap"),
                                            ((4096, 10, 5.0, None, big, 16384), b"bad argument"),
                                            ((4096, 10, 5.0, 8192, big, None), b"bad argument")):
        assert lib.mdil_tsne_affinities(D, N, perp, beta, P, ws, None) == -1
        assert text in err(), (text, err())

    def run(P=4096, N=10, Y=8192, u=12288, g=16384, iters=5, first=0, ex_iters=250, ex=12.0, lr=200.0, every=5,
            log=20480, ws=1 << 20):
        return lib.mdil_tsne_run(P, N, Y, u, g, iters, first, ex_iters, ex, lr, every, log, ws, None)
    for kw, text in ((dict(N=1), b"N=1 "), (dict(N=32769), b"N=32769"), (dict(P=None), b"bad argument"),
                     (dict(iters=-1), b"bad argument"), (dict(first=-1), b"bad argument"), (dict(log=None), b"kl_log"),
                     (dict(lr=0.0), b"learning_rate"), (dict(ex=-1.0), b"exaggeration"), (dict(P=4100), b"alignment"),
                     (dict(Y=8196), b"alignment"), (dict(ws=(1 << 20) + 8), b"alignment")):
        assert run(**kw) == -1, kw
        assert text in err(), (kw, err())
    assert run(iters=0) == 0                      # nothing to enqueue


# ------------------------------------------------------------------ the checker against sklearn
def test_reference_joint_probabilities_match_sklearn(golden):
    """sklearn rounds the distances to fp32 before its search; so does this call.  1e-9 absolute is
    fp64 rounding of entries of about 1e-4 with room for sklearn's fp32 conditional matrix."""
    D = R.sqdist(golden["p150_X"]).astype(np.float32)
    betas, C = R.binary_search(D, 20)
    P = R.joint(C)
    assert np.abs(R.condensed(P) - golden["p150_P"]).max() <= 1e-9
    # the clamp at eps lifts the sum by at most eps per entry
    assert abs(P.sum() - 1.0) <= 150 * 150 * R.EPS + 1e-13 and (P == P.T).all() and (np.diag(P) == 0).all()
    H, _ = R.entropies(D, betas)
    assert np.abs(H - np.log(20)).max() <= 1e-5


@pytest.mark.parametrize("probe", [0, 1])
def test_reference_kl_and_gradient_match_sklearn(golden, probe):
    P = _dense(golden["p150_P"], 150)
    kl, grad, absterm = R.kl_and_grad(P, golden[f"p150_Y{probe}"])
    want_kl, want_grad = float(golden[f"p150_kl{probe}"]), golden[f"p150_grad{probe}"]
    assert abs(kl - want_kl) <= 1e-10 * abs(want_kl)
    assert np.abs(grad - want_grad).max() <= 1e-9 * np.abs(want_grad).max()
    assert (absterm >= np.abs(grad) * (1 - 1e-12)).all()
    # the float32 spelling of the same code stays close
    kl32, grad32, _ = R.kl_and_grad(P, golden[f"p150_Y{probe}"], dtype=np.float32)
    assert abs(kl32 - want_kl) <= 1e-4 * abs(want_kl)
    assert np.abs(grad32 - want_grad).max() <= 1e-4 * np.abs(want_grad).max()


def test_reference_descent_ends_where_sklearn_does(golden):
    """500 iterations from the seed-0 init on kl450: the final KL lies within the spread of
    sklearn's four seeds (2.1 %) of sklearn's seed-0 value, and every point's nearest neighbour is
    of its own cluster."""
    X, labels, sk = golden["kl450_X"], golden["kl450_labels"], golden["kl450_kl"]
    P = R.joint(R.binary_search(R.sqdist(X), 30)[1])
    Y, log, _ = R.descend(P, R.random_init(450, 0), 500)
    print("final KL", log[-1][0], "sklearn", sk)
    assert len(log) == 10
    assert abs(log[-1][0] - sk[0]) <= sk.max() - sk.min()
    assert R.purity(Y, labels) == 1.0
    assert (golden["kl450_purity"] == 1.0).all()


# ------------------------------------------------------------------------------------ refusals
def test_entry_points_refuse_host_tensors_and_wrong_dtypes():
    from mdil_ss_amd import latent as L
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    msg = "must be a contiguous float32 device tensor.*no CPU fallback in the latent-space path"
    with pytest.raises(RuntimeError, match="points " + msg):
        L.sqdist(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="points " + msg):
        L.sqdist(torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="points " + msg):
        L.sqdist(np.zeros((4, 3), dtype=np.float32))
    with pytest.raises(RuntimeError, match="D " + msg):
        L.affinities(torch.zeros(8, 8), 3)
    with pytest.raises(RuntimeError, match="D " + msg):
        L.affinities(torch.zeros(8, 8, dtype=torch.float16), 3)
    with pytest.raises(RuntimeError, match="P " + msg):
        L.run(torch.zeros(8, 8), torch.zeros(8, 2), torch.zeros(8, 2), torch.ones(8, 2), 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.tsne(torch.zeros(8, 4), perplexity=3)
    with pytest.raises(RuntimeError, match="MI355X only.*no CPU fallback in the product path"):
        L.latents(Net([20], 1, 0), torch.zeros(1, 3, 32, 64), 0, "encoder")
    with pytest.raises(RuntimeError, match="layer must be one of"):
        L.latents(Net([20], 1, 0), torch.zeros(1, 3, 32, 64), 0, "decoder")


def test_entry_points_refuse_sizes_outside_the_limits():
    from mdil_ss_amd import latent as L
    assert (L.MAX_POINTS, L.MAX_DIM) == (32768, 128)
    with pytest.raises(RuntimeError, match="32769 points .supported: 2 to 32768"):
        L.sqdist(torch.zeros(32769, 1))
    with pytest.raises(RuntimeError, match="1 points"):
        L.sqdist(torch.zeros(1, 4))
    with pytest.raises(RuntimeError, match="129 dimensions .supported: 1 to 128"):
        L.sqdist(torch.zeros(4, 129))
    with pytest.raises(RuntimeError, match=r"points must be float32 \[N,d\]"):
        L.sqdist(torch.zeros(4))
    for perplexity in (8, 8.5, 100, 0.5):
        with pytest.raises(RuntimeError, match="perplexity .* must be at least 1 and less than the 8 points"):
            L.affinities(torch.zeros(8, 8), perplexity)
    with pytest.raises(RuntimeError, match=r"D must be float32 \[N,N\]"):
        L.affinities(torch.zeros(8, 7), 3)
    with pytest.raises(RuntimeError, match=r"P must be float32 \[N,N\]"):
        L.run(torch.zeros(8, 2), torch.zeros(8, 2), torch.zeros(8, 2), torch.ones(8, 2), 5)


# ------------------------------------------------------------------------- host-side functions
def test_resize_labels_is_nearest():
    from mdil_ss_amd import latent as L
    g = torch.Generator().manual_seed(0)
    lab = torch.randint(0, 20, (64, 128), generator=g, dtype=torch.uint8)
    assert torch.equal(L.resize_labels(lab, 8, 16), lab[::8, ::8])
    assert torch.equal(L.resize_labels(lab, 32, 64), lab[::2, ::2])
    assert torch.equal(L.resize_labels(lab, 64, 128), lab)
    odd = torch.randint(0, 27, (50, 70), generator=g, dtype=torch.int64)
    for h, w in ((7, 9), (13, 70), (50, 11), (3, 3)):
        want = F.interpolate(odd[None, None].float(), size=(h, w), mode="nearest")[0, 0].long()
        got = L.resize_labels(odd, h, w)
        assert got.dtype == odd.dtype and torch.equal(got, want)
        rows = torch.div(torch.arange(h) * 50, h, rounding_mode="floor")
        cols = torch.div(torch.arange(w) * 70, w, rounding_mode="floor")
        assert torch.equal(got, odd[rows][:, cols])
    batch = torch.randint(0, 20, (2, 16, 32), generator=g, dtype=torch.uint8)
    assert torch.equal(L.resize_labels(batch, 2, 4), batch[:, ::8, ::8])


def test_sample_points_is_the_notebooks_draw():
    from mdil_ss_amd import latent as L
    a = L.sample_points(524288, 20000, 2)
    assert np.array_equal(a, np.random.RandomState(2).choice(np.arange(524288), 20000, replace=False))
    assert np.array_equal(a, L.sample_points(524288, 20000, 2))
    assert not np.array_equal(a, L.sample_points(524288, 20000, 3))
    assert len(np.unique(a)) == 20000
    assert np.array_equal(L.sample_points(128, 20000, 2), np.arange(128))
    assert np.array_equal(L.sample_points(128, 128, 2), np.arange(128))
    with pytest.raises(RuntimeError, match="32769 points .supported: up to 32768"):
        L.sample_points(524288, 32769, 2)
    with pytest.raises(RuntimeError, match="40000 points"):
        L.sample_points(40000, 50000, 2)
    with pytest.raises(RuntimeError, match="at least 2"):
        L.sample_points(100, 1, 2)
    assert np.array_equal(L.random_init(450, 3).numpy(), R.random_init(450, 3))


def test_scatter_png_is_fixed(tmp_path):
    from PIL import Image

    from mdil_ss_amd import latent as L
    Y = np.array([[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.5, 0.5], [1.0, 0.0]])
    labels = np.array([0, 1, 2, 3, 1])
    palette = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [9, 9, 9]], dtype=np.uint8)
    a = L.scatter_png(Y, labels, palette, str(tmp_path / "a.png"), size=16, marker=3)
    b = L.scatter_png(torch.tensor(Y), torch.tensor(labels), torch.from_numpy(palette), str(tmp_path / "b.png"),
                      size=16, marker=3)
    assert open(a, "rb").read() == open(b, "rb").read()
    # the box [0, 1] with a 4 % margin on 16 pixels: 0 -> pixel 1, 1 -> pixel 14; y points up
    want = np.full((16, 16, 3), 255, dtype=np.uint8)
    want[13:16, 0:3] = palette[0]                  # (0, 0)
    want[0:3, 13:16] = palette[1]                  # (1, 1)
    want[13:16, 13:16] = palette[1]                # (1, 0)
    want[0:3, 0:3] = palette[2]                    # (0, 1)
    got = np.asarray(Image.open(a))                # class 3, the last one, is the ignore class: not drawn
    assert got.shape == (16, 16, 3) and np.array_equal(got, want)
    c = L.scatter_png(Y, labels, palette, str(tmp_path / "c.png"), size=16, marker=3, skip=())
    want[6:9, 7:10] = palette[3]                   # (0.5, 0.5): x rint(7.5) = 8, y 15 - 8 = 7
    assert np.array_equal(np.asarray(Image.open(c)), want)
    # later classes are drawn over earlier ones
    d = L.scatter_png(np.array([[0.0, 0.0], [0.0, 0.0], [1.0, 1.0]]), np.array([1, 0, 0]), palette,
                      str(tmp_path / "d.png"), size=16, marker=3)
    assert np.asarray(Image.open(d))[14, 1].tolist() == [0, 255, 0]


def test_save_npz_is_fixed(tmp_path):
    from mdil_ss_amd import latent as L
    arrays = dict(Y=np.arange(6, dtype=np.float32).reshape(3, 2), labels=np.array([1, 2, 3], dtype=np.uint8),
                  arguments=np.array('{"a": 1}'))
    L.save_npz(str(tmp_path / "a.npz"), **arrays)
    L.save_npz(str(tmp_path / "b.npz"), **arrays)
    assert open(tmp_path / "a.npz", "rb").read() == open(tmp_path / "b.npz", "rb").read()
    back = np.load(tmp_path / "a.npz")
    assert sorted(back.files) == ["Y", "arguments", "labels"]
    assert np.array_equal(back["Y"], arrays["Y"]) and str(back["arguments"]) == '{"a": 1}'


def test_parser_defaults_and_refusals():
    from mdil_ss_amd import latent as L
    p = L.build_parser()
    base = ["--state", "c", "--num-classes", "20", "20", "--task", "0", "--out", "o"]
    a = p.parse_args(base + ["--synthetic", "1", "--layer", "logits"])
    assert (a.points, a.perplexity, a.iterations, a.seed, a.height, a.width) == (20000, 100.0, 2000, 2, 512, 1024)
    assert (a.learning_rate, a.kl_every, a.index, a.classes_at_least, a.subset) == (200.0, 50, 0, 0, "val")
    b = p.parse_args(base + ["--dataset", "BDD", "--datadir", "d", "--index", "7", "--layer", "encoder",
                             "--learning-rate", "auto", "--classes-at-least", "12"])
    assert (b.dataset, b.datadir, b.index, b.learning_rate, b.classes_at_least) == ("bdd", "d", 7, "auto", 12)
    assert L.positions(b) == 64 * 128
    c = p.parse_args(base + ["--image", "i.png", "--label", "l.png", "--layer", "penultimate"])
    assert (c.image, c.label) == ("i.png", "l.png") and L.positions(c) == 256 * 512
    small = ["--synthetic", "1", "--height", "64", "--width", "128", "--layer", "encoder"]
    assert p.parse_args(base + small + ["--perplexity", "5"]).perplexity == 5.0
    for argv in (base + ["--layer", "encoder"],                                               # no source
                 base + ["--synthetic", "1", "--dataset", "idd", "--datadir", "d", "--layer", "encoder"],   # two
                 base + ["--dataset", "idd", "--layer", "encoder"],                         # no --datadir
                 base + ["--image", "i.png", "--layer", "encoder"],                         # no --label
                 base + ["--synthetic", "1"],                                               # no --layer
                 base + small + ["--perplexity", "200"],                                    # 128 points
                 base + small,                                                              # default 100 fits,
                 base + small + ["--perplexity", "128"],                                    # 128 does not
                 base + ["--synthetic", "1", "--layer", "penultimate", "--points", "40000"],
                 base + ["--synthetic", "1", "--layer", "encoder", "--height", "100"],
                 base + ["--synthetic", "1", "--layer", "encoder", "--iterations", "0"]):
        if argv == base + small:
            assert p.parse_args(argv).perplexity == 100.0
            continue
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    assert callable(L.main)
