"""CPU: the similarity add-on (include/mdil_similarity.h, mdil_ss_amd/similarity.py) -- the library
exports exactly what its header declares, refuses bad arguments before any launch, and the fp64
host metrics agree with the checker (tests/similarity_reference.py), which works from the rows."""
import os
import re

import numpy as np
import pytest
import torch

from tests import similarity_reference as R
from tests.helpers import declared_names, dynamic_exports

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, C, NC = 4099, 20, 5


# ------------------------------------------------------------------------------------------ ABI
def test_library_exports_exactly_the_declared_symbols():
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _similarity_lib as B
    lib = B.load()
    names = declared_names("mdil_similarity.h")
    assert names == ["mdil_sim_accumulate", "mdil_sim_last_error", "mdil_sim_state_bytes", "mdil_sim_version",
                     "mdil_sim_workspace_bytes"]
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/mdil_similarity.h but not exported"
    assert sorted(B.EXPORTS) == names
    assert dynamic_exports(B.LIB_PATH) == names
    assert lib.mdil_sim_version() >= 100
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mdil_similarity.h")).read(), flags=re.S)
    protos = re.findall(r"\b(mdil_sim_[a-z_]+)\s*\(([^)]*)\)\s*;", hdr)
    assert sorted(n for n, _ in protos) == names
    for name, args in protos:
        n_args = 0 if args.strip() == "void" else len(args.split(","))
        assert len(getattr(lib, name).argtypes) == n_args, name
    for macro, value in (("MDIL_SIM_MAX_CX", B.MAX_CX), ("MDIL_SIM_MAX_CY", B.MAX_CY),
                         ("MDIL_SIM_MAX_CLASSES", B.MAX_CLASSES), ("MDIL_SIM_MAX_ROWS", B.MAX_ROWS),
                         ("MDIL_SIM_CHAIN", B.CHAIN)):
        assert re.search(rf"#define {macro} {value}\b", hdr), macro
    assert (B.MAX_CX, B.MAX_CY, B.MAX_CLASSES, B.MAX_ROWS) == (128, 128, 32, 1 << 24) and B.CHAIN <= 1024


def test_build_checks_the_bindings_exports():
    src = open(os.path.join(REPO, "__graft_entry__.py")).read()
    assert "_similarity_lib" in src


def test_state_and_workspace_sizes():
    from mdil_ss_amd import _similarity_lib as B
    lib = B.load()
    assert lib.mdil_sim_state_bytes(1, 0, 1) == 8 * (1 + 1 + 1 + 1)
    assert lib.mdil_sim_state_bytes(128, 128, 32) == 8 * (33 + 32 * 256 + 3 * 128 * 128)
    assert lib.mdil_sim_state_bytes(20, 27, 20) == 8 * (21 + 20 * 47 + 400 + 729 + 540)
    for cx, cy, nc in ((0, 0, 1), (129, 0, 1), (1, -1, 1), (1, 129, 1), (1, 0, 0), (1, 0, 33)):
        assert lib.mdil_sim_state_bytes(cx, cy, nc) == -1
        assert lib.mdil_sim_workspace_bytes(10, cx, cy, nc) == -1
    assert lib.mdil_sim_workspace_bytes(0, 16, 16, 20) == -1
    assert lib.mdil_sim_workspace_bytes((1 << 24) + 1, 16, 16, 20) == -1
    # the partial traffic stays well under the input traffic at the two sizes of the validation pass
    for rows, c in ((6 * 256 * 512, 16), (1 << 24, 16), (1 << 24, 128)):
        ws = lib.mdil_sim_workspace_bytes(rows, c, c, 20)
        assert 0 < ws <= rows * 2 * c * 4 / 4, (rows, c, ws)
    assert lib.mdil_sim_workspace_bytes(1, 1, 0, 1) % 16 == 0


def test_library_refuses_bad_arguments_without_a_device():
    """Argument checks come before any launch: sizes, NULL pointers, alignment, overlap."""
    from mdil_ss_amd import _similarity_lib as B
    lib = B.load()
    err = lib.mdil_sim_last_error
    big = 1 << 40

    def run(x=4096, y=1 << 20, labels=1 << 21, rows=100, cx=16, cy=16, nc=20, px=1 << 22, py=(1 << 22) + 1024,
            state=big, ws=2 * big):
        return lib.mdil_sim_accumulate(x, y, labels, rows, cx, cy, nc, px, py, state, ws, None)

    for kw, text in ((dict(rows=0), b"rows=0 "), (dict(rows=(1 << 24) + 1), b"rows=16777217"),
                     (dict(cx=0), b"cx=0 "), (dict(cx=129), b"cx=129"), (dict(cy=-1), b"cy=-1"),
                     (dict(cy=129), b"cy=129"), (dict(nc=0), b"nc=0 "), (dict(nc=33), b"nc=33"),
                     (dict(x=None), b"bad argument"), (dict(px=None), b"bad argument"),
                     (dict(state=None), b"bad argument"), (dict(ws=None), b"bad argument"),
                     (dict(y=None), b"cy=16"), (dict(py=None), b"cy=16"),
                     (dict(cy=0), b"cy=0"), (dict(cy=0, y=None), b"cy=0"),
                     (dict(labels=None), b"nc=20"),
                     (dict(x=4100), b"alignment"), (dict(y=(1 << 20) + 8), b"alignment"),
                     (dict(state=big + 8), b"alignment"), (dict(ws=2 * big + 4), b"alignment"),
                     (dict(px=(1 << 22) + 2), b"alignment"), (dict(py=(1 << 22) + 1025), b"alignment"),
                     (dict(state=4096 + 64), b"overlap x"), (dict(ws=(1 << 20) + 16), b"overlap y"),
                     (dict(state=(1 << 21) + 16), b"overlap labels"), (dict(ws=(1 << 22) - 16), b"overlap pivot_x"),
                     (dict(state=(1 << 22) + 1024 + 48), b"overlap pivot_y"),
                     (dict(ws=big + 16), b"state and workspace overlap")):
        assert run(**kw) == -1, kw
        assert text in err(), (kw, err())
    # one population and no labels: the same checks
    assert lib.mdil_sim_accumulate(4096, None, None, 10, 16, 0, 2, 1 << 22, None, big, 2 * big, None) == -1
    assert b"nc=2" in err()
    assert lib.mdil_sim_accumulate(4096, None, None, 10, 16, 0, 1, 1 << 22, 1 << 23, big, 2 * big, None) == -1
    assert b"pivot_y" in err()


# ----------------------------------------------------------------------------- the host metrics
@pytest.fixture(scope="module")
def data():
    """M rows of C channels in NC classes (labels 5 and 6 on some rows: skipped), a second
    population that is the first one moved class by class, never modified."""
    g = np.random.default_rng(7)
    lab = g.integers(0, NC + 2, M)
    centres = 2.0 * g.standard_normal((NC + 2, C))
    scales = 0.5 + 1.5 * g.random(C)
    x = centres[lab] + g.standard_normal((M, C)) * scales + 3.0
    y = x @ (np.eye(C) + 0.2 * g.standard_normal((C, C))) + 0.5 * g.standard_normal((NC + 2, C))[lab]
    return x, y, lab


def test_host_metrics_match_the_checker(data):
    from mdil_ss_amd import similarity as S
    x, y, lab = data
    px, py = x[:64].mean(0), y[:64].mean(0)
    m = R.moments(x, y, lab, NC, px, py, dtype=np.float64)
    assert m["skipped"] == (lab >= NC).sum() > 0 and m["n"].sum() + m["skipped"] == M
    xk, lk = R.kept(x, lab, NC)
    yk, _ = R.kept(y, lab, NC)
    c = S.covariances(m)
    (mx, cxx), (my, cyy) = R.mean_cov(xk), R.mean_cov(yk)
    scale = np.abs(cxx).max()
    assert np.abs(c["mean_x"] - mx).max() <= 1e-12 * np.abs(mx).max()
    assert np.abs(c["mean_y"] - my).max() <= 1e-12 * np.abs(my).max()
    assert np.abs(c["cxx"] - cxx).max() <= 1e-12 * scale and np.abs(c["cyy"] - cyy).max() <= 1e-12 * np.abs(cyy).max()
    assert np.abs(c["cxy"] - (xk - mx).T @ (yk - my) / len(xk)).max() <= 1e-12 * scale
    assert abs(S.linear_cka(m) - R.linear_cka(xk, yk)) <= 1e-12
    sep = S.separability(m)
    assert abs(sep["x"] - R.separability(xk, lk)) <= 1e-10 * sep["x"]
    assert abs(sep["y"] - R.separability(yk, lk)) <= 1e-10 * sep["y"]
    shift = S.class_shift(m)
    classes, want, rel = R.class_shift(xk, yk, lk)
    assert shift["classes"] == classes == list(range(NC))
    assert np.abs(np.array(shift["shift"]) - want).max() <= 1e-10 * want.max()
    assert np.abs(np.array(shift["relative"]) - rel).max() <= 1e-10 * rel.max()
    # one population against another one
    ma = R.moments(x, None, lab, NC, px, dtype=np.float64)
    mb = R.moments(y, None, lab, NC, py, dtype=np.float64)
    assert S.separability(ma)["y"] is None
    want_f = R.frechet(xk, yk)
    assert abs(S.frechet(ma, mb) - want_f) <= 1e-9 * (np.trace(cxx) + np.trace(cyy))
    between = S.class_shift(ma, mb)
    assert np.abs(np.array(between["shift"]) - want).max() <= 1e-10 * want.max()
    with pytest.raises(RuntimeError, match="two populations"):
        S.linear_cka(ma)


def test_cka_is_one_under_an_orthogonal_map_and_small_for_noise(data):
    from mdil_ss_amd import similarity as S
    x, _, lab = data
    g = np.random.default_rng(11)
    Q, _ = np.linalg.qr(g.standard_normal((C, C)))
    y = 2.5 * x @ Q + 1.0
    m = R.moments(x, y, lab, NC, x[0], y[0], dtype=np.float64)
    assert abs(S.linear_cka(m) - 1.0) <= 1e-12
    noise = g.standard_normal((M, C))
    cka = S.linear_cka(R.moments(x, noise, lab, NC, x[0], noise[0], dtype=np.float64))
    print("CKA against independent noise", cka)
    assert 0 <= cka < 0.02


def test_frechet_of_a_population_with_itself_and_with_a_scaled_copy(data):
    from mdil_ss_amd import similarity as S
    x, _, _ = data
    m = R.moments(x, None, None, 1, x[:10].mean(0), dtype=np.float64)
    mu, cov = R.mean_cov(x)
    tr = np.trace(cov)
    same = S.frechet(m, m)
    print("frechet(m, m)", same, "tr", tr)
    assert abs(same) <= 1e-9 * tr
    other = 2.0 * (x - mu) + mu + 1.0                       # (mu + 1, 4 cov): C + tr cov
    mo = R.moments(other, None, None, 1, other[3], dtype=np.float64)
    got = S.frechet(m, mo)
    print("frechet against (mu + 1, 4 cov)", got, "C + tr", C + tr)
    assert abs(got - (C + tr)) <= 1e-9 * (C + tr)


def test_metrics_do_not_depend_on_the_pivot(data):
    from mdil_ss_amd import similarity as S
    x, y, lab = data
    a = R.moments(x, y, lab, NC, x[:64].mean(0), y[:64].mean(0), dtype=np.float64)
    b = R.moments(x, y, lab, NC, x[100] + 2.0, np.zeros(C), dtype=np.float64)
    assert abs(S.linear_cka(a) - S.linear_cka(b)) <= 1e-9
    for side in ("x", "y"):
        assert abs(S.separability(a)[side] - S.separability(b)[side]) <= 1e-9 * S.separability(a)[side]
    sa, sb = S.class_shift(a), S.class_shift(b)
    assert np.abs(np.array(sa["shift"]) - np.array(sb["shift"])).max() <= 1e-9 * max(sa["shift"])
    assert np.abs(np.array(sa["relative"]) - np.array(sb["relative"])).max() <= 1e-9 * max(sa["relative"])
    pa = R.moments(x, None, lab, NC, x[:64].mean(0), dtype=np.float64)
    pb = R.moments(y, None, lab, NC, y[7], dtype=np.float64)
    pa2 = R.moments(x, None, lab, NC, np.zeros(C), dtype=np.float64)
    assert abs(S.frechet(pa, pb) - S.frechet(pa2, pb)) <= 1e-9 * S.frechet(pa, pb)


def test_unshifted_fp32_grams_cancel_and_pivoted_ones_do_not():
    """The numerics argument of DESIGN.md: mean 30, std 0.1, 20,000 rows, accumulated in fp32."""
    g = np.random.default_rng(0)
    x = (30.0 + 0.1 * g.standard_normal(20000)).astype(np.float32)
    exact = x.astype(np.float64).var()

    def fp32_variance(w):
        gram, s = np.float32(0), np.float32(0)
        for chunk in np.split(w, 20):                        # chains of 1000 rows, then fp64
            gram = np.cumsum(np.concatenate([[np.float32(0)], chunk * chunk]), dtype=np.float32)[-1]
            s = np.cumsum(np.concatenate([[np.float32(0)], chunk]), dtype=np.float32)[-1]
            fp32_variance.g += float(gram)
            fp32_variance.s += float(s)
        n = len(w)
        return fp32_variance.g / n - (fp32_variance.s / n) ** 2

    fp32_variance.g = fp32_variance.s = 0.0
    raw = abs(fp32_variance(x) - exact) / exact
    fp32_variance.g = fp32_variance.s = 0.0
    piv = abs(fp32_variance(x - x[0]) - exact) / exact
    print("relative error of the variance: unshifted", raw, "pivoted", piv)
    assert raw > 1e-4 and piv < 1e-5


def test_unpack_state_follows_the_header(data):
    from mdil_ss_amd import similarity as S
    x, y, lab = data
    m = R.moments(x, y[:, :7], lab, NC, x[0], y[0, :7], dtype=np.float64)
    back = S.unpack_state(R.pack(m), C, 7, NC, m["pivot_x"], m["pivot_y"])
    for k in ("n", "sx", "sy", "gxx", "gyy", "gxy", "pivot_x", "pivot_y"):
        assert back[k].shape == np.asarray(m[k]).shape and np.array_equal(back[k], m[k]), k
    assert back["skipped"] == m["skipped"]
    with pytest.raises(RuntimeError, match="does not fit"):
        S.unpack_state(R.pack(m)[:-1], C, 7, NC, m["pivot_x"], m["pivot_y"])


# ------------------------------------------------------------------------------------ refusals
def test_module_refuses_host_tensors_wrong_dtypes_and_sizes():
    from mdil_ss_amd import similarity as S
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    assert (S.MAX_CX, S.MAX_CY, S.MAX_CLASSES, S.LAYERS) == (128, 128, 32, ("encoder", "penultimate", "logits"))
    msg = "must be a contiguous float32 device tensor.*no CPU fallback in the similarity path"
    meter = S.MomentMeter(16, 16, 20, "cuda:0")            # allocates nothing before the first add
    with pytest.raises(RuntimeError, match="x " + msg):
        meter.add(torch.zeros(8, 16), torch.zeros(8, 16), torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="x " + msg):
        meter.add(torch.zeros(8, 16, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="x " + msg):
        meter.add(np.zeros((8, 16), dtype=np.float32))
    with pytest.raises(RuntimeError, match="x " + msg):
        meter.add(torch.zeros(16, 8).t())
    with pytest.raises(RuntimeError, match="moments.. before the first add"):
        meter.moments()
    meter.reset()
    with pytest.raises(RuntimeError, match="device must be a cuda device.*no CPU fallback in the similarity path"):
        S.MomentMeter(16, 16, 20, "cpu")
    for args, text in (((0, 0, 1), "cx 0 channels .supported: 1 to 128"), ((129, 0, 1), "cx 129 channels"),
                       ((16, -1, 1), "cy -1 channels .supported: 0 to 128"), ((16, 129, 1), "cy 129 channels"),
                       ((16, 16, 0), "nc 0 classes .supported: 1 to 32"), ((16, 16, 33), "nc 33 classes")):
        with pytest.raises(RuntimeError, match=text):
            S.MomentMeter(*args, "cuda:0")
    with pytest.raises(RuntimeError, match="pivot_x must have 16 values"):
        S.MomentMeter(16, 0, 1, "cuda:0", pivot_x=np.zeros(3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.compare(Net([20], 1, 0), Net([20], 1, 0), torch.zeros(1, 3, 32, 64), 0, "encoder")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.population(Net([20], 1, 0), torch.zeros(1, 3, 32, 64), 0, "logits")
    with pytest.raises(RuntimeError, match="layer must be one of"):
        S.population(Net([20], 1, 0), torch.zeros(1, 3, 32, 64), 0, "decoder")
    with pytest.raises(RuntimeError, match="no rows were counted"):
        S.covariances(R.moments(np.zeros((4, 3)), None, np.full(4, 9), 2, np.zeros(3)))


def test_parser_defaults_and_refusals():
    from mdil_ss_amd import similarity as S
    p = S.build_parser()
    ckpt = ["--before", "a", "--before-num-classes", "20", "--after", "b", "--after-num-classes", "20", "20",
            "--task", "0"]
    a = p.parse_args(ckpt + ["--synthetic", "4"])
    assert (a.layers, a.height, a.width, a.batch_size, a.subset, a.json) == (list(S.LAYERS), 512, 1024, 6, "val", None)
    assert (a.before, a.after, a.task, a.synthetic, a.state) == ("a", "b", 0, 4, None)
    b = p.parse_args(ckpt + ["--dataset", "BDD", "--layers", "encoder", "logits", "--json", "r.json"])
    assert (b.dataset, b.layers, b.json) == ("BDD", ["encoder", "logits"], "r.json")
    dom = ["--state", "c", "--num-classes", "20", "20", "--task-a", "0", "--task-b", "1"]
    c = p.parse_args(dom + ["--dataset-a", "cityscapes", "--dataset-b", "IDD", "--datadir-b", "/d"])
    assert (c.dataset_a, c.dataset_b, c.datadir_a, c.datadir_b, c.task_a, c.task_b) == \
        ("cityscapes", "IDD", None, "/d", 0, 1)
    assert p.parse_args(dom + ["--synthetic", "2"]).synthetic == 2
    for argv in (["--synthetic", "2"],                                              # neither mode
                 ckpt + dom + ["--synthetic", "2"],                                 # both
                 ckpt,                                                              # no data
                 ckpt + ["--synthetic", "2", "--dataset", "BDD"],                   # two sources
                 ckpt[:-2] + ["--synthetic", "2"],                                  # no --task
                 ckpt[:-1] + ["1", "--synthetic", "2"],                             # the model before has one task
                 ["--before", "a", "--before-num-classes", "20", "--synthetic", "2", "--task", "0"],
                 ["--before", "a", "--before-num-classes", "20", "--after", "b", "--after-num-classes", "27",
                  "--task", "0", "--synthetic", "2"],                               # heads differ
                 ckpt + ["--synthetic", "2", "--height", "100"],
                 ckpt + ["--synthetic", "2", "--batch-size", "0"],
                 ckpt + ["--synthetic", "2", "--layers", "encoder", "encoder"],
                 ckpt + ["--synthetic", "2", "--layers", "decoder"],
                 dom,                                                               # no data
                 dom + ["--dataset-a", "BDD"],                                      # one data set
                 dom + ["--dataset-a", "BDD", "--dataset-b", "IDD", "--synthetic", "2"],
                 dom[:-2] + ["--synthetic", "2"],                                   # no --task-b
                 dom[:-1] + ["2", "--synthetic", "2"],                              # no such task
                 dom[:-1] + ["0", "--synthetic", "2"],                              # the same synthetic domain twice
                 ["--state", "c", "--task-a", "0", "--task-b", "1", "--synthetic", "2"],
                 ["--state", "c", "--num-classes", "20", "40", "--task-a", "0", "--task-b", "1", "--synthetic", "2"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    assert callable(S.main)
