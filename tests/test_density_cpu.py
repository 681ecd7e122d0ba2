"""CPU: the density add-on (include/mdil_density.h, mdil_ss_amd/density.py) -- ``fit_model`` from
``unpack_state``-shaped moments against the fit from rows directly (tests/density_reference.py), the
whitening identity, the ``.npz`` round trip and ``load_model``'s refusals, the library's exports and
argument checks (every refusal before any launch), and the wrappers' and the command line's refusals."""
import os
import re

import numpy as np
import pytest
import torch

from tests import density_reference as R
from tests.helpers import declared_names, dynamic_exports

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mdil_density_head", "mdil_density_last_error", "mdil_density_rows", "mdil_density_version"]


# ------------------------------------------------------------------------------------- the fit
def moments_of(x, labels, classes, pivot):
    """The state ``similarity.MomentMeter`` would hold, formed in fp64 from the rows, through ``unpack_state``."""
    from mdil_ss_amd import similarity as S
    x64, lab = x.double().numpy(), labels.numpy()
    C = x64.shape[1]
    p = np.asarray(pivot, dtype=np.float32).astype(np.float64)
    used = lab < classes
    z = x64[used] - p
    n = np.bincount(lab[used], minlength=classes).astype(np.float64)
    sx = np.stack([z[lab[used] == k].sum(0) for k in range(classes)])
    state = np.concatenate([n, [float((~used).sum())], sx.reshape(-1), (z.T @ z).reshape(-1)])
    return S.unpack_state(state, C, 0, classes, p)


def case(name):
    """-> (x float32 [rows, C], labels u8, classes, min_rows)"""
    if name == "clustered":
        x, lab, _ = R.clustered(16, 19, 3000, seed=1)
        return x, lab, 19, None
    if name == "wide":
        x, lab, _ = R.clustered(64, 7, 2500, seed=2)
        return x, lab, 7, None
    if name == "constant channel":                                  # post-ReLU: a channel that never fires
        x, lab, _ = R.clustered(16, 5, 1500, seed=3)
        x = torch.relu(x)
        x[:, 3] = 0.0
        x[:, 11] = 1.5
        return x, lab, 5, None
    if name == "class below min_rows":
        x, lab, _ = R.clustered(16, 6, 2000, seed=4)
        few = (lab == 2).nonzero().reshape(-1)[5:]
        lab[few] = 4                                                # class 2 keeps five rows
        empty = lab == 5
        lab[empty] = 0                                              # class 5 has none
        return x, lab, 6, 32
    raise AssertionError(name)


def close(a, b, rel=1e-9):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and float(np.abs(a - b).max()) <= rel * float(np.abs(b).max())


@pytest.mark.parametrize("name", ["clustered", "wide", "constant channel", "class below min_rows"])
def test_fit_model_matches_the_fit_from_rows(name):
    from mdil_ss_amd import density as D
    x, lab, classes, min_rows = case(name)
    pivot = x[:64].double().mean(0).float().numpy()
    got = D.fit_model(moments_of(x, lab, classes, pivot), min_rows=min_rows, layer="penultimate", task=1)
    want = R.fit(x, lab, classes, min_rows=min_rows, pivot=pivot)
    assert got["cls"].dtype == np.uint8 and got["cls"].tolist() == want["cls"].tolist()
    assert got["dropped"].tolist() == want["dropped"].tolist() and got["counts"].tolist() == want["counts"].tolist()
    assert (got["C"], got["nc"], got["rows"], got["ridge"]) == (x.shape[1], classes + 1, want["rows"], 1e-4)
    for key in ("means", "mean_total", "cov_within", "cov_total"):
        assert close(got[key], want[key]), key
    if name == "class below min_rows":
        assert got["cls"].tolist() == [0, 1, 3, 4] and got["dropped"].tolist() == [2, 5]
    # A cov A^T = I, from the fp64 factor the fp32 buffer was rounded from: re-derive it from the covariance
    C, K = got["C"], len(got["cls"])
    assert got["buffer"].dtype == np.float32 and got["buffer"].size == R.model_floats(C, K)
    p, A, A0, m0, m = (t.double().numpy() for t in R.parts(got["buffer"], C, K))
    for factor, cov in ((A, got["cov_within"]), (A0, got["cov_total"])):
        exact = np.tril(np.linalg.inv(np.linalg.cholesky(cov)))
        assert float(np.abs(exact @ cov @ exact.T - np.eye(C)).max()) <= 1e-8
        assert float(np.abs(factor - exact).max()) <= 2.0 ** -23 * float(np.abs(exact).max())
        assert not np.triu(factor, 1).any()
    assert close(p, pivot, 0.0)
    assert float(np.abs(m - (got["means"] - p) @ A.T).max()) <= 1e-4 * max(1.0, float(np.abs(m).max()))
    assert float(np.abs(m0 - A0 @ (got["mean_total"] - p)).max()) <= 1e-4 * max(1.0, float(np.abs(m0).max()))


def test_fit_model_refusals():
    from mdil_ss_amd import density as D
    x, lab, classes, _ = case("clustered")
    mom = moments_of(x, lab, classes, np.zeros(16))
    with pytest.raises(RuntimeError, match="no class has min_rows"):
        D.fit_model(mom, min_rows=100000)
    with pytest.raises(RuntimeError, match="ridge"):
        D.fit_model(mom, ridge=-1.0)
    with pytest.raises(RuntimeError, match="min_rows 0"):
        D.fit_model(mom, min_rows=0)
    const = torch.zeros(200, 16)
    const[:, 2] = 1.0
    with pytest.raises(RuntimeError, match="not positive definite"):
        D.fit_model(moments_of(const, torch.zeros(200, dtype=torch.uint8), 2, np.zeros(16)))
    ok = moments_of(x[:, :16], lab, classes, np.zeros(16))
    ok["cx"] = 24
    with pytest.raises(RuntimeError, match="24 channels"):
        D.fit_model(ok)


def test_ridge_alone_keeps_a_constant_channel_defined():
    from mdil_ss_amd import density as D
    x, lab, classes, _ = case("constant channel")
    mom = moments_of(x, lab, classes, x[:64].double().mean(0).float().numpy())
    with pytest.raises(RuntimeError, match="not positive definite"):
        D.fit_model(mom, ridge=0.0)
    model = D.fit_model(mom)
    assert np.isfinite(model["buffer"]).all() and model["cov_within"][3, 3] > 0


def test_npz_round_trip_and_load_refusals(tmp_path):
    from mdil_ss_amd import density as D
    x, lab, classes, _ = case("clustered")
    model = D.fit_model(moments_of(x, lab, classes, np.zeros(16)), layer="penultimate", task=1)
    path = str(tmp_path / "model.npz")
    D.save_model(model, path)
    with np.load(path, allow_pickle=False) as z:                    # arrays and settings only: nothing pickled
        assert sorted(z.files) == sorted(D._ARRAYS + D._SETTINGS)
    back = D.load_model(path, layer="penultimate", nc=20, C=16, task=1)
    for k, v in model.items():
        if isinstance(v, np.ndarray):
            assert back[k].dtype == v.dtype and np.array_equal(back[k], v), k
        else:
            assert back[k] == v and type(back[k]) is type(v), k
    for kw, text in ((dict(layer="encoder"), "fitted for layer penultimate, this run has encoder"),
                     (dict(nc=27), "num-classes of the task 20, this run has 27"),
                     (dict(C=128), "channels 16, this run has 128"), (dict(task=0), "task 1, this run has 0")):
        with pytest.raises(RuntimeError, match=text):
            D.load_model(path, **kw)
    with pytest.raises(RuntimeError, match="no such file"):
        D.load_model(str(tmp_path / "absent.npz"))
    other = str(tmp_path / "other.npz")
    np.savez(other, a=np.zeros(3))
    with pytest.raises(RuntimeError, match="not a density model"):
        D.load_model(other)
    cut = dict(model, buffer=model["buffer"][:-1])
    D.save_model(cut, other)
    with pytest.raises(RuntimeError, match="does not fit C 16"):
        D.load_model(other)


# -------------------------------------------------------------------------------------- library
def test_library_exports_exactly_the_declared_symbols():
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _density_lib
    lib = _density_lib.load()
    assert declared_names("mdil_density.h") == NAMES
    for n in NAMES:
        assert hasattr(lib, n), f"{n} declared in include/mdil_density.h but not exported"
    assert sorted(_density_lib.EXPORTS) == NAMES
    assert dynamic_exports(_density_lib.LIB_PATH) == NAMES
    mapped = re.findall(r"^\s*(mdil_density_\w+);", open(os.path.join(REPO, "mdil_ss_amd", "ext", "density_exports.map")).read(),
                        flags=re.M)
    assert sorted(mapped) == NAMES
    assert lib.mdil_density_version() >= 100
    assert (_density_lib.MIN_CLASSES, _density_lib.MAX_CLASSES, _density_lib.MAX_MEANS) == (2, 32, 32)


HEAD_OK = dict(x=4096, w=8192, b=12288, N=1, H=4, W=4, nc=20, model=16384, cls=20480, K=19, tgt=24576, lut=28672, cg=0,
               kinds=3, mk=1, label=32768, near=36864, code=40960, hist=45056, nonf=49152, agree=53248)
ROWS_OK = dict(x=4096, rows=64, C=48, model=8192, cls=12288, K=5, group=16384, cg=0, kinds=3, mk=0, near=20480, code=24576,
               hist=28672, nonf=32768)


def _head(lib, **kw):
    a = dict(HEAD_OK, **kw)
    return lib.mdil_density_head(a["x"], a["w"], a["b"], a["N"], a["H"], a["W"], a["nc"], a["model"], a["cls"], a["K"],
                                 a["tgt"], a["lut"], a["cg"], a["kinds"], a["mk"], a["label"], a["near"], a["code"],
                                 a["hist"], a["nonf"], a["agree"], None)


def _rows(lib, **kw):
    a = dict(ROWS_OK, **kw)
    return lib.mdil_density_rows(a["x"], a["rows"], a["C"], a["model"], a["cls"], a["K"], a["group"], a["cg"], a["kinds"],
                                 a["mk"], a["near"], a["code"], a["hist"], a["nonf"], None)


@pytest.mark.parametrize("call, bad, text", [
    (_head, dict(nc=1), b"nc=1"), (_head, dict(nc=33), b"nc=33"),
    (_head, dict(x=None), b"bad argument"), (_head, dict(w=None), b"bad argument"), (_head, dict(b=None), b"bad argument"),
    (_head, dict(N=0), b"bad argument"), (_head, dict(H=-1), b"bad argument"), (_head, dict(W=0), b"bad argument"),
    (_head, dict(label=None, near=None, code=None, mk=-1, hist=None, nonf=None, agree=None), b"nothing to write"),
    (_head, dict(model=None), b"the model"), (_head, dict(cls=None), b"the model"),
    (_head, dict(K=0), b"K=0"), (_head, dict(K=33), b"K=33"),
    (_head, dict(kinds=0), b"kinds=0"), (_head, dict(kinds=4), b"kinds=4"),
    (_head, dict(mk=2), b"map_kind=2"), (_head, dict(mk=-2), b"map_kind=-2"),
    (_head, dict(mk=-1), b"map_kind=-1"), (_head, dict(code=None), b"map_kind=1"),
    (_head, dict(cg=3), b"const_group=3"), (_head, dict(cg=-1), b"const_group=-1"),
    (_head, dict(lut=None), b"a target needs its group_lut"),
    (_head, dict(x=4100), b"alignment"), (_head, dict(w=8194), b"alignment"), (_head, dict(b=12290), b"alignment"),
    (_head, dict(model=16386), b"alignment"), (_head, dict(tgt=24577), b"alignment"), (_head, dict(label=32769), b"alignment"),
    (_head, dict(near=36865), b"alignment"), (_head, dict(code=40962), b"alignment"), (_head, dict(hist=45060), b"alignment"),
    (_head, dict(nonf=49156), b"alignment"), (_head, dict(agree=53252), b"alignment"),
    (_head, dict(W=1 << 30), b"too large"), (_head, dict(N=1 << 20, H=1 << 10, W=1 << 10), b"too large"),
    (_rows, dict(x=None), b"bad argument"), (_rows, dict(rows=0), b"bad argument"),
    (_rows, dict(rows=(1 << 24) + 1), b"bad argument"),
    (_rows, dict(C=0), b"C=0"), (_rows, dict(C=24), b"C=24"), (_rows, dict(C=144), b"C=144"),
    (_rows, dict(near=None, code=None, mk=-1, hist=None, nonf=None), b"nothing to write"),
    (_rows, dict(model=None), b"the model"), (_rows, dict(cls=None), b"the model"), (_rows, dict(K=0), b"K=0"),
    (_rows, dict(K=33), b"K=33"), (_rows, dict(kinds=0), b"kinds=0"), (_rows, dict(kinds=4), b"kinds=4"),
    (_rows, dict(mk=2), b"map_kind=2"), (_rows, dict(mk=-1), b"map_kind=-1"), (_rows, dict(code=None), b"map_kind=0"),
    (_rows, dict(cg=3), b"const_group=3"),
    (_rows, dict(x=4104), b"alignment"), (_rows, dict(model=8194), b"alignment"), (_rows, dict(code=24577), b"alignment"),
    (_rows, dict(hist=28676), b"alignment"), (_rows, dict(nonf=32772), b"alignment"),
])
def test_library_refuses_bad_arguments_without_a_device(call, bad, text):
    """Argument checks come before the launch, so fake pointers never reach a device."""
    from mdil_ss_amd import _density_lib
    lib = _density_lib.load()
    assert call(lib, **bad) == -1, bad
    assert text in lib.mdil_density_last_error(), (bad, lib.mdil_density_last_error())


# -------------------------------------------------------------------------------------- wrappers
def _model():
    from mdil_ss_amd import density as D
    x, lab, classes, _ = case("clustered")
    return D.fit_model(moments_of(x, lab, classes, np.zeros(16)))


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from mdil_ss_amd import density as D
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    model = _model()
    x, w, b = torch.zeros(1, 2, 2, 16), torch.zeros(16, 20, 2, 2), torch.zeros(20)
    with pytest.raises(RuntimeError, match="features must be a contiguous float32 device tensor.*no CPU fallback in "
                                           "the density path"):
        D.density_head(x, w, b, model)
    with pytest.raises(RuntimeError, match="x must be a contiguous float32 device tensor.*no CPU fallback in the density path"):
        D.density_rows(torch.zeros(8, 16), model)
    with pytest.raises(RuntimeError, match="no CPU fallback in the density path"):
        D.DensityMeter(20, model).add(x, w, b)
    with pytest.raises(RuntimeError, match="no CPU fallback in the density path"):
        D.DensityMeter(20, model).add(Net([20], 1, 0), torch.zeros(1, 3, 32, 64), 0)
    with pytest.raises(RuntimeError, match="expects"):
        D.DensityMeter(20, model).add(x, w)
    for nc in (1, 33):
        with pytest.raises(RuntimeError, match=f"{nc} classes \\(supported: 2 to 32\\)"):
            D.DensityMeter(nc, model)
    with pytest.raises(RuntimeError, match="const_group 3"):
        D.DensityMeter(20, model, const_group=3)
    with pytest.raises(RuntimeError, match="score kind"):
        D.DensityMeter(20, model, ["energy"])
    with pytest.raises(RuntimeError, match="lut must be"):
        D.DensityMeter(20, model, lut=torch.zeros(255, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="layer must be"):
        D.DensityMeter(20, model, layer="logits")
    empty = D.DensityMeter(20, model, ["rmaha", "maha"])
    assert empty.kinds == ("maha", "rmaha") and empty.nonfinite() == 0 and int(empty.hist().sum()) == 0
    assert empty.agree() == (0, 0) and tuple(empty.hist().shape) == (2, 2, 65536)
    with pytest.raises(RuntimeError, match="group is empty"):
        empty.report()
    assert D.kinds_mask(["maha"]) == 1 and D.kinds_mask([1]) == 2 and D.kinds_mask(D.KINDS) == 3
    assert D.model_floats(16, 19) == R.model_floats(16, 19) == model["buffer"].size


# ---------------------------------------------------------------------------------- command line
BASE = ["--state", "ckpt.pth.tar", "--num-classes", "20", "20", "27", "--task", "0"]
M = ["--model", "m.npz"]


def test_parser_defaults():
    from mdil_ss_amd import density as D
    a = D.build_parser().parse_args(BASE + ["--dataset", "cityscapes", "--subset", "train", "--fit", "m.npz"])
    assert (a.fit, a.dataset, a.subset, a.layer, a.ridge, a.min_rows, a.model) == \
        ("m.npz", "cityscapes", "train", None, 1e-4, None, None)
    b = D.build_parser().parse_args(BASE + M + ["--dataset", "IDD", "--data-task", "2", "--unknown-ids", "18", "25", "--score",
                                                "--json", "r.json", "--with-logit-scores"])
    assert (b.model, b.score, b.json, b.with_logit_scores, b.data_task, b.unknown_ids, b.tpr) == \
        ("m.npz", True, "r.json", True, 2, [18, 25], 0.95)
    c = D.build_parser().parse_args(BASE + M + ["--dataset", "cityscapes", "--fit-threshold", "t.json"])
    assert (c.fit_threshold, c.known_fpr) == ("t.json", 0.05)
    d = D.build_parser().parse_args(BASE + M + ["--images", "pics", "--threshold", "t.json", "--kind", "rmaha", "--out", "o",
                                                "--unknown-id", "254", "--colour", "--nearest"])
    assert (d.images, d.threshold, d.kind, d.out, d.unknown_id, d.colour, d.nearest) == \
        ("pics", "t.json", "rmaha", "o", 254, True, True)
    e = D.build_parser().parse_args(BASE + ["--synthetic", "4", "--fit", "m.npz", "--layer", "encoder", "--ridge", "0.01",
                                            "--min-rows", "8"])
    assert (e.layer, e.ridge, e.min_rows, e.synthetic, e.kind, e.height, e.width, e.batch_size) == \
        ("encoder", 0.01, 8, 4, "maha", 512, 1024, 6)
    assert callable(D.main)


@pytest.mark.parametrize("argv, text", [
    (["--dataset", "BDD"], "give one of --fit"),
    (M + ["--dataset", "BDD", "--score", "--json", "r", "--fit-threshold", "t"], "give one of --fit"),
    (M + ["--dataset", "BDD", "--fit", "m2.npz"], "give one of them"),
    (["--dataset", "BDD", "--score", "--json", "r"], "need --model"),
    (["--dataset", "BDD", "--fit-threshold", "t"], "need --model"),
    (M + ["--dataset", "BDD", "--score"], "--score writes its report to --json"),
    (M + ["--score", "--json", "r"], "give --dataset"),
    (M + ["--dataset", "BDD", "--synthetic", "2", "--score", "--json", "r"], "give --dataset"),
    (["--fit", "m.npz"], "give --dataset"),
    (M + ["--images", "p", "--score", "--json", "r"], "--images DIR has no labels"),
    (M + ["--images", "p", "--out", "o"], "--out DIR needs --threshold"),
    (M + ["--dataset", "BDD", "--fit-threshold", "t", "--threshold", "x"], "--threshold FILE goes with --out"),
    (M + ["--dataset", "BDD", "--threshold", "t", "--out", "o"], "one source of images"),
    (M + ["--threshold", "t", "--out", "o"], "one source of images"),
    (M + ["--images", "p", "--threshold", "t", "--out", "o", "--kind", "energy"], "--kind energy"),
    (M + ["--images", "p", "--threshold", "t", "--out", "o", "--unknown-id", "256"], "--unknown-id 256"),
    (M + ["--images", "p", "--threshold", "t", "--out", "o", "--layer", "encoder"], "need the penultimate layer"),
    (M + ["--dataset", "BDD", "--fit-threshold", "t", "--layer", "encoder"], "need the penultimate layer"),
    (M + ["--dataset", "BDD", "--score", "--json", "r", "--layer", "encoder", "--with-logit-scores"], "needs --layer penultimate"),
    (M + ["--dataset", "BDD", "--fit-threshold", "t", "--with-logit-scores"], "--with-logit-scores goes with --score"),
    (M + ["--dataset", "BDD", "--score", "--json", "r", "--nearest"], "--nearest writes"),
    (M + ["--dataset", "BDD", "--fit-threshold", "t", "--foreign-dataset", "IDD"], "--foreign-dataset goes with --score"),
    (M + ["--dataset", "BDD", "--score", "--json", "r", "--foreign-dataset", "IDD", "--foreign-synthetic", "2"], "exclude each other"),
    (M + ["--dataset", "BDD", "--score", "--json", "r", "--foreign-dataset", "IDD", "--unknown-ids", "3"], "does not go with it"),
    (["--dataset", "BDD", "--fit", "m.npz", "--unknown-ids", "3"], "--fit uses every labelled pixel"),
    (M + ["--dataset", "BDD", "--score", "--json", "r", "--tpr", "0"], "--tpr"),
    (M + ["--dataset", "BDD", "--score", "--json", "r", "--tpr", "1.5"], "--tpr"),
    (M + ["--dataset", "BDD", "--fit-threshold", "t", "--known-fpr", "1.5"], "--known-fpr"),
    (["--dataset", "BDD", "--fit", "m.npz", "--batch-size", "0"], "must be positive"),
    (["--dataset", "BDD", "--fit", "m.npz", "--height", "100"], "multiples of 8"),
    (["--dataset", "BDD", "--fit", "m.npz", "--ridge", "-1"], "--ridge"),
    (["--dataset", "BDD", "--fit", "m.npz", "--ridge", "nan"], "--ridge"),
    (["--dataset", "BDD", "--fit", "m.npz", "--min-rows", "0"], "--min-rows 0"),
    (M + ["--dataset", "BDD", "--score", "--json", "r", "--unknown-ids", "3", "--ignore-ids", "3"], "share an id"),
])
def test_parser_refusals(argv, text, capsys):
    from mdil_ss_amd import density as D
    with pytest.raises(SystemExit):
        D.build_parser().parse_args(BASE + argv)
    assert re.search(text, capsys.readouterr().err)


def test_main_refuses_before_it_opens_anything(tmp_path):
    """The checkpoint does not exist: every refusal below comes before it would be opened."""
    from mdil_ss_amd import density as D
    args = D.build_parser().parse_args(BASE + M + ["--dataset", "BDD", "--score", "--json", "r.json"])
    args.json = None
    with pytest.raises(RuntimeError, match="--score writes its report"):
        D.main(args)
    args.json, args.task = "r.json", 3
    with pytest.raises(RuntimeError, match="--task 3: the model has tasks 0 to 2"):
        D.main(args)
    args.task, args.data_task = 0, 5
    with pytest.raises(RuntimeError, match="--data-task 5: the model has tasks 0 to 2"):
        D.main(args)
    args.data_task, args.unknown_ids = 2, [27]
    with pytest.raises(RuntimeError, match=r"--unknown-ids \[27\]: task 2's labels lie in \[0, 27\)"):
        D.main(args)
    args.unknown_ids, args.data_task, args.dataset, args.synthetic, args.foreign_synthetic = [], None, None, 2, 2
    with pytest.raises(RuntimeError, match="the same images"):
        D.main(args)
    args.foreign_synthetic = 0
    with pytest.raises(RuntimeError, match="--model m.npz: no such file"):
        D.main(args)
    fit = D.build_parser().parse_args(BASE + ["--dataset", "BDD", "--fit", "m.npz", "--data-task", "1"])
    with pytest.raises(RuntimeError, match="--data-task does not go with it"):
        D.main(fit)
    maps = D.build_parser().parse_args(BASE + M + ["--images", "p", "--threshold", "no_such_file.json", "--out", "o"])
    with pytest.raises(RuntimeError, match="--threshold no_such_file.json: no such file"):
        D.main(maps)
    # a model fitted for another layer, task width or task is refused by name; an encoder model writes no maps
    x, lab, classes, _ = case("clustered")
    model = D.fit_model(moments_of(x, lab, classes, np.zeros(16)), layer="encoder", task=0, nc=20)
    path = str(tmp_path / "enc.npz")
    D.save_model(model, path)
    score = D.build_parser().parse_args(BASE + ["--model", path, "--synthetic", "2", "--score", "--json", "r.json"])
    score.layer = "penultimate"
    with pytest.raises(RuntimeError, match="fitted for layer encoder, this run has penultimate"):
        D.main(score)
    score.layer, score.task = None, 1
    with pytest.raises(RuntimeError, match="fitted for task 0, this run has 1"):
        D.main(score)
    score.task, score.num_classes = 0, [27, 20]
    with pytest.raises(RuntimeError, match="num-classes of the task 20, this run has 27"):
        D.main(score)
    thr = D.build_parser().parse_args(BASE + ["--model", path, "--synthetic", "2", "--fit-threshold", "t.json"])
    with pytest.raises(RuntimeError, match="was fitted on the encoder layer"):
        D.main(thr)
    assert not os.path.exists("o") and not os.path.exists("t.json")
