"""What the GPU suites of the annotator family (acquire, ripu, audit) share: the checkpoint and the base of their
command lines on --synthetic 4, the procedural targets, the reader of a written label tree, one draw of the five
maps the two apply kernels read, the counter check -- and the recorder of tests/golden/annotate_cli.json.

    python tests/annotate_cases.py FILE.json           # record (needs an MI355X)

The golden file holds, for ten command lines of the three programs, the SHA-256 of every file written and of the
returned report.  It was recorded from the sources as they were BEFORE the three drivers came to share
mdil_ss_amd/_annotate_common.py and the two apply kernels the rule in map_common.h; two recordings of those
sources agreed in every digest.  It is the proof that sharing changed no byte and is not re-recorded.  The
recorder uses public names only (``main``, ``build_parser``), so it runs on both sides."""
import contextlib
import functools
import glob
import hashlib
import importlib
import json
import os
import sys
import tempfile

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, REPO)

from tests import head_cases as HC  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden", "annotate_cli.json")
IGNORE, DROP = 255, 250
SENTINEL = torch.tensor([0xA5] * 8, dtype=torch.uint8).view(torch.int64)
N_IMAGES, SIZE = 4, (64, 128)
CLI_BASE = ["--num-classes", "20", "20", "--task", "1", "--synthetic", str(N_IMAGES), "--height", str(SIZE[0]),
            "--width", str(SIZE[1]), "--batch-size", "3"]
# the sizes of the apply tests: N x Hl x Wl; 1001 and 1024 cross the packed / byte-wise border of an item
APPLY_N, APPLY_NC, APPLY_HEIGHTS, APPLY_WIDTHS = 2, 20, (1, 5), (1, 3, 5, 1001, 1024)
APPLY_TILES = ((2, 2), (4, 6))


@pytest.fixture(scope="module")
def checkpoint(dev, tmp_path_factory):
    """The tiny model's checkpoint, once per suite that imports this fixture (it takes the suite's own ``dev``)."""
    path = tmp_path_factory.mktemp("annotate") / "checkpoint.pth.tar"
    HC.save_checkpoint(HC.tiny_model(dev), path)
    return str(path)


def run_cli(program, base, state, extra):
    """``main`` of mdil_ss_amd.<program> on ``--state state`` + ``base`` + ``extra`` -> its report."""
    mod = importlib.import_module(f"mdil_ss_amd.{program}")
    return mod.main(mod.build_parser().parse_args(["--state", state] + base + [str(v) for v in extra]))


def synthetic_targets():
    from mdil_ss_amd.dataset import ProceduralSeg
    ds = ProceduralSeg(N_IMAGES, SIZE[0], SIZE[1], 20, seed=13, domain=1)
    return torch.stack([ds[i][1][0] for i in range(N_IMAGES)]).to(torch.uint8)


def read_tree(root, layout, images=N_IMAGES, size=SIZE):
    """The label maps of a written tree, opened by the trainers' dataset class of ``layout``."""
    import numpy as np
    from mdil_ss_amd import dataset as D
    ds = (D.BDD100k if layout == "BDD" else D.cityscapes)(str(root), subset="val")
    assert len(ds) == images and len(ds.filenamesGt) == images
    maps = []
    for i in range(images):
        image, label = ds[i]
        assert image.size == (size[1], size[0])
        maps.append(torch.from_numpy(np.array(label)))
    return torch.stack(maps)


def images_base(folder):
    """``CLI_BASE`` on the images of ``folder`` (unlabelled) in place of the procedural ones."""
    return CLI_BASE[:5] + ["--images", str(folder)] + CLI_BASE[7:]


def assert_select_maps(folder, stems, chosen):
    """``<stem>_select.png`` is 255 exactly where ``chosen`` (bool [images,H,W]) holds in the image the stem numbers."""
    import numpy as np
    from PIL import Image
    for stem in stems:
        with Image.open(folder / f"{stem}_select.png") as im:
            assert torch.equal(torch.from_numpy(np.array(im)) == 255, chosen[int(stem[-4:])])


def assert_same_files(a, b, count, but=("report.json",)):
    """Folder ``a`` holds ``count`` files and ``b`` the same bytes, but for ``but`` (a report lists the paths it wrote)."""
    files = sorted(os.path.relpath(p, a) for p in glob.glob(str(a / "**" / "*"), recursive=True) if os.path.isfile(p))
    assert len(files) == count
    for name in files:
        if name not in but:
            assert open(a / name, "rb").read() == open(b / name, "rb").read(), name


def apply_seed(Hl, Wl):
    """The seed of ``apply_maps`` and ``tile_selection`` at Hl x Wl: the first of Hl * 2000 + Wl + 10000 i at which
    both references show, keep and fill something and meet a bad target (tests/test_annotate_cpu.py says where)."""
    return Hl * 2000 + Wl + {(1, 3): 10000, (5, 1): 20000}.get((Hl, Wl), 0)


@functools.lru_cache(maxsize=None)
def apply_maps(N, Hl, Wl, nc, seed):
    """(sel, target, previous, fill, label) u8 [N,Hl,Wl] on the host, never modified.  ``previous`` and ``fill``: values
    over [0, nc + 2) and the drop id 250 on 60 % and 40 % of the pixels; ``sel``: ripu's, 255 chosen, 128 and 1 marks."""
    g = torch.Generator().manual_seed(seed)
    shape = (N, Hl, Wl)
    target = HC.make_target(nc, shape, IGNORE, seed)
    previous = torch.where(torch.rand(shape, generator=g) < 0.4, torch.randint(0, nc + 2, shape, generator=g, dtype=torch.uint8),
                           torch.tensor(DROP, dtype=torch.uint8))
    fill = torch.where(torch.rand(shape, generator=g) < 0.6, torch.randint(0, nc + 2, shape, generator=g, dtype=torch.uint8),
                       torch.tensor(DROP, dtype=torch.uint8))
    label = torch.randint(0, nc, shape, generator=g, dtype=torch.uint8)
    r = torch.rand(shape, generator=g)
    sel = torch.where(r < 0.3, 255, torch.where(r < 0.5, 128, torch.where(r < 0.55, 1, 0))).to(torch.uint8)
    return sel, target, previous, fill, label


def tile_selection(N, grid, seed):
    """acquire's ``selected``: u8 [N,Ty,Tx], about 40 % of the tiles chosen, by any non-zero byte."""
    g = torch.Generator().manual_seed(seed)
    shape = (N,) + tuple(grid)
    return (torch.rand(shape, generator=g) < 0.4).to(torch.uint8) * torch.randint(1, 256, shape, generator=g, dtype=torch.uint8)


def check_arena(arena, given, want, scalars):
    """What an apply kernel wrote for the outputs ``given`` into an ``HC.Arena`` that was read back: the maps, and on
    top of their sentinel the per-class counters and the ``scalars`` (one that stays 0 is not written); nothing else."""
    arena.assert_untouched([k for k in given if k not in scalars or want[k]], given)
    for k in given:
        if k in ("out", "mask"):
            assert torch.equal(arena.cut(k), want[k].reshape(-1)), (k, given)
        elif k in scalars:
            assert int(arena.cut(k).view(torch.int64) - SENTINEL) == want[k], (k, given)
        else:
            assert torch.equal(arena.cut(k).view(torch.int64) - SENTINEL, want[k]), (k, given)


def check_counters(counters, want, times):
    """Every device counter holds ``times`` x the reference's (an int or a tensor per name)."""
    for k, v in counters.items():
        w = want[k] if isinstance(want[k], torch.Tensor) else torch.tensor([want[k]])
        assert torch.equal(v.cpu(), times * w), (k, times)


# --------------------------------------------------------------------------- the CLI byte golden
@contextlib.contextmanager
def _inside(folder):
    """The working directory is ``folder``: every path of a case is relative, so no report names a temp folder."""
    before = os.getcwd()
    os.chdir(folder)
    try:
        yield
    finally:
        os.chdir(before)


_ACQ, _RIPU = ["--tile", "16", "16", "--budget", "0.1"], ["--radius", "4"]
_ROUND1 = ["--by", "random", "--seed", "3", "--out-root", "round1", "--layout", "BDD"]
_ROUND2 = ["--by", "uncertainty", "--previous", "round1/selection.json", "--out-root", "round2", "--layout", "BDD"]
_FULL = ["--json", "report.json", "--out-root", "tree", "--out", "maps"]
# name -> (program, the runs before it, its own flags); every path is relative to the case's own folder
CLI_CASES = {
    "acquire-ripu": ("acquire", [], _ACQ + _FULL + ["--by", "ripu", "--layout", "BDD"]),
    "acquire-oracle": ("acquire", [], _ACQ + _FULL + ["--by", "oracle", "--layout", "cityscapes"]),
    "acquire-round2": ("acquire", [_ACQ + _ROUND1],
                       _ACQ + _ROUND2 + ["--previous-root", "round1", "--max-per-image", "0.5", "--json", "r2.json"]),
    "acquire-fill": ("acquire", [_ACQ + _ROUND1], _ACQ + _ROUND2 + ["--fill-root", "round1", "--max-per-image", "0.5"]),
    "ripu-region": ("ripu", [], _RIPU + _FULL + ["--budget", "0.1", "--by", "ripu", "--layout", "BDD"]),
    "ripu-pixel": ("ripu", [], _RIPU + _FULL + ["--budget", "0.005", "--by", "oracle", "--layout", "cityscapes",
                                                "--select-radius", "0"]),
    "ripu-round2": ("ripu", [_RIPU + ["--budget", "0.1"] + _ROUND1],
                    _RIPU + ["--budget", "0.1"] + _ROUND2 + ["--previous-root", "round1", "--json", "r2.json"]),
    "ripu-images": ("ripu", [_RIPU + ["--budget", "0.1"] + _ROUND1], None),
    "audit-prune": ("audit", [], ["--json", "report.json", "--out", "maps", "--clean-root", "clean", "--layout", "BDD",
                                  "--mode", "prune", "--top", "5"]),
    "audit-relabel": ("audit", [], ["--json", "report.json", "--out", "maps", "--clean-root", "clean", "--layout",
                                    "cityscapes", "--mode", "relabel", "--top", "5"]),
}


def _sha(data):
    return hashlib.sha256(data).hexdigest()


def run_cli_case(name, state, folder):
    """Runs case ``name`` inside the empty ``folder`` -> {"report": sha256, "files": {relative path: sha256}}."""
    program, before, flags = CLI_CASES[name]
    with _inside(folder):
        for extra in before:
            run_cli(program, CLI_BASE + ["--subset", "val"], state, extra)
        if flags is None:                                  # ripu on the images an earlier run wrote, unlabelled
            report = run_cli(program, images_base("round1/images/val"), state,
                             _RIPU + ["--budget", "0.1", "--by", "ripu", "--out", "plain", "--json", "plain.json"])
        else:
            report = run_cli(program, CLI_BASE + ["--subset", "val"], state, flags)
        report = dict(report, written=[os.path.relpath(p, ".") for p in report["written"]])
        files = {}
        for root, _, names in os.walk("."):
            for n in names:
                path = os.path.relpath(os.path.join(root, n), ".")
                with open(path, "rb") as f:
                    files[path] = _sha(f.read())
    return {"report": _sha(json.dumps(report, sort_keys=True).encode()), "files": dict(sorted(files.items()))}


def record(path):
    sys.path.insert(0, REPO)
    import mdil_ss_amd  # noqa: F401
    assert torch.cuda.is_available(), "recording needs an MI355X"
    dev = torch.device("cuda", 0)
    digests = {}
    with tempfile.TemporaryDirectory() as tmp:
        state = os.path.join(tmp, "checkpoint.pth.tar")
        HC.save_checkpoint(HC.tiny_model(dev), state)
        for name in CLI_CASES:
            folder = os.path.join(tmp, name)
            os.makedirs(folder)
            digests[name] = run_cli_case(name, state, folder)
    with open(path, "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} invocations recorded in {path}")


if __name__ == "__main__":
    record(sys.argv[1])
