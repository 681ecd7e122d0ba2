"""No GPU: what acquire, ripu and audit share on the host (mdil_ss_amd/_annotate_common.py) -- the label tree
writer on CPU tensors, opened by the trainers' dataset classes, and every shared refusal through every parser
that uses it -- and the conditions on the one draw of maps that the two GPU suites' apply tests rely on
(tests/annotate_cases.py), against both references."""
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import acquire_reference as QR
from tests import annotate_cases as AC
from tests import ripu_reference as RR

N, H, W, NC = 3, 8, 12, 20
IGNORE = NC - 1                                   # the trainers' relabelled ignore class


# ------------------------------------------------------------------------- the label tree writer
@pytest.mark.parametrize("layout", ("BDD", "cityscapes"))
def test_label_tree_writer_on_cpu_tensors(tmp_path, layout):
    """Two batches (2 + 1 images); image 1 has nothing selected.  The tree opens in the layout's own dataset class."""
    from PIL import Image
    from mdil_ss_amd import _annotate_common as ac
    from mdil_ss_amd import _head_common as hc
    from mdil_ss_amd import dataset as D
    g = torch.Generator().manual_seed(5)
    images = torch.rand(N, 3, H, W, generator=g)
    labels = torch.randint(0, NC, (N, H, W), generator=g, dtype=torch.uint8)
    assert bool((labels == IGNORE).any())
    stems = [f"synthetic_{j:04d}" for j in range(N)]
    root, out = tmp_path / "tree", tmp_path / "maps"
    args = Namespace(synthetic=N, layout=layout, subset="val", dataset=None)
    with hc.png_pool() as pool:
        writer = ac.LabelTreeWriter(pool, args, "--out-root", str(root), str(out), images=N)
        assert writer.batch_names([1]) == [writer.names[1]]
        writer.wait()
        writer.write_maps(stems[:1], select=labels[:1])
        writer.write_batch(stems[:2], images[:2], labels[:1], IGNORE, rows=[0])          # image 1: nothing selected
        assert writer.seen == 2 and writer.batch_names([0]) == [writer.names[2]]
        writer.wait()
        writer.write_batch(stems[2:], images[2:], labels[2:], IGNORE)
        written = writer.close()
    assert len(written) == len(set(written)) == 1 + 2 * N and all(os.path.isfile(p) for p in written)
    on_disk = sorted(os.path.join(d, f) for d, _, files in os.walk(tmp_path) for f in files)
    assert sorted(written) == on_disk                                                     # every file, once
    assert written[0] == str(out / "synthetic_0000_select.png")                           # maps, then labels, then images
    ds = (D.BDD100k if layout == "BDD" else D.cityscapes)(str(root), subset="val")
    assert len(ds) == N and len(ds.filenamesGt) == N
    want = torch.where(labels == IGNORE, torch.tensor(255, dtype=torch.uint8), labels)
    want[1] = 255
    for i in range(N):
        image, label = ds[i]
        assert image.size == (W, H)
        assert torch.equal(torch.from_numpy(np.array(label)), want[i]), i
        with Image.open(written[1 + N + i]) as im:                                        # the procedural image itself
            pic = (images[i].permute(1, 2, 0) * 255.0).round().clamp(0, 255).to(torch.uint8)
            assert torch.equal(torch.from_numpy(np.array(im)), pic)


def test_label_tree_writer_counts_the_names(tmp_path):
    from mdil_ss_amd import _annotate_common as ac
    from mdil_ss_amd import _head_common as hc
    args = Namespace(synthetic=N, layout="BDD", subset="val", dataset=None)
    with hc.png_pool() as pool:
        with pytest.raises(RuntimeError, match=f"--clean-root: {N} label names for {N + 1} images"):
            ac.LabelTreeWriter(pool, args, "--clean-root", str(tmp_path / "a"), None, images=N + 1)
        writer = ac.LabelTreeWriter(pool, args, "--out-root", str(tmp_path / "b"), None)
        writer.write_batch(["synthetic_0000"], torch.zeros(1, 3, H, W), None, IGNORE, rows=[])
        with pytest.raises(RuntimeError, match=f"--out-root: {N} label names for 1 images"):
            writer.close()
        none = ac.LabelTreeWriter(pool, args, "--out-root", None, None)                  # neither folder: nothing written
        none.write_batch(["synthetic_0000"], torch.zeros(1, 3, H, W), None, IGNORE)
        assert none.close() == []


# ------------------------------------------------------------------------- the shared refusals
BASE = ["--state", "ckpt.pth.tar", "--num-classes", "20", "20", "--task", "1"]
SYN = ["--synthetic", "2", "--budget", "0.1"]
ROOT = {"acquire": "--out-root", "ripu": "--out-root", "audit": "--clean-root"}
# (the parsers that share it, argv after BASE with @ROOT for the tree's flag, the message)
REFUSALS = (
    (("acquire", "ripu"), ["--budget", "0.1", "--json", "r"], "give one source of images"),
    (("acquire", "ripu"), SYN + ["--dataset", "BDD", "--json", "r"], "give one source of images"),
    (("acquire", "ripu"), SYN + ["--batch-size", "0", "--json", "r"], "sizes and --batch-size must be positive"),
    (("acquire", "ripu"), SYN + ["--height", "63", "--json", "r"], "--height and --width must be even"),
    (("acquire", "ripu"), SYN, "nothing to do: give --json FILE, --out DIR or --out-root ROOT"),
    (("acquire", "ripu"), ["--synthetic", "2", "--budget", "1.5", "--json", "r"], r"--budget 1.5 outside \(0, 1\]: a share of"),
    (("acquire", "ripu"), ["--images", "d", "--budget", "0.1", "--by", "oracle", "--json", "r"], "--by oracle needs labels"),
    (("acquire", "ripu"), ["--images", "d", "--budget", "0.1", "@ROOT", "x", "--layout", "BDD"], "it needs labels"),
    (("acquire", "ripu"), SYN + ["@ROOT", "x"], "@ROOT and --layout cityscapes.BDD go together"),
    (("acquire", "ripu"), SYN + ["--json", "r", "--layout", "BDD"], "@ROOT and --layout cityscapes.BDD go together"),
    (("audit",), ["--synthetic", "2", "@ROOT", "x"], "@ROOT and --layout cityscapes.BDD go together"),
    (("acquire", "ripu"), ["--dataset", "IDD", "--budget", "0.1", "@ROOT", "x", "--layout", "BDD"], "@ROOT does not take --dataset IDD"),
    (("audit",), ["--dataset", "IDD", "@ROOT", "x", "--layout", "BDD"], "@ROOT does not take --dataset IDD"),
    (("acquire", "ripu"), SYN + ["--json", "r", "--fill-root", "f"], "they need --out-root and --layout"),
    (("acquire", "ripu"), SYN + ["@ROOT", "x", "--layout", "BDD", "--previous-root", "p"], "goes with --previous SEL.json"),
)


@pytest.mark.parametrize("programs, argv, text", REFUSALS)
def test_shared_refusals_through_every_parser(programs, argv, text, capsys):
    import importlib
    for program in programs:
        parser = importlib.import_module(f"mdil_ss_amd.{program}").build_parser()
        with pytest.raises(SystemExit):
            parser.parse_args(BASE + [ROOT[program] if a == "@ROOT" else a for a in argv])
        assert re.search(text.replace("@ROOT", ROOT[program]), capsys.readouterr().err), (program, text)


def test_shared_flags_read_alike():
    """The seventeen shared flags of acquire and ripu: the same defaults from the same code."""
    from mdil_ss_amd import acquire as A
    from mdil_ss_amd import ripu as P
    a, p = (m.build_parser().parse_args(BASE + SYN + ["--json", "r"]) for m in (A, P))
    for name in ("state", "num_classes", "task", "images", "dataset", "subset", "synthetic", "height", "width", "batch_size",
                 "budget", "kind", "by", "seed", "previous", "previous_root", "fill_root", "json", "out", "out_root", "layout"):
        assert getattr(a, name) == getattr(p, name), name
    assert a.subset == "train" and a.kind == "entropy" and a.by == "ripu" and a.seed == 0


def test_open_head_checks_paths_before_the_checkpoint(tmp_path):
    """The checkpoint does not exist: the task and the paths of earlier rounds are refused before it would be opened."""
    from mdil_ss_amd import _annotate_common as ac
    args = Namespace(state=str(tmp_path / "none.pth.tar"), num_classes=[20, 20], task=2, previous=None, previous_root=None,
                     fill_root=None)
    with pytest.raises(RuntimeError, match="--task 2: the model has tasks 0 to 1"):
        ac.open_head(args)
    for name, flag, what in (("previous", "--previous", "file"), ("previous_root", "--previous-root", "folder"),
                             ("fill_root", "--fill-root", "folder")):
        bad = Namespace(**dict(vars(args), task=1, **{name: str(tmp_path / "missing")}))
        with pytest.raises(RuntimeError, match=f"{flag} .*missing: no such {what}"):
            ac.open_head(bad)


def test_drivers_bind_the_shared_functions():
    from mdil_ss_amd import _annotate_common as ac
    from mdil_ss_amd import acquire as A
    from mdil_ss_amd import audit as U
    from mdil_ss_amd import ripu as P
    assert A._read_labels is ac.read_labels
    for fn in (A.plan_label_tree, U.plan_clean_tree, A.read_selection, P.read_selection, A.new_apply_counters,
               P.new_apply_counters):
        assert callable(fn)


# --------------------------------------------------------------------- the draw of the apply tests
@pytest.mark.parametrize("Wl", AC.APPLY_WIDTHS)
@pytest.mark.parametrize("Hl", AC.APPLY_HEIGHTS)
def test_the_draw_meets_every_branch_in_both_references(Hl, Wl):
    """previous and fill hold nc and nc + 1 and the drop id on a large share; at every size with at least 4 pixels
    both references show, keep and fill something, and at the wide sizes a chosen target is out of range."""
    N_, nc = AC.APPLY_N, AC.APPLY_NC
    sel, target, previous, fill, label = AC.apply_maps(N_, Hl, Wl, nc, AC.apply_seed(Hl, Wl))
    for m in (sel, target, previous, fill, label):
        assert m.dtype == torch.uint8 and tuple(m.shape) == (N_, Hl, Wl)
    if Wl >= 1001:
        for m in (previous, fill):
            assert bool((m == nc).any()) and bool((m == nc + 1).any()) and int(m[m != AC.DROP].max()) == nc + 1
            assert 0.3 < float((m == AC.DROP).float().mean()) < 0.7
    wants = [RR.apply_ref(sel, nc, target, previous, fill, label, AC.IGNORE, AC.DROP)]
    for tile in AC.APPLY_TILES:
        chosen = AC.tile_selection(N_, QR.grid((Hl, Wl), tile), AC.apply_seed(Hl, Wl))
        wants.append(QR.apply_ref(chosen, (Hl, Wl), tile, nc, target, previous, fill, AC.IGNORE, AC.DROP))
    if N_ * Hl * Wl >= 4:
        for want in wants:
            assert want["shown"] > 0 and int(want["kept"].sum()) > 0 and int(want["filled"].sum()) > 0
            if Wl >= 1001:
                assert want["bad_targets"] > 0
