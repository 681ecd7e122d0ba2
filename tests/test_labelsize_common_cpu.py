"""CPU: what the label-size drivers share (mdil_ss_amd/_labelsize_common.py).  The batch loop on the
CPU device with a stub sampler, a folder of label PNGs and a recording writer; the meters' shared
prologue up to the point where the device call would start; the runs of equal sizes; and the surface
of the five parsers against tests/golden/labelsize_parsers.json, recorded before the drivers came to
share their flag builder."""
import json
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from tests import labelsize_cli_cases as C

A, B = (6, 9), (4, 9)
SIZES = (A, A, B, A, A)
STEMS = [f"item_{i}" for i in range(5)]
METERS = (("BoundaryMeter", "boundary_count", "boundary"), ("SegmentMeter", "segments_label", "segments"),
          ("SignificanceMeter", "signif_count", "significance"))


def _labels():
    rng = np.random.default_rng(3)
    return [rng.integers(0, 20, size, dtype=np.uint8) for size in SIZES]


def _write_maps(folder, sizes=SIZES):
    from PIL import Image
    rng = np.random.default_rng(4)
    maps = [rng.integers(0, 20, size, dtype=np.uint8) for size in sizes]
    for stem, m in zip(STEMS, maps):
        Image.fromarray(m).save(folder / f"{stem}_label.png")
    return maps


class Recorder:
    """A PngWriter's two methods, recorded in the order they are called."""

    def __init__(self):
        self.calls = []

    def wait(self):
        self.calls.append("wait")

    def submit(self, arr, name):
        self.calls.append((name, arr.copy()))


def test_runs_of_equal_sizes():
    from mdil_ss_amd._labelsize_common import runs
    assert runs([(2, 3)]) == [(0, 1)]
    assert runs([(2, 3), (2, 3), (4, 3), (2, 3), (2, 3), (2, 3)]) == [(0, 2), (2, 3), (3, 6)]


def test_loop_yields_the_runs_of_every_batch_and_bounds_the_writer(tmp_path):
    from mdil_ss_amd import _labelsize_common as ls
    labels, maps = _labels(), _write_maps(tmp_path)
    sampled = []

    def sample(i):
        sampled.append(i)
        return np.zeros((2, 2, 3), dtype=np.uint8), labels[i]

    png, seen = Recorder(), []
    with ThreadPoolExecutor(2) as pool:
        for run in ls.label_runs((5, STEMS, sample), pool, torch.device("cpu"), 4, folders=[str(tmp_path)], png=png):
            seen.append(run)
            run.write("_twice.png", run.sources[0].numpy() * 2)
            run.write("_none.png", None)
    assert sorted(sampled) == [0, 1, 2, 3, 4]
    spans = [(0, 2), (2, 3), (3, 4), (4, 5)]                   # batch 1: [0,2) [2,3) [3,4); batch 2: [0,1)
    assert [run.stems for run in seen] == [STEMS[s:e] for s, e in spans]
    for run, (s, e) in zip(seen, spans):
        assert run.target.dtype == torch.uint8 and torch.equal(run.target, torch.from_numpy(np.stack(labels[s:e])))
        assert len(run.sources) == 1 and torch.equal(run.sources[0], torch.from_numpy(np.stack(maps[s:e])))
    # the writer: wait, the first batch's four maps in order, wait, the second batch's one, the final wait
    names = [c if c == "wait" else c[0] for c in png.calls]
    assert names == ["wait"] + [f"{s}_twice.png" for s in STEMS[:4]] + ["wait", "item_4_twice.png", "wait"]
    for (name, arr), m in zip([c for c in png.calls if c != "wait"], maps):
        assert np.array_equal(arr, m * 2)


def test_loop_refuses_a_map_of_another_size(tmp_path):
    from mdil_ss_amd import _labelsize_common as ls
    labels = _labels()
    _write_maps(tmp_path, (A, B, B, A, A))                     # item_1: 4 x 9 where its label is 6 x 9
    data = (5, STEMS, lambda i: (np.zeros((2, 2, 3), dtype=np.uint8), labels[i]))
    with ThreadPoolExecutor(2) as pool:
        with pytest.raises(RuntimeError, match=r"item_1_label.png is 4 x 9, its label 6 x 9"):
            list(ls.label_runs(data, pool, torch.device("cpu"), 4, folders=[str(tmp_path)]))


def test_loop_hands_the_hook_every_samplers_images():
    """Two samplers (the ensemble's one per input size) and a stub model: the hook gets the batch's
    images per sampler, and its cut the bounds of every run."""
    from mdil_ss_amd import _labelsize_common as ls
    labels, got = _labels(), []

    def sampler(fill):
        return lambda i: (np.full((2, 2, 3), fill + i, dtype=np.uint8), labels[i])

    def heads(models, task, images, dev):
        got.append((models, task, [[int(im[0, 0, 0]) for im in per] for per in images]))
        return lambda s, e: [("cut", s, e)]

    with ThreadPoolExecutor(2) as pool:
        runs = list(ls.label_runs((5, STEMS, [sampler(0), sampler(100)]), pool, torch.device("cpu"), 4, ["model"], 1,
                                  heads=heads))
    assert got == [(["model"], 1, [[0, 1, 2, 3], [100, 101, 102, 103]]), (["model"], 1, [[4], [104]])]
    assert [run.sources for run in runs] == [[("cut", 0, 2)], [("cut", 2, 3)], [("cut", 3, 4)], [("cut", 0, 1)]]


@pytest.mark.parametrize("who", METERS, ids=[m[0] for m in METERS])
def test_prologue_refusals_are_worded_by_the_meter(who):
    from mdil_ss_amd import _labelsize_common as ls
    meter, fn, path = who
    pred, target = torch.zeros(1, 6, 9, dtype=torch.uint8), torch.zeros(1, 6, 9, dtype=torch.uint8)
    x, w, b = torch.zeros(1, 2, 2, 16), torch.zeros(16, 20, 2, 2), torch.zeros(20)
    expects = (rf"mdil {meter}\.add: expects \(pred, target\), \(model, images, task, target=\.\.\.\) or "
               r"\(features, weight, bias, target=\.\.\.\)$")
    for source, t in (((pred,), None), ((pred, target, pred), None), ((x, w), target), ((x, w, b, b), target)):
        with pytest.raises(RuntimeError, match=expects):
            ls.label_maps(who, source, t)
    with pytest.raises(RuntimeError, match=rf"mdil {meter}\.add: expects \(a, b, target=\.\.\.\), each of a and b a "
                                           r"label map, \(model, images, task\) or \(features, weight, bias\)$"):
        ls.label_maps(who, (pred, target), None, paired=True)
    for bad in ("target", np.zeros((1, 6, 9), dtype=np.uint8), torch.zeros(6, 9, dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match=rf"mdil {meter}\.add: target must be a uint8 \[N,H,W\] device tensor$"):
            ls.label_maps(who, (x, w, b), bad)
    # accepted up to the device: the target is judged first, then every predictor in turn
    device = rf"mdil {fn}: target must be a contiguous uint8 device tensor .*no CPU fallback in the {path} path"
    with pytest.raises(RuntimeError, match=device):
        ls.label_maps(who, (pred, target), None)
    with pytest.raises(RuntimeError, match=device):
        ls.label_maps(who, (x, w, b), target)
    with pytest.raises(RuntimeError, match=device):
        ls.label_maps(who, (pred, (x, w, b)), target, paired=True)


@pytest.mark.parametrize("who", METERS, ids=[m[0] for m in METERS])
def test_prologue_checks_every_predictor_against_the_target(who, monkeypatch):
    """With the device check of the tensors' home stubbed out: the size mismatch and the predictor
    that is neither a map nor a triple are refused in the meter's name, and the paired form with a
    map and a triple gives the map and the head's label map, in order."""
    from mdil_ss_amd import _labelsize_common as ls
    from mdil_ss_amd import fullres as F
    meter = who[0]
    monkeypatch.setattr(ls.hc, "chk", lambda *a, **k: None)
    monkeypatch.setattr(F, "fullres_head",
                        lambda x, w, b, size: (torch.full((x.shape[0],) + size, 7, dtype=torch.uint8), None))
    pred, target = torch.zeros(2, 6, 9, dtype=torch.uint8), torch.ones(2, 6, 9, dtype=torch.uint8)
    x, w, b = torch.zeros(2, 2, 2, 16), torch.zeros(16, 20, 2, 2), torch.zeros(20)
    with pytest.raises(RuntimeError, match=rf"mdil {meter}\.add: pred \(2, 4, 9\) and target \(2, 6, 9\) must be uint8 "
                                           r"\[N,H,W\] maps of one size$"):
        ls.label_maps(who, (pred[:, :4].contiguous(), target), None)
    with pytest.raises(RuntimeError, match=rf"mdil {meter}\.add: a predictor is a uint8 \[N,H,W\] label map, \(model, "
                                           r"images, task\) or \(features, weight, bias\)$"):
        ls.label_maps(who, (pred, "folder"), target, paired=True)
    (a, head), t = ls.label_maps(who, (pred, (x, w, b)), target, paired=True)
    assert a is pred and t is target and head.shape == target.shape and int(head.min()) == 7
    (only,), t = ls.label_maps(who, (x, w, b), target)
    assert t is target and torch.equal(only, head)
    (only,), t = ls.label_maps(who, (pred, target), None)
    assert only is pred and t is target


def test_bad_pixels_are_refused_in_the_meters_name():
    from mdil_ss_amd import _report_common as rc
    zero, three = torch.zeros(1, dtype=torch.int64), torch.tensor([3])
    rc.refuse_bad_pixels("SegmentMeter", 20, 19, zero)
    rc.refuse_bad_pixels("SegmentMeter", 20, 19, zero, zero)
    with pytest.raises(RuntimeError, match=r"mdil SegmentMeter: 3 target pixels are outside \[0, 20\) and are not the "
                                           r"ignore index 19$"):
        rc.refuse_bad_pixels("SegmentMeter", 20, 19, three, three)
    with pytest.raises(RuntimeError, match=r"mdil BoundaryMeter: 3 predicted pixels are outside \[0, 20\)$"):
        rc.refuse_bad_pixels("BoundaryMeter", 20, 19, zero, three)
    with pytest.raises(RuntimeError, match="mdil DriftMeter: 3 target pixels are outside"):
        rc.refuse_bad_targets("DriftMeter", {"bad_targets": three}, 20, 19)


@pytest.mark.parametrize("program", C.PROGRAMS)
def test_parser_surface_is_the_recorded_one(program):
    """Option strings, dest, default, required, choices, nargs and help of every flag, as recorded
    before the five parsers came to share ``add_flags``."""
    with open(C.PARSERS_GOLDEN) as f:
        want = json.load(f)[program]
    got = C.parser_surface(program)
    assert [row[1] for row in got] == [row[1] for row in want]
    for g, w in zip(got, want):
        assert g == w, g[1]
