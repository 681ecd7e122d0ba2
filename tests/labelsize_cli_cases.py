"""The cases of tests/test_labelsize_cli_gpu.py and of the parser test in
tests/test_labelsize_common_cpu.py: the five label-size command lines (fullres, ensemble, boundary,
segments, significance) run in-process on ``--synthetic 3`` at a native size of 96 x 200 through a
64 x 128 network, two batches of which the second is a partial one, and the surface of their five
parsers.  Per run the returned report (the paths of ``written`` relative to the run's folder) and a
SHA-256 of the decoded pixels of every PNG written, to be compared with tests/golden/labelsize_cli.json;
per parser the sorted list of (option strings, dest, default, required, choices, nargs, help), to be
compared with tests/golden/labelsize_parsers.json.

    python tests/labelsize_cli_cases.py FILE.json              # record the runs (needs an MI355X)
    python tests/labelsize_cli_cases.py --parsers FILE.json    # record the parsers

Both files were recorded from the drivers as they were BEFORE they came to share
mdil_ss_amd/_labelsize_common.py and are not re-recorded: they are the proof that sharing changed no
report, no pixel and no flag.  Every counter is a sum of integer atomics, the resampling draws from a
counter-based generator and the scores are host arithmetic on those integers, so equality is exact.
A run is ``M.main(M.build_parser().parse_args(argv))`` and nothing else, so the file runs on both sides."""
import copy
import hashlib
import importlib
import json
import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "labelsize_cli.json")
PARSERS_GOLDEN = os.path.join(REPO, "tests", "golden", "labelsize_parsers.json")
PROGRAMS = ("fullres", "ensemble", "boundary", "segments", "significance")
CLASSES = ["--num-classes", "20", "20"]
DATA = ["--task", "1", "--synthetic", "3", "--native-height", "96", "--native-width", "200", "--height", "64",
        "--width", "128", "--batch-size", "2"]
REPLICATES = ["--replicates", "200"]


def runs(root):
    """[(name, program, argv)] in the order they run: the ``--pred`` runs read the maps of
    ``fullres-plain`` (and of ``ensemble``, the second folder of the pair)."""
    def at(name):
        return os.path.join(root, name)

    state = ["--state", at("a.pth.tar")] + CLASSES
    plain = ["--pred", at("fullres-plain")] + CLASSES
    return [
        ("fullres", "fullres", state + DATA + ["--score", "--out", at("fullres"), "--colour", "--label-ids",
                                               "cityscapes"]),
        ("fullres-plain", "fullres", state + DATA + ["--out", at("fullres-plain")]),
        ("ensemble", "ensemble", state + DATA + ["--scales", "1", "0.75", "--flip", "--confidence", "--score", "--out",
                                                 at("ensemble")]),
        ("boundary-state", "boundary", state + DATA + ["--widths", "1", "3", "8", "--score", "--out",
                                                       at("boundary-state")]),
        ("boundary-pred", "boundary", plain + DATA + ["--ratio", "0.02", "--score"]),
        ("segments-state", "segments", state + DATA + ["--score", "--out", at("segments-state")]),
        ("segments-pred", "segments", plain + DATA + ["--score", "--out", at("segments-pred")]),
        ("significance-state", "significance", state + DATA + REPLICATES),
        ("significance-pair", "significance", ["--before", at("a.pth.tar"), "--before-num-classes", "20", "20",
                                               "--after", at("b.pth.tar"), "--after-num-classes", "20", "20"] + DATA
         + REPLICATES),
        ("significance-pred", "significance", plain + ["--pred-b", at("ensemble")] + DATA + REPLICATES),
    ]


def checkpoints(dev, root):
    """``a.pth.tar``: HC.tiny_model; ``b.pth.tar``: the same with the bias of task 1's head moved by a seeded draw."""
    from tests import head_cases as HC
    model = HC.tiny_model(dev)
    HC.save_checkpoint(model, os.path.join(root, "a.pth.tar"))
    moved = copy.deepcopy(model)
    bias = moved.head_params(1)[1]
    with torch.no_grad():
        bias.add_(0.5 * torch.randn(bias.shape, generator=torch.Generator().manual_seed(41)).to(dev))
    HC.save_checkpoint(moved, os.path.join(root, "b.pth.tar"))


def pixel_digest(path):
    """SHA-256 of the decoded pixels (with their shape and type), not of the file's bytes."""
    from PIL import Image
    with Image.open(path) as im:
        arr = np.array(im)
    return hashlib.sha256(f"{arr.shape} {arr.dtype} ".encode() + np.ascontiguousarray(arr).tobytes()).hexdigest()


def run_all(dev):
    """{name: {"report": the report as canonical JSON text, "pixels": {relative path: sha256}}}."""
    out = {}
    with tempfile.TemporaryDirectory() as root:
        checkpoints(dev, root)
        for name, program, argv in runs(root):
            M = importlib.import_module(f"mdil_ss_amd.{program}")
            report = dict(M.main(M.build_parser().parse_args(argv)))
            written = report.get("written", [])
            if "written" in report:
                report["written"] = [os.path.relpath(p, root) for p in written]
            out[name] = {"report": json.dumps(report, sort_keys=True),
                         "pixels": {os.path.relpath(p, root): pixel_digest(p) for p in written}}
    return out


def parser_surface(program):
    """The sorted list of [option strings, dest, default, required, choices, nargs, help] of a parser."""
    p = importlib.import_module(f"mdil_ss_amd.{program}").build_parser()
    rows = [[list(a.option_strings), a.dest, a.default, bool(a.required),
             None if a.choices is None else list(a.choices), a.nargs, a.help] for a in p._actions]
    return json.loads(json.dumps(sorted(rows, key=lambda r: (r[1], r[0]))))


def _write(obj, path):
    with open(path, "w") as f:
        json.dump(obj, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    import mdil_ss_amd  # noqa: F401
    if sys.argv[1] == "--parsers":
        _write({program: parser_surface(program) for program in PROGRAMS}, sys.argv[2])
    else:
        assert torch.cuda.is_available(), "recording needs an MI355X"
        _write(run_all(torch.device("cuda", 0)), sys.argv[1])
