"""GPU: the five label-size command lines (fullres, ensemble, boundary, segments, significance) return
the reports and write the pixels they did before they came to share mdil_ss_amd/_labelsize_common.py.
The runs of tests/labelsize_cli_cases.py -- every branch of the shared loop: with and without a model,
one and two models, one and two folders of maps, one and several samplers, with and without maps to
write, a partial last batch -- are compared with tests/golden/labelsize_cli.json, recorded on an
MI355X from the drivers as they were.  Equality is exact: the counters are integer atomics, the
resampling is counter-based and the scores are host arithmetic on those integers."""
import json

import pytest

from tests import head_cases as HC
from tests import labelsize_cli_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(C.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got():
    return C.run_all(HC.device("label-size"))


def test_every_run_is_recorded(recorded):
    assert sorted(recorded) == sorted(name for name, _, _ in C.runs(""))


@pytest.mark.parametrize("name", [name for name, _, _ in C.runs("")])
def test_same_report_and_pixels_as_recorded(got, recorded, name):
    have, want = got[name], recorded[name]
    a, b = json.loads(have["report"]), json.loads(want["report"])
    assert sorted(a) == sorted(b)
    for key in a:
        assert json.dumps(a[key], sort_keys=True) == json.dumps(b[key], sort_keys=True), f"{name}: {key}"
    assert have["report"] == want["report"]
    assert have["pixels"] == want["pixels"], f"{name}: " + ", ".join(k for k in want["pixels"]
                                                                     if have["pixels"].get(k) != want["pixels"][k])
