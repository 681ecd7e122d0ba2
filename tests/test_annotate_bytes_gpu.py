"""GPU: the command lines of acquire, ripu and audit write the bytes they wrote before the three drivers came to
share mdil_ss_amd/_annotate_common.py and the two apply kernels the annotator's rule in mdil_ss_amd/ext/map_common.h.
For the ten invocations of tests/annotate_cases.py (both criteria, a second round on an earlier round's tree and
on fill labels, region and pixel mode, unlabelled images, both cleaning modes) every file written and the returned
report are compared, as SHA-256, with tests/golden/annotate_cli.json, recorded on an MI355X from the sources before
the move.  Equality is exact: there is no tolerance."""
import json

import pytest

from tests import annotate_cases as AC
from tests import head_cases as HC
from tests.annotate_cases import checkpoint  # noqa: F401  (a fixture: the tiny model's checkpoint)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return HC.device("annotator")


@pytest.fixture(scope="module")
def recorded():
    with open(AC.GOLDEN) as f:
        return json.load(f)


def test_every_invocation_is_recorded(recorded):
    assert sorted(recorded) == sorted(AC.CLI_CASES)


@pytest.mark.parametrize("name", list(AC.CLI_CASES))
def test_same_files_and_report_as_recorded(dev, checkpoint, recorded, tmp_path, name):  # noqa: F811
    got, want = AC.run_cli_case(name, checkpoint, str(tmp_path)), recorded[name]
    assert sorted(got["files"]) == sorted(want["files"]), name
    assert got["files"] == want["files"], f"{name}: " + ", ".join(k for k in got["files"] if got["files"][k] != want["files"][k])
    assert got["report"] == want["report"], f"{name}: the report"
