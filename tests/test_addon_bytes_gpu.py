"""GPU: the three inference add-ons and the two report add-ons (drift, calib) write the bytes they
wrote before they came to share mdil_ss_amd/ext/head_common.h.  Every output buffer (label, colour,
confidence as raw float bytes, confusion, bad-target count; of drift and calib every map, counter
and fp64 sum, of their meters the report) of the cases in tests/addon_bytes_cases.py is compared, as
a SHA-256, with tests/golden/addon_bytes.json, recorded on an MI355X from the unshared kernel sources.
Equality is exact: there is no tolerance."""
import json

import pytest
import torch

from tests import addon_bytes_cases as A

pytestmark = pytest.mark.gpu

CASES = A.cases()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the add-ons need an MI355X"
    import mdil_ss_amd  # noqa: F401
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def recorded():
    with open(A.GOLDEN) as f:
        return json.load(f)


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_same_bytes_as_recorded(dev, recorded, name):
    got = CASES[name](dev)
    assert all(v is not None for v in got.values()), got
    assert got == recorded[name], f"{name}: " + ", ".join(k for k in got if got[k] != recorded[name].get(k))
