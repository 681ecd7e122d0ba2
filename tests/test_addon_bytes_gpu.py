"""GPU: the three inference add-ons and the two report add-ons (drift, calib) write the bytes they
wrote before they came to share mdil_ss_amd/ext/head_common.h, and the map add-ons (pseudo, openset,
audit, acquire, route) the bytes they wrote before they came to share mdil_ss_amd/ext/map_common.h.
Every output buffer (label, colour, confidence as raw float bytes, confusion, bad-target count; of drift
and calib every map, counter and fp64 sum, of their meters the report; of the map add-ons every map and
every counter of their eleven kernels) of the cases in tests/addon_bytes_cases.py is compared, as a
SHA-256, with tests/golden/addon_bytes.json and tests/golden/map_addon_bytes.json, recorded on an
MI355X from the unshared kernel sources.  Equality is exact: there is no tolerance."""
import json

import pytest
import torch

from tests import addon_bytes_cases as A

pytestmark = pytest.mark.gpu

TABLES = ((A.cases(), A.GOLDEN), (A.map_cases(), A.MAP_GOLDEN))
CASES = {name: run for table, _ in TABLES for name, run in table.items()}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the add-ons need an MI355X"
    import mdil_ss_amd  # noqa: F401
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def recorded():
    files = []
    for _, path in TABLES:
        with open(path) as f:
            files.append(json.load(f))
    return files


def test_every_case_is_recorded(recorded):
    assert sum(len(table) for table, _ in TABLES) == len(CASES)          # no name in both tables
    for (table, _), golden in zip(TABLES, recorded):
        assert sorted(golden) == sorted(table)


@pytest.mark.parametrize("name", list(CASES))
def test_same_bytes_as_recorded(dev, recorded, name):
    want = next(golden[name] for golden in recorded if name in golden)
    got = CASES[name](dev)
    assert all(v is not None for v in got.values()), got
    assert got == want, f"{name}: " + ", ".join(k for k in got if got[k] != want.get(k))
