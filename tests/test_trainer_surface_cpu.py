"""CPU: the public surface of the six trainers and evaluate.py -- every flag of every parser, the
signatures of build_parser / main / train / eval / make_loaders and the names bench.py, the tools
and the other tests import -- against tests/golden/trainer_surface.json, which
tools/dump_trainer_surface.py recorded from the commit before the trainers were moved onto
mdil_ss_amd/trainer_common.py."""
import json
import os

import pytest

from tools import dump_trainer_surface as D

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "trainer_surface.json")


@pytest.fixture(scope="module")
def surfaces():
    mp = pytest.MonkeyPatch()
    D.pin_environment(mp.setenv, lambda k: mp.delenv(k, raising=False))
    try:
        return D.surface(), json.load(open(GOLDEN))
    finally:
        mp.undo()


@pytest.mark.parametrize("module", D.MODULES)
def test_parser_actions(surfaces, module):
    got, want = (s[module]["actions"] for s in surfaces)
    assert [a["dest"] for a in got] == [a["dest"] for a in want]
    for g, w in zip(got, want):
        assert g == w, w["dest"]


@pytest.mark.parametrize("module", D.MODULES)
def test_signatures_and_names(surfaces, module):
    got, want = (s[module] for s in surfaces)
    assert got["signatures"] == want["signatures"]
    assert want["names"] == sorted(D.NAMES[module])        # the fixture's commit had every listed name
    assert got["names"] == want["names"]


def test_module_globals_stay_assignable():
    """``T.current_task = t`` followed by ``T.is_DS_curr(n)`` is how bench.py and the tests drive it."""
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import train_new_task_step2 as T2
    from mdil_ss_amd import train_new_task_step3 as T3
    name = "encoder.layers.1.bns_1.{}.weight"
    for T in (T2, T3):
        before = T.current_task
        try:
            for t in (1, 2):
                T.current_task = t
                assert T.is_DS_curr(name.format(t)) and not T.is_DS_curr(name.format(t - 1))
                assert T.is_DS_curr("decoder.{}.output_conv.weight".format(t))
        finally:
            T.current_task = before
    assert T3.is_DS_curr is not T2.is_DS_curr          # each reads its own module global
