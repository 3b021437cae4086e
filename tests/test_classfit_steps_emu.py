"""The cases of tests/classfit_steps_cases.py (the decider's run of plain steps and what makes it leave) on the SIMT emulator, where the C++ step takes
every job: placements, failure codes and head_matched of match_algo 3 against the oracle and match_algo 2, form 3 without a refusal, and the events
each case is built around (epochs at 8 live overlay lanes in the emulated build).  A case the form refused, or whose event did not happen, would test
nothing on the GPU either."""
import pytest

from tests import classfit_steps_cases as C


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd.engine import Engine
    from tests.simt_emu import build_emu
    so = build_emu.build()
    return lambda params: Engine(params, lib_path=so)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_decider_runs(make_engine, name):
    C.check_case(make_engine, name)
