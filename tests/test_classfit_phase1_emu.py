"""The class-ordered walk's batch-end summary pass (one pass over the batch's log, lane = entry) on the SIMT emulator: placements, failure codes
and the walked count of match_algo 3 against the oracle, match_algo 2 and a second, freshly built engine.  The cases: tests/classfit_phase1_cases.py
(the emulated build ends an epoch at 8 live overlay lanes, so epochs fall inside batches in most of them)."""
import pytest

from tests import classfit_phase1_cases as C


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd.engine import Engine
    from tests.simt_emu import build_emu
    so = build_emu.build()
    return lambda params: Engine(params, lib_path=so)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_batch_end_summaries(make_engine, name):
    C.check_case(make_engine, name)
