"""The class-ordered walk's batch-end summary pass on the GPU (libcookmatch.so, gfx950): the cases of tests/classfit_phase1_cases.py, as
tests/test_classfit_phase1_emu.py runs them on the emulator.  No CPU fallback: without the library or the GPU these tests FAIL."""
import pytest

from tests import classfit_phase1_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd import build
    from cook_amd.engine import Engine
    so = build.build()
    return lambda params: Engine(params, lib_path=so)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_batch_end_summaries(make_engine, name):
    C.check_case(make_engine, name)
