"""The decider's run of plain steps on the GPU (libcookmatch.so, gfx950): the cases of tests/classfit_steps_cases.py, as
tests/test_classfit_steps_emu.py runs them on the emulator.  No CPU fallback: without the library or the GPU these tests FAIL.
(Which steps the hand-placed loop took and which the C++ step, per case: profiles/r10a_decider_loop.txt, from a -DCF_PROF build.)"""
import pytest

from tests import classfit_steps_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd import build
    from cook_amd.engine import Engine
    so = build.build()
    return lambda params: Engine(params, lib_path=so)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_decider_runs(make_engine, name):
    C.check_case(make_engine, name)
