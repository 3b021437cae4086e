"""The class-ordered walk (match_algo 3) at the limits of its tables, on the SIMT emulator (512 threads, an overlay of 8 lanes): the cases of
tests/classfit_limits_cases.py that fit the emulated suite's time (every pair, the smallest calls, one stale-state sequence, the EQUALS sweep, the twelve pools);
test_classfit_limits_gpu.py runs all of them."""
import pytest

from cook_amd.engine import Engine
from tests import classfit_limits_cases as L


@pytest.fixture(scope="module")
def make_engine():
    from tests.simt_emu import build_emu
    so = build_emu.build()
    return lambda params: Engine(params, lib_path=so)


@pytest.mark.parametrize("name", list(L.PAIRS))
def test_limit_pair(make_engine, name):
    """at the limit: the class-ordered form, at capacity, equal to the oracle and to match_algo 2; one beyond: refused with the word the rule gives"""
    L.run_pair(make_engine, name)


@pytest.mark.parametrize("which", L.SMALLEST)
def test_smallest_calls(make_engine, which):
    L.run_smallest(make_engine, which)


def test_lds_sum_equals_sweep(make_engine):
    L.run_sweep_equals(make_engine)


def test_stale_state_on_one_engine(make_engine, name="classes"):
    L.run_stale(make_engine, name)


# Left to the GPU file, for the time they take here (measured on one core of the build machine): the stale-state sequences of one_class and offers
# (37 s, 27 s: what they exercise — buffers that only grow, cf_init clearing by the current call's sizes — is host code and a clearing kernel that do
# not differ between the builds, and the classes sequence above runs it) and the sweep over running cotasks (576 s: thirteen calls of 4180 jobs, 4096
# of them group members, on 4096 offers; its form-3 side is the groups pair, its refused side the same sum as the EQUALS sweep's).


def test_more_pools_than_one_walk_launch_holds(make_engine):
    L.run_many_pools(make_engine)
