"""The class-ordered walk (match_algo 3) at the limits of its tables, on the GPU: every pair, the smallest calls, the stale-state sequences and
both LDS sweeps of tests/classfit_limits_cases.py.  No CPU fallback: without the library or the GPU these tests FAIL."""
import pytest

from cook_amd.engine import Engine
from tests import classfit_limits_cases as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd import build
    so = build.build()
    return lambda params: Engine(params, lib_path=so)


@pytest.mark.parametrize("name", list(L.PAIRS))
def test_limit_pair(make_engine, name):
    """at the limit: the class-ordered form, at capacity, equal to the oracle and to match_algo 2; one beyond: refused with the word the rule gives"""
    L.run_pair(make_engine, name)


@pytest.mark.parametrize("which", L.SMALLEST)
def test_smallest_calls(make_engine, which):
    L.run_smallest(make_engine, which)


@pytest.mark.parametrize("name", L.STALE)
def test_stale_state_on_one_engine(make_engine, name):
    L.run_stale(make_engine, name)

def test_lds_sum_equals_sweep(make_engine):
    L.run_sweep_equals(make_engine)


def test_lds_sum_groups_sweep(make_engine):
    L.run_sweep_groups(make_engine)


def test_more_pools_than_one_walk_launch_holds(make_engine):
    L.run_many_pools(make_engine)
