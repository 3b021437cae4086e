"""The rebalancer over the pool's resident cycle state (cook_cycle_rebalance_stage, cook_cycle_rebalance_fetch) on the MI355X
(cook_amd/libcookmatch.so, gfx950): the cases of tests/resident_rebalance_cases.py against the oracle of
tests/resident_rebalance_oracle.py."""
import os
import subprocess
import sys

import pytest

from cook_amd.engine import Engine
from tests import resident_rebalance_cases as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd import build
    so = build.build()
    return lambda params: Engine(params, lib_path=so)


def test_resident_rebalance_base(make_engine):
    X.check_base(make_engine)


@pytest.mark.parametrize("R", X.boundary_sizes())
def test_resident_rebalance_running_rows(make_engine, R):
    X.check_running_rows(make_engine, R)


def test_resident_rebalance_row_ends(make_engine):
    X.check_row_ends(make_engine)


def test_resident_rebalance_max_preemption(make_engine):
    X.check_max_preemption(make_engine)


def test_resident_rebalance_masks(make_engine):
    X.check_masks(make_engine)


def test_resident_rebalance_fullest_host(make_engine):
    X.check_fullest_host(make_engine)


def test_resident_rebalance_rescoring_paths(make_engine):
    X.check_rescoring_paths(make_engine)


def test_resident_rebalance_update(make_engine):
    X.check_update(make_engine)


def test_resident_rebalance_update_without_host(make_engine):
    X.check_update_without_host(make_engine)


def test_resident_rebalance_skip_matched(make_engine):
    X.check_skip_matched(make_engine)


def test_resident_rebalance_sources(make_engine):
    X.check_sources(make_engine)


def test_resident_rebalance_golden(make_engine):
    X.check_golden(make_engine)


def test_resident_rebalance_refusals(make_engine):
    X.check_refusals(make_engine)


def test_resident_rebalance_untouched(make_engine):
    X.check_untouched(make_engine)


def test_resident_rebalance_loop(make_engine):
    X.check_loop(make_engine)


def test_resident_rebalance_guarded_run():
    """the base, boundary, update and sources cases once more in a process of its own with every device buffer between two guard bands
    (COOK_GUARD=1 is read when the library is loaded): all pass, and no write outside a buffer is reported"""
    env = dict(os.environ, COOK_GUARD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "base or running_rows or row_ends or update or sources or max_preemption"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "COOK_GUARD: " not in r.stderr, r.stderr[-1500:]
