"""The launch-rate limiters kept on the device (cook_cycle_set_limiters, cook_cycle_set_clock, cook_cycle_limiters_spend,
cook_cycle_fetch_limiters) on the MI355X (cook_amd/libcookmatch.so, gfx950): the cases of tests/limiter_cases.py, every cycle against
the oracle of tests/limiter_oracle.py."""
import os
import subprocess
import sys

import pytest

from cook_amd.engine import Engine
from tests import limiter_cases as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd import build
    so = build.build()
    return lambda params: Engine(params, lib_path=so)


def test_limiter_by_hand(make_engine):
    X.check_by_hand(make_engine)


@pytest.mark.parametrize("users,k", X.CASES)
def test_limiter_differential(make_engine, users, k):
    X.check_differential(make_engine, users, k)


def test_limiter_earn_set(make_engine):
    X.check_earn_set(make_engine)


@pytest.mark.parametrize("how", ["none", "backwards", "fraction"])
def test_limiter_clock(make_engine, how):
    X.check_clock(make_engine, how)


def test_limiter_spend(make_engine):
    X.check_spend(make_engine)


@pytest.mark.parametrize("n", [1, 65])
def test_limiter_listed_replace(make_engine, n):
    X.check_listed(make_engine, n)


def test_limiter_persistence(make_engine):
    X.check_persistence(make_engine)


def test_limiter_drop(make_engine):
    X.check_drop(make_engine)


def test_limiter_late_install(make_engine):
    X.check_late_install(make_engine)


def test_limiter_multi(make_engine, multi_mode):
    X.check_multi(make_engine)


@pytest.mark.parametrize("algo,form", [(1, 1), (3, 3)])
def test_limiter_placement_forms(make_engine, algo, form):
    X.check_forms(make_engine, algo, form)


def test_limiter_edges(make_engine):
    X.check_edges(make_engine)


def test_limiter_refusals(make_engine):
    X.check_refusals(make_engine)


def test_limiter_guarded_run():
    """every other test of this file once more in a process of its own with every device buffer between two guard bands (COOK_GUARD=1
    is read when the library is loaded): all pass, and no write outside a buffer is reported"""
    env = dict(os.environ, COOK_GUARD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "not guarded_run"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "COOK_GUARD: " not in r.stderr, r.stderr[-1500:]
