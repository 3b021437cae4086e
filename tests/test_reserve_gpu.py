"""The host reservations (cook_cycle_set_reservations, cook_cycle_run_queue_reserve*, cook_cycle_fetch_reservations) on the MI355X
(cook_amd/libcookmatch.so, gfx950): the cases of tests/reserve_cases.py, every cycle against the oracle of tests/reserve_oracle.py."""
import os
import subprocess
import sys

import pytest

from cook_amd.engine import Engine
from tests import reserve_cases as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

@pytest.fixture(scope="module")
def make_engine():
    from cook_amd import build
    so = build.build()
    return lambda params: Engine(params, lib_path=so)


def test_reserve_base(make_engine):
    X.check_base(make_engine)


def test_reserve_by_hand(make_engine):
    X.check_by_hand(make_engine)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_reserve_list_length(make_engine, n):
    X.check_list_length(make_engine, n)


@pytest.mark.parametrize("k", [63, 64, 65])
def test_reserve_considered(make_engine, k):
    X.check_considered(make_engine, k)


def test_reserve_host_ids(make_engine):
    X.check_host_ids(make_engine)


def test_reserve_skipped_and_removal(make_engine):
    X.check_skipped_and_removal(make_engine)


def test_reserve_no_advance(make_engine):
    X.check_no_advance(make_engine)


def test_reserve_rank_cycle(make_engine):
    X.check_rank_cycle(make_engine)


def test_reserve_last_match_stays_described(make_engine):
    X.check_last_match_described(make_engine)


def test_reserve_class_ordered_walk(make_engine):
    X.check_classfit(make_engine)


def test_reserve_multi(make_engine, multi_mode):
    X.check_multi(make_engine)


def test_reserve_refusals(make_engine):
    X.check_refusals(make_engine)


def test_reserve_explain(make_engine):
    X.check_explain(make_engine)


@pytest.mark.parametrize("case", X.golden()["atom"], ids=lambda c: c["name"].replace(" ", "_"))
def test_reserve_golden_atom(make_engine, case):
    X.check_golden_atom(case)
    X.check_golden_engine(make_engine, case)


@pytest.mark.parametrize("case", X.golden()["match"], ids=lambda c: c["name"].replace(" ", "_"))
def test_reserve_golden_match(make_engine, case):
    X.check_golden_match(make_engine, case)


def test_reserve_guarded_run():
    """every other test of this file once more in a process of its own with every device buffer between two guard bands (COOK_GUARD=1
    is read when the library is loaded): all pass, and no write outside a buffer is reported"""
    env = dict(os.environ, COOK_GUARD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "not guarded_run"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "COOK_GUARD: " not in r.stderr, r.stderr[-1500:]
