"""The resident pod table (cook_offers_stage_pod_ids, cook_offers_update, cook_offers_fetch_pods, cook_cycle_set_built_offers,
cook_cycle_run_queue_pods*) on the MI355X (cook_amd/libcookmatch.so, gfx950): the cases of tests/podtable_cases.py, every cycle against the oracle of
tests/podtable_oracle.py."""
import os
import subprocess
import sys

import pytest

from cook_amd.engine import Engine
from tests import podtable_cases as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

@pytest.fixture(scope="module")
def make_engine():
    from cook_amd import build
    so = build.build()
    return lambda params: Engine(params, lib_path=so)


def test_podtable_by_hand(make_engine):
    X.check_by_hand(make_engine)


@pytest.mark.parametrize("n_nodes", X.BOUNDARY_NODES)
@pytest.mark.parametrize("n_pods", X.BOUNDARY_PODS)
def test_podtable_boundary(make_engine, n_pods, n_nodes):
    X.check_boundary(make_engine, n_pods, n_nodes)


def test_podtable_big_node(make_engine):
    X.check_big_node(make_engine)


def test_podtable_order_rule(make_engine):
    X.check_order_rule(make_engine)


@pytest.mark.parametrize("slots", [1, 4])
def test_podtable_every_column(make_engine, slots):
    X.check_columns(make_engine, slots)


@pytest.mark.parametrize("users,k", X.QUEUE_CASES)
def test_podtable_queue(make_engine, users, k):
    X.check_queue(make_engine, users, k)


@pytest.mark.parametrize("algo,form", [(1, 1), (3, 3)])
def test_podtable_placement_forms(make_engine, algo, form):
    X.check_queue(make_engine, 6, 64, algo=algo, expect_form=form)


def test_podtable_queue_groups(make_engine):
    X.check_queue_groups(make_engine)


def test_podtable_reservations_and_limiters(make_engine):
    X.check_reserve_limiters(make_engine)


def test_podtable_queue_edges(make_engine):
    X.check_queue_edges(make_engine)


def test_podtable_rank_between(make_engine):
    X.check_rank_between(make_engine)


def test_podtable_multi(make_engine):
    X.check_multi(make_engine)


def test_podtable_refusals_and_state(make_engine):
    X.check_refusals(make_engine)


def test_podtable_guarded_run():
    """every other test of this file once more in a process of its own with every device buffer between two guard bands (COOK_GUARD=1
    is read when the library is loaded): all pass, and no write outside a buffer is reported"""
    env = dict(os.environ, COOK_GUARD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "not guarded_run"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "COOK_GUARD: " not in r.stderr, r.stderr[-1500:]
