"""The host churn (cook_cycle_run_queue_hosts*) and cook_cycle_fetch_offers on a machine WITHOUT a GPU: the cook_amd/csrc sources
compiled against the SIMT emulator (tests/simt_emu), every cycle against the oracle of tests/churn_oracle.py (cases in
tests/churn_cases.py)."""
import pytest

from cook_amd.engine import Engine
from tests import churn_cases as X


@pytest.fixture(scope="module")
def make_engine():
    from tests.simt_emu import build_emu
    so = build_emu.build()
    return lambda params: Engine(params, lib_path=so)


def test_churn_base(make_engine):
    X.check_base(make_engine)


def test_churn_non_dyadic(make_engine):
    X.check_base(make_engine, fractional=True)


def test_churn_order_rule(make_engine):
    X.check_order(make_engine)


@pytest.mark.parametrize("slots", [1, 4])
def test_churn_every_column(make_engine, slots):
    X.check_columns(make_engine, slots=slots)


def test_churn_null_columns(make_engine):
    X.check_null_columns(make_engine)


@pytest.mark.parametrize("M", [63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_churn_boundary(make_engine, M):
    X.check_boundary(make_engine, M)


def test_churn_empty_tables(make_engine):
    X.check_empty_tables(make_engine)


def test_churn_no_advance(make_engine):
    X.check_no_advance(make_engine)


def test_churn_sparse_host_ids(make_engine):
    X.check_no_advance(make_engine, hosts=(5, 4000000, 9000000))


def test_churn_groups(make_engine):
    X.check_groups(make_engine)


def test_churn_class_ordered_walk(make_engine):
    X.check_classfit(make_engine)


def test_churn_multi(make_engine, multi_mode):
    X.check_multi(make_engine)


def test_churn_refusals_and_persistence(make_engine):
    X.check_refusals(make_engine)


def test_churn_built_offers(make_engine):
    X.check_built_offers(make_engine)


def test_fetch_offers(make_engine):
    X.check_fetch(make_engine)


def test_fetch_offers_by_every_route(make_engine):
    X.check_fetch_routes(make_engine)
