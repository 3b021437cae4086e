"""Rounding traps for the fp64 sums (tests/sum_order_cases.py) on the MI355X (cook_amd/libcookmatch.so, gfx950): the emulator
suite's cases, larger random placements, and the per-user usage written to a device buffer."""
import pytest

from tests import sum_order_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd import build
    from cook_amd.engine import Engine
    so = build.build()
    return lambda params: Engine(params, lib_path=so)


def test_pool_usage_traps(make_engine):
    S.check_pool_usage_cases(make_engine)


def test_pool_usage_random(make_engine):
    S.check_pool_usage_random(make_engine, seeds=range(24), n=300)
    S.check_pool_usage_random(make_engine, seeds=range(24, 32), n=175_000)


def test_pool_usage_multi(make_engine):
    S.check_pool_usage_multi(make_engine)


def test_rank_with_computed_pool_usage(make_engine):
    S.check_rank_pool_quota(make_engine)


def test_cycle_with_computed_pool_usage(make_engine):
    S.check_cycle_pool_quota(make_engine)


def test_user_usage_traps(make_engine):
    S.check_user_usage_cases(make_engine, device=True)


def test_user_usage_random(make_engine):
    S.check_user_usage_random(make_engine, seeds=range(6), n_users=30, n=3000, device=True)
    S.check_user_usage_random(make_engine, seeds=range(6, 8), n_users=400, n=60_000)


def test_rank_dru_and_over_quota_prefixes(make_engine):
    S.check_rank_traps(make_engine)
    S.check_rank_traps(make_engine, seeds=(4, 5), n_users=40, per_user=600)


def test_rank_queue_quota_prefixes(make_engine):
    S.check_rank_queue_quota(make_engine)


def test_considerable_computed_pool_usage(make_engine):
    S.check_considerable(make_engine)


def test_cycle_considerable_and_autoscale(make_engine):
    S.check_cycle_considerable_and_autoscale(make_engine)


def test_user_stats_traps(make_engine):
    S.check_user_stats(make_engine)
    S.check_user_stats(make_engine, n_users=60, seed=6)
