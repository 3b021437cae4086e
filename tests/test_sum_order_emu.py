"""Rounding traps for the fp64 sums (tests/sum_order_cases.py) on a machine WITHOUT a GPU: the cook_amd/csrc sources compiled
against the SIMT emulator (tests/simt_emu), once with the emulated suite's small launch shapes and once with the shipped ones."""
import pytest

from tests import sum_order_cases as S


@pytest.fixture(scope="module", params=[False, True], ids=["small-shapes", "shipped-shapes"])
def make_engine(request):
    from cook_amd.engine import Engine
    from tests.simt_emu import build_emu
    so = build_emu.build(shipped_shapes=request.param)
    return lambda params: Engine(params, lib_path=so)


def test_pool_usage_traps(make_engine):
    S.check_pool_usage_cases(make_engine)


def test_pool_usage_random(make_engine):
    S.check_pool_usage_random(make_engine, seeds=range(12), n=300)
    S.check_pool_usage_random(make_engine, seeds=range(12, 16), n=40000)


def test_pool_usage_multi(make_engine):
    S.check_pool_usage_multi(make_engine)


def test_rank_with_computed_pool_usage(make_engine):
    S.check_rank_pool_quota(make_engine)


def test_cycle_with_computed_pool_usage(make_engine):
    S.check_cycle_pool_quota(make_engine)


def test_user_usage_traps(make_engine):
    S.check_user_usage_cases(make_engine)


def test_user_usage_random(make_engine):
    S.check_user_usage_random(make_engine, seeds=range(6), n_users=30, n=3000)


def test_rank_dru_and_over_quota_prefixes(make_engine):
    S.check_rank_traps(make_engine)


def test_rank_queue_quota_prefixes(make_engine):
    S.check_rank_queue_quota(make_engine)


def test_considerable_computed_pool_usage(make_engine):
    S.check_considerable(make_engine)


def test_cycle_considerable_and_autoscale(make_engine):
    S.check_cycle_considerable_and_autoscale(make_engine)


def test_user_stats_traps(make_engine):
    S.check_user_stats(make_engine)
