"""cook_usage_breakdown / cook_usage_breakdown_multi on a machine WITHOUT a GPU: the cook_amd/csrc sources compiled against the SIMT
emulator (tests/simt_emu), against the reference's golden answers and tests/usage_oracle.py (small sizes)."""
import pytest

from cook_amd import synth
from cook_amd.engine import Engine
from tests import usage_cases as S


@pytest.fixture(scope="module")
def make_engine():
    from tests.simt_emu import build_emu
    so = build_emu.build()
    return lambda params: Engine(params, lib_path=so)


def test_usage_golden(make_engine):
    S.check_golden(make_engine)


@pytest.mark.parametrize("kw", [
    dict(seed=71, n_pending=700, n_running=500, n_users=40, n_groups=60),
    dict(seed=72, n_pending=900, n_running=2600, n_users=9, n_groups=30, fractional=True, must_fold=True),  # multi-block scans, sums that round
    dict(seed=73, n_pending=400, n_running=300, n_users=60, n_groups=20, fractional=True, gpus=True, must_fold=True),
    dict(seed=74, n_pending=300, n_running=0, n_users=20, n_groups=5),
    dict(seed=75, n_pending=0, n_running=300, n_users=20, n_groups=300, fractional=True),
    dict(seed=76, n_pending=0, n_running=0, n_users=5, n_groups=3),
    dict(seed=77, n_pending=500, n_running=1500, n_users=300, n_groups=70000),  # group ids of three radix digits
], ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_usage_random(make_engine, kw):
    kw = dict(kw)
    must_fold, n_groups = kw.pop("must_fold", False), kw.pop("n_groups")
    S.check_random(make_engine, synth.make_pool(n_offers=8, **kw), n_groups, seed=kw["seed"], must_fold=must_fold)


def test_usage_every_row_its_own_group(make_engine):
    S.check_every_row_its_own_group(make_engine, synth.make_pool(seed=78, n_pending=300, n_running=900, n_users=30, n_offers=8, fractional=True))


def test_usage_one_group_for_all(make_engine):
    S.check_one_group_for_all(make_engine, synth.make_pool(seed=79, n_pending=300, n_running=900, n_users=30, n_offers=8, fractional=True))


def test_usage_long_segment_and_bucket(make_engine):
    """one user's segment and one of its buckets span several scan blocks: the cross-block carries of both scans, and the folds"""
    got, _ = S.check_long_segment_and_bucket(make_engine, S.one_user_pool(80, n_running=4200, n_pending=900), seed=80)
    assert got["bucket_usage"][:, 3].max() >= 3000


@pytest.mark.parametrize("n_engines,with_map", [(2, False), (3, True), (8, False), (5, True)])
def test_usage_multi(make_engine, n_engines, with_map):
    S.check_multi(make_engine, n_engines, seed=81 + n_engines, n_users=25, n_groups=40, with_map=with_map)


def test_usage_rounding_traps(make_engine):
    S.check_traps(make_engine)


def test_usage_negative_zero(make_engine):
    S.check_negative_zero(make_engine)


def test_usage_state_rule(make_engine):
    S.check_state_rule(make_engine)


def test_usage_leaves_the_cycle_alone(make_engine):
    S.check_cycle_undisturbed(make_engine, synth.make_pool(seed=88, n_pending=600, n_running=400, n_users=30, n_offers=24))
