"""cook_unscheduled on a machine WITHOUT a GPU: the cook_amd/csrc sources compiled against the SIMT emulator (tests/simt_emu),
against the reference's golden reasons and tests/unscheduled_oracle.py (small sizes)."""
import pytest

from cook_amd import synth
from tests import unscheduled_cases as S
from cook_amd.engine import Engine


@pytest.fixture(scope="module")
def make_engine():
    from tests.simt_emu import build_emu
    so = build_emu.build()
    return lambda params: Engine(params, lib_path=so)


def test_unscheduled_golden(make_engine):
    S.check_golden(make_engine)


@pytest.mark.parametrize("kw", [
    dict(seed=61, n_pending=700, n_running=500, n_users=40),
    dict(seed=62, n_pending=900, n_running=2600, n_users=9, fractional=True, must_fold=True),  # multi-block scans, prefixes that round
    dict(seed=63, n_pending=400, n_running=300, n_users=60, fractional=True, gpus=True, must_fold=True),
    dict(seed=64, n_pending=300, n_running=0, n_users=20),
    dict(seed=65, n_pending=0, n_running=300, n_users=20, fractional=True),
    dict(seed=66, n_pending=0, n_running=0, n_users=5),
], ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_unscheduled_random(make_engine, kw):
    kw = dict(kw)
    must_fold = kw.pop("must_fold", False)
    S.check_random(make_engine, synth.make_pool(n_offers=8, **kw), seed=kw["seed"], must_fold=must_fold)


def test_unscheduled_one_long_segment(make_engine):
    """one user's segment spans several scan blocks: the cross-block carry of the listed counts and of the running sums"""
    S.check_random(make_engine, S.one_user_pool(67, n_running=3000, n_pending=2500), seed=67, must_fold=True)


def test_unscheduled_state_rule(make_engine):
    S.check_state_rule(make_engine)


def test_unscheduled_leaves_the_cycle_alone(make_engine):
    S.check_cycle_undisturbed(make_engine, synth.make_pool(seed=68, n_pending=600, n_running=400, n_users=30, n_offers=24))
