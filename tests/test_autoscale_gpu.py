"""cook_cycle_autoscale on the MI355X (cook_amd/libcookmatch.so, gfx950): the emulator suite's cases at GPU sizes, one C4 pool at
K = 1000 and at K = all, a 500 000-pending queue, and the eight pools of the timed configuration after cook_cycle_match_multi under both
placement modes, every call against the oracle of tests/autoscale_cases.py."""
import pytest

from cook_amd import _abi as A
from cook_amd import synth, workload
from cook_amd.engine import Engine
from tests import autoscale_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd import build
    so = build.build()
    return lambda params: Engine(params, lib_path=so)


def test_autoscale_golden(make_engine):
    S.check_golden(make_engine)


@pytest.mark.parametrize("kw", [
    dict(seed=81, n_pending=20000, n_running=10000, n_users=300, n_offers=800, k=4000),
    dict(seed=82, n_pending=9000, n_running=30000, n_users=9, n_offers=300, k=9000, fractional=True),
    dict(seed=83, n_pending=30000, n_running=20000, n_users=2000, n_offers=2000, k=3000, fractional=True, gpus=True, constraints=True),
    dict(seed=84, n_pending=6000, n_running=0, n_users=50, n_offers=8, k=1000, tokens=False, pool_quota=False),
], ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_autoscale_random(make_engine, kw):
    kw = dict(kw)
    seed, k = kw.pop("seed"), kw.pop("k")
    state = {x: kw.pop(x) for x in ("tokens", "pool_quota", "enforce") if x in kw}
    pool = synth.make_pool(seed=seed, **kw)
    S.check_random(make_engine, pool, seed, k, fractional=kw.get("fractional", False), **state)


def test_autoscale_c4_pool_k1000(make_engine):
    got = S.check_random(make_engine, workload.make_pool(workload.ClusterSpec(), 0), 40, 1000)
    assert got[0][1]["considered"] > 0


def test_autoscale_c4_pool_k_all(make_engine):
    """K = every pending job (the placement of 125 000 jobs is compared by the parity suites; here the oracle takes the engine's)"""
    pool = workload.make_pool(workload.ClusterSpec(), 1)
    S.check_random(make_engine, pool, 41, pool.pending_jobs.n, oracle_match=False)


def test_autoscale_500k_pending(make_engine):
    pool = synth.make_pool(seed=0xC00C0005, n_pending=500_000, n_running=200_000, n_users=10_000, n_offers=20_000)
    S.check_random(make_engine, pool, 50, 1000, n_calls=3, masked_queue=True)


def test_autoscale_timed_pools(make_engine, multi_mode):
    spec = workload.ClusterSpec()
    pools = [workload.make_pool(spec, p) for p in range(spec.pools)]
    S.check_multi(make_engine, pools, A.default_params(), 1000)


def test_autoscale_state_rule(make_engine):
    S.check_state_rule(make_engine, synth.make_pool(seed=86, n_pending=3000, n_running=2000, n_users=120, n_offers=160))


def test_autoscale_leaves_the_cycle_alone(make_engine):
    S.check_cycle_undisturbed(make_engine, synth.make_pool(seed=87, n_pending=20000, n_running=10000, n_users=300, n_offers=500), k=1000)
