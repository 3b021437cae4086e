"""cook_cycle_autoscale_multi / cook_match_metrics_multi on the MI355X (cook_amd/libcookmatch.so, gfx950): the cases of
tests/followup_cases.py at GPU sizes — four pools taken from the argument sets of test_autoscale_random, nine tiny pools (more than one
cook_multi launch takes), the failing engine, the rejections, the untouched cycle, the edge shapes — and the eight pools of the timed
configuration at K = 1000 after cook_cycle_match_multi."""
import numpy as np
import pytest

from cook_amd import _abi as A
from cook_amd import synth, workload
from cook_amd.engine import Engine, cycle_autoscale_multi, match_metrics_multi
from tests import autoscale_cases as S
from tests import followup_cases as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd import build
    so = build.build()
    return lambda params: Engine(params, lib_path=so)


def test_followups_ragged_pools(make_engine, multi_mode):
    """the pools of test_autoscale_random's argument sets: multi-block scans and sorts, fix-up paths, gpus and constraints, no running task"""
    sets = [dict(seed=81, n_pending=20000, n_running=10000, n_users=300, n_offers=800, k=4000),
            dict(seed=82, n_pending=9000, n_running=30000, n_users=9, n_offers=300, k=9000, fractional=True),
            dict(seed=83, n_pending=30000, n_running=20000, n_users=2000, n_offers=2000, k=3000, fractional=True, gpus=True, constraints=True),
            dict(seed=84, n_pending=6000, n_running=0, n_users=50, n_offers=8, k=1000, tokens=False, pool_quota=False)]
    pools, states, ks = [], [], []
    for kw in sets:
        kw = dict(kw)
        seed, k = kw.pop("seed"), kw.pop("k")
        state = {x: kw.pop(x) for x in ("tokens", "pool_quota", "enforce") if x in kw}
        pools.append(synth.make_pool(seed=seed, **kw))
        states.append(S.random_state(pools[-1], seed, fractional=kw.get("fractional", False), **state))
        ks.append(k)
    n_users = [300, 9 + 5, 0, 50]  # (pool 2: the per-user arrays are left out)
    got, met = F.check_parity(make_engine, pools, A.default_params(good_enough_fitness=1.0), states, ks, F.mixed_call_sets(pools), n_users)
    info = [[r[1] for r in g] for g in got]
    assert all(m["considerable"] > 0 and m["offers_scheduled"] > 0 for m in met)
    assert info[0][0]["autoscalable"] == info[0][0]["scaled"] == info[0][0]["unmatched"] > 0  # max_jobs cut the list at N = u
    assert 0 < info[0][1]["n_out"] < info[0][1]["autoscalable"]                                 # the exclude list took candidates
    assert info[1][3]["unmatched"] == info[1][3]["considered"] > 0                              # every match skipped


def test_followups_nine_pools(make_engine):
    F.check_nine_pools(make_engine)


def test_followups_one_engine_fails(make_engine):
    F.check_one_engine_fails(make_engine, n_pending=3000)


def test_followups_whole_call_rejections(make_engine):
    F.check_rejections(make_engine)


def test_followups_leave_the_cycle_alone(make_engine):
    F.check_cycle_undisturbed(make_engine, n_pending=8000, k=1000)


def test_followups_edge_shapes(make_engine):
    F.check_edges(make_engine)


def test_followups_timed_pools(make_engine):
    """the eight timed pools at K = 1000, both multi calls after cook_cycle_match_multi; the autoscale oracle takes the engine's placement
    (the placement itself is the parity suites' business)"""
    spec = workload.ClusterSpec()
    pools = [workload.make_pool(spec, p) for p in range(spec.pools)]
    states = [S.random_state(pl, 40 + i) for i, pl in enumerate(pools)]
    rng = np.random.default_rng(3)
    calls = [[dict(offer_skipped=(rng.random(pl.offers.n) < 0.3).astype(np.uint8) if i % 2 else None, max_jobs=1000 if i % 4 else 300,
                   exclude_tasks="exclude" if i % 3 == 0 else None) for i, pl in enumerate(pools)]]
    got, met = F.check_parity(make_engine, pools, A.default_params(), states, 1000, calls, [spec.users] * len(pools), oracle_match=False)
    assert all(m["considerable"] > 0 for m in met) and any(r[1]["n_out"] > 0 for r in got[0])
    with F.Pools(make_engine, pools[:2], A.default_params(), states[:2], 1000) as P:  # (what the batch did: a pool batch of two)
        cycle_autoscale_multi(P.engines, [None, None])
        a = P.engines[0].batch_stats()
        match_metrics_multi(P.engines, n_users=spec.users)
        m = P.engines[0].batch_stats()
        assert a["pools"] == 2 and m["pools"] == 2 and a["grouped_launches"] >= 1 and m["grouped_launches"] >= 1, (a, m)
