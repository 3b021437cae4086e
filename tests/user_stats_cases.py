"""The cases of cook_user_stats / cook_user_stats_multi, shared by the emulator (test_user_stats_emu.py) and GPU
(test_user_stats_gpu.py) suites: the reference's golden counters, hand-derived merge quirks, random pools against
tests/user_stats_oracle.py bit for bit, the multi form, the state rule, and that a stats call leaves the cycle alone."""
from __future__ import annotations

import numpy as np
import pytest

from cook_amd import _abi as A
from cook_amd import synth
from cook_amd.engine import CookError, user_stats_multi
from tests import golden_util as _G
from tests import user_stats_oracle as O

STATES = A.USER_STATS_STATES
COOK_E_INVALID, COOK_E_STATE = -1, -4


def _tasks(rows):
    """rows of (user id, cpus, mem, pending) -> Tasks (priority 50, creation order = row order)"""
    n = len(rows)
    col = lambda k, dt: np.array([r[k] for r in rows], dtype=dt)  # noqa: E731
    pend = col(3, np.uint8) if n else np.zeros(0, np.uint8)
    return A.Tasks(cpus=col(1, np.float64) if n else np.zeros(0), mem=col(2, np.float64) if n else np.zeros(0),
                   user=col(0, np.uint32) if n else np.zeros(0, np.uint32), priority=np.full(n, 50, np.int32),
                   start_ms=np.where(pend == 1, 0, 1_000 + np.arange(n)).astype(np.int64), task_id=(10_000 + np.arange(n)).astype(np.int64),
                   job_id=(100 + np.arange(n)).astype(np.int64), pending=pend)


def _users_for(n):
    return A.Users(div_cpus=np.full(max(n, 0), A.DMAX), div_mem=np.full(max(n, 0), A.DMAX))


def golden_limits(case, n):
    def q(k, default):
        return np.full(n, float(case["quota"][k]) if case["quota"] else default)
    sh = case["shares"]
    extra = None
    if case["quota"]:
        extra = np.full(n, int(case["quota"]["launch-rate-saved"] > 0 and case["quota"]["launch-rate-per-minute"] > 0), np.uint8)
    return A.UserLimits(share_cpus=np.full(n, float(sh["cpus"]) if sh else A.DMAX), share_mem=np.full(n, float(sh["mem"]) if sh else A.DMAX),
                        quota_count=q("count", 2.0 ** 31 - 1), quota_cpus=q("cpus", A.DMAX), quota_mem=q("mem", A.DMAX), quota_gpus=q("gpus", A.DMAX),
                        extra_quota_positive=extra)


def _check_golden(case, names, got):
    for state, rows in case["expect"].items():
        s = STATES.index(state)
        for who, want in rows.items():
            row = got["all"][s] if who == "all" else got["per_user"][names.index(who), s]
            assert [O.long_cast(v) for v in row] == want, (case["ref"], case["pool"], state, who, row.tolist(), want)
    for k, v in case["counts"].items():
        assert got["counts"][k] == v, (case["ref"], k, got["counts"], v)


def check_golden(make_engine):
    for case in _G.load("user_stats"):
        names = sorted({j["user"] for j in case["jobs"]} | {u for rows in case["expect"].values() for u in rows if u != "all"})
        n = len(names)
        lim = golden_limits(case, n)
        engines, pools = [], []
        try:
            for pool in case["member_pools"]:
                rows = [(names.index(j["user"]), j["cpus"], j["mem"], int(j["state"] == "waiting")) for j in case["jobs"] if j["pool"] == pool]
                t = _tasks(rows)
                e = make_engine(A.default_params())
                engines.append(e)
                e.rank_stage(t, _users_for(n))
                e.rank_run()
                pools.append((t, None))
            want = O.user_stats(pools, n, lim)
            got = engines[0].user_stats(lim) if len(engines) == 1 else user_stats_multi(engines, lim)
            _check_golden(case, names, want)  # (the restatement reproduces the reference's counters ...)
            _check_golden(case, names, got)   # (... and so does the engine)
            O.assert_same(got, want)
        finally:
            for e in engines:
                e.close()


def check_quirks(make_engine):
    """hand-derived: starved :jobs = min(w.jobs, r.jobs) with running stats (monitor.clj:77-78: :jobs only exists in running), w.jobs
    without; shares / quotas at 0 and MAX; extra quota keys at 0; users without tasks"""
    # users: 0 "ann" 2 running (1 cpu, 10 mem each) + 5 waiting (2 / 20); 1 "ben" 3 waiting; 2 "cy" no task; 3 "dee" 1 running
    rows = [(0, 1.0, 10.0, 0), (0, 1.0, 10.0, 0)] + [(0, 2.0, 20.0, 1)] * 5 + [(1, 3.0, 30.0, 1)] * 3 + [(3, 4.0, 40.0, 0)]
    t = _tasks(rows)
    lim = A.UserLimits(share_cpus=np.array([100.0, 8.0, 5.0, A.DMAX]), share_mem=np.array([1000.0, 50.0, 5.0, A.DMAX]),
                       quota_count=np.array([4.0, 10.0, 0.0, 2.0 ** 31 - 1]), quota_cpus=np.array([A.DMAX, 0.0, 1.0, A.DMAX]),
                       quota_mem=np.array([A.DMAX, A.DMAX, 1.0, A.DMAX]), quota_gpus=np.array([1.0, 1.0, 1.0, 0.0]))
    with make_engine(A.default_params()) as e:
        e.rank_stage(t, _users_for(4))
        e.rank_run()
        got = e.user_stats(lim)
        O.assert_same(got, O.user_stats([(t, None)], 4, lim))
        pu = got["per_user"]
        assert pu[0, 2].tolist() == [2.0, 10.0, 100.0]   # starved ann: jobs min(5, 2), cpus min(10, 100 - 2), mem min(100, 1000 - 20)
        assert pu[1, 2].tolist() == [3.0, 8.0, 50.0]     # starved ben, no running stats: jobs w.jobs, min(w, share)
        assert pu[0, 3].tolist() == [2.0, 10.0, 100.0]   # ann under quota: jobs min(5, max(4 - 2, 0))
        assert got["state"].tolist() == [15, 6, 0, 1]     # ben: quota cpus 0 -> not under quota; cy: absent everywhere
        assert got["counts"] == {"total": 3, "starved": 2, "waiting-under-quota": 1, "hungry": 0, "satisfied": 1}
        assert got["all"][1].tolist() == [8.0, 19.0, 190.0]
        # extra quota keys at 0 (a launch-rate quota of 0): nobody waits under quota
        lim0 = A.UserLimits(lim.share_cpus, lim.share_mem, lim.quota_count, lim.quota_cpus, lim.quota_mem, lim.quota_gpus,
                            extra_quota_positive=np.array([0, 1, 1, 1], np.uint8))
        got0 = e.user_stats(lim0)
        O.assert_same(got0, O.user_stats([(t, None)], 4, lim0))
        assert got0["counts"]["waiting-under-quota"] == 0 and got0["state"][0] == 7
        # shares at 0: nobody starves; at MAX everyone waiting does
        for v, starved in ((0.0, 0), (A.DMAX, 2)):
            lv = A.UserLimits(np.full(4, v), np.full(4, v))
            gv = e.user_stats(lv)
            O.assert_same(gv, O.user_stats([(t, None)], 4, lv))
            assert gv["counts"]["starved"] == starved
        # no limits: the staged users (divisors as shares)
        users = A.Users(div_cpus=lim.share_cpus, div_mem=lim.share_mem, quota_count=lim.quota_count, quota_cpus=lim.quota_cpus,
                        quota_mem=lim.quota_mem, quota_gpus=lim.quota_gpus)
        e.rank_stage(t, users)
        e.rank_run()
        O.assert_same(e.user_stats(), got)


def random_limits(seed, n):
    rng = np.random.default_rng(seed)
    pick = lambda vals: np.asarray(vals, dtype=np.float64)[rng.integers(0, len(vals), n)]  # noqa: E731
    return A.UserLimits(share_cpus=pick([0.0, 8.0, 64.0, 64.1, A.DMAX]), share_mem=pick([0.0, 40960.0, 262144.0, 262144.3, A.DMAX]),
                        quota_count=pick([0.0, 5.0, 50.0, 2.0 ** 31 - 1]), quota_cpus=pick([0.0, 20.0, 200.5, A.DMAX]),
                        quota_mem=pick([1.0, 1e5, 1e6, A.DMAX]), quota_gpus=pick([0.0, 10.0, A.DMAX, A.DMAX]),
                        extra_quota_positive=(rng.random(n) < 0.9).astype(np.uint8))


def check_random(make_engine, pool: synth.Pool, seed=1):
    n = pool.users.n
    lim = random_limits(seed, n)
    with make_engine(A.default_params()) as e:
        e.rank_stage(pool.tasks, pool.users)
        e.rank_run()
        got = e.user_stats(lim)
        want = O.user_stats([(pool.tasks, None)], n, lim)
        O.assert_same(got, want)
        O.assert_same(e.user_stats(), O.user_stats([(pool.tasks, None)], n, A.UserLimits.from_users(pool.users)))
    return got


def check_multi(make_engine, pools, n_users, seed=7):
    """the group form over pools whose user ids map into the group's by a non-identity map (a permutation into a larger id space),
    against the restatement over the concatenated pools; against the single form for one pool; an engine twice is refused"""
    rng = np.random.default_rng(seed)
    maps = [rng.permutation(n_users)[:pl.users.n].astype(np.uint32) for pl in pools]
    lim = random_limits(seed, n_users)
    engines = [make_engine(A.default_params()) for _ in pools]
    try:
        for e, pl in zip(engines, pools):
            e.rank_stage(pl.tasks, pl.users)
            e.rank_run()
        got = user_stats_multi(engines, lim, maps)
        want = O.user_stats([(pl.tasks, m) for pl, m in zip(pools, maps)], n_users, lim)
        O.assert_same(got, want)
        # reversed pool order: the concatenation changes, so may the sums; the restatement follows
        O.assert_same(user_stats_multi(engines[::-1], lim, maps[::-1]),
                      O.user_stats([(pl.tasks, m) for pl, m in zip(pools[::-1], maps[::-1])], n_users, lim))
        # one pool, identity map == the single form
        l0 = random_limits(seed + 1, pools[0].users.n)
        O.assert_same(user_stats_multi(engines[:1], l0), engines[0].user_stats(l0))
        for bad in ([engines[0], engines[0]],):
            with pytest.raises(CookError) as ex:
                user_stats_multi(bad, lim, [maps[0], maps[0]])
            assert ex.value.code == COOK_E_INVALID
        with pytest.raises(CookError) as ex:  # not one-to-one
            user_stats_multi(engines[:1], lim, [np.zeros(pools[0].users.n, np.uint32)])
        assert ex.value.code == COOK_E_INVALID
        return got
    finally:
        for e in engines:
            e.close()


def check_state_rule(make_engine):
    """COOK_E_STATE before any rank and after a cook_cycle_update no rank has followed; fine again after the next rank"""
    pool = synth.make_pool(seed=31, n_pending=300, n_running=200, n_users=12, n_offers=16)
    lim = A.UserLimits.from_users(pool.users)
    with make_engine(A.default_params()) as e:
        with pytest.raises(CookError) as ex:
            e.user_stats(lim)
        assert ex.value.code == COOK_E_STATE
        e.rank_stage(pool.tasks, pool.users)
        with pytest.raises(CookError) as ex:
            e.user_stats(lim)
        assert ex.value.code == COOK_E_STATE
        e.rank_run()
        before = e.user_stats(lim)
        with pytest.raises(CookError) as ex:  # limits of another size
            e.user_stats(A.UserLimits(np.ones(3), np.ones(3)))
        assert ex.value.code == COOK_E_INVALID
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        e.cycle_run(50)
        O.assert_same(e.user_stats(lim), before)
        # the first running task leaves: the rank's per-user order describes the old table until the next rank
        e.cycle_update(remove_task=[int(np.flatnonzero(pool.tasks.pending == 0)[0])])
        with pytest.raises(CookError) as ex:
            e.user_stats(lim)
        assert ex.value.code == COOK_E_STATE
        e.cycle_run(50)
        after = e.user_stats(lim)
        keep = np.ones(pool.tasks.n, bool)
        keep[int(np.flatnonzero(pool.tasks.pending == 0)[0])] = False
        t = pool.tasks
        t2 = A.Tasks(cpus=t.cpus[keep], mem=t.mem[keep], user=t.user[keep], priority=t.priority[keep], start_ms=t.start_ms[keep],
                     task_id=t.task_id[keep], job_id=t.job_id[keep], pending=t.pending[keep])
        O.assert_same(after, O.user_stats([(t2, None)], pool.users.n, lim))
        assert after["all"][0][0] == before["all"][0][0] - 1


def check_cycle_undisturbed(make_engine, pool: synth.Pool, k=200):
    """a cycle fetched after stats calls (single and multi) is the one fetched without them"""
    lim = random_limits(3, pool.users.n)
    outs = []
    for with_stats in (False, True):
        with make_engine(A.default_params()) as e, make_engine(A.default_params()) as e2:
            e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
            e2.rank_stage(pool.tasks, pool.users)
            e2.rank_run()
            e.cycle_run(k)
            if with_stats:
                e.user_stats(lim)
                user_stats_multi([e, e2], lim)
                user_stats_multi([e2, e], lim)
            ranked, j2o, head = e.cycle_fetch()
            outs.append((ranked.copy(), j2o.copy(), head, e.cycle_fetch_considerable().copy()))
    a, b = outs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3])
