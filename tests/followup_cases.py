"""The cases of cook_cycle_autoscale_multi / cook_match_metrics_multi / cook_batch_stats, shared by the emulator (test_followups_emu.py) and
GPU (test_followups_gpu.py) suites: the per-cycle follow-ups of every pool of a GPU in two calls.  The oracles are the existing ones:
autoscale_cases.oracle for the candidates, the checks of parity_cases.metrics_parity on top of pyoracle.resource_stats for the metrics;
every multi result is also compared with the single call on the same engine."""
from __future__ import annotations

import dataclasses

import numpy as np

from cook_amd import _abi as A
from cook_amd import synth
from cook_amd.engine import CookError, _MetricsOut, cycle_autoscale_multi, cycle_match_multi, cycle_run_rank_multi, match_metrics_multi
from oracle import pyoracle
from tests import autoscale_cases as S

COOK_OK, COOK_E_INVALID, COOK_E_STATE = 0, -1, -4


# ---- a set of pools of one device through one cycle -----------------------------------------------------------------------------
def stage(e, pool, cons):
    e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
    if cons is not None:
        e.cycle_set_considerable(*cons)


def run_cycle_multi(engines, ks):
    cycle_run_rank_multi(engines, ks)
    cycle_match_multi(engines)


class Pools:
    """engines of several pools, staged with their user states and run through ONE cook_cycle_run_rank_multi + ONE cook_cycle_match_multi"""

    def __init__(self, make_engine, pools, params, states, ks):
        self.pools, self.params, self.states = list(pools), params, list(states)
        self.ks = [int(ks)] * len(self.pools) if np.isscalar(ks) else [int(k) for k in ks]
        self.engines = [make_engine(params) for _ in self.pools]
        try:
            for e, pl, st in zip(self.engines, self.pools, self.states):
                stage(e, pl, st)
            run_cycle_multi(self.engines, self.ks)
        except BaseException:
            self.close()
            raise

    def close(self):
        for e in self.engines:
            e.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


# ---- the oracles ------------------------------------------------------------------------------------------------------------------
def check_metrics(m, jobs, offers, j2o, n_users, n_models, tag=""):
    """the checks of parity_cases.metrics_parity for the considered jobs `jobs` (in match order) and their placement j2o"""
    j2o = np.asarray(j2o)
    assert m["considerable"] == jobs.n and m["matched"] == int((j2o >= 0).sum()) and m["unmatched"] == int((j2o < 0).sum()), tag
    assert m["offers"] == offers.n and m["offers_scheduled"] == len(set(j2o[j2o >= 0].tolist())), tag
    assert m["head_matched"] == (bool(j2o[0] >= 0) if jobs.n else False), tag
    for got, cols in ((m["jobs"], (jobs.cpus, jobs.mem)), (m["offers_stats"], (offers.cpus, offers.mem))):
        want = pyoracle.resource_stats(*cols)
        for k, v in want.items():
            assert got[k] == v or (np.isnan(v) and np.isnan(got[k])), (tag, k, got[k], v)
    assert len(m["user_considerable"]) == n_users and len(m["user_matched"]) == n_users, tag
    if n_users:
        assert np.array_equal(m["user_considerable"], np.bincount(jobs.user, minlength=n_users)), tag
        assert np.array_equal(m["user_matched"], np.bincount(jobs.user[j2o >= 0], minlength=n_users)), tag
    if jobs.gpus is not None:
        jm = jobs.gpu_model if jobs.gpu_model is not None else np.zeros(jobs.n, np.uint32)
        want = np.bincount(jm[jobs.gpus > 0], weights=jobs.gpus[jobs.gpus > 0], minlength=n_models + 1)[: n_models + 1]
        assert np.array_equal(m["job_gpus_by_model"], want.astype(np.int64)), tag
    if offers.gpu_model is not None:
        gm, gc = offers.gpu_model.reshape(-1), offers.gpu_count.reshape(-1)
        sel = gm != 0
        want = np.bincount(gm[sel], weights=gc[sel], minlength=n_models + 1)[: n_models + 1]
        assert np.array_equal(m["offer_gpus_by_model"], want.astype(np.int64)), tag


def considered_jobs(pool, ranked, pos):
    pend_ord = np.cumsum(pool.tasks.pending) - 1
    return pool.pending_jobs.take(pend_ord[np.asarray(ranked)[np.asarray(pos, dtype=np.int64)]])


def check_pool(P, i, calls, got_auto, got_met, n_users, n_models, oracle_match=True):
    """pool i of P: every autoscale result of got_auto (one per keyword set of `calls`) and the metrics got_met against the oracles, then against
    the single calls on the same engine.  oracle_match=False: the oracle takes the engine's placement (the parity suites' business)."""
    e, pool, (st, el), k = P.engines[i], P.pools[i], P.states[i], P.ks[i]
    ranked, j2o, _ = e.cycle_fetch()
    pos = e.cycle_fetch_considerable()
    for kw, (out, info) in zip(calls, got_auto):
        o_out, o_info, d = S.oracle(P.params, pool, st, k, el, **kw, j2o=None if oracle_match else j2o)
        assert np.array_equal(ranked, d.ranked) and np.array_equal(j2o, d.j2o) and np.array_equal(pos, d.pos), i
        assert np.array_equal(out, o_out), (i, len(out), len(o_out), kw)
        assert info == o_info, (i, info, o_info)
        oracle_match = False  # (one oracle placement per pool: it does not depend on the call's keywords)
        s_out, s_info = e.cycle_autoscale(**kw)
        assert np.array_equal(out, s_out) and info == s_info, (i, "single call")
    if got_met is not None:
        check_metrics(got_met, considered_jobs(pool, ranked, pos), pool.offers, j2o, n_users, n_models, tag=i)
        S._same(got_met, e.match_metrics(n_users=n_users, n_gpu_models=n_models))


def exclusions(P, i, kw, every=3):
    """an exclude list that names every `every`-th candidate of pool i under kw, and one task that is no candidate"""
    st, el = P.states[i]
    out, _, _ = S.oracle(P.params, P.pools[i], st, P.ks[i], el, **kw, j2o=P.engines[i].cycle_fetch()[1])
    running = np.flatnonzero(P.pools[i].tasks.pending == 0)
    return [int(t) for t in out[::every]] + [int(t) for t in running[:1]]


# ---- 1 / 2 / 9: parity ------------------------------------------------------------------------------------------------------------
def check_parity(make_engine, pools, params, states, ks, call_sets, n_users, n_models=2, oracle_match=True):
    """ONE cook_cycle_autoscale_multi per call set (call_sets[c][i]: the keywords of pool i in set c; "exclude" as exclude_tasks is
    replaced by the pool's exclusions) and ONE cook_match_metrics_multi, every pool against the oracles and the single calls"""
    with Pools(make_engine, pools, params, states, ks) as P:
        sets = []
        for cs in call_sets:
            cs = [dict(kw) for kw in cs]
            for i, kw in enumerate(cs):
                if isinstance(kw.get("exclude_tasks"), str):
                    kw["exclude_tasks"] = exclusions(P, i, {k: v for k, v in kw.items() if k != "exclude_tasks"})
            sets.append(cs)
        got = [cycle_autoscale_multi(P.engines, cs) for cs in sets]
        met = match_metrics_multi(P.engines, n_users=n_users, n_gpu_models=n_models)
        for i in range(len(pools)):
            check_pool(P, i, [cs[i] for cs in sets], [g[i] for g in got], met[i], n_users[i], n_models, oracle_match=oracle_match)
        return got, met


def ragged_pools():
    """the shapes of test_autoscale_after_match_multi, plus a pool where every job matches (u = 0, N = 0)"""
    pools = [synth.make_pool(seed=88 + i, n_pending=npd, n_running=nr, n_users=nu, n_offers=no, fractional=(i == 1))
             for i, (npd, nr, nu, no) in enumerate([(500, 300, 20, 30), (300, 100, 12, 200), (0, 20, 4, 8)])]
    pools.append(synth.make_pool(seed=91, n_pending=40, n_running=30, n_users=6, n_offers=300))
    states = [S.random_state(pl, 90 + i, fractional=(i == 1)) for i, pl in enumerate(pools[:3])]
    states.append((S.open_state(6), np.ones(40, np.uint8)))
    return pools, states


def mixed_call_sets(pools):
    """two call sets that mix the calls across four pools: offer_skipped, an exclude list, neither, max_jobs small enough to cut the list"""
    rng = np.random.default_rng(7)
    sk = lambda i: (rng.random(pools[i].offers.n) < 0.3).astype(np.uint8)  # noqa: E731
    sk0 = sk(0)
    return [[dict(max_jobs=5, scale_factor=0.5, offer_skipped=sk0), dict(offer_skipped=sk(1), exclude_tasks="exclude", max_jobs=2000), dict(), dict()],
            [dict(offer_skipped=sk0), dict(exclude_tasks="exclude", scale_factor=2.5), dict(offer_skipped=sk(2)),
             dict(offer_skipped=np.ones(pools[3].offers.n, np.uint8), exclude_tasks="exclude")]]


def check_ragged(make_engine):
    pools, states = ragged_pools()
    params = A.default_params(good_enough_fitness=1.0, match_algo=2)
    n_users = [pools[0].users.n, pools[1].users.n + 5, 0, pools[3].users.n]  # (pool 2: the per-user arrays are left out)
    got, met = check_parity(make_engine, pools, params, states, [400, 300, 150, 150], mixed_call_sets(pools), n_users)
    info = [[r[1] for r in g] for g in got]
    # what the shapes and the calls were chosen for
    assert info[0][0]["autoscalable"] == info[0][0]["scaled"] == info[0][0]["unmatched"] > 0         # max_jobs cut the list at N = u
    assert 0 < info[0][1]["n_out"] < info[0][1]["autoscalable"]                                        # the exclude list took candidates
    assert info[0][2]["considered"] == 0 and met[2]["considerable"] == 0                               # nothing pending
    assert info[0][3]["considered"] > 0 and info[0][3]["unmatched"] == 0 and info[0][3]["scaled"] == 0 and len(got[0][3][0]) == 0  # u = 0, N = 0
    assert info[1][0]["matched"] < met[0]["matched"] and info[1][0]["autoscalable"] > info[0][0]["autoscalable"]  # skipped offers dropped matches; uncut
    assert info[1][3]["unmatched"] == info[1][3]["considered"] and 0 < info[1][3]["n_out"] < info[1][3]["autoscalable"]


def check_nine_pools(make_engine, scale=1):
    """more pools than one cook_multi launch takes (COOK_MULTI_MAX = 8)"""
    rng = np.random.default_rng(11)
    pools = [synth.make_pool(seed=400 + i, n_pending=int(rng.integers(200, 601)) * scale, n_running=100 * scale, n_users=10 + i,
                             n_offers=int(rng.integers(8, 41)) * scale, fractional=(i % 4 == 1)) for i in range(9)]
    states = [S.random_state(pl, 410 + i, fractional=(i % 4 == 1)) for i, pl in enumerate(pools)]
    calls = [[dict(max_jobs=50 + 10 * i, scale_factor=1.5, exclude_tasks="exclude" if i % 3 == 0 else None,
                   offer_skipped=(rng.random(pl.offers.n) < 0.4).astype(np.uint8) if i % 2 else None) for i, pl in enumerate(pools)]]
    got, met = check_parity(make_engine, pools, A.default_params(good_enough_fitness=1.0, match_algo=2), states, 100, calls,
                            [pl.users.n for pl in pools])
    assert all(m["considerable"] > 0 for m in met)


# ---- 3: one engine fails, the others do not --------------------------------------------------------------------------------------
def _codes(res):
    return [r.code if isinstance(r, CookError) else COOK_OK for r in res]


def check_one_engine_fails(make_engine, n_pending=300):
    params = A.default_params(good_enough_fitness=1.0, match_algo=2)
    pools = [synth.make_pool(seed=420 + i, n_pending=n_pending + 50 * i, n_running=100, n_users=10, n_offers=6) for i in range(3)]
    states = [S.random_state(pl, 430 + i) for i, pl in enumerate(pools)]
    k = 100
    nu = [10, 10, 10]
    no_user = dataclasses.replace(pools[1], pending_jobs=dataclasses.replace(pools[1].pending_jobs, user=None))
    calls = [dict(), dict(max_jobs=300, scale_factor=2.0, offer_skipped=np.ones(6, np.uint8)), dict(max_jobs=40)]
    with Pools(make_engine, [pools[0], no_user, pools[2]], params, [states[0], None, states[2]], k) as P:
        lib = P.engines[0]._lib
        msg = lambda e: lib.cook_last_error(e._h).decode()  # noqa: E731

        def ok_engines(auto, met):
            for i in (0, 2):
                check_pool(P, i, [calls[i]], [auto[i]], met[i] if met is not None else None, nu[i], 2)

        # engine 1 ran its cycle without a staged user state (autoscale: COOK_E_STATE) and without the jobs' user column (metrics with
        # per-user arrays: COOK_E_INVALID)
        auto = cycle_autoscale_multi(P.engines, calls, raise_errors=False)
        assert _codes(auto) == [COOK_OK, COOK_E_STATE, COOK_OK] and "cook_cycle_autoscale needs" in msg(P.engines[1])
        met = match_metrics_multi(P.engines, n_users=nu, n_gpu_models=2, raise_errors=False)
        assert _codes(met) == [COOK_OK, COOK_E_INVALID, COOK_OK] and "user column" in msg(P.engines[1])
        ok_engines(auto, met)
        try:
            cycle_autoscale_multi(P.engines, calls)
            raise AssertionError("the failing engine's error is raised")
        except CookError as ex:
            assert ex.code == COOK_E_STATE  # the return value is engine 1's code
        # the fault removed: engine 1 staged with the user column and a user state, the cycle again for all
        P.pools[1], P.states[1] = pools[1], states[1]
        stage(P.engines[1], pools[1], states[1])
        run_cycle_multi(P.engines, P.ks)
        auto = cycle_autoscale_multi(P.engines, calls)
        met = match_metrics_multi(P.engines, n_users=nu, n_gpu_models=2)
        for i in range(3):
            check_pool(P, i, [calls[i]], [auto[i]], met[i], nu[i], 2)
        # its exclude index out of range
        bad = [calls[0], dict(calls[1], exclude_tasks=[pools[1].tasks.n]), calls[2]]
        res = cycle_autoscale_multi(P.engines, bad, raise_errors=False)
        assert _codes(res) == [COOK_OK, COOK_E_INVALID, COOK_OK] and "exclude_task index out of range" in msg(P.engines[1])
        ok_engines(res, None)
        # its cap too small: the info still says how many
        assert auto[1][1]["n_out"] > 3
        res = cycle_autoscale_multi(P.engines, [calls[0], dict(calls[1], cap=3), calls[2]], raise_errors=False)
        assert _codes(res) == [COOK_OK, COOK_E_INVALID, COOK_OK] and "more jobs than cap" in msg(P.engines[1])
        assert res[1].info == auto[1][1]
        ok_engines(res, None)
        # a further engine that has only been staged: metrics COOK_E_STATE beside a pool that is fine
        with make_engine(params) as fresh:
            stage(fresh, pools[1], states[1])
            res = match_metrics_multi([P.engines[0], fresh, P.engines[2]], n_users=nu, n_gpu_models=2, raise_errors=False)
            assert _codes(res) == [COOK_OK, COOK_E_STATE, COOK_OK] and "before a match ran" in msg(fresh)
            S._same(res[0], met[0]), S._same(res[2], met[2])
            res = cycle_autoscale_multi([fresh, P.engines[1]], [None, calls[1]], raise_errors=False)
            assert _codes(res) == [COOK_E_STATE, COOK_OK]
        # no engine is left wedged: the same calls succeed
        S._same(cycle_autoscale_multi(P.engines, calls), auto)
        S._same(match_metrics_multi(P.engines, n_users=nu, n_gpu_models=2), met)
        assert [msg(e) for e in P.engines] == ["", "", ""]


# ---- 4: whole-call rejections ------------------------------------------------------------------------------------------------------
def check_rejections(make_engine):
    import ctypes as C
    params = A.default_params(good_enough_fitness=1.0, match_algo=2)
    pools = [synth.make_pool(seed=440 + i, n_pending=200, n_running=50, n_users=8, n_offers=12) for i in range(2)]
    states = [S.random_state(pl, 450 + i) for i, pl in enumerate(pools)]
    with Pools(make_engine, pools, params, states, 60) as P:
        lib = P.engines[0]._lib
        h = [e._h for e in P.engines]
        want_auto = [e.cycle_autoscale() for e in P.engines]
        want_met = [e.match_metrics(n_users=8) for e in P.engines]
        ps = [A.CookAutoscaleParams(1000, 0, 1.0, None, None) for _ in h]
        outs = [np.full(1000, 0xFFFFFFFF, np.uint32) for _ in h]
        info = (A.CookAutoscaleInfo * 2)()
        rc = (C.c_int * 2)(7, 7)
        arr = lambda *x: (C.c_void_p * len(x))(*x)  # noqa: E731
        eng, pp, tp, cp = arr(*h), arr(*[C.addressof(p) for p in ps]), arr(*[o.ctypes.data for o in outs]), (C.c_uint32 * 2)(1000, 1000)
        auto = lib.cook_cycle_autoscale_multi
        assert auto(None, 2, pp, tp, cp, info, rc) == COOK_E_INVALID
        assert auto(eng, 0, pp, tp, cp, info, rc) == COOK_E_INVALID
        assert auto(eng, 2, None, tp, cp, info, rc) == COOK_E_INVALID
        assert auto(eng, 2, pp, tp, None, info, rc) == COOK_E_INVALID
        assert auto(arr(h[0], None), 2, pp, tp, cp, info, rc) == COOK_E_INVALID          # a NULL engine
        assert auto(eng, 2, arr(C.addressof(ps[0]), None), tp, cp, info, rc) == COOK_E_INVALID  # a NULL params entry
        assert auto(arr(h[0], h[0]), 2, pp, tp, cp, info, rc) == COOK_E_INVALID          # an engine named twice
        outs_m = [_MetricsOut(8, 0) for _ in h]
        reqs = (A.CookMetricsReq * 2)(*[o.req() for o in outs_m])
        met = lib.cook_match_metrics_multi
        assert met(None, 2, reqs, rc) == COOK_E_INVALID
        assert met(eng, 0, reqs, rc) == COOK_E_INVALID
        assert met(eng, 2, None, rc) == COOK_E_INVALID
        assert met(arr(h[0], None), 2, reqs, rc) == COOK_E_INVALID
        assert met(arr(h[1], h[1]), 2, reqs, rc) == COOK_E_INVALID
        # nothing ran: no output, no info, no code was written
        assert all((o == 0xFFFFFFFF).all() for o in outs) and list(rc) == [7, 7] and all(o.m.offers == 0 for o in outs_m)
        # a NULL task_idx entry is engine i's own error iff cap[i] > 0
        assert auto(eng, 2, pp, arr(outs[0].ctypes.data, None), cp, info, rc) == COOK_E_INVALID and list(rc) == [COOK_OK, COOK_E_INVALID]
        assert info[0].n_out == want_auto[0][1]["n_out"] and np.array_equal(outs[0][: info[0].n_out], want_auto[0][0])
        # ... and the calls still work
        S._same(cycle_autoscale_multi(P.engines, [None, None]), want_auto)
        S._same(match_metrics_multi(P.engines, n_users=8), want_met)
        assert lib.cook_batch_stats(None, (C.c_uint32 * 5)()) == COOK_E_INVALID and lib.cook_batch_stats(h[0], None) == COOK_E_INVALID


# ---- 5: the cycle is left alone ----------------------------------------------------------------------------------------------------
def check_cycle_undisturbed(make_engine, n_pending=400, k=120):
    params = A.default_params()
    pools = [synth.make_pool(seed=460 + i, n_pending=n_pending + 100 * i, n_running=200, n_users=15, n_offers=24) for i in range(3)]
    states = [S.random_state(pl, 470 + i, fractional=True) for i, pl in enumerate(pools)]
    removed = [[int(np.flatnonzero(pl.tasks.pending == 1)[0]), int(np.flatnonzero(pl.tasks.pending == 0)[0])] for pl in pools]
    nxt = []
    for with_calls in (False, True):
        with Pools(make_engine, pools, params, states, k) as P:
            before = [S._snapshot(e, 15) for e in P.engines]
            if with_calls:
                cycle_autoscale_multi(P.engines, [None] * 3)
                cycle_autoscale_multi(P.engines, [dict(max_jobs=5, scale_factor=0.5, offer_skipped=np.ones(pl.offers.n, np.uint8),
                                                       exclude_tasks=b[0][:7]) for pl, b in zip(pools, before)])
                match_metrics_multi(P.engines, n_users=[15, 0, 20], n_gpu_models=2)
                S._same([S._snapshot(e, 15) for e in P.engines], before)
            for e, rm in zip(P.engines, removed):
                e.cycle_update(remove_task=rm)
            run_cycle_multi(P.engines, P.ks)
            nxt.append(([S._snapshot(e, 15) for e in P.engines], cycle_autoscale_multi(P.engines, [None] * 3),
                        match_metrics_multi(P.engines, n_users=15, n_gpu_models=1)))
    S._same(nxt[0], nxt[1])


# ---- 7: edge shapes ----------------------------------------------------------------------------------------------------------------
def check_edges(make_engine):
    params = A.default_params(good_enough_fitness=1.0, match_algo=2)
    pools = [synth.make_pool(seed=480, n_pending=200, n_running=80, n_users=9, n_offers=16),   # K = 0: nothing is considered
             synth.make_pool(seed=481, n_pending=150, n_running=60, n_users=9, n_offers=0),    # M = 0: nothing matches
             synth.make_pool(seed=482, n_pending=250, n_running=90, n_users=9, n_offers=20)]
    states = [S.random_state(pl, 490 + i) for i, pl in enumerate(pools)]
    calls = [[dict(), dict(max_jobs=60, scale_factor=0.4), dict(exclude_tasks="exclude")]]
    got, met = check_parity(make_engine, pools, params, states, [0, 80, 80], calls, [9, 9, 9])
    assert got[0][0][1]["considered"] == 0 and met[0]["considerable"] == 0 and np.isnan(met[0]["jobs"]["p50_cpus"])
    assert got[0][1][1]["matched"] == 0 and met[1]["offers"] == 0 and np.isnan(met[1]["offers_stats"]["p50_mem"])
    # n = 1: the call is the single call (no pool batch)
    with Pools(make_engine, pools[2:], params, states[2:], 80) as P:
        one_before = P.engines[0].batch_stats()
        (auto,) = cycle_autoscale_multi(P.engines, [dict(max_jobs=30)])
        (m,) = match_metrics_multi(P.engines, n_users=9)
        check_pool(P, 0, [dict(max_jobs=30)], [auto], m, 9, 0)
        assert P.engines[0].batch_stats() == one_before  # (what the rank part of ONE engine left: no batch)
