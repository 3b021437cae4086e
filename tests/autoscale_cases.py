"""The cases of cook_cycle_autoscale, shared by the emulator (test_autoscale_emu.py) and GPU (test_autoscale_gpu.py) suites: the golden
cases of tests/golden/autoscale.json, random pools against an oracle composed of the frozen oracle.pyoracle calls (rank -> considerable ->
match, the kept matches removed, considerable over Q' without the eligible mask, the exclusion), the same Q' through cook_considerable
from the host, the state rule, and that the call leaves the cycle as it was."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest

from cook_amd import _abi as A
from cook_amd.engine import CookError
from oracle import pyoracle
from tests import golden_util as G
from tests.parity_cases import make_considerable_case

COOK_E_INVALID, COOK_E_STATE = -1, -4
INFO = ("considered", "matched", "unmatched", "scaled", "autoscalable", "n_out", "fraction_unmatched")


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
def scaled_n(k, u, max_jobs, scale):
    """scheduler.clj:1288-1306: (max u (int (* (min (* fraction scale) 1) max-jobs))), fraction = (/ (float u) k) or 0"""
    fraction = float(np.float32(u)) / k if k else 0.0
    v = min(fraction * scale, 1.0) * max_jobs
    return max(u, int(v) if v > 0 else 0), fraction


def oracle(params, pool, st, k, eligible, max_jobs=1000, scale_factor=1.0, offer_skipped=None, exclude_tasks=None, j2o=None):
    """-> (Out as task indices, info dict, details).  j2o: the placement of the considered jobs as given (pools whose oracle placement
    takes minutes on one core: the match itself is the parity suites' business), else pyoracle.match's"""
    ranked, _ = pyoracle.rank(params, pool.tasks, pool.users)
    jq = (np.cumsum(pool.tasks.pending) - 1)[ranked]
    J = pool.pending_jobs
    gp = J.gpus[jq] if J.gpus is not None else np.zeros(len(jq))
    queue = A.Queue(cpus=J.cpus[jq], mem=J.mem[jq], gpus=gp, user=J.user[jq],
                    eligible=np.asarray(eligible, dtype=np.uint8)[jq] if eligible is not None else None)
    pos, _, _ = pyoracle.considerable(queue, st, k)
    if j2o is None:
        j2o, _, _ = pyoracle.match(params, J.take(jq[pos]), pool.offers, pool.groups)
    hit = j2o >= 0
    if offer_skipped is not None:
        sk = np.asarray(offer_skipped, dtype=np.uint8)
        hit &= sk[np.maximum(j2o, 0)] == 0
    kk, m = len(pos), int(hit.sum())
    N, fraction = scaled_n(kk, kk - m, max_jobs, scale_factor)
    keep = np.ones(len(ranked), bool)
    keep[pos[hit]] = False
    qp = np.flatnonzero(keep)
    q2 = A.Queue(cpus=queue.cpus[qp], mem=queue.mem[qp], gpus=queue.gpus[qp], user=queue.user[qp])
    apos = pyoracle.considerable(q2, st, N)[0] if len(qp) else np.zeros(0, np.uint32)
    cand = ranked[qp[apos]]
    ex = {int(t) for t in (exclude_tasks if exclude_tasks is not None else [])}
    out = np.array([t for t in cand.tolist() if t not in ex], dtype=np.uint32)
    info = dict(considered=kk, matched=m, unmatched=kk - m, scaled=N, autoscalable=len(cand), n_out=len(out), fraction_unmatched=fraction)
    return out, info, SimpleNamespace(ranked=ranked, pos=pos, j2o=j2o, queue2=q2, apos=apos)


# ---- engine side -------------------------------------------------------------------------------------------------------------
def run_cycle(e, pool, st, k, eligible):
    e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
    e.cycle_set_considerable(st, eligible)
    e.cycle_run(k)


def check_against_oracle(make_engine, params, pool, st, k, eligible, calls, masked_queue=True, oracle_match=True):
    """one cycle, then every call of `calls` (keyword sets of Engine.cycle_autoscale) against the oracle, element for element"""
    got = []
    with make_engine(params) as e:
        run_cycle(e, pool, st, k, eligible)
        ranked, j2o, _ = e.cycle_fetch()
        for kw in calls:
            got.append(e.cycle_autoscale(**kw))
    for kw, (out, info) in zip(calls, got):
        o_out, o_info, d = oracle(params, pool, st, k, eligible, **kw, j2o=None if oracle_match else j2o)
        assert np.array_equal(ranked, d.ranked) and np.array_equal(j2o, d.j2o)  # (the cycle itself is the parity suites' business)
        assert np.array_equal(out, o_out), (len(out), len(o_out), kw)
        assert info == o_info, (info, o_info, kw)
        if masked_queue:  # the same Q' built on the host and uploaded through cook_considerable
            with make_engine(params) as e2:
                idx, _, _ = e2.considerable(d.queue2, st, info["scaled"])
            assert np.array_equal(idx, d.apos)
    return got


# ---- golden cases ------------------------------------------------------------------------------------------------------------
def golden_inputs(case):
    J, O, names, _ = G.build_match_all(case)
    n = len(names)
    J.user = np.zeros(n, dtype=np.uint32)
    tasks = A.Tasks(cpus=J.cpus.copy(), mem=J.mem.copy(), gpus=J.gpus.copy(), user=np.zeros(n, np.uint32), priority=np.full(n, 50, np.int32),
                    start_ms=np.zeros(n, np.int64), task_id=(10_000 + np.arange(n)).astype(np.int64),
                    job_id=(100 + np.arange(n)).astype(np.int64), pending=np.ones(n, np.uint8))
    pool = SimpleNamespace(tasks=tasks, users=A.Users(div_cpus=np.full(1, A.DMAX), div_mem=np.full(1, A.DMAX)), pending_jobs=J, offers=O,
                           groups=None)
    cons = dict(queue=[dict(name=j["name"], user="u", cpus=j["cpus"], mem=j["mem"]) for j in case["jobs"]], user_usage=case["user_usage"],
                user_quota=case["user_quota"], enforce=case.get("enforce", False))
    for key in ("tokens", "pool_quota", "pool_usage"):
        if key in case:
            cons[key] = case[key]
    _, st, _, unames = G.build_considerable_inputs(cons)
    assert unames == ["u"]
    eligible = np.array([0 if nm in case["ineligible"] else 1 for nm in names], dtype=np.uint8)
    skipped = None
    if case["skipped"]:
        skipped = np.zeros(len(case["offers"]), np.uint8)
        skipped[case["skipped"]] = 1
    kw = dict(max_jobs=case["max_jobs"], scale_factor=case["scale_factor"], offer_skipped=skipped,
              exclude_tasks=[names.index(nm) for nm in case["exclude"]])
    return pool, st, eligible, kw, names


def check_golden(make_engine):
    cases = G.load("autoscale")
    assert len(cases) >= 11
    for case in cases:
        pool, st, eligible, kw, names = golden_inputs(case)
        params = A.default_params(good_enough_fitness=case["good_enough"])
        k = case["num_considerable"]
        (out, info), = check_against_oracle(make_engine, params, pool, st, k, eligible, [kw])
        assert [names[t] for t in out] == case["expect_out"], (case["name"], [names[t] for t in out])
        want = dict(case["expect_info"], considered=case["expect_info"]["matched"] + case["expect_info"]["unmatched"])
        assert {f: info[f] for f in want} == want, (case["name"], info, want)
        with make_engine(params) as e:  # the kept matches the case names
            run_cycle(e, pool, st, k, eligible)
            _, j2o, _ = e.cycle_fetch()
            pos = e.cycle_fetch_considerable()
        sk = kw["offer_skipped"]
        kept = [names[int(p)] for p, o in zip(pos, j2o) if o >= 0 and (sk is None or not sk[o])]
        assert kept == case["expect_matched"], (case["name"], kept)


# ---- random pools ------------------------------------------------------------------------------------------------------------
def random_state(pool, seed, *, fractional=False, tokens=True, enforce=True, pool_quota=True):
    _, st = make_considerable_case(seed, n=max(1, pool.pending_jobs.n), n_users=pool.users.n, fractional=fractional, tokens=tokens,
                                   enforce=enforce, pool_quota=pool_quota)
    rng = np.random.default_rng(seed + 1)
    eligible = (rng.random(pool.pending_jobs.n) < 0.9).astype(np.uint8)
    return st, eligible


def random_calls(pool, seed, k, n_calls=3):
    rng = np.random.default_rng(seed + 2)
    calls = [dict(max_jobs=1000, scale_factor=1.0), dict(max_jobs=max(1, k // 3), scale_factor=1000.0)]
    for _ in range(n_calls - 2):
        ex = rng.choice(pool.tasks.n, size=min(pool.tasks.n, 1 + pool.tasks.n // 50), replace=False) if pool.tasks.n else []
        calls.append(dict(max_jobs=int(rng.integers(1, 5000)), scale_factor=float(rng.choice([0.0, 0.37, 2.5, 1000.0])),
                          offer_skipped=(rng.random(pool.offers.n) < 0.3).astype(np.uint8), exclude_tasks=ex))
    return calls


def check_random(make_engine, pool, seed, k, params=None, n_calls=3, masked_queue=True, oracle_match=True, **state_kw):
    params = params or A.default_params(good_enough_fitness=1.0)
    st, eligible = random_state(pool, seed, **state_kw)
    got = check_against_oracle(make_engine, params, pool, st, k, eligible, random_calls(pool, seed, k, n_calls), masked_queue=masked_queue,
                               oracle_match=oracle_match)
    return got


# ---- the state rule and errors --------------------------------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(CookError) as ex:
        fn()
    return ex.value.code


def open_state(n_users):
    """no user, rate or pool limit: every unmatched job of the queue is a candidate"""
    z, big = np.zeros(n_users), np.full(n_users, A.DMAX)
    return A.UserState(quota_count=np.full(n_users, 2.0 ** 31 - 1), quota_cpus=big, quota_mem=big, quota_gpus=big, usage_count=z, usage_cpus=z,
                       usage_mem=z, usage_gpus=z)


def check_state_rule(make_engine, pool):
    st, eligible = open_state(pool.users.n), np.ones(pool.pending_jobs.n, np.uint8)
    with make_engine(A.default_params()) as e:
        assert _code(e.cycle_autoscale) == COOK_E_STATE  # before any cycle
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        assert _code(e.cycle_autoscale) == COOK_E_STATE  # a stage no cycle has followed
        e.cycle_run(50)
        assert _code(e.cycle_autoscale) == COOK_E_STATE  # a cycle without a staged user state (plain take-K)
        e.cycle_set_considerable(st, eligible)
        assert _code(e.cycle_autoscale) == COOK_E_STATE  # staged, not run
        e.cycle_run(50)
        sk = np.ones(pool.offers.n, np.uint8)  # (every match dropped: u = k, N = 1000)
        first = e.cycle_autoscale(offer_skipped=sk)
        # invalid arguments
        assert _code(lambda: e.cycle_autoscale(scale_factor=float("nan"))) == COOK_E_INVALID
        assert _code(lambda: e.cycle_autoscale(scale_factor=float("inf"))) == COOK_E_INVALID
        assert _code(lambda: e.cycle_autoscale(max_jobs=2 ** 31)) == COOK_E_INVALID
        assert _code(lambda: e.cycle_autoscale(exclude_tasks=[pool.tasks.n])) == COOK_E_INVALID
        assert len(first[0]) > 0
        import ctypes as C
        p = A.CookAutoscaleParams(1000, 0, 1.0, sk.ctypes.data_as(C.POINTER(C.c_uint8)), None)
        info = A.CookAutoscaleInfo()
        buf = np.zeros(1, np.uint32)
        rc = e._lib.cook_cycle_autoscale(e._h, C.byref(p), buf.ctypes.data_as(C.POINTER(C.c_uint32)), 0, C.byref(info))
        assert rc == COOK_E_INVALID and info.n_out == first[1]["n_out"]  # |Out| > cap: the info says how many
        # an in-range excluded task that is no candidate is ignored
        out, info2 = e.cycle_autoscale(offer_skipped=sk, exclude_tasks=[int(np.flatnonzero(pool.tasks.pending == 0)[0])] if (pool.tasks.pending == 0).any() else [])
        assert np.array_equal(out, first[0]) and info2 == first[1]
        # a cycle update no cycle has followed, then the cycle
        e.cycle_update(remove_task=[int(np.flatnonzero(pool.tasks.pending == 0)[0])])
        assert _code(e.cycle_autoscale) == COOK_E_STATE
        e.cycle_run(50)
        e.cycle_autoscale()
        # cook_considerable replaces the staged user state; cycle_set_considerable(None) turns the filters off
        q, st2 = make_considerable_case(9, n=20, n_users=4)
        e.considerable(q, st2, 10)
        assert _code(e.cycle_autoscale) == COOK_E_STATE
        e.cycle_set_considerable(st, eligible)
        e.cycle_run(50)
        e.cycle_autoscale()
        e.cycle_set_considerable(None)
        assert _code(e.cycle_autoscale) == COOK_E_STATE
        e.cycle_run(50)
        assert _code(e.cycle_autoscale) == COOK_E_STATE


def _snapshot(e, n_users):
    ranked, j2o, head = e.cycle_fetch()
    pos = e.cycle_fetch_considerable()
    met = e.match_metrics(n_users=n_users)
    why = e.match_explain(np.arange(min(len(pos), 40)))
    us = e.user_stats()
    return (ranked, j2o, head, pos, met, why, us)


def _same(a, b):
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            _same(a[k], b[k])
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    else:
        assert a == b or (a != a and b != b), (a, b)


def check_cycle_undisturbed(make_engine, pool, k=200):
    """every fetch after the call is the one before it, and the next cycle_update + cycle_run is the one without the call"""
    st, eligible = random_state(pool, 6, fractional=True)
    n_users = pool.users.n
    removed = [int(np.flatnonzero(pool.tasks.pending == 1)[0]), int(np.flatnonzero(pool.tasks.pending == 0)[0])]
    nxt = []
    for with_call in (False, True):
        with make_engine(A.default_params()) as e:
            run_cycle(e, pool, st, k, eligible)
            before = _snapshot(e, n_users)
            if with_call:
                e.cycle_autoscale()
                e.cycle_autoscale(max_jobs=5, scale_factor=0.5, offer_skipped=np.ones(pool.offers.n, np.uint8), exclude_tasks=before[0][:7])
                _same(_snapshot(e, n_users), before)
            e.cycle_update(remove_task=removed)
            e.cycle_run(k)
            nxt.append((_snapshot(e, n_users), e.cycle_autoscale()))
    _same(nxt[0], nxt[1])


def check_multi(make_engine, pools, params, k, seed=90):
    """pools of one device: their rank parts through one cook_cycle_run_rank_multi, their placements through one cook_cycle_match_multi,
    then one cook_cycle_autoscale per pool (one after another), each against the oracle"""
    from cook_amd.engine import cycle_match_multi, cycle_run_rank_multi
    states = [random_state(pl, seed + i) for i, pl in enumerate(pools)]
    calls = [random_calls(pl, seed + i, k, 3) for i, pl in enumerate(pools)]
    engines = [make_engine(params) for _ in pools]
    try:
        for e, pl, (st, el) in zip(engines, pools, states):
            e.cycle_stage(pl.tasks, pl.users, pl.pending_jobs, pl.offers, pl.groups)
            e.cycle_set_considerable(st, el)
        cycle_run_rank_multi(engines, [k] * len(pools))
        cycle_match_multi(engines)
        got = [[e.cycle_autoscale(**kw) for kw in cs] for e, cs in zip(engines, calls)]
        fetched = [e.cycle_fetch() for e in engines]
    finally:
        for e in engines:
            e.close()
    for pl, (st, el), cs, g, (ranked, j2o, _) in zip(pools, states, calls, got, fetched):
        for kw, (out, info) in zip(cs, g):
            o_out, o_info, d = oracle(params, pl, st, k, el, **kw)
            assert np.array_equal(ranked, d.ranked) and np.array_equal(j2o, d.j2o)
            assert np.array_equal(out, o_out) and info == o_info, (info, o_info)
    return got
