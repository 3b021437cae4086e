"""The cases of cook_usage_breakdown / cook_usage_breakdown_multi, shared by the emulator (test_usage_emu.py) and GPU
(test_usage_gpu.py) suites: the reference's golden answers and hand-derived edges (tests/golden/usage.json), seeded random pools
against tests/usage_oracle.py bit for bit (all users, a list of users, several engines with and without user maps; fractional pools
whose sums round), rounding traps whose three values only the regrouping brings together, the state rule, and that a call leaves the
cycle alone.  Every output is compared with == / bit patterns: there is no tolerance anywhere."""
from __future__ import annotations

import numpy as np
import pytest

from cook_amd import _abi as A
from cook_amd import synth
from cook_amd.engine import CookError, usage_breakdown_multi
from tests import golden_util as _G
from tests import sum_order_cases as SO
from tests import usage_oracle as O

COOK_E_INVALID, COOK_E_STATE = -1, -4
LITERAL_MAX = 4000  # tables up to this size are also answered user by user over dicts (usage_literal)
NONE = A.NONE_U32


# ---- golden ---------------------------------------------------------------------------------------------------------------------------
def golden_pool(case, p, seq0):
    """-> (Tasks, group_of_row or None, the engine's user names); ids and start times in creation order"""
    names = p["users"] or case["users"]
    ts = p["tasks"]
    n = len(ts)
    pend = np.array([t["state"] == "waiting" for t in ts], dtype=np.uint8) if n else np.zeros(0, np.uint8)
    seq = seq0 + np.arange(n, dtype=np.int64)
    tasks = A.Tasks(cpus=np.array([t["cpus"] for t in ts], dtype=np.float64), mem=np.array([t["mem"] for t in ts], dtype=np.float64),
                    gpus=None if p["no_gpus"] else np.array([t.get("gpus", 0.0) for t in ts], dtype=np.float64),
                    user=np.array([names.index(t["user"]) for t in ts], dtype=np.uint32),
                    priority=np.array([t.get("priority", 50) for t in ts], dtype=np.int32),
                    start_ms=np.where(pend == 1, 0, 1_600_000_000_000 + seq).astype(np.int64), task_id=17_592_186_050_000 + seq,
                    job_id=17_592_186_045_000 + seq, pending=pend)
    grp = None if p["no_groups"] else np.array([t.get("group", NONE) if t.get("group") is not None else NONE for t in ts], dtype=np.uint32)
    return tasks, grp, names


def _check_answer(where, want, got, names, ask, multi):
    """want: {total: {user: [..]}, buckets: {user: [[group, usage, rows]]}}; got: the dict of Engine.usage_breakdown"""
    ids = list(range(len(names))) if ask is None else ask
    assert len(got["bucket_off"]) == len(ids) + 1 and len(got["total"]) == len(ids), where
    for k, u in enumerate(ids):
        name = names[u]
        assert got["total"][k].tolist() == [float(v) for v in want["total"][name]], (where, name, got["total"][k].tolist())
        b0, b1 = int(got["bucket_off"][k]), int(got["bucket_off"][k + 1])
        exp = want["buckets"][name]
        assert b1 - b0 == len(exp), (where, name, b0, b1)
        for b, (g, usage, rows) in zip(range(b0, b1), exp):
            assert int(got["bucket_group"][b]) == (NONE if g is None else g), (where, name, b)
            assert got["bucket_usage"][b].tolist() == [float(v) for v in usage], (where, name, b, got["bucket_usage"][b].tolist())
            r0, r1 = int(got["row_off"][b]), int(got["row_off"][b + 1])
            assert got["rows"][r0:r1].tolist() == rows, (where, name, b, got["rows"][r0:r1].tolist())
    assert len(got["bucket_group"]) == int(got["bucket_off"][-1]) and len(got["rows"]) == int(got["row_off"][-1]), where


def _stage(make_engine, tasks, n_users):
    e = make_engine(A.default_params())
    e.rank_stage(tasks, A.Users(div_cpus=np.full(n_users, A.DMAX), div_mem=np.full(n_users, A.DMAX)))
    e.rank_run()
    return e


def check_golden(make_engine):
    for case in _G.load("usage")["cases"]:
        names, multi, ask, exp = case["users"], case["multi"], case["ask"], case["expect"]
        built = [golden_pool(case, p, 1000 * i) for i, p in enumerate(case["pools"])]
        pools = [(t, g) for t, g, _ in built]
        maps = [None if p["users"] is None else np.array([names.index(x) for x in p["users"]], np.uint32) for p in case["pools"]]
        maps = maps if any(m is not None for m in maps) else None
        engines = [_stage(make_engine, t, len(en)) for t, _, en in built]
        try:
            def call():
                if multi:
                    return usage_breakdown_multi(engines, len(names), [g for _, g in pools], case["n_groups"], maps, users=ask)
                return engines[0].usage_breakdown(pools[0][1], case["n_groups"], users=ask)
            where = (case["name"], case["ref"])
            if exp.get("error"):
                with pytest.raises(CookError) as ex:
                    call()
                assert ex.value.code == COOK_E_INVALID, where
                continue
            want = O.usage_literal(pools, len(names), maps, ask, multi)
            _check_answer(where, exp, want, names, ask, multi)  # (the restatement reproduces the reference's answers ...)
            O.assert_same(O.usage(pools, len(names), maps, ask, multi), want, where)
            got = call()
            _check_answer(where, exp, got, names, ask, multi)   # (... and so does the engine)
            O.assert_same(got, want, where)
            for i, pe in enumerate(exp.get("pools") or []):     # the :pools sub-map: the call with that pool, engine by engine
                if pe is not None:
                    one = engines[i].usage_breakdown(pools[i][1], case["n_groups"])
                    _check_answer(where + (i,), pe, one, names, None, False)
                    O.assert_same(one, O.usage_literal([pools[i]], len(names)), where + (i,))
        finally:
            for e in engines:
                e.close()


# ---- random pools ---------------------------------------------------------------------------------------------------------------------
def random_groups(seed, tasks: A.Tasks, n_groups: int, ungrouped=0.5):
    """about half the rows ungrouped, group sizes skewed (Zipf over the ids), groups that cross users (the draw ignores the user);
    pending rows carry ids too"""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, n_groups + 1) ** 1.2
    g = rng.choice(n_groups, size=tasks.n, p=p / p.sum()).astype(np.uint32)
    g = rng.permutation(n_groups).astype(np.uint32)[g]
    g[rng.random(tasks.n) < ungrouped] = NONE
    return g


def _oracle(pools, n_users, maps=None, users=None, multi=False):
    want = O.usage(pools, n_users, maps, users, multi)
    if sum(t.n for t, _ in pools) <= LITERAL_MAX:
        O.assert_same(want, O.usage_literal(pools, n_users, maps, users, multi), "numpy form against the literal one")
    return want


def assert_must_fold(pools, n_users, maps=None, total_too=True):
    """a condition on the INPUT, checked with the oracle alone before the engine is called: some bucket (and some user) sums
    differently as a tree than left to right, so the engine's fold path is taken for it"""
    buckets, users = O.sums_that_depend_on_order(pools, n_users, maps, limit=1)
    assert buckets, "choose an input in which a bucket's sum depends on the order of addition"
    assert users or not total_too, "choose an input in which a user's total depends on the order of addition"


def check_one(make_engine, tasks: A.Tasks, users: A.Users, grp, n_groups, seed=1, must_fold=False):
    """all users; a list of users (repeats, users without rows); the engine's answer against the oracle bit for bit"""
    n = users.n
    pools = [(tasks, grp)]
    if must_fold:
        assert_must_fold(pools, n)
    rng = np.random.default_rng(seed)
    ul = rng.integers(0, max(n, 1), min(40, 2 * n)).astype(np.uint32) if n else np.zeros(0, np.uint32)
    with make_engine(A.default_params()) as e:
        e.rank_stage(tasks, users)
        e.rank_run()
        got = e.usage_breakdown(grp, n_groups)
        O.assert_same(got, _oracle(pools, n), "all users")
        O.assert_same(e.usage_breakdown(grp, n_groups, users=ul), _oracle(pools, n, users=ul), "a list of users")
        O.assert_same(e.usage_breakdown(None, 0), _oracle([(tasks, None)], n), "group_of_row NULL")
    assert int(got["bucket_usage"][:, 3].sum()) == int((tasks.pending == 0).sum()) == len(got["rows"])  # grouped + ungrouped jobs = all jobs
    return got


def check_random(make_engine, pool: synth.Pool, n_groups, seed=1, must_fold=False, ungrouped=0.5):
    return check_one(make_engine, pool.tasks, pool.users, random_groups(seed, pool.tasks, n_groups, ungrouped), n_groups, seed, must_fold)


def check_every_row_its_own_group(make_engine, pool: synth.Pool):
    """B = R"""
    N = pool.tasks.n
    got = check_one(make_engine, pool.tasks, pool.users, np.arange(N, dtype=np.uint32), N, seed=5)
    assert len(got["bucket_group"]) == len(got["rows"])


def check_one_group_for_all(make_engine, pool: synth.Pool):
    """one bucket per user with rows"""
    got = check_one(make_engine, pool.tasks, pool.users, np.zeros(pool.tasks.n, np.uint32), 1, seed=6)
    assert len(got["bucket_group"]) == len(np.unique(pool.tasks.user[pool.tasks.pending == 0]))


def one_user_pool(seed, n_running, n_pending, fractional=True):
    """one user holding nearly every row (a segment far longer than a scan block covers), a second user with a handful"""
    pool = synth.make_pool(seed=seed, n_pending=n_pending, n_running=n_running, n_users=2, n_offers=8, fractional=fractional)
    rng = np.random.default_rng(seed)
    pool.tasks.user[:] = (rng.random(pool.tasks.n) < 0.0005).astype(np.uint32)
    return pool


def check_long_segment_and_bucket(make_engine, pool: synth.Pool, seed, big_share=0.8):
    """one user's segment and ONE bucket of it spanning several scan blocks: group 0 takes most rows, the rest are spread over a few
    groups and the ungrouped bucket, interleaved with it in the user's task order"""
    rng = np.random.default_rng(seed)
    g = rng.integers(1, 6, pool.tasks.n).astype(np.uint32)
    g[rng.random(pool.tasks.n) < 0.3] = NONE
    g[rng.random(pool.tasks.n) < big_share] = 0
    got = check_one(make_engine, pool.tasks, pool.users, g, 6, seed, must_fold=True)
    return got, g


def check_multi(make_engine, n_engines, seed, n_users, n_groups, with_map, n_running=300, n_pending=200, fractional=True):
    """the call without a pool over several engines: groups that cross pools, users in another order per engine (user_map)"""
    rng = np.random.default_rng(seed)
    pools, maps, engines = [], [], []
    try:
        for i in range(n_engines):
            ue = n_users if not with_map else int(rng.integers(max(1, n_users // 2), n_users + 1))
            pl = synth.make_pool(seed=seed * 100 + i, n_pending=n_pending, n_running=n_running if i != 1 else 0, n_users=ue, n_offers=8,
                                 fractional=fractional, gpus=(i % 2 == 0))
            pools.append((pl.tasks, random_groups(seed * 100 + i, pl.tasks, n_groups) if i != 2 else None))
            maps.append(rng.permutation(n_users)[:ue].astype(np.uint32) if with_map and i % 3 != 2 else None)
            if maps[-1] is None and ue < n_users:
                pass  # (the identity over the engine's own, fewer users)
            e = make_engine(A.default_params())
            engines.append(e)
            e.rank_stage(pl.tasks, pl.users)
            e.rank_run()
        m = maps if with_map else None
        if fractional:
            assert_must_fold(pools, n_users, m)
        groups = [g for _, g in pools]
        got = usage_breakdown_multi(engines, n_users, groups, n_groups, m)
        O.assert_same(got, _oracle(pools, n_users, m, None, True), "all users")
        ul = rng.integers(0, n_users, 12).astype(np.uint32)
        O.assert_same(usage_breakdown_multi(engines, n_users, groups, n_groups, m, users=ul), _oracle(pools, n_users, m, ul, True), "a list")
        if not with_map:  # the :pools sub-map: every engine's own answer
            for e, pl in zip(engines, pools):
                O.assert_same(e.usage_breakdown(pl[1], n_groups), _oracle([pl], e._n_users), "one pool")
    finally:
        for e in engines:
            e.close()
    return got


# ---- rounding traps -------------------------------------------------------------------------------------------------------------------
SS_IPT, SS_TILE = SO.SS_IPT, SO.SS_TILE


def bucket_trap_placements():
    """(name, places of B and the two halves among the rows of the trap bucket, rows of the bucket).  The bucket is the ungrouped one
    of user 0, so its rows are the first of the sorted order and place k of the bucket is place k of the scan.  In the user's segment
    every bucket row is followed by two rows of other buckets: only the regrouping brings the three values together.  The halves
    stand at places 2k, 2k + 1 of a bucket of 2^m rows: the oracle's tree adds them to each other first, as a kernel does whose
    layout puts them into one thread, one wave or one block apart from B."""
    return [
        ("one-thread", (0, 2, 3), 8),                        # B, 0, h, h are one thread's four items: its own sequential fold
        ("next-thread", (0, 4, 5), 16),                      # the halves are the next thread's first items: h + h, then B + 2h across lanes
        ("wave", (0, 100, 101), 512),                        # in another lane's partial sum of the same wave
        ("cross-wave", (0, 300, 301), 512),                  # in another wave of the block
        ("cross-block", (0, SS_TILE + 4, SS_TILE + 5), 2 * SS_TILE),  # in the next scan block: the carry B meets 2h
        ("halves-first", (40, 2, 3), 64),                    # a control: every order is exact, B + ulp(B)
    ]


def bucket_trap(name, places, n_bucket, big_c=1000.5, big_m=65536.0):
    """-> (Tasks, Users, group_of_row, n_groups): user 0 owns a trap bucket (ungrouped) whose rows are interleaved 1 : 2 with rows of two
    groups; user 1 a few plain rows and two pending ones"""
    n0 = 3 * n_bucket
    kind = np.arange(n0) % 3                      # 0: the trap bucket, 1 / 2: groups 0 / 1
    idx = np.flatnonzero(kind == 0)
    cpus, mem, gpus = np.full(n0, 1.0), np.full(n0, 2.0), np.full(n0, 1.0)
    at_big, at_half = idx[places[0]], idx[list(places[1:])]
    cpus[idx], mem[idx], gpus[idx] = 0.0, 0.0, 0.0
    cpus[at_big], mem[at_big], gpus[at_big] = big_c, big_m, 4.0
    cpus[at_half], mem[at_half], gpus[at_half] = SO.half(big_c), SO.half(big_m), SO.half(4.0)
    grp = np.where(kind == 0, NONE, kind - 1).astype(np.uint32)
    user = np.zeros(n0, np.uint32)
    cpus, mem, gpus = np.r_[cpus, np.full(7, 3.0)], np.r_[mem, np.full(7, 5.0)], np.r_[gpus, np.zeros(7)]
    grp, user = np.r_[grp, np.full(7, 1, np.uint32)].astype(np.uint32), np.r_[user, np.ones(7, np.uint32)].astype(np.uint32)
    pend = np.zeros(n0 + 7, np.uint8)
    pend[-2:] = 1
    return SO.tasks_of(cpus, mem, user, pend, gpus), SO.users_of(2), grp, 2


def total_trap(n_run, k, big_c=3.0 * 2.0 ** 4, big_m=2.0 ** 30):
    """the same for the per-user total in the rank's own order: user 0 has n_run = 2^m running rows, B the first, the halves the rows
    k and k + 1 (k even), each of the three in ANOTHER bucket (no bucket rounds, the total does); a pending row follows every fourth
    running row, so the segment the scan walks is longer than the list the total is made of"""
    cpus, mem, gpus, grp, pend = [], [], [], [], []
    for i in range(n_run):
        c, m, g, gr = 0.0, 0.0, 0.0, i % 5
        if i == 0:
            c, m, g, gr = big_c, big_m, 8.0, 10
        elif i in (k, k + 1):
            c, m, g, gr = SO.half(big_c), SO.half(big_m), SO.half(8.0), 11 + (i - k)
        cpus.append(c), mem.append(m), gpus.append(g), grp.append(gr), pend.append(0)
        if i % 4 == 3:
            cpus.append(7.0), mem.append(7.0), gpus.append(7.0), grp.append(10), pend.append(1)
    n = len(cpus)
    return SO.tasks_of(cpus, mem, np.zeros(n, np.uint32), pend, gpus), SO.users_of(1), np.array(grp, np.uint32), 13


def check_traps(make_engine):
    for name, places, n_bucket in bucket_trap_placements():
        tasks, users, grp, ng = bucket_trap(name, places, n_bucket)
        buckets, _ = O.sums_that_depend_on_order([(tasks, grp)], users.n, limit=1)
        assert bool(buckets) == (name != "halves-first"), name  # (the input rounds left to right and not as a tree — the control in no order)
        got = check_one(make_engine, tasks, users, grp, ng, seed=3)
        want_c = 1000.5 if name != "halves-first" else 1000.5 + 2 * SO.half(1000.5)
        assert got["bucket_usage"][0, 0] == want_c and int(got["bucket_group"][0]) == NONE, (name, got["bucket_usage"][0])
    for n_run, k in ((8, 2), (64, 6), (512, 300), (2 * SS_TILE, SS_TILE + 6), (4 * SS_TILE, 2 * SS_TILE + 552)):
        tasks, users, grp, ng = total_trap(n_run, k)
        buckets, us = O.sums_that_depend_on_order([(tasks, grp)], 1, limit=1)
        assert us == [0] and not buckets, (n_run, k)  # (the user's total depends on the order, no bucket's sum does)
        got = check_one(make_engine, tasks, users, grp, ng, seed=4)
        assert got["total"][0, 0] == 3.0 * 2.0 ** 4, (n_run, k, got["total"][0])


def check_negative_zero(make_engine):
    """0.0 + -0.0 is +0.0: a bucket of -0.0 values sums to +0.0, which a scan that starts from its first value would not give"""
    n = 12
    cpus = np.where(np.arange(n) % 2 == 0, -0.0, 1.0)
    tasks = SO.tasks_of(cpus, np.full(n, -0.0), np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.full(n, -0.0))
    grp = (np.arange(n) % 2).astype(np.uint32)
    got = check_one(make_engine, tasks, SO.users_of(1), grp, 2, seed=8)
    assert not np.signbit(got["bucket_usage"][:, :3]).any() and not np.signbit(got["total"][:, :3]).any()


# ---- state rule, the cycle ------------------------------------------------------------------------------------------------------------
def check_state_rule(make_engine):
    """COOK_E_STATE before any rank and after a stage / cook_cycle_update no rank has followed; COOK_E_INVALID for a group id that is no
    group, a user that is no user and too little room, each of which writes nothing"""
    pool = synth.make_pool(seed=31, n_pending=300, n_running=200, n_users=12, n_offers=16)
    grp = random_groups(31, pool.tasks, 9)
    with make_engine(A.default_params()) as e:
        with pytest.raises(CookError) as ex:
            e.usage_breakdown(grp, 9)
        assert ex.value.code == COOK_E_STATE
        e.rank_stage(pool.tasks, pool.users)
        with pytest.raises(CookError) as ex:
            e.usage_breakdown(grp, 9)
        assert ex.value.code == COOK_E_STATE
        e.rank_run()
        before = e.usage_breakdown(grp, 9)
        O.assert_same(before, _oracle([(pool.tasks, grp)], 12))
        bad = grp.copy()
        bad[np.flatnonzero(pool.tasks.pending == 0)[3]] = 9
        for call in (lambda: e.usage_breakdown(bad, 9), lambda: e.usage_breakdown(grp, 9, users=[0, 12]),
                     lambda: e.usage_breakdown(grp, 9, cap_rows=150)):
            with pytest.raises(CookError) as ex:
                call()
            assert ex.value.code == COOK_E_INVALID
        bad[np.flatnonzero(pool.tasks.pending == 0)[3]] = grp[np.flatnonzero(pool.tasks.pending == 0)[3]]
        bad[np.flatnonzero(pool.tasks.pending == 1)] = 77  # (pending rows' values are ignored)
        O.assert_same(e.usage_breakdown(bad, 9), before)
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        e.cycle_run(50)
        O.assert_same(e.usage_breakdown(grp, 9), before)
        # the first running task leaves: the rank's per-user order describes the old table until the next rank
        gone = int(np.flatnonzero(pool.tasks.pending == 0)[0])
        e.cycle_update(remove_task=[gone])
        with pytest.raises(CookError) as ex:
            e.usage_breakdown(np.delete(grp, gone), 9)
        assert ex.value.code == COOK_E_STATE
        e.cycle_run(50)
        keep = np.ones(pool.tasks.n, bool)
        keep[gone] = False
        t = pool.tasks
        t2 = A.Tasks(cpus=t.cpus[keep], mem=t.mem[keep], user=t.user[keep], priority=t.priority[keep], start_ms=t.start_ms[keep],
                     task_id=t.task_id[keep], job_id=t.job_id[keep], pending=t.pending[keep])
        O.assert_same(e.usage_breakdown(grp[keep], 9), _oracle([(t2, grp[keep])], 12))


def check_cycle_undisturbed(make_engine, pool: synth.Pool, k=200, n_groups=50):
    """a cycle fetched after the calls (all users, a list, the multi form) is the one fetched without them"""
    grp = random_groups(3, pool.tasks, n_groups)
    outs = []
    for with_calls in (False, True):
        with make_engine(A.default_params()) as e:
            e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
            e.cycle_run(k)
            if with_calls:
                e.usage_breakdown(grp, n_groups)
                e.usage_breakdown(None, 0, users=[1, 0, 1])
                usage_breakdown_multi([e], pool.users.n, [grp], n_groups)
            ranked, j2o, head = e.cycle_fetch()
            outs.append((ranked.copy(), j2o.copy(), head, e.cycle_fetch_considerable().copy(), e.rank_user_usage(pool.users.n).copy()))
    a, b = outs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3])
    assert np.array_equal(a[4].view(np.uint64), b[4].view(np.uint64))
