"""The cases of the release (cook_cycle_run_queue_release*: a queue cycle gives the resources of finished tasks back to the staged
offers, the staged user state and the groups' running cotasks on the device), shared by the emulator (test_release_emu.py) and GPU
(test_release_gpu.py) suites.  Expected values come from tests/release_oracle.py alone.  Per cycle the queue, rank_pos, job_to_offer,
head_matched, the considered count and cook_cycle_release_info are compared element for element.  The engine has no fetch of its staged
columns, so the released values are compared through their effect, as in tests/carry_cases.py: the conditions that make a released
column matter are asserted on the oracle alone, before the engine is called (the same cycles with that one release left out give
another result)."""
from __future__ import annotations

import copy
import ctypes as C
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

from cook_amd import _abi as A
from cook_amd import synth
from cook_amd.engine import CookError, cycle_match_multi, cycle_run_queue_release_multi, cycle_run_rank_multi
from tests import carry_cases as K
from tests import queue_cases as S
from tests import release_oracle as R
from tests.autoscale_cases import _same

COOK_E_INVALID, COOK_E_STATE = -1, -4
NONE = A.NONE_U32
P1 = K.P1


# ---- engine side -------------------------------------------------------------------------------------------------------------------
def run_step(e, cy):
    fin = getattr(cy, "finished", None)
    assert not callable(fin), "run the oracle first: it draws the lists"
    e.cycle_run_queue_release(cy.k, K.carry_of(cy), fin, **K.step_kw(cy))


def run_engine(make_engine, params, pool, cycles, *, expect_form=None, between=None):
    """-> per cycle what S.fetch returns, with .info = cook_cycle_release_info.  between(e, c): called after cycle c was fetched"""
    got = []
    with make_engine(params) as e:
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        for c, cy in enumerate(cycles):
            if cy.state is not None:
                e.cycle_set_considerable(cy.state, cy.eligible)
            if c == 0:
                e.cycle_run(cy.k)
            else:
                run_step(e, cy)
            g = S.fetch(e, False)
            g.info = e.release_info()
            got.append(g)
            if expect_form is not None and len(g.j2o):
                ms = e.match_stats()
                assert ms["placement_form"] == expect_form, (c, ms["placement_form"], hex(ms["classfit_refused"]))
            if between is not None:
                between(e, c)
    return got


def compare(got, want, cycles, tag=""):
    S.compare(got, want, cycles, tag)
    for c, (g, w) in enumerate(zip(got, want)):
        assert g.info == w.info, (f"{tag} cycle {c}", "release_info", g.info, w.info)


def check(make_engine, params, pool, cycles, want, **kw):
    got = run_engine(make_engine, params, pool, cycles, **kw)
    compare(got, want, cycles)
    return got


def assert_matters(params, pool, cycles, want, cols):
    for col in cols:
        assert K.differs(want, R.oracle(params, pool, cycles, stale=(col,))), f"the release of {col} changes no result: re-seed the case"


# ---- 1: base, non-dyadic --------------------------------------------------------------------------------------------------------------
def base_case(seed=301, *, fractional=False, scale=1.0, n_cycles=5, frac=0.35):
    pool, cycles = K.base_case(seed, fractional=fractional, scale=scale, n_cycles=n_cycles)
    groups = 1 if pool.groups is not None and pool.pending_jobs.group is not None else 0
    ends = R.finisher(seed, frac, offers=1, usage=1, groups=groups)  # (ONE for all cycles: no task ends twice)
    for c in range(1, n_cycles):
        cycles[c].finished = ends
    return pool, cycles


def base_oracle(params, pool, cycles, *, fractional=False):
    want = R.oracle(params, pool, cycles)
    K.assert_every_cycle_mixed(want)
    assert all(w.finished is not None and w.finished.n > 20 for w in want[1:]), "a queue cycle releases next to nothing: re-seed the case"
    assert all(w.info["with_row"] == w.finished.n and w.info["without_row"] == 0 for w in want[1:])
    assert K.differs(want[1:], R.oracle(params, pool, cycles, with_release=False)[1:]), "the releases change no result: re-seed the case"
    assert_matters(params, pool, cycles, want, ("cpus", "mem", "usage_count", "usage_cpus", "usage_mem", "pool_usage"))
    if fractional:
        # a tree in the kernel cannot pass: for some row and for some user the left-to-right sum differs in its bits from the same
        # numbers summed pairwise
        row_differs = user_differs = False
        for w in want[1:]:
            f = w.finished
            rows = np.asarray(R.rows_of(w.offers, f))
            for v in np.unique(rows[rows >= 0]):
                for col in (f.cpus, f.mem):
                    xs = col[rows == v]
                    row_differs = row_differs or R.seq_sum(xs) != R.pairwise_sum(xs)
            for u in np.unique(f.user):
                for col in (f.cpus, f.mem):
                    xs = col[f.user == u]
                    user_differs = user_differs or R.seq_sum(xs) != R.pairwise_sum(xs)
        assert row_differs and user_differs, "every segment sums the same pairwise as left to right: re-seed the case"
    return want


def check_base(make_engine, *, fractional=False, scale=1.0, algo=2, expect_form=0, seed=301):
    params = P1(match_algo=algo)
    pool, cycles = base_case(seed, fractional=fractional, scale=scale)
    want = base_oracle(params, pool, cycles, fractional=fractional)
    return check(make_engine, params, pool, cycles, want, expect_form=expect_form)


# ---- 2: every column, one hand-made pool each ------------------------------------------------------------------------------------------
def tiny_pool(n_jobs, offers, *, cpus=1.0, mem=100.0, groups=None, n_users=1, **job_cols):
    """n_jobs pending jobs of one user in submit order (priority 50, ascending job ids: the rank keeps the order)"""
    n = n_jobs
    cp = np.full(n, float(cpus)) if np.isscalar(cpus) else np.asarray(cpus, float)
    mm = np.full(n, float(mem)) if np.isscalar(mem) else np.asarray(mem, float)
    user = np.zeros(n, np.uint32)
    tasks = A.Tasks(cpus=cp, mem=mm, user=user, priority=np.full(n, 50, np.int32), start_ms=np.zeros(n, np.int64),
                    task_id=(10_000 + np.arange(n)).astype(np.int64), job_id=(100 + np.arange(n)).astype(np.int64), pending=np.ones(n, np.uint8))
    jobs = A.Jobs(cpus=cp.copy(), mem=mm.copy(), user=user.copy(), **job_cols)
    users = A.Users(div_cpus=np.full(n_users, A.DMAX), div_mem=np.full(n_users, A.DMAX))
    return SimpleNamespace(tasks=tasks, users=users, pending_jobs=jobs, offers=offers, groups=groups)


def one_host(null_cols=False, **kw):
    """one k8s host with room for everything; kw replaces columns.  null_cols: run_* / num_tasks / ports staged as NULL unless given"""
    d = dict(cpus=np.array([64.0]), mem=np.array([65536.0]), host=np.array([7], np.uint32), k8s=np.ones(1, np.uint8))
    if not null_cols:
        d.update(run_cpus=np.array([6.0]), run_mem=np.array([600.0]), run_count=np.array([0], np.int32), num_tasks=np.array([0], np.int32),
                 ports=np.array([50], np.int32))
    d.update(kw)
    return A.Offers(**d)


def tiny_state(*, quota_count=None, quota_cpus=None, quota_mem=None, pool_count=None):
    """one user who runs 3 jobs of 1 cpu / 100 mem; a quota given leaves room for ONE more job"""
    big = 2.0 ** 31 - 1
    pq = pu = None
    if pool_count is not None:
        pq, pu = A.quota(count=pool_count), A.usage(3.0, 3.0, 300.0, 0.0)
    return A.UserState(quota_count=np.array([quota_count or big]), quota_cpus=np.array([quota_cpus or A.DMAX]), quota_mem=np.array([quota_mem or A.DMAX]),
                       quota_gpus=np.full(1, A.DMAX), usage_count=np.array([3.0]), usage_cpus=np.array([3.0]), usage_mem=np.array([300.0]),
                       usage_gpus=np.zeros(1), pool_quota=pq, pool_usage=pu)


def column_cases(null_cols=False):
    """name -> (pool, user state or None, the columns whose release decides).  Two equal jobs, one host, K = 1: cycle 0 places job 0;
    the carry leaves no room for job 1 in that one column; once job 0 has finished and is released, job 1 is placed."""
    H = lambda **kw: one_host(null_cols, **kw)
    two = lambda offers, **kw: tiny_pool(2, offers, **kw)
    gpu = dict(gpus=np.ones(2), gpu_model=np.ones(2, np.uint32))
    cases = {
        "cpus": (two(H(cpus=np.array([4.0])), cpus=3.0), None, ("cpus",)),
        "mem": (two(H(mem=np.array([150.0]))), None, ("mem",)),
        "ports": (two(H(ports=np.array([3], np.int32)), ports=np.full(2, 2, np.int32)), None, ("ports",)),
        "scalar": (two(H(scalars=np.array([[9.0, 5.0]])), scalars=np.array([[np.nan, 3.0], [np.nan, 3.0]])), None, ("scalars",)),
        "num_tasks": (two(H(max_tasks=np.array([3], np.int32), num_tasks=np.array([2], np.int32))), None, ("num_tasks",)),
        # a k8s gpu host takes a gpu job only while it runs nothing, and only with the gpus free under the job's model
        "run_count_and_gpu_slot": (two(H(gpu_model=np.array([[2, 1]], np.uint32), gpu_count=np.array([[8.0, 1.0]]), run_cpus=None, run_mem=None,
                                         run_count=np.array([0], np.int32)), **gpu), None, ("run_count", "gpu_count")),
        "disk_slot": (two(H(disk_type=np.array([[1, 2]], np.uint32), disk_space=np.array([[900.0, 100.5]])), disk_request=np.full(2, 80.25),
                          disk_type=np.full(2, 2, np.uint32)), None, ("disk_space",)),
        "user_count": (two(H()), tiny_state(quota_count=4.0), ("usage_count",)),
        "user_cpus": (two(H()), tiny_state(quota_cpus=4.0), ("usage_cpus",)),
        "user_mem": (two(H()), tiny_state(quota_mem=400.0), ("usage_mem",)),
        "pool_usage": (two(H()), tiny_state(pool_count=4.0), ("pool_usage",)),
    }
    return cases


def column_cycles(state):
    usage = state is not None
    first = lambda h: R.finished_of(h, [(0, 0)], offers=1, usage=int(usage))
    return [R.cycle(1, state=state, eligible=np.ones(2, np.uint8) if usage else None), R.cycle(1, carry_offers=True, carry_usage=usage),
            R.cycle(1, carry_offers=True, carry_usage=usage, finished=first)]


def check_columns(make_engine, *, null_cols=False):
    params = P1()
    for name, (pool, state, cols) in column_cases(null_cols).items():
        cycles = column_cycles(state)
        want = R.oracle(params, pool, cycles)
        # job 0 placed; job 1 refused (or, under a quota, not even considered); job 0 released: job 1 placed
        assert want[0].j2o.tolist() == [0], name
        assert want[1].j2o.tolist() == ([] if state is not None else [-1]), (name, want[1].j2o)
        assert want[2].j2o.tolist() == [0] and want[2].info["with_row"] == 1, (name, want[2].j2o)
        for col in cols:
            stale = R.oracle(params, pool, cycles, stale=(col,))
            assert stale[2].j2o.tolist() != [0], f"{name}: job 1 is placed without the release of {col}"
        compare(run_engine(make_engine, params, pool, cycles), want, cycles, name)


# ---- 3: groups -------------------------------------------------------------------------------------------------------------------------
def _offers(cpus, attr=None, host=None):
    m = len(cpus)
    return A.Offers(cpus=np.asarray(cpus, float), mem=np.full(m, 1000.0), host=np.arange(m, dtype=np.uint32) if host is None else np.asarray(host, np.uint32),
                    attr=np.asarray(attr, np.uint32).reshape(m, -1) if attr is not None else None)


def entries(host, group, *, cpus=1.0, mem=100.0, offers=0, groups=1, **kw):
    n = len(host)
    return A.Finished(host=np.asarray(host, np.uint32), cpus=np.full(n, float(cpus)), mem=np.full(n, float(mem)), group=np.asarray(group, np.uint32),
                      offers=offers, groups=groups, **kw)


def check_groups(make_engine):
    params = P1()
    unique = lambda **kw: A.Groups(type=np.array([1], np.uint8), **kw)
    # -- unique: three members, ONE host.  Cycle 0 launches job 0 there; cycle 1 cannot place job 1 (the cotask is folded in); the cotask
    #    finishes: cycle 2 places job 1
    pool = tiny_pool(3, _offers([64.0]), groups=unique(), group=np.zeros(3, np.uint32))
    cycles = [R.cycle(1), R.cycle(1), R.cycle(1, finished=entries([0], [0]))]
    want = R.oracle(params, pool, cycles)
    assert [w.j2o.tolist() for w in want] == [[0], [-1], [0]] and want[2].info["cotasks_removed"] == 1
    assert R.oracle(params, pool, cycles, stale=("groups",))[2].j2o.tolist() == [-1]
    check(make_engine, params, pool, cycles, want)
    # -- ... placed last cycle, folded in THIS advance and released in the same advance: cycle 1 places job 1 at once
    cycles = [R.cycle(1), R.cycle(1, finished=entries([0], [0])), R.cycle(1)]
    want = R.oracle(params, pool, cycles)
    assert [w.j2o.tolist() for w in want] == [[0], [0], [-1]] and want[1].info["cotasks_removed"] == 1
    assert R.oracle(params, pool, cycles, with_release=False)[1].j2o.tolist() == [-1]
    check(make_engine, params, pool, cycles, want)
    # -- the same host twice in the list and ONE entry for it: one occurrence stays (the host stays taken); a second entry frees it.
    #    The entry for host 5 of group 0 and the one for group 1 find nothing: missing, and nothing changes
    g = A.Groups(type=np.array([1, 1], np.uint8), run_hosts=[[3, 0, 0], []])
    pool = tiny_pool(3, _offers([64.0]), groups=g, group=np.array([0, 0, NONE], np.uint32))
    cycles = [R.cycle(1), R.cycle(1, finished=entries([0, 5, 0], [0, 0, 1])), R.cycle(1, finished=entries([0, 0], [0, 0]))]
    want = R.oracle(params, pool, cycles)
    assert [w.j2o.tolist() for w in want] == [[-1], [-1], [0]]
    assert (want[1].info["cotasks_removed"], want[1].info["cotasks_missing"]) == (1, 2) and want[1].table.run_hosts == [[3, 0], []]
    assert (want[2].info["cotasks_removed"], want[2].info["cotasks_missing"]) == (1, 1) and want[2].table.run_hosts == [[3], []]
    check(make_engine, params, pool, cycles, want)
    # -- an entry with no match alone: cotasks_missing == 1 and the placement is the one without the step's release
    cycles = [R.cycle(1), R.cycle(1, finished=entries([9], [0]))]
    want = R.oracle(params, pool, cycles)
    assert want[1].info == dict(R.NO_INFO, cotasks_missing=1) and not K.differs(want, R.oracle(params, pool, cycles, with_release=False))
    check(make_engine, params, pool, cycles, want)
    # -- balanced: attribute 0 is 1, 1, 2 on hosts 0, 1, 2 and the group runs {1: two cotasks (hosts 0, 1), 2: one (host 2)}: the next
    #    member must go to value 2 (host 2).  The cotask on host 2 finishes and one on host 0: value 1 and 2 run one each... the counts
    #    decide, so the case is asserted through the oracle: the release changes where the member goes
    g = A.Groups(type=np.array([2], np.uint8), attr_key=np.array([0], np.uint32), minimum=np.array([0], np.int32), run_hosts=[[0, 1, 2]],
                 run_attrs=[[1, 1, 2]])
    pool = tiny_pool(2, _offers([2.0, 3.0, 8.0], attr=[1, 1, 2]), groups=g, group=np.zeros(2, np.uint32), cpus=2.0)
    cycles = [R.cycle(0), R.cycle(1, finished=entries([0, 1], [0, 0]))]
    want = R.oracle(params, pool, cycles)
    off = R.oracle(params, pool, cycles, with_release=False)
    assert want[1].table.run_hosts == [[2]] and want[1].j2o.tolist() != off[1].j2o.tolist(), (want[1].j2o, off[1].j2o)
    check(make_engine, params, pool, cycles, want)


# ---- 4: kernel boundaries --------------------------------------------------------------------------------------------------------------
def synthetic_list(pool, state, hosts, users, seed, **flags):
    """a list with the given hosts and users per entry (each shuffled on its own) and non-dyadic amounts; the staged offers and the
    user state are lowered / raised beforehand by about what the list gives back, so that hosts stay as full and users as close to their
    quotas as the case had them"""
    rng = np.random.default_rng(seed)
    n = len(hosts)
    hosts = np.asarray(hosts, np.uint32)[rng.permutation(n)]
    users = np.asarray(users, np.uint32)[rng.permutation(n)]
    cpus, mem = rng.choice([0.1, 0.3, 0.7, 1.1], size=n), rng.choice([10.1, 20.3, 40.7], size=n)
    o = pool.offers
    row = {int(h): v for v, h in enumerate(o.host)}
    for t in range(n):
        v = row.get(int(hosts[t]))
        if v is not None:
            o.cpus[v] = max(1.0, o.cpus[v] - np.floor(cpus[t] * 8) / 8)
            o.mem[v] = max(64.0, o.mem[v] - np.floor(mem[t]))
        u = int(users[t])
        state.usage_count[u] += 1.0
        state.usage_cpus[u] += np.floor(cpus[t] * 8) / 8
        state.usage_mem[u] += np.floor(mem[t])
    if state.pool_usage is not None:
        p = state.pool_usage
        state.pool_usage = A.usage(p.count + n, p.cpus + float(np.floor(cpus.sum())), p.mem + float(np.floor(mem.sum())), p.gpus)
        q = state.pool_quota
        state.pool_quota = A.quota(count=q.count + n)
    return A.Finished(host=hosts, cpus=cpus, mem=mem, user=users, **flags)


def check_segment_lengths(make_engine, *, seed=311):
    """ONE list with rows of 64, 65 and 129 entries (a wave's chunk, one more, two chunks and one), users of 256, 257 and 513 entries (a
    workgroup's chunk, one more, two chunks and one), entries on a host without a row and on a host id above the greatest staged one"""
    params = P1()
    n_cycles, k = 4, 150
    pool = K.base_pool(seed, n_pending=1300, n_running=50, k=k, n_cycles=n_cycles, fractional=True)
    state, eligible = K.base_state(pool, seed, fractional=True, pool_slack=0.93 * n_cycles * k)
    M, U = pool.offers.n, pool.users.n
    assert M >= 8 and U >= 6
    rng = np.random.default_rng(seed)
    others = [u for u in range(U) if u != pool.top_user]
    users = [others[0]] * 256 + [others[1]] * 257 + [others[2]] * 513
    users += [int(x) for x in rng.choice(others[3:], 1100 - len(users))]
    gone = int(pool.offers.host[5])  # (a host whose offer is not staged: its row leaves the pool below)
    keep = np.arange(M) != 5
    o = pool.offers
    pool.offers = A.Offers(cpus=o.cpus[keep], mem=o.mem[keep], host=o.host[keep], k8s=o.k8s[keep], run_cpus=o.run_cpus[keep], run_mem=o.run_mem[keep],
                           run_count=o.run_count[keep])
    hs = [int(h) for h in pool.offers.host]
    hosts = [hs[0]] * 64 + [hs[1]] * 65 + [hs[2]] * 129 + [gone] * 3 + [max(hs) + 1000] * 2
    hosts += [int(x) for x in rng.choice(hs[3:], 1100 - len(hosts))]
    fin = synthetic_list(pool, state, hosts, users, seed, offers=1, usage=1)
    cycles = [R.cycle(k, state=state, eligible=eligible), R.cycle(k, carry_offers=True, carry_usage=True, finished=fin)]
    cycles += [R.cycle(k, carry_offers=True, carry_usage=True) for _ in range(n_cycles - 2)]
    want = R.oracle(params, pool, cycles)
    K.assert_every_cycle_mixed(want)
    rows = np.asarray(R.rows_of(want[0].offers, fin))
    assert sorted(np.bincount(rows[rows >= 0]).tolist())[-1] == 129 and {64, 65, 129} <= set(np.bincount(rows[rows >= 0]).tolist())
    assert {256, 257, 513} <= set(np.bincount(fin.user).tolist())
    assert want[1].info["without_row"] == 5 and want[1].info["with_row"] == 1095
    assert K.differs(want[1:], R.oracle(params, pool, cycles, with_release=False)[1:])
    assert_matters(params, pool, cycles, want, ("cpus", "usage_count"))
    return check(make_engine, params, pool, cycles, want)


def check_many_segments(make_engine, *, seed=321):
    """more than 256 offers and more than 256 users with entries: each key set takes more than one radix pass"""
    params = P1()
    pool = synth.make_pool(seed=seed, n_pending=700, n_running=60, n_users=300, n_offers=300, fractional=True)
    o = pool.offers
    pool.offers = A.Offers(cpus=o.cpus, mem=o.mem, host=(o.host * 3 + 1).astype(np.uint32), k8s=o.k8s, run_cpus=o.run_cpus, run_mem=o.run_mem,
                           run_count=o.run_count)
    pool.top_user = int(np.bincount(pool.pending_jobs.user, minlength=300).argmax())
    state, eligible = K.base_state(pool, seed, fractional=True, pool_slack=400.0)
    M, U = pool.offers.n, pool.users.n
    rng = np.random.default_rng(seed)
    hosts = [int(h) for h in pool.offers.host] + [int(x) for x in rng.choice(pool.offers.host, 500)] + [0, 2, 3 * M + 7]
    users = list(range(U)) + [int(x) for x in rng.integers(0, U, len(hosts) - U)]
    fin = synthetic_list(pool, state, hosts, users, seed, offers=1, usage=1)
    k = 200
    cycles = [R.cycle(k, state=state, eligible=eligible), R.cycle(k, carry_offers=True, carry_usage=True, finished=fin),
              R.cycle(k, carry_offers=True, carry_usage=True)]
    want = R.oracle(params, pool, cycles)
    assert len(set(R.rows_of(want[0].offers, fin))) == M + 1 > 257 and len(set(fin.user.tolist())) == U > 256
    assert want[1].info["without_row"] == 3
    assert K.differs(want[1:], R.oracle(params, pool, cycles, with_release=False)[1:]), "re-seed the case"
    return check(make_engine, params, pool, cycles, want)


def check_long_group_list(make_engine):
    """a unique group that runs 130 cotasks, the last two on the pool's two hosts (rows 128 and 129: the list's third chunk of 64), one
    of them also in the first chunk: the entry for host 1 takes its FIRST row (row 5) and the host stays taken; host 0's only row goes"""
    params = P1()
    lst = [1000 + x for x in range(128)] + [0, 1]
    lst[5] = 1
    g = A.Groups(type=np.array([1], np.uint8), run_hosts=[lst])
    pool = tiny_pool(3, _offers([8.0, 2.0]), groups=g, group=np.zeros(3, np.uint32), cpus=2.0)
    cycles = [R.cycle(1), R.cycle(1, finished=entries([1, 0, 1127, 999], [0, 0, 0, 0])), R.cycle(1, finished=entries([1], [0]))]
    want = R.oracle(params, pool, cycles)
    # host 1 fits tighter: it is where the job goes as soon as it may
    assert [w.j2o.tolist() for w in want] == [[-1], [0], [1]], [w.j2o.tolist() for w in want]
    assert (want[1].info["cotasks_removed"], want[1].info["cotasks_missing"]) == (3, 1)
    assert len(want[1].table.run_hosts[0]) == 127 and want[1].table.run_hosts[0][-1] == 1 and 1 not in want[1].table.run_hosts[0][:-1]
    return check(make_engine, params, pool, cycles, want)


def check_no_rows(make_engine, hosts=(0, 2, 5)):
    """n == 1; entries only for hosts without a row (one between the staged ids, two above the greatest): without_row == n and the offers
    are as they were.  hosts: the staged host ids — small ones go through the host-indexed table, sparse ones (the greatest id far above
    8 x offers + 65536) through release_keys' lookup in o_host itself"""
    params = P1()
    assert hosts[0] + 1 < hosts[1] < hosts[2] < 4000000000 - 4
    pool = tiny_pool(4, _offers([4.0, 4.0, 4.0], host=hosts), cpus=3.0)
    lost = A.Finished(host=np.array([hosts[0] + 1, hosts[2] + 4, 4000000000], np.uint32), cpus=np.full(3, 50.0), mem=np.full(3, 100.0), offers=1)
    one = A.Finished(host=np.array([hosts[1]], np.uint32), cpus=np.array([3.0]), mem=np.array([100.0]), offers=1)
    mixed = A.Finished(host=np.array([hosts[2], hosts[1] + 1, hosts[0], hosts[2]], np.uint32), cpus=np.full(4, 0.75), mem=np.full(4, 100.0), offers=1)
    cycles = [R.cycle(4), R.cycle(4, carry_offers=True, finished=lost), R.cycle(4, carry_offers=True, finished=one),
              R.cycle(4, carry_offers=True, finished=mixed)]
    want = R.oracle(params, pool, cycles)
    assert [w.j2o.tolist() for w in want] == [[0, 1, 2, -1], [-1], [1], []], [w.j2o.tolist() for w in want]
    assert want[1].info == dict(R.NO_INFO, without_row=3) and want[2].info == dict(R.NO_INFO, with_row=1)
    assert want[3].info == dict(R.NO_INFO, with_row=3, without_row=1, counts_clamped=1), want[3].info
    assert not K.differs(want[:2], R.oracle(params, pool, cycles, with_release=False)[:2])
    return check(make_engine, params, pool, cycles, want)


# ---- 5: the last cycle considered nothing ------------------------------------------------------------------------------------------------
def check_no_advance(make_engine):
    params = P1()
    first = lambda h: R.finished_of(h, [(0, 0)], offers=1)
    # -- K = 0: cycle 1 carries cycle 0's placement and considers nothing; cycle 2's advance has nothing to advance over, and releases
    pool = tiny_pool(2, one_host(cpus=np.array([4.0])), cpus=3.0)
    cycles = [R.cycle(1), R.cycle(0, carry_offers=True), R.cycle(1, carry_offers=True, finished=first)]
    want = R.oracle(params, pool, cycles)
    assert [w.j2o.tolist() for w in want] == [[0], [], [0]] and want[2].info["with_row"] == 1
    assert R.oracle(params, pool, cycles, with_release=False)[2].j2o.tolist() == [-1]
    check(make_engine, params, pool, cycles, want)
    # -- an empty queue: the one job is placed and leaves; the release still runs (its counts say so) and a rank sees the offers
    pool = tiny_pool(1, one_host(cpus=np.array([4.0])), cpus=3.0)
    cycles = [R.cycle(1), R.cycle(1, carry_offers=True), R.cycle(1, carry_offers=True, finished=first)]
    want = R.oracle(params, pool, cycles)
    assert [len(w.Q) for w in want] == [1, 0, 0] and want[2].info["with_row"] == 1
    check(make_engine, params, pool, cycles, want)


# ---- 6: without a carry, behind a carry; the last match's inputs stay -------------------------------------------------------------------
def check_explain(make_engine, *, scale=0.5, seed=331):
    """queue cycles that release WITHOUT a carry (a fresh set of columns of the release's own) and BEHIND one (the carry's fresh set, in
    place) in turns.  cook_match_explain after every cycle answers as on an engine that is handed the oracle's offers and user state
    for that cycle through step->offers and cook_cycle_set_considerable: from the inputs of the match that ran last.
    That a release never writes the columns the LAST match read could only be seen between an advance and its placement (the deferred
    form); there cook_match_explain does not answer at all (COOK_E_STATE, asserted below: a set-up placement is no match that ran), so the
    property is held by construction — a release without a carry writes CarryBufs' other column set, a release behind one the set that
    carry has just written — and what this case pins is that each of the two paths hands the NEXT match the right columns."""
    params = P1()
    pool, cycles = base_case(seed, fractional=True, scale=scale, n_cycles=5, frac=0.5)
    for c in (1, 3):
        cycles[c].carry = False
    want = R.oracle(params, pool, cycles)
    K.assert_every_cycle_mixed(want)
    assert K.differs(want[1:], R.oracle(params, pool, cycles, with_release=False)[1:])
    seen = [[], []]

    def look(into):
        return lambda e, c: into.append(e.match_explain(np.arange(len(want[c].pos))))
    compare(run_engine(make_engine, params, pool, cycles, between=look(seen[0])), want, cycles)
    handed = [cycles[0]] + [R.cycle(cy.k, state=w.state, eligible=cycles[0].eligible, offers=w.offers, carry=False) for cy, w in zip(cycles[1:], want[1:])]
    plain = R.oracle(params, pool, handed)
    assert not K.differs(plain, want)
    S.compare(run_engine(make_engine, params, pool, handed, between=look(seen[1])), want, cycles, "handed:")
    _same(seen[0], seen[1])
    with make_engine(params) as e:  # between a deferred advance (with a release without a carry) and its placement: no answer
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        e.cycle_set_considerable(cycles[0].state, cycles[0].eligible)
        e.cycle_run(cycles[0].k)
        cycle_run_queue_release_multi([e], [cycles[1].k], [K.step_kw(cycles[1])], [None], [cycles[1].finished])
        assert _code(lambda: e.match_explain(np.arange(4))) == COOK_E_STATE
        cycle_match_multi([e])
        g = S.fetch(e, False)
        g.info = e.release_info()
        compare([g], want[1:2], cycles[1:2], "deferred:")


# ---- 7: clamp --------------------------------------------------------------------------------------------------------------------------
def check_clamp(make_engine):
    """more entries than the host runs: run_count and num_tasks stop at 0, counts_clamped says so, and the host then takes exactly
    max_tasks jobs (it would take more had the count gone below 0)"""
    params = P1()
    pool = tiny_pool(6, one_host(max_tasks=np.array([3], np.int32), num_tasks=np.array([2], np.int32), run_count=np.array([2], np.int32)))
    five = A.Finished(host=np.full(5, 7, np.uint32), cpus=np.full(5, 0.5), mem=np.full(5, 10.0), offers=1)
    cycles = [R.cycle(1), R.cycle(1, carry_offers=True), R.cycle(1, carry_offers=True, finished=five)] + [R.cycle(1, carry_offers=True) for _ in range(3)]
    want = R.oracle(params, pool, cycles)
    assert [w.j2o.tolist() for w in want] == [[0], [-1], [0], [0], [0], [-1]], [w.j2o.tolist() for w in want]
    assert want[2].info == dict(R.NO_INFO, with_row=5, counts_clamped=1) and int(want[2].offers.num_tasks[0]) == 0
    return check(make_engine, params, pool, cycles, want)


# ---- 8: multi --------------------------------------------------------------------------------------------------------------------------
def check_multi(make_engine, *, scale=0.5):
    """three ragged pools through cook_cycle_run_queue_release_multi: pool 0 carries and releases, pool 1 carries only (no list), pool 2
    carries and releases and has its list refused in round 2: it stays untouched (the same step runs next), the others go on"""
    params = P1(match_algo=2)
    shapes = [(1.0, 341, 5), (0.5, 342, 5), (0.7, 343, 4)]
    cases = [base_case(seed, scale=s * scale, n_cycles=n, fractional=(seed == 343)) for s, seed, n in shapes]
    for cy in cases[1][1][1:]:
        cy.finished = None
    want = [R.oracle(params, pl, cs) for pl, cs in cases]
    for w in want:
        K.assert_every_cycle_mixed(w)
    assert all(w.finished is not None for i in (0, 2) for w in want[i][1:]) and all(w.finished is None for w in want[1])
    engines = [make_engine(params) for _ in cases]
    got = [[] for _ in cases]

    def fetch(i):
        g = S.fetch(engines[i], False)
        g.info = engines[i].release_info()
        got[i].append(g)
    try:
        for e, (pl, cs) in zip(engines, cases):
            e.cycle_stage(pl.tasks, pl.users, pl.pending_jobs, pl.offers, pl.groups)
            e.cycle_set_considerable(cs[0].state, cs[0].eligible)
        cycle_run_rank_multi(engines, [cs[0].k for _, cs in cases])
        cycle_match_multi(engines)
        for i in range(3):
            fetch(i)
        nxt = [1, 1, 1]
        for rnd in range(1, 6):
            cur = [cs[min(nxt[i], len(cs) - 1)] for i, (_, cs) in enumerate(cases)]
            steps, carries, fins, ks = [K.step_kw(cy) for cy in cur], [K.carry_of(cy) for cy in cur], [cy.finished for cy in cur], [cy.k for cy in cur]
            if rnd == 2:  # a user id out of range in pool 2's list: refused for pool 2 alone
                bad = copy.copy(fins[2])
                bad.user = bad.user.copy()
                bad.user[-1] = cases[2][0].users.n
                fins[2] = bad
                with pytest.raises(CookError) as ex:
                    cycle_run_queue_release_multi(engines, ks, steps, carries, fins)
                assert ex.value.code == COOK_E_INVALID
                live = [0, 1]
            else:
                live = [0, 1, 2]
                if any(nxt[i] >= len(cases[i][1]) for i in live):
                    break
                cycle_run_queue_release_multi(engines, ks, steps, carries, fins)
            cycle_match_multi([engines[i] for i in live])
            for i in live:
                fetch(i)
                nxt[i] += 1
    finally:
        for e in engines:
            e.close()
    for i, (pl, cs) in enumerate(cases):
        assert len(got[i]) >= 3
        compare(got[i], want[i][:len(got[i])], cs, f"pool {i}")
    return got


# ---- 9: the class-ordered walk ----------------------------------------------------------------------------------------------------------
def classfit_case(seed=105, k=150, n_cycles=5):
    """test_queue_random_groups' pool for the class-ordered walk with a third of the jobs in unique groups of 2 to 6 whose cotasks
    the releases take out again"""
    pool = synth.make_pool(seed=seed, n_pending=500, n_running=200, n_users=25, n_offers=24, gpus=True, constraints=True, fractional=False)
    rng = np.random.default_rng(seed)
    P = pool.pending_jobs.n
    grp = np.full(P, NONE, np.uint32)
    members, n_g, q = rng.permutation(P)[:P // 3], 0, 0
    while q < len(members):
        size = int(rng.integers(2, 7))
        grp[members[q:q + size]] = n_g
        n_g, q = n_g + 1, q + size
    pool.pending_jobs = dataclasses.replace(pool.pending_jobs, group=grp)
    hosts = [int(h) for h in pool.offers.host]
    pool.groups = A.Groups(type=np.ones(n_g, np.uint8), run_hosts=[[int(h) for h in rng.choice(hosts, int(rng.integers(0, 3)), replace=False)] for _ in range(n_g)])
    ends = R.finisher(seed, 0.5, offers=1, groups=1)
    return pool, [R.cycle(k)] + [R.cycle(k, carry_offers=True, finished=ends) for _ in range(n_cycles - 1)]


def check_classfit(make_engine):
    params = P1(match_algo=3)
    pool, cycles = classfit_case()
    want = R.oracle(params, pool, cycles)
    K.assert_every_cycle_mixed(want)
    assert sum(w.info["cotasks_removed"] for w in want) >= 10
    assert_matters(params, pool, cycles, want, ("groups", "cpus"))
    return check(make_engine, params, pool, cycles, want, expect_form=3)


# ---- 10: refusals and persistence -------------------------------------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(CookError) as ex:
        fn()
    return ex.value.code


def check_refusals(make_engine, *, scale=0.5):
    params = P1()
    pool, cycles = base_case(305, scale=scale, n_cycles=4)
    k, state, eligible = cycles[0].k, cycles[0].state, cycles[0].eligible
    U = pool.users.n
    want = R.oracle(params, pool, cycles)
    ok = want[1].finished
    assert ok.n > 5
    n = ok.n
    rep = lambda **kw: dataclasses.replace(ok, **kw)
    col = lambda a, x: np.concatenate([a[:-1], [x]]).astype(a.dtype)
    dup = A.Offers(cpus=pool.offers.cpus, mem=pool.offers.mem, host=col(pool.offers.host, pool.offers.host[0]))
    both = A.QueueCarry(offers=True, usage=True)
    gtab = A.Groups(type=np.ones(2, np.uint8))
    with make_engine(params) as e:
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, gtab)
        e.cycle_run(k)  # no user state staged
        assert _code(lambda: e.cycle_run_queue_release(k, None, ok)) == COOK_E_STATE
        e.cycle_set_considerable(state, eligible)
        e.cycle_run(k)
        got = [S.fetch(e, False)]
        bad = [
            (rep(offers=2), {}), (rep(usage=2), {}), (rep(groups=7), {}),
            (ok, dict(offers=pool.offers)),                                    # offers = 1 together with step->offers
            (rep(groups=1, group=np.zeros(n, np.uint32)), dict(groups=gtab)),  # groups = 1 together with step->groups
            (rep(user=None, offers=0), {}),                                    # usage = 1 without user
            (rep(scalars=np.zeros((n, 4))), {}),                               # n_scalars > COOK_MAX_SCALARS
            (rep(cpus=col(ok.cpus, -1.0)), {}), (rep(mem=col(ok.mem, np.inf)), {}), (rep(cpus=col(ok.cpus, np.nan)), {}),
            (rep(gpus=col(np.zeros(n), -0.5)), {}), (rep(scalars=col(np.zeros(n), -2.0).reshape(n, 1)), {}),
            (rep(user=col(ok.user, U)), {}),
            (rep(group=col(np.full(n, NONE, np.uint32), 2)), {}),              # a group >= G that is not COOK_NONE_U32
        ]
        for fin, step in bad:
            assert _code(lambda: e.cycle_run_queue_release(k, both, fin, **step)) == COOK_E_INVALID, (fin, step)
        for miss in ("host", "cpus", "mem"):  # (the dataclass insists on them: the struct as a C caller could pass it)
            st, keep = ok.as_struct()
            setattr(st, miss, None)
            qs, keep2 = e._queue_step()
            assert e._lib.cook_cycle_run_queue_release(e._h, C.byref(qs), None, C.byref(st), k) == COOK_E_INVALID, miss
        assert e.release_info() == R.NO_INFO
        _same(vars(S.fetch(e, False)), vars(got[0]))
        # the same steps without the offending part: the queue, the offers, the user state and the groups are as they were
        for cy in cycles[1:3]:
            run_step(e, cy)
            got.append(S.fetch(e, False))
        S.compare(got, want[:3], cycles[:3], "after the refusals:")
        # a rank sees the released offers and usage: the same cycle as a fresh engine staged with the oracle's values
        e.cycle_run(k)
        again = S.fetch(e, False)
        assert e.release_info() == want[2].info  # (of the last QUEUE cycle)
        # two staged offers on one host: offers = 1 is refused, usage alone goes through
        e.cycle_run_queue(k, offers=dup)
        assert _code(lambda: e.cycle_run_queue_release(k, None, ok)) == COOK_E_INVALID
        e.cycle_run_queue_release(k, None, rep(offers=0))
    from oracle import pyoracle
    last = want[2]  # its offers and state hold the carries and releases of steps 1 and 2; cycle 2's own placements are not in
    Q0 = want[0].Q
    jq, queue = S._queue_of(pool, Q0, eligible)
    pos = pyoracle.considerable(queue, last.state, k)[0]
    j2o, _, head = pyoracle.match(params, pool.pending_jobs.take(jq[pos]), last.offers, None)
    assert np.array_equal(again.Q, Q0) and np.array_equal(again.pos, pos) and np.array_equal(again.j2o, j2o) and again.head == head
    assert not np.array_equal(j2o, want[0].j2o)
    # finished = NULL, n = 0 and all flags 0 are cook_cycle_run_queue_carry, byte for byte
    outs = []
    for mode in ("carry", "null", "empty", "nothing"):
        with make_engine(params) as e:
            e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
            e.cycle_set_considerable(state, eligible)
            e.cycle_run(k)
            for _ in range(2):
                if mode == "carry":
                    e.cycle_run_queue_carry(k, both)
                else:
                    fin = {"null": None, "empty": A.Finished(host=np.zeros(0, np.uint32), cpus=np.zeros(0), mem=np.zeros(0), offers=1),
                           "nothing": rep(offers=0, usage=0, groups=0)}[mode]
                    e.cycle_run_queue_release(k, both, fin)
                    assert e.release_info() == R.NO_INFO
            outs.append((vars(S.fetch(e, False)), e.match_metrics(n_users=U), e.match_explain(np.arange(30))))
    for o in outs[1:]:
        _same(o, outs[0])


# ---- 11: ABI ----------------------------------------------------------------------------------------------------------------------------
def struct_layout_sources():
    fields = [("cook_finished", f) for f, _ in A.CookFinished._fields_] + [("cook_release_info", f) for f, _ in A.CookReleaseInfo._fields_]
    prints = "".join(f'printf("%zu ", offsetof({s}, {f}));' for s, f in fields)
    text = ('#include <stdio.h>\n#include <stddef.h>\n#include "cookmatch.h"\nint main(){printf("%zu %zu ", sizeof(cook_finished), '
            f'sizeof(cook_release_info));{prints}printf("%d\\n", COOK_ABI_VERSION);return 0;}}')
    want = [C.sizeof(A.CookFinished), C.sizeof(A.CookReleaseInfo)]
    want += [getattr(A.CookFinished, f).offset for f, _ in A.CookFinished._fields_] + [getattr(A.CookReleaseInfo, f).offset for f, _ in A.CookReleaseInfo._fields_]
    return text, want + [A.ABI_VERSION]
