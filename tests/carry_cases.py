"""The cases of the carry (cook_cycle_run_queue_carry*: a queue cycle moves the last cycle's kept placements into the staged offers and
the staged user state on the device), shared by the emulator (test_carry_emu.py) and GPU (test_carry_gpu.py) suites.  Expected values
come from tests/carry_oracle.py alone.  Per cycle the queue, rank_pos, job_to_offer, head_matched and the considered count are compared
element for element.  The engine has no fetch of its staged offer columns or user arrays, so the carried values are compared through
their effect: every case runs queue cycles with no upload whose considerable output and placement depend on them, and the conditions
that make a carried column matter are asserted on the oracle alone, before the engine is called (`matters`: the same cycles with that
one column left stale give another result)."""
from __future__ import annotations

import copy
import ctypes as C
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

from cook_amd import _abi as A
from cook_amd import synth
from cook_amd.engine import CookError, cycle_match_multi, cycle_run_queue_carry_multi, cycle_run_rank_multi
from oracle import pyoracle
from tests import carry_oracle as O
from tests import queue_cases as S
from tests.autoscale_cases import _same

COOK_E_INVALID, COOK_E_STATE = -1, -4
P1 = lambda **kw: A.default_params(good_enough_fitness=1.0, **kw)


# ---- pools -------------------------------------------------------------------------------------------------------------------------
def base_pool(seed, *, n_pending=2600, n_running=100, n_users=12, n_offers=40, k=300, n_cycles=5, fractional=False, fill=0.9):
    """synth's pool with (1) the largest user's share raised so that its jobs rank first — one cycle then keeps more than 256 jobs of
    ONE user —, (2) 2 % of the pending jobs asking for more memory than any host has — every cycle leaves a considered job
    unmatched —, (3) the offers scaled to hold about `fill` of the n_cycles * k jobs the cycles consider: K binds in every cycle (so
    every cycle considers new jobs), a host takes dozens of jobs, and the last cycles meet hosts the earlier ones filled."""
    pool = synth.make_pool(seed=seed, n_pending=n_pending, n_running=n_running, n_users=n_users, n_offers=n_offers, fractional=fractional)
    rng = np.random.default_rng(seed + 7)
    J, T = pool.pending_jobs, pool.tasks
    pidx = np.flatnonzero(T.pending)
    top = int(np.bincount(J.user, minlength=n_users).argmax())
    for col in (pool.users.div_cpus, pool.users.div_mem, pool.users.div_gpus):
        col[top] = 1e12
    huge = rng.random(J.n) < 0.02
    J.mem[huge] = 1e9
    T.mem[pidx[huge]] = 1e9
    o = pool.offers
    scale = fill * n_cycles * k * float(np.mean(J.cpus)) / float(np.sum(o.cpus))
    cpus = np.floor(o.cpus * scale)
    pool.offers = A.Offers(cpus=cpus, mem=np.floor(cpus * rng.uniform(3000.0, 4500.0, o.n)), host=o.host, k8s=o.k8s, run_cpus=o.run_cpus, run_mem=o.run_mem, run_count=o.run_count)
    pool.top_user = top
    return pool


def base_state(pool, seed, *, fractional=False, tokens=None, enforce=False, pool_usage_given=True, pool_slack=None):
    """a user state whose quotas the kept placements of the first cycles use up"""
    rng = np.random.default_rng(seed + 11)
    U = pool.users.n
    ucount = rng.integers(0, 20, U).astype(np.float64)
    ucpus = ucount * 3.0 + (0.1 if fractional else 0.0)
    umem = ucount * 10240.0 + (0.3 if fractional else 0.0)
    # every second user is limited in ONE resource — count, cpus or mem in turn —, with room for 15 to 50 more jobs
    qcount, qcpus, qmem = np.full(U, 2.0 ** 31 - 1), np.full(U, A.DMAX), np.full(U, A.DMAX)
    others = [u for u in range(U) if u != pool.top_user]
    for x, u in enumerate(others[::2]):
        room = float(rng.integers(15, 50))
        if x % 3 == 0:
            qcount[u] = ucount[u] + room
        elif x % 3 == 1:
            qcpus[u] = ucpus[u] + 3.0 * room + (0.7 if fractional else 0.0)
        else:
            qmem[u] = umem[u] + 10240.0 * room
    pu = None
    if pool_usage_given:  # (what the host would pass: the users' sum, left to right)
        s = [0.0, 0.0, 0.0]
        for u in range(U):
            s = [s[0] + ucount[u], s[1] + ucpus[u], s[2] + umem[u]]
        pu = A.usage(s[0], s[1], s[2], 0.0)
    pq = A.quota(count=float(ucount.sum()) + pool_slack) if pool_slack is not None else None
    st = A.UserState(quota_count=qcount, quota_cpus=qcpus, quota_mem=qmem, quota_gpus=np.full(U, A.DMAX), usage_count=ucount,
                     usage_cpus=ucpus, usage_mem=umem, usage_gpus=np.zeros(U), tokens_left=tokens, enforce_rate_limit=enforce,
                     pool_quota=pq, pool_usage=pu if pq is not None else None)
    eligible = (rng.random(pool.pending_jobs.n) < 0.9).astype(np.uint8)
    return st, eligible


def carry_cycles(k, n_cycles, state, eligible, **kw):
    """a rank cycle, then queue cycles with offers = usage = 1 and NO upload"""
    return [O.cycle(k, state=state, eligible=eligible)] + [O.cycle(k, carry_offers=True, carry_usage=True, **kw) for _ in range(n_cycles - 1)]


def columns_pool(seed, *, null_cols=False, n_pending=500, n_offers=24):
    """k8s offers with 2 gpu slots and 2 disk slots, ports, 2 named scalars, max_tasks; jobs with disk requests, ports and scalar
    requests (some NaN).  cpus and mem are plentiful: the other columns decide.  null_cols: run_* / num_tasks / ports staged as NULL."""
    pool = synth.make_pool(seed=seed, n_pending=n_pending, n_running=40, n_users=8, n_offers=n_offers, gpus=True)
    rng = np.random.default_rng(seed + 3)
    J = pool.pending_jobs
    P, M = J.n, n_offers
    scal = np.where(rng.random((P, 2)) < 0.5, np.nan, rng.choice([0.5, 1.0, 2.5], size=(P, 2)))
    pool.pending_jobs = dataclasses.replace(
        J, disk_request=np.where(rng.random(P) < 0.6, rng.choice([100.0, 250.5, 1000.0], size=P), -1.0),
        disk_type=rng.choice([1, 2], size=P).astype(np.uint32),
        ports=None if null_cols else np.where(rng.random(P) < 0.3, rng.integers(1, 4, P), 0).astype(np.int32), scalars=scal)
    gh = rng.random(M) < 0.25
    gm = np.zeros((M, 2), np.uint32)
    gc = np.zeros((M, 2))
    gm[gh] = [1, 2]
    gc[gh] = rng.choice([1.0, 2.0, 4.0, 8.0], size=(int(gh.sum()), 2))
    cpus = rng.choice([64.0, 96.0, 128.0], size=M)
    run_n = np.where(gh, 0, rng.integers(0, 4, M)).astype(np.int32)
    pool.offers = A.Offers(
        cpus=cpus, mem=cpus * 8192.0, host=np.arange(M, dtype=np.uint32), k8s=np.ones(M, np.uint8), gpu_model=gm, gpu_count=gc,
        disk_type=np.tile(np.array([1, 2], np.uint32), (M, 1)), disk_space=rng.choice([1500.0, 3000.5], size=(M, 2)),
        max_tasks=rng.integers(8, 20, M).astype(np.int32), num_tasks=None if null_cols else run_n.copy(),
        run_cpus=None if null_cols else run_n * 3.0, run_mem=None if null_cols else run_n * 10240.0, run_count=None if null_cols else run_n,
        ports=None if null_cols else rng.integers(3, 9, M).astype(np.int32), scalars=rng.choice([4.0, 9.5], size=(M, 2)))
    return pool


# ---- what must hold on the oracle alone ----------------------------------------------------------------------------------------------
def differs(a, b):
    return any(not np.array_equal(x.Q, y.Q) or not np.array_equal(x.pos, y.pos) or not np.array_equal(x.j2o, y.j2o) for x, y in zip(a, b))


def assert_every_cycle_mixed(want):
    for c, w in enumerate(want):
        assert (w.j2o >= 0).any() and (w.j2o < 0).any(), f"cycle {c} keeps no match or leaves no considered job unmatched: re-seed the case"


def oracle_stale(params, pool, cycles, offer_cols=(), state_cols=()):
    """the oracle's cycles with the named columns NOT carried (they keep their stale values); everything else carried"""
    def patched_offers(off, jobs, j2o, hit):
        new = real_offers(off, jobs, j2o, hit)
        return dataclasses.replace(new, **{c: getattr(off, c) for c in offer_cols})

    def patched_usage(st, jobs, hit, spend):
        new = real_usage(st, jobs, hit, spend)
        return dataclasses.replace(new, **{c: getattr(st, c) for c in state_cols})
    real_offers, real_usage = O.carry_offers, O.carry_usage
    O.carry_offers, O.carry_usage = patched_offers, patched_usage
    try:
        return O.oracle(params, pool, cycles)
    finally:
        O.carry_offers, O.carry_usage = real_offers, real_usage


def assert_matters(params, pool, cycles, want, offer_cols=(), state_cols=()):
    for c in offer_cols:
        assert differs(want, oracle_stale(params, pool, cycles, offer_cols=(c,))), f"the carry of the offers' {c} changes no result: re-seed the case"
    for c in state_cols:
        assert differs(want, oracle_stale(params, pool, cycles, state_cols=(c,))), f"the carry of the users' {c} changes no result: re-seed the case"


def assert_quota_only_by_carry(pool, want):
    """a job of some queue cycle that the per-user quota filter rejects under the carried usage and passes under the staged one"""
    for w in want[1:]:
        carried = set(O.quota_rejected(w.queue, w.state).tolist())
        stale = set(O.quota_rejected(w.queue, want[0].state).tolist())
        if carried - stale:
            return
    raise AssertionError("no job is rejected by the user-quota filter because of carried usage: re-seed the case")


# ---- engine side -------------------------------------------------------------------------------------------------------------------
def step_kw(cy):
    return dict(offer_skipped=cy.offer_skipped, remove_mode=cy.remove_mode, offers=cy.offers, groups=cy.groups)


def carry_of(cy):
    return A.QueueCarry(offers=cy.carry_offers, usage=cy.carry_usage, tokens_left=cy.tokens_left) if cy.carry else None


def run_step(e, cy):
    if cy.carry:
        e.cycle_run_queue_carry(cy.k, carry_of(cy), **step_kw(cy))
    else:
        e.cycle_run_queue(cy.k, **step_kw(cy))


def run_engine(make_engine, params, pool, cycles, *, expect_form=None, stage=None):
    got = []
    with make_engine(params) as e:
        (stage or (lambda e: e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)))(e)
        for c, cy in enumerate(cycles):
            if cy.state is not None:
                e.cycle_set_considerable(cy.state, cy.eligible)
            if c == 0:
                e.cycle_run(cy.k)
            else:
                run_step(e, cy)
            got.append(S.fetch(e, False))
            if expect_form is not None and len(got[-1].j2o):
                ms = e.match_stats()
                assert ms["placement_form"] == expect_form, (c, ms["placement_form"], hex(ms["classfit_refused"]))
    return got


def check(make_engine, params, pool, cycles, want, **kw):
    got = run_engine(make_engine, params, pool, cycles, **kw)
    S.compare(got, want, cycles)
    return got


# ---- 1 / 2: base, non-dyadic ----------------------------------------------------------------------------------------------------------
def base_case(seed=201, *, fractional=False, scale=1.0, n_cycles=5):
    k = int(300 * scale)
    pool = base_pool(seed, n_pending=int(2600 * scale), n_running=int(100 * scale), k=k, n_cycles=n_cycles, fractional=fractional)
    state, eligible = base_state(pool, seed, fractional=fractional, pool_slack=0.93 * n_cycles * k)
    return pool, carry_cycles(k, n_cycles, state, eligible)


def base_oracle(params, pool, cycles, *, big_user=True):
    want = O.oracle(params, pool, cycles)
    assert_every_cycle_mixed(want)
    k = cycles[0].k
    assert all(len(w.pos) > min(256, k // 2) for w in want[:-1]), "the considered jobs of a cycle do not span two 256-thread blocks"
    assert max(np.bincount(w.j2o[w.j2o >= 0]).max() for w in want) >= 3, "no offer takes several kept jobs"
    if big_user:
        assert max(np.bincount(w.jobs.user[w.j2o >= 0]).max() for w in want) > 256, "no user has more than 256 kept jobs in one cycle"
    assert differs(want[1:], O.oracle(params, pool, cycles, with_carry=False)[1:]), "stale offers and usage place the same: re-seed the case"
    assert_quota_only_by_carry(pool, want)
    assert_matters(params, pool, cycles, want, offer_cols=("cpus", "mem"), state_cols=("usage_count", "usage_cpus", "usage_mem", "pool_usage"))
    return want


def check_base(make_engine, *, fractional=False, scale=1.0, algo=2, expect_form=0, seed=201):
    params = P1(match_algo=algo)
    pool, cycles = base_case(seed, fractional=fractional, scale=scale)
    want = base_oracle(params, pool, cycles, big_user=scale >= 1.0)
    return check(make_engine, params, pool, cycles, want, expect_form=expect_form)


# ---- 2b: the folds' chunk boundaries ----------------------------------------------------------------------------------------------------
SEG_OFFERS, SEG_USERS = (64, 65, 129, 768), (256, 257, 513)


SEG_EXTRA = 18  # jobs behind the 1026


def segment_pool(left=(700.0, 701.0, 702.0, 703.0), user_mem=0.3):
    """1026 jobs of 1 cpu and a non-dyadic mem (0.1 .. 0.9) that three users own 256, 257 and 513 of, and four hosts of 64, 65, 129 and
    768 cpus with mem that never limits: whatever order the matcher places in, K = 1026 fills every host exactly.  Behind them in rank
    order (the dru of a user's n-th 1-cpu job is n): eleven more jobs of the largest user — one of 1 cpu; per host, greatest `left`
    first, a pair of NO cpus whose mem is left[host] and the next double above it; two more of 1 cpu —, two jobs of 1000 cpus of each
    of the other two users (user 1's first asks for user_mem, its second for no mem: only the count can reject it), and three jobs of a fourth user whose share is tiny."""
    n = sum(SEG_USERS)
    user = np.array([u for i in range(SEG_USERS[2]) for u in range(3) if i < SEG_USERS[u]] + [2] * 11 + [0, 0, 1, 1] + [3] * 3, np.uint32)
    assert np.array_equal(np.bincount(user[:n]), SEG_USERS) and len(user) == n + SEG_EXTRA
    N = len(user)
    cpus, mem = np.ones(N), 0.1 * (1 + np.arange(N) % 9)
    cpus[n + 1:n + 9] = 0.0
    mem[n + 1:n + 9] = [x for v in np.argsort(left)[::-1] for x in (left[v], np.nextafter(left[v], np.inf))]
    cpus[n + 11:n + 15], mem[n + 13:n + 15] = 1000.0, (user_mem, 0.0)
    tasks = A.Tasks(cpus=cpus, mem=mem, user=user, priority=np.full(N, 50, np.int32), start_ms=np.zeros(N, np.int64),
                    task_id=(10_000 + np.arange(N)).astype(np.int64), job_id=(100 + np.arange(N)).astype(np.int64), pending=np.ones(N, np.uint8))
    users = A.Users(div_cpus=np.array([1.0, 1.0, 1.0, 1e-6]), div_mem=np.full(4, A.DMAX))
    oc = np.array(SEG_OFFERS, np.float64)
    offers = A.Offers(cpus=oc, mem=oc.copy(), host=np.arange(4, dtype=np.uint32), k8s=np.zeros(4, np.uint8), run_cpus=np.ones(4), run_mem=np.ones(4),
                      run_count=np.ones(4, np.int32))
    return SimpleNamespace(tasks=tasks, users=users, pending_jobs=A.Jobs(cpus=cpus.copy(), mem=mem.copy(), user=user.copy()), offers=offers, groups=None)


def segment_state(quota_mem_1=A.DMAX):
    """nobody is limited in the first cycle; behind its carry users 0 and 1 have room for ONE more job each, the largest user for nine,
    the pool for twelve; user 1's mem quota is quota_mem_1"""
    ucount = np.array([3.0, 5.0, 7.0, 2.0])
    qcount = np.full(4, 2.0 ** 31 - 1)
    qcount[:3] = ucount[:3] + np.array(SEG_USERS) + np.array([1.0, 1.0, 9.0])
    qmem = np.full(4, A.DMAX)
    qmem[1] = quota_mem_1
    pu = A.usage(17.0, 17.0 * 3.0 + 0.1, 17.0 * 0.7, 0.0)
    return A.UserState(quota_count=qcount, quota_cpus=np.full(4, A.DMAX), quota_mem=qmem, quota_gpus=np.full(4, A.DMAX),
                       usage_count=ucount, usage_cpus=ucount * 3.0 + 0.1, usage_mem=ucount * 0.7, usage_gpus=np.zeros(4),
                       pool_quota=A.quota(count=pu.count + sum(SEG_USERS) + 12.0), pool_usage=pu)


def oracle_stale_user(params, pool, cycles, col, u, put=lambda old, new: old):
    """the oracle's cycles with ONE user's entry of a usage column not carried (put: what it holds instead, from the stale and the
    carried value)"""
    real = O.carry_usage

    def patched(st, jobs, hit, spend):
        new = real(st, jobs, hit, spend)
        getattr(new, col)[u] = put(getattr(st, col)[u], getattr(new, col)[u])
        return new
    O.carry_usage = patched
    try:
        return O.oracle(params, pool, cycles)
    finally:
        O.carry_usage = real


def check_segment_lengths(make_engine):
    """ONE advance whose kept placements fill offers with exactly 64, 65 and 129 jobs (a wave's chunk, one more, two chunks and one) and
    belong to users with exactly 256, 257 and 513 of them (a workgroup's chunk, one more, two chunks and one); the pool's fold runs over
    all 1026.  The next cycle reads every one of those sums: no cpus are left anywhere; EVERY host's mem is left to the last bit (a job
    that asks for exactly the remainder fits there and nowhere else, one that asks for the next double fits nowhere); each of the three
    users' counts admits exactly the jobs it should (one more or one fewer kept job moves the line); user 1's carried mem admits a job
    at equality with its quota (the next double above the carried sum does not; a smaller sum is not seen: a user's filter rejects
    everything behind a rejected job, so one user cannot show both sides); the pool's count stops the last user."""
    params = P1()
    n = sum(SEG_USERS)
    eligible = np.ones(n + SEG_EXTRA, np.uint8)
    cycles = lambda state: [O.cycle(n, state=state, eligible=eligible), O.cycle(n, carry_offers=True, carry_usage=True)]
    # the carried sums, from the oracle (the jobs behind the 1026 are not seen by the first cycle, whatever they ask for)
    first = O.oracle(params, segment_pool(), cycles(segment_state()))[1]
    left, a1 = first.offers.mem, float(first.state.usage_mem[1])
    assert len(set(left.tolist())) == 4
    m1 = next(m for m in (0.3, 0.7, 1.1, 1.3, 1.7, 1.9, 2.3) if np.nextafter(a1, np.inf) + m > a1 + m)
    pool, cyc = segment_pool(left, m1), cycles(segment_state(quota_mem_1=a1 + m1))
    want = O.oracle(params, pool, cyc)
    w0, w1 = want
    assert len(w0.pos) == n and (w0.j2o >= 0).all(), "a placement of the first cycle is not kept"
    assert np.array_equal(np.sort(np.bincount(w0.j2o)), np.sort(SEG_OFFERS)) and {64, 65, 129} <= set(np.bincount(w0.j2o).tolist())
    assert {256, 257, 513} <= set(np.bincount(w0.jobs.user).tolist())
    assert int((np.diff(w0.jobs.user.astype(np.int64)) != 0).sum()) > 500, "the users' jobs are not interleaved in the queue"
    assert np.array_equal(w1.offers.cpus, np.zeros(4)) and np.array_equal(w1.offers.mem, left) and w1.state.usage_mem[1] == a1
    # the second cycle: the largest user's 1-cpu job and eight probes pass the filters, its last two do not; ONE job of each of the two
    # other users does; one job of the last user does.  Only the probes that ask for exactly what a host has left are placed, each there
    by_left = np.argsort(left)[::-1]
    assert np.array_equal(w1.jobs.user, [2] * 9 + [0, 1, 3]), w1.jobs.user
    assert np.array_equal(w1.j2o, [-1] + [x for v in by_left for x in (v, -1)] + [-1, -1, -1]), w1.j2o
    assert w1.jobs.mem[10] == m1
    assert_matters(params, pool, cyc, want, offer_cols=("cpus", "mem"), state_cols=("usage_count", "pool_usage"))
    for u in range(3):
        assert differs(want, oracle_stale_user(params, pool, cyc, "usage_count", u)), f"the carry of user {u}'s count changes no result"
    one_up = lambda old, new: np.nextafter(new, np.inf)
    assert differs(want, oracle_stale_user(params, pool, cyc, "usage_mem", 1, one_up)), "user 1's carried mem is not read to the last bit"
    return check(make_engine, params, pool, cyc, want)


# ---- 3: every column ------------------------------------------------------------------------------------------------------------------
def check_columns(make_engine, *, null_cols=False, seed=232, k=120, n_cycles=4, n_pending=500):
    params = P1()
    pool = columns_pool(seed - 2 * null_cols, null_cols=null_cols, n_pending=n_pending)
    cycles = [O.cycle(k)] + [O.cycle(k, carry_offers=True) for _ in range(n_cycles - 1)]
    want = O.oracle(params, pool, cycles)
    assert_every_cycle_mixed(want)
    if not null_cols:
        # a later cycle refuses a job for max-tasks-per-host, one for ports, one for a scalar, one for disk, each ONLY through the carry:
        # with that one column left stale (everything else carried) some cycle gives another result
        assert_matters(params, pool, cycles, want, offer_cols=("num_tasks", "ports", "scalars", "disk_space", "run_count"))
    else:
        assert_matters(params, pool, cycles, want, offer_cols=("num_tasks", "run_count"))
    return check(make_engine, params, pool, cycles, want)


# ---- 4: skipped offers, remove_mode 1 ---------------------------------------------------------------------------------------------------
def check_skipped(make_engine, *, scale=1.0, seed=240):
    params = P1()
    k, n_cycles = int(300 * scale), 5
    pool = base_pool(seed, n_pending=int(2600 * scale), n_running=int(100 * scale), k=k, n_cycles=n_cycles, fractional=True)
    state, eligible = base_state(pool, seed, fractional=True, pool_slack=0.95 * n_cycles * k)
    rng = np.random.default_rng(seed)
    cycles = carry_cycles(k, n_cycles, state, eligible)
    for c in range(1, n_cycles):
        cycles[c].offer_skipped = (rng.random(pool.offers.n) < 0.3).astype(np.uint8)
        cycles[c].remove_mode = 1 if c in (2, 4) else 0
    want = O.oracle(params, pool, cycles)
    assert_every_cycle_mixed(want)
    for c in range(1, n_cycles):  # a skipped offer held matches: they carry nothing and (mode 0) stay queued
        last = want[c - 1]
        dropped = (last.j2o >= 0) & ~O.kept(last.j2o, cycles[c].offer_skipped)
        assert dropped.any(), "offer_skipped drops no match: re-seed the case"
        if cycles[c].remove_mode == 0:
            assert np.isin(last.Q[last.pos[dropped]], want[c].Q).all()
        else:
            assert not np.isin(last.Q[last.pos], want[c].Q).any()
    plain = [copy.copy(cy) for cy in cycles]
    for cy in plain:
        cy.offer_skipped = None
    assert differs(want, O.oracle(params, pool, plain)), "the skipped offers change nothing: re-seed the case"
    return check(make_engine, params, pool, cycles, want)


# ---- 5: tokens ------------------------------------------------------------------------------------------------------------------------
def check_tokens(make_engine, *, scale=1.0, seed=250):
    params = P1()
    k, n_cycles = int(300 * scale), 5
    pool = base_pool(seed, n_pending=int(2600 * scale), n_running=int(100 * scale), k=k, n_cycles=n_cycles)
    rng = np.random.default_rng(seed)
    tokens = rng.integers(int(30 * scale), int(200 * scale), pool.users.n).astype(np.int64)
    tokens[pool.top_user] = 2 * k
    state, eligible = base_state(pool, seed, tokens=tokens, enforce=True, pool_usage_given=False, pool_slack=0.97 * n_cycles * k)
    cycles = carry_cycles(k, n_cycles, state, eligible)
    cycles[3].tokens_left = tokens.copy()  # (the host's refill: replaces the counts, nothing is spent on top)
    want = O.oracle(params, pool, cycles)
    assert_every_cycle_mixed(want)
    # a user runs out of tokens in a later cycle, and only because the kept placements were spent: the rate limit stops a user there
    # that the staged counts would let through
    ran_out = False
    for w in want[1:3]:
        rl = pyoracle.considerable(w.queue, w.state, k)[1]
        rl0 = pyoracle.considerable(w.queue, dataclasses.replace(w.state, tokens_left=tokens), k)[1]
        ran_out = ran_out or bool(((rl > 0) & (rl0 == 0)).any())
    assert ran_out, "no user runs out of tokens: re-seed the case"
    assert_matters(params, pool, cycles, want, state_cols=("tokens_left",))
    assert np.array_equal(want[3].state.tokens_left, tokens)
    assert not np.array_equal(want[4].state.tokens_left, tokens)  # spent again afterwards
    got = check(make_engine, params, pool, cycles, want)
    # tokens alone: neither flag set, the refill still lands
    only = [O.cycle(k, state=state, eligible=eligible), O.cycle(k, tokens_left=np.zeros(pool.users.n, np.int64))]
    w2 = O.oracle(params, pool, only)
    assert len(w2[1].pos) < len(w2[0].pos)
    check(make_engine, params, pool, only, w2)
    return got


# ---- 6: split equivalence -------------------------------------------------------------------------------------------------------------
def split_case(seed=260, n_pending=500, n_offers=30, k1=150):
    pool = synth.make_pool(seed=seed, n_pending=n_pending, n_running=80, n_users=10, n_offers=n_offers)
    o = pool.offers
    pool.offers = A.Offers(cpus=o.cpus, mem=o.mem, host=o.host, k8s=o.k8s, run_cpus=o.run_cpus, run_mem=o.run_mem, run_count=o.run_count)
    return pool, [O.cycle(k1), O.cycle(n_pending, carry_offers=True)]


def placements(pool, results):
    """{task index: host} over the cycles' kept matches"""
    out = {}
    for r, offers in results:
        for t, o in zip(r.Q[r.pos], r.j2o):
            if o >= 0:
                assert int(t) not in out
                out[int(t)] = int(offers.host[o])
    return out


def check_split(make_engine, **kw):
    """K1 jobs in a rank cycle, then ONE carry queue cycle over the rest, place every job where a single match of all the jobs in
    rank order places it: integer resources make the carried remainder equal the match's own "lease minus assigned" bit for bit, and
    a job the first part could not place finds no room later either.  No carry code on the expected side."""
    params = P1()
    pool, cycles = split_case(**kw)
    Q, _ = pyoracle.rank(params, pool.tasks, pool.users)
    jq = (np.cumsum(pool.tasks.pending) - 1)[Q]
    j2o, _, _ = pyoracle.match(params, pool.pending_jobs.take(jq), pool.offers, None)
    single = {int(t): int(pool.offers.host[o]) for t, o in zip(Q, j2o) if o >= 0}
    assert 0 < len(single) < len(Q) and (j2o[:cycles[0].k] >= 0).any() and (j2o[cycles[0].k:] >= 0).any()
    want = O.oracle(params, pool, cycles)  # first on the CPU: the oracle's composition has the property itself
    assert placements(pool, [(w, pool.offers) for w in want]) == single
    got = run_engine(make_engine, params, pool, cycles)
    assert placements(pool, [(g, pool.offers) for g in got]) == single
    S.compare(got, want, cycles)


# ---- 7: forms -------------------------------------------------------------------------------------------------------------------------
def check_classfit(make_engine, *, scale=1.0):
    """six engines on the device: the engine's own choice (match_algo 0) is the class-ordered walk"""
    idle = [make_engine(A.default_params()) for _ in range(5)]
    try:
        return check_base(make_engine, scale=scale, algo=0, expect_form=3)
    finally:
        for e in idle:
            e.close()


def check_multi(make_engine, *, scale=1.0):
    """three ragged pools through cook_cycle_run_queue_carry_multi; pool 1 runs with carry = NULL throughout; in cycle 2 pool 2's step
    is refused: it stays untouched (the same step without the offending part runs next), the others go on"""
    params = P1(match_algo=2)
    shapes = [(1.0, 201, 5), (0.5, 202, 5), (0.7, 203, 4)]
    cases = [base_case(seed, scale=s * scale, n_cycles=n) for s, seed, n in shapes]
    for cy in cases[1][1][1:]:
        cy.carry = False
    want = [O.oracle(params, pl, cs) for pl, cs in cases]
    for w in want:
        assert_every_cycle_mixed(w)
    engines = [make_engine(params) for _ in cases]
    got = [[] for _ in cases]
    try:
        for e, (pl, cs) in zip(engines, cases):
            e.cycle_stage(pl.tasks, pl.users, pl.pending_jobs, pl.offers, pl.groups)
            e.cycle_set_considerable(cs[0].state, cs[0].eligible)
        cycle_run_rank_multi(engines, [cs[0].k for _, cs in cases])
        cycle_match_multi(engines)
        for i, e in enumerate(engines):
            got[i].append(S.fetch(e, False))
        nxt = [1, 1, 1]  # the next cycle of each pool
        for rnd in range(1, 5):
            steps = [step_kw(cs[nxt[i]]) for i, (_, cs) in enumerate(cases)]
            carries = [carry_of(cs[nxt[i]]) for i, (_, cs) in enumerate(cases)]
            live = [0, 1, 2]
            if rnd == 2:  # offers = 1 together with step->offers: refused for pool 2 alone
                steps[2] = dict(steps[2], offers=cases[2][0].offers)
                with pytest.raises(CookError) as ex:
                    cycle_run_queue_carry_multi(engines, [cs[nxt[i]].k for i, (_, cs) in enumerate(cases)], steps, carries)
                assert ex.value.code == COOK_E_INVALID
                live = [0, 1]
            else:
                live = [i for i in live if nxt[i] < len(cases[i][1])]
                if len(live) < 3:
                    break
                cycle_run_queue_carry_multi(engines, [cs[nxt[i]].k for i, (_, cs) in enumerate(cases)], steps, carries)
            cycle_match_multi([engines[i] for i in live])
            for i in live:
                got[i].append(S.fetch(engines[i], False))
                nxt[i] += 1
    finally:
        for e in engines:
            e.close()
    for i, (pl, cs) in enumerate(cases):
        assert len(got[i]) >= 3
        S.compare(got[i], want[i][:len(got[i])], cs, f"pool {i}")
    return got


# ---- 8: built offers in place ---------------------------------------------------------------------------------------------------------
def check_built_offers(make_engine, n_nodes=60, n_pods=300, n_jobs=400, k=150):
    from oracle import k8s_offers
    params = P1()
    nodes, pods, op = synth.make_cluster_state(seed=31, n_nodes=n_nodes, n_pods=n_pods, n_attr_keys=0, fractional=True, max_pods=14)
    pool = synth.make_pool(seed=32, n_pending=n_jobs, n_running=n_jobs // 4, n_users=10, n_offers=10, gpus=True, fractional=True)
    rows = k8s_offers.build_rows(nodes, pods, op)["rows"]
    M = len(rows["cpus"])
    pool.offers = A.Offers(cpus=rows["cpus"], mem=rows["mem"], host=rows["host"], k8s=np.ones(M, np.uint8), gpu_model=rows["gpu_model"],
                           gpu_count=rows["gpu_count"], disk_type=rows["disk_type"], disk_space=rows["disk_space"],
                           max_tasks=np.full(M, op.max_pods_per_node, np.int32), num_tasks=rows["num_pods"])
    cycles = [O.cycle(k), O.cycle(k, carry_offers=True), O.cycle(k, carry_offers=True)]
    want = O.oracle(params, pool, cycles)
    assert_every_cycle_mixed(want)
    assert_matters(params, pool, cycles, want, offer_cols=("cpus", "num_tasks"))
    before = []

    def stage(e):
        e.offers_stage(nodes, pods, op)
        e.offers_run()
        before.append(e.offers_fetch())
        e.cycle_stage_built_offers(pool.tasks, pool.users, pool.pending_jobs, None, with_task_limits=True)
    got = []
    with make_engine(params) as e:
        stage(e)
        e.cycle_run(k)
        got.append(S.fetch(e, False))
        for cy in cycles[1:]:
            run_step(e, cy)
            got.append(S.fetch(e, False))
        after = e.offers_fetch()
    S.compare(got, want, cycles)
    _same(dataclasses.asdict(after), dataclasses.asdict(before[0]))


# ---- 9: refusals and persistence ------------------------------------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(CookError) as ex:
        fn()
    return ex.value.code


def check_refusals(make_engine, *, scale=0.5):
    params = P1()
    pool, cycles = base_case(205, scale=scale, n_cycles=4)
    k, state, eligible = cycles[0].k, cycles[0].state, cycles[0].eligible
    U = pool.users.n
    want = O.oracle(params, pool, cycles)
    both = A.QueueCarry(offers=True, usage=True)
    with make_engine(params) as e:
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        e.cycle_run(k)  # no user state staged
        assert _code(lambda: e.cycle_run_queue_carry(k, A.QueueCarry(usage=True))) == COOK_E_STATE
        assert _code(lambda: e.cycle_run_queue_carry(k, A.QueueCarry(tokens_left=np.ones(U, np.int64)))) == COOK_E_STATE
        e.cycle_set_considerable(state, eligible)  # (no limiter in it)
        e.cycle_run(k)
        got = [S.fetch(e, False)]
        assert _code(lambda: e.cycle_run_queue_carry(k, both, offers=pool.offers)) == COOK_E_INVALID
        assert _code(lambda: e.cycle_run_queue_carry(k, A.QueueCarry(offers=2))) == COOK_E_INVALID
        assert _code(lambda: e.cycle_run_queue_carry(k, A.QueueCarry(usage=3))) == COOK_E_INVALID
        assert _code(lambda: e.cycle_run_queue_carry(k, A.QueueCarry(offers=True, usage=True, tokens_left=np.ones(U, np.int64)))) == COOK_E_INVALID
        assert _code(lambda: e.cycle_run_queue_carry(k, both, remove_mode=2)) == COOK_E_INVALID
        _same(vars(S.fetch(e, False)), vars(got[0]))
        # the same steps without the offending part: the queue, the offers and the user state are as they were
        for cy in cycles[1:3]:
            run_step(e, cy)
            got.append(S.fetch(e, False))
        S.compare(got, want[:3], cycles[:3], "after the refusals:")
        # a rank sees the carried offers and usage: the same cycle as a fresh engine staged with the oracle's carried values
        e.cycle_run(k)
        again = S.fetch(e, False)
    last = want[2]  # its offers and state carry the placements of cycles 0 and 1; cycle 2's own are not in (a rank does not carry)
    Q0 = want[0].Q
    jq, queue = S._queue_of(pool, Q0, eligible)
    pos = pyoracle.considerable(queue, last.state, k)[0]
    j2o, _, head = pyoracle.match(params, pool.pending_jobs.take(jq[pos]), last.offers, None)
    assert np.array_equal(again.Q, Q0) and np.array_equal(again.pos, pos) and np.array_equal(again.j2o, j2o) and again.head == head
    assert not np.array_equal(j2o, want[0].j2o)  # (and not what the staged offers give)
    # carry = NULL (and a carry of nothing) is cook_cycle_run_queue, byte for byte
    outs = []
    for mode in ("queue", "null", "nothing"):
        with make_engine(params) as e:
            e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
            e.cycle_set_considerable(state, eligible)
            e.cycle_run(k)
            for _ in range(2):
                if mode == "queue":
                    e.cycle_run_queue(k)
                else:
                    e.cycle_run_queue_carry(k, None if mode == "null" else A.QueueCarry())
            outs.append((vars(S.fetch(e, False)), e.match_metrics(n_users=U), e.match_explain(np.arange(30))))
    _same(outs[1], outs[0])
    _same(outs[2], outs[0])


# ---- 10: ABI ----------------------------------------------------------------------------------------------------------------------------
def struct_size_sources():
    return ('#include <stdio.h>\n#include "cookmatch.h"\nint main(){printf("%zu %d\\n", sizeof(cook_queue_carry), COOK_ABI_VERSION);return 0;}',
            [C.sizeof(A.CookQueueCarry), 4])
