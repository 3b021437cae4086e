"""The cases of the launch-rate limiters kept on the device (cook_cycle_set_limiters, cook_cycle_set_clock, cook_cycle_limiters_spend,
cook_cycle_fetch_limiters), shared by the emulator (test_limiter_emu.py) and GPU (test_limiter_gpu.py) suites.  Expected
values come from tests/limiter_oracle.py alone.  Per cycle, element for element: the queue, rank_pos, job_to_offer, head_matched, the
rate-limit stage's rate_limited / passed, the limiter state behind the cycle (tokens, last_update_ms, time_until_ms) and the info counters.
What a case is there to show is asserted on the oracle before the engine is called."""
from __future__ import annotations

import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

from cook_amd import _abi as A
from cook_amd import synth
from cook_amd.engine import CookError, cycle_match_multi, cycle_run_queue_reserve_multi, cycle_run_rank_multi
from tests import limiter_oracle as O
from tests import queue_cases as S

COOK_E_INVALID, COOK_E_STATE = -1, -4
P1 = lambda **kw: A.default_params(good_enough_fitness=1.0, **kw)
CASES = [(1, 64), (63, 1), (64, 65), (65, 64), (257, 65)]  # (users, K)


# ---- pools, states, limiters ---------------------------------------------------------------------------------------------------------
def make_pool(seed, U, *, n_pending=420, n_offers=12):
    """synth's jobs and users; a dozen hosts whose cpus hold a part of what a cycle considers, so every cycle keeps some matches and
    leaves some considered jobs unmatched"""
    pool = synth.make_pool(seed=seed, n_pending=n_pending, n_running=30, n_users=U, n_offers=n_offers)
    rng = np.random.default_rng(seed + 5)
    cpus = rng.integers(25, 60, n_offers).astype(np.float64)
    J, T = pool.pending_jobs, pool.tasks
    huge = rng.random(J.n) < 0.04  # (a job no host has the memory for: considered, never matched, stays in the queue)
    J.mem[huge] = 1e9
    T.mem[np.flatnonzero(T.pending)[huge]] = 1e9
    pool.offers = A.Offers(cpus=cpus, mem=cpus * 70000.0, host=np.arange(n_offers, dtype=np.uint32), k8s=np.zeros(n_offers, np.uint8))
    pool.groups = None
    return pool


def open_state(U, *, tokens=None, enforce=True, blocked=()):
    """nobody is limited by a quota, except the users in `blocked`, whose count quota is used up: none of their jobs reaches the
    rate-limit stage"""
    qcount = np.full(U, 2.0 ** 31 - 1)
    qcount[list(blocked)] = 0.0
    return A.UserState(quota_count=qcount, quota_cpus=np.full(U, A.DMAX), quota_mem=np.full(U, A.DMAX), quota_gpus=np.full(U, A.DMAX),
                       usage_count=np.zeros(U), usage_cpus=np.zeros(U), usage_mem=np.zeros(U), usage_gpus=np.zeros(U), tokens_left=tokens,
                       enforce_rate_limit=enforce)


def random_limiters(seed, U, *, now0=1000):
    """rates from a token in ten seconds to ten a second, small buckets, some users in debt, last updates around the first clock"""
    rng = np.random.default_rng(seed + 9)
    per_minute = rng.choice([6.0, 7.3, 30.0, 60.0, 133.0, 600.0], size=U)
    bucket = rng.integers(0, 12, U)
    tokens = np.minimum(rng.integers(-6, 12, U), bucket)
    last = now0 - rng.integers(0, 900, U)
    if U == 1:  # (the one user is neither always nor never limited)
        per_minute[0], bucket[0], tokens[0] = 133.0, 5, 3
    return A.Limiters(per_minute, bucket, tokens, last)


def seeded_cycles(seed, U, k, *, n_cycles=5, carry=True, dt=(700, 1900), lim=None, state=None):
    rng = np.random.default_rng(seed + 13)
    now, cycles = 1000, []
    for c in range(n_cycles):
        cycles.append(O.cycle(k, state=(state if state is not None else open_state(U)) if c == 0 else None,
                              eligible=None, now=now, spend_ms=now - 40 if c else now, carry=carry and c > 0, carry_offers=carry, carry_usage=carry,
                              set_limiters=(lim if lim is not None else random_limiters(seed, U)) if c == 0 else None))
        now += int(rng.integers(*dt))
    return cycles


# ---- engine side -------------------------------------------------------------------------------------------------------------------
def run_cycle(e, cy, c, U, *, defer=False):
    """everything of one cycle up to and including its run"""
    if cy.explicit_spend is not None:
        e.cycle_limiters_spend(cy.explicit_spend[0], cy.explicit_spend[1])
    if getattr(cy, "before", None):
        cy.before(e)
    if cy.set_limiters is False:
        e.cycle_set_limiters(None)
    if cy.state is not None:
        e.cycle_set_considerable(cy.state, cy.eligible)
    if cy.set_limiters not in (None, False):
        e.cycle_set_limiters(cy.set_limiters)
    if cy.now is not None:
        e.cycle_set_clock(cy.now, cy.spend_ms)
    if defer:
        return
    if c == 0 or cy.rank:
        e.cycle_run(cy.k)
    elif cy.carry:
        e.cycle_run_queue_carry(cy.k, A.QueueCarry(offers=cy.carry_offers, usage=cy.carry_usage, tokens_left=cy.tokens_left),
                                offer_skipped=cy.offer_skipped, remove_mode=cy.remove_mode, offers=cy.offers)
    else:
        e.cycle_run_queue(cy.k, offer_skipped=cy.offer_skipped, remove_mode=cy.remove_mode, offers=cy.offers)


def fetch(e, U, *, filters=True, limiters=True):
    g = S.fetch(e, False)
    g.rate_limited, g.passed = e.fetch_rate_limit(U) if filters else (None, None)
    g.tokens, g.last, g.until = e.fetch_limiters(U) if limiters else (None, None, None)
    g.info = e.limiter_info()
    return g


def run_engine(make_engine, params, pool, cycles, U, *, expect_form=None):
    got = []
    with make_engine(params) as e:
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        held = False
        for c, cy in enumerate(cycles):
            run_cycle(e, cy, c, U)
            held = (held or cy.set_limiters not in (None, False)) and cy.set_limiters is not False
            got.append(fetch(e, U, limiters=held))
            if expect_form is not None and len(got[-1].j2o):
                ms = e.match_stats()
                assert ms["placement_form"] == expect_form, (c, ms["placement_form"], hex(ms["classfit_refused"]))
    return got


def compare(got, want, tag=""):
    for c, (g, w) in enumerate(zip(got, want)):
        where = f"{tag} cycle {c}"
        assert np.array_equal(g.Q, w.Q), (where, "queue", len(g.Q), len(w.Q))
        if g.rate_limited is not None:
            assert np.array_equal(g.rate_limited, w.rate_limited), (where, "rate_limited", g.rate_limited, w.rate_limited)
            assert np.array_equal(g.passed, w.passed), (where, "passed", g.passed, w.passed)
        assert np.array_equal(g.pos, w.pos), (where, "rank_pos", len(g.pos), len(w.pos))
        assert np.array_equal(g.j2o, w.j2o), (where, "job_to_offer", int((g.j2o != w.j2o).sum()) if len(g.j2o) == len(w.j2o) else (len(g.j2o), len(w.j2o)))
        assert g.head == w.head, (where, "head_matched")
        if w.tokens is not None:
            assert np.array_equal(g.tokens, w.tokens), (where, "tokens", np.flatnonzero(g.tokens != w.tokens)[:8], g.tokens[:8], w.tokens[:8])
            assert np.array_equal(g.last, w.last), (where, "last_update_ms", np.flatnonzero(g.last != w.last)[:8])
            assert np.array_equal(g.until, w.until), (where, "time_until_ms", np.flatnonzero(g.until != w.until)[:8])
            assert g.info == w.info, (where, "info", g.info, w.info)


def check(make_engine, params, pool, cycles, U, **kw):
    want = O.oracle(params, pool, cycles)
    got = run_engine(make_engine, params, pool, cycles, U, **kw)
    compare(got, want)
    return got, want


def assert_exercised(want, *, limited=True):
    """on the oracle alone: the queue cycles keep matches (so tokens are spent), and the limiters decide something"""
    assert sum(1 for w in want if (w.j2o >= 0).any()) >= 3, "fewer than three cycles keep a match: re-seed the case"
    assert sum(w.info["spent"] for w in want) > 0, "nothing is ever spent: re-seed the case"
    if limited:
        assert sum(int(w.rate_limited.sum()) for w in want) > 0 and sum(int(w.passed.sum()) for w in want) > 0, "the limiters decide nothing: re-seed the case"


# ---- by hand ---------------------------------------------------------------------------------------------------------------------------
def hand_pool(n0=6, n2=6):
    """user 0 has n0 jobs, user 1 none, user 2 n2; every job is 1 cpu; one host with room for all"""
    user = np.array([0] * n0 + [2] * n2, np.uint32)
    N = len(user)
    cpus, mem = np.ones(N), np.full(N, 100.0)
    tasks = A.Tasks(cpus=cpus, mem=mem, user=user, priority=np.full(N, 50, np.int32), start_ms=np.zeros(N, np.int64),
                    task_id=(10_000 + np.arange(N)).astype(np.int64), job_id=(100 + np.arange(N)).astype(np.int64), pending=np.ones(N, np.uint8))
    users = A.Users(div_cpus=np.ones(3), div_mem=np.full(3, A.DMAX))
    offers = A.Offers(cpus=np.array([100.0]), mem=np.array([1e6]), host=np.zeros(1, np.uint32), k8s=np.zeros(1, np.uint8))
    return SimpleNamespace(tasks=tasks, users=users, pending_jobs=A.Jobs(cpus=cpus.copy(), mem=mem.copy(), user=user.copy()), offers=offers, groups=None)


def check_by_hand(make_engine):
    """a token a second.  User 0 starts 2 in debt: all its jobs are limited in the cycles at 1 s and 2 s, at 3 s it holds one token and
    ONE job passes, launches and spends it, and the second it took to come round earns the next; user 1 is idle: its bucket is never touched; user 2 is never limited"""
    pool = hand_pool()
    lim = A.Limiters([60.0, 60.0, 60.0], [5, 5, 1000], [-2, 3, 1000], [0, 0, 0])
    cycles = [O.cycle(64, state=open_state(3) if c == 0 else None, now=1000 * (c + 1), set_limiters=lim if c == 0 else None) for c in range(5)]
    want = O.oracle(P1(), pool, cycles)
    assert [int(w.rate_limited[0]) for w in want] == [6, 6, 5, 4, 3] and [int(w.passed[0]) for w in want] == [0, 0, 1, 1, 1]
    assert [int(w.tokens[0]) for w in want] == [-1, 0, 1, 1, 1] and [int(w.until[0]) for w in want] == [1000, 0, 0, 0, 0]
    assert all(int(w.tokens[1]) == 3 and int(w.last[1]) == 0 for w in want) and all(int(w.rate_limited[2]) == 0 for w in want)
    assert [w.info["in_debt"] for w in want] == [1, 0, 0, 0, 0] and [w.info["spent"] for w in want] == [0, 6, 0, 1, 1]
    compare(run_engine(make_engine, P1(), pool, cycles, 3), want)


# ---- seeded: every size; the same run driven the parent's way --------------------------------------------------------------------------
def check_seeded(make_engine, U, k, seed=301):
    pool = make_pool(seed + U, U)
    cycles = seeded_cycles(seed, U, k)
    got, want = check(make_engine, P1(), pool, cycles, U)
    assert_exercised(want, limited=U > 1 or k > 1)
    return pool, cycles, got, want


def check_differential(make_engine, U, k, seed=301):
    """the same seeded run with the host doing the clock: it computes the tokens with the oracle and passes tokens_left every cycle,
    spending nothing on the device.  Identical placements and identical rate_limited / passed in every cycle"""
    pool, cycles, got, want = check_seeded(make_engine, U, k, seed)
    theirs = []
    with make_engine(P1()) as e:
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        for c, (cy, w) in enumerate(zip(cycles, want)):
            if c == 0:
                e.cycle_set_considerable(dataclasses.replace(cy.state, tokens_left=w.view), None)
                e.cycle_run(cy.k)
            else:
                e.cycle_run_queue_carry(cy.k, A.QueueCarry(offers=True, usage=True, tokens_left=w.view))
            theirs.append(fetch(e, U, limiters=False))
    for c, (a, b) in enumerate(zip(theirs, got)):
        for f in ("Q", "pos", "j2o", "rate_limited", "passed"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), (c, f)
        assert a.head == b.head, c


# ---- the earn set ----------------------------------------------------------------------------------------------------------------------
def check_earn_set(make_engine, U=65, k=64, seed=311):
    """a user whose count quota is used up has no job at the rate-limit stage for three cycles: its bucket does not move.  Then its quota
    opens and the catch-up is ONE earn from where it stood — three intermediate earns would have dropped fractions"""
    pool = make_pool(seed, U)
    x = int(np.bincount(pool.pending_jobs.user, minlength=U).argmax())
    lim = random_limiters(seed, U)
    lim.per_minute[x], lim.bucket[x], lim.tokens[x], lim.last_update_ms[x] = 600.0, 50, -3, 0
    nows = [199, 250, 280, 300, 900]
    cycles = [O.cycle(k, state=open_state(U, blocked=[x]) if c == 0 else (open_state(U) if c == 3 else None), now=t, carry=c > 0, carry_offers=True,
                      carry_usage=c not in (0, 3), set_limiters=lim if c == 0 else None) for c, t in enumerate(nows)]
    want = O.oracle(P1(), pool, cycles)
    for w in want[:3]:
        assert w.rate_limited[x] + w.passed[x] == 0 and w.tokens[x] == -3 and w.last[x] == 0
    assert want[3].rate_limited[x] + want[3].passed[x] > 0 and want[3].last[x] == 300
    b0 = O.Bucket(O.rate_of(600.0), 50, 0, -3)
    step = b0
    for t in nows[:4]:
        step = O.earn(step, t)
    assert O.earn(b0, 300).tokens == 0 and step.tokens == -1 and want[3].view[x] == 0, "the intermediate earns would not show"
    compare(run_engine(make_engine, P1(), pool, cycles, U), want)


def check_fraction_rule():
    """the issue's example on the oracle alone: at 0.01 tokens per ms, earn(199); earn(300) gives 2, earn(300) alone 3"""
    b = O.Bucket(0.01, 100, 0, 0)
    assert O.earn(O.earn(b, 199), 300).tokens == 2 and O.earn(b, 300).tokens == 3
    assert O.earn(b, 99) is b and O.earn(b, 99).last == 0  # less than a token: nothing changes, last stays


# ---- the clock -------------------------------------------------------------------------------------------------------------------------
def check_clock(make_engine, how, U=64, k=65, seed=321):
    pool = make_pool(seed, U)
    lim = random_limiters(seed, U)
    if how == "none":  # nobody earns; the spends still subtract
        cycles = seeded_cycles(seed, U, k, lim=lim)
        for cy in cycles:
            cy.now = None
    elif how == "backwards":  # the clock is behind every last update: max(t, last) == last, nobody earns
        lim.last_update_ms[:] = 50_000 + np.arange(U)
        cycles = seeded_cycles(seed, U, k, lim=lim)
    else:  # a token in ten seconds: d == 0 at 3, 6 and 9 s, 1 at 10 s — last moves only then
        lim.per_minute[:], lim.last_update_ms[:] = 6.0, 0
        cycles = seeded_cycles(seed, U, k, n_cycles=6, lim=lim)
        for cy, t in zip(cycles, [3000, 6000, 9000, 10000, 12000, 20000]):
            cy.now, cy.spend_ms = t, 0  # (spends at a time that earns nothing)
    want = O.oracle(P1(), pool, cycles)
    if how in ("none", "backwards"):
        assert all(w.info["earned"] == 0 for w in want) and all(np.array_equal(w.last, lim.last_update_ms) for w in want)
        assert sum(w.info["spent"] for w in want) > 0
    else:
        assert all((w.last == 0).all() for w in want[:3]) and (want[3].last == 10000).any() and want[3].info["earned"] > 0
        assert not (want[4].last == 12000).any() and (want[5].last == 20000).any()
    compare(run_engine(make_engine, P1(), pool, cycles, U), want)


# ---- the spend -------------------------------------------------------------------------------------------------------------------------
def check_spend(make_engine, U=63, k=65, seed=331):
    """in the advance without a carry (cycle 1), with one and with offer_skipped, where a dropped match spends nothing (2); an explicit
    spend and then an advance spend once (3); a rank cycle does not spend what the cycle in front of it placed (4); the queue cycle
    behind it spends the rank cycle's (5)"""
    pool = make_pool(seed, U)
    lim = random_limiters(seed, U)
    lim.tokens[:] = np.maximum(lim.tokens, 2)  # (everybody launches something)
    lim.bucket[:] = np.maximum(lim.bucket, lim.tokens)
    M = pool.offers.n
    skip = (np.arange(M) % 3 == 0).astype(np.uint8)
    skip3 = (np.arange(M) % 4 == 1).astype(np.uint8)
    cycles = seeded_cycles(seed, U, k, n_cycles=6, lim=lim)
    cycles[1].carry = False
    cycles[2].offer_skipped = skip
    cycles[3].explicit_spend, cycles[3].offer_skipped = (cycles[3].spend_ms - 100, skip3), skip3
    cycles[4].rank, cycles[4].carry = True, False
    want = O.oracle(P1(), pool, cycles)
    kept2 = int(((want[1].j2o >= 0) & (skip[np.maximum(want[1].j2o, 0)] == 0)).sum())
    assert 0 < kept2 < int((want[1].j2o >= 0).sum()) and want[2].info["spent"] == kept2, "offer_skipped drops no match of cycle 1"
    assert want[1].info["spent"] == int((want[0].j2o >= 0).sum()) > 0 and want[3].info["spent"] > 0
    assert want[4].info["spent"] == 0 and (want[3].j2o >= 0).any() and want[5].info["spent"] == int((want[4].j2o >= 0).sum()) > 0
    compare(run_engine(make_engine, P1(), pool, cycles, U), want)


# ---- listed replace, persistence, drop ---------------------------------------------------------------------------------------------------
def check_listed(make_engine, n_listed, U=257, k=64, seed=341):
    """the host's flush! of n_listed users in front of cycle 2: tokens = bucket, last = now; nobody else's state moves"""
    pool = make_pool(seed, U, n_pending=560)
    cycles = seeded_cycles(seed, U, k)
    rng = np.random.default_rng(seed + n_listed)
    who = rng.choice(U, size=n_listed, replace=False).astype(np.uint32)  # (in no order)
    top = int(np.bincount(pool.pending_jobs.user, minlength=U).argmax())
    if top not in who:
        who[0] = top  # (somebody whose jobs are at the stage)
    bucket = rng.integers(3, 30, len(who))
    cycles[2].set_limiters = A.Limiters(rng.choice([45.0, 600.0], size=len(who)), bucket, bucket, np.full(len(who), cycles[2].now), user=who)
    got, want = check(make_engine, P1(), pool, cycles, U)
    assert_exercised(want)
    others = np.setdiff1d(np.arange(U), who)
    spenders = want[1].jobs.user[want[1].j2o >= 0]
    idle = np.setdiff1d(others[(want[2].rate_limited + want[2].passed)[others] == 0], spenders)
    assert len(idle) and np.array_equal(want[2].last[idle], want[1].last[idle]) and np.array_equal(want[2].tokens[idle], want[1].tokens[idle])
    quiet = ~np.isin(who, spenders)  # (a listed user with kept placements in cycle 1 spends them from the flushed state)
    assert quiet.any() and np.array_equal(want[2].view[who[quiet]], bucket[quiet])  # tokens = bucket, last = now: what the filter saw


def check_persistence(make_engine, U=65, k=64, seed=351):
    """the limiters survive a cook_cycle_update and the rank behind it: the last queue cycle's placements spend explicitly, the update
    drops the standing queue, the rank cycle reads the same buckets"""
    pool = make_pool(seed, U)
    cycles = seeded_cycles(seed, U, k, n_cycles=5)
    cycles[3].rank, cycles[3].carry = True, False
    cycles[3].explicit_spend = (cycles[3].spend_ms, None)
    cycles[3].before = lambda e: e.cycle_update()
    want = O.oracle(P1(), pool, cycles)
    assert_exercised(want)
    assert want[3].info["spent"] > 0 and want[3].info["earned"] > 0 and want[4].info["spent"] > 0
    compare(run_engine(make_engine, P1(), pool, cycles, U), want)


def check_drop(make_engine, U=64, k=65, seed=361):
    """cook_cycle_set_limiters(NULL) in front of cycle 3 brings the staged tokens_left back as it was staged (the limiters' spends never
    touched it); a cook_cycle_stage drops the limiters too"""
    pool = make_pool(seed, U)
    rng = np.random.default_rng(seed)
    staged = rng.integers(0, 4, U).astype(np.int64)
    cycles = seeded_cycles(seed, U, k, state=open_state(U, tokens=staged))
    cycles[3].set_limiters = False
    want = O.oracle(P1(), pool, cycles)
    assert_exercised(want[:3])
    assert want[3].tokens is None and want[3].rate_limited.sum() > 0 and not np.array_equal(want[3].rate_limited, want[2].rate_limited)
    got = run_engine(make_engine, P1(), pool, cycles, U)
    compare(got, want)
    with make_engine(P1()) as e:
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        e.cycle_set_limiters(random_limiters(seed, U))
        assert code(lambda: e.cycle_set_considerable(open_state(U, tokens=staged))) == COOK_E_INVALID
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        assert code(lambda: e.fetch_limiters(U)) == COOK_E_STATE and e.limiter_info()["spent"] == 0
        e.cycle_set_considerable(open_state(U, tokens=staged))  # (accepted again)
        e.cycle_run(k)
        assert np.array_equal(e.fetch_rate_limit(U)[0], O.oracle(P1(), pool, [O.cycle(k, state=open_state(U, tokens=staged))])[0].rate_limited)


def check_late_install(make_engine, U=65, k=64, seed=366):
    """two cycles on the staged tokens_left, then the first cook_cycle_set_limiters in front of cycle 2: its counts are current, the
    placements of cycle 1 do not spend again; from cycle 3 on the advance spends"""
    pool = make_pool(seed, U)
    staged = np.random.default_rng(seed).integers(1, 6, U).astype(np.int64)
    lim = random_limiters(seed, U)
    cycles = seeded_cycles(seed, U, k, state=open_state(U, tokens=staged))
    cycles[0].set_limiters, cycles[2].set_limiters = None, lim
    want = O.oracle(P1(), pool, cycles)
    assert want[1].tokens is None and (want[1].j2o >= 0).any() and want[2].info["spent"] == 0 and want[3].info["spent"] > 0
    compare(run_engine(make_engine, P1(), pool, cycles, U), want)


# ---- pool forms, placement forms, edges ------------------------------------------------------------------------------------------------------
def check_multi(make_engine, seed=371):
    """cook_cycle_run_rank_multi, then cook_cycle_run_queue_reserve_multi steps, over three pools of which the middle one has no limiters
    (its staged tokens_left counts)"""
    Us, k = (63, 65, 257), 64
    pools = [make_pool(seed + i, U, n_pending=300 + 60 * i) for i, U in enumerate(Us)]
    rng = np.random.default_rng(seed)
    staged = rng.integers(0, 5, Us[1]).astype(np.int64)
    cyc = [seeded_cycles(seed + i, U, k, n_cycles=4, state=open_state(U, tokens=staged if i == 1 else None)) for i, U in enumerate(Us)]
    for cy in cyc[1]:
        cy.set_limiters, cy.now = None, None
    want = [O.oracle(P1(), p, cs) for p, cs in zip(pools, cyc)]
    assert_exercised(want[0]), assert_exercised(want[2])
    assert sum(int(w.rate_limited.sum()) for w in want[1]) > 0
    engines = [make_engine(P1()) for _ in pools]
    got = [[] for _ in pools]
    try:
        for e, p in zip(engines, pools):
            e.cycle_stage(p.tasks, p.users, p.pending_jobs, p.offers, p.groups)
        for c in range(4):
            for e, cs, U in zip(engines, cyc, Us):
                run_cycle(e, cs[c], c, U, defer=True)
            if c == 0:
                cycle_run_rank_multi(engines, k)
            else:
                cycle_run_queue_reserve_multi(engines, k, carries=[A.QueueCarry(offers=True, usage=True) for _ in engines])
            cycle_match_multi(engines)
            for i, (e, U) in enumerate(zip(engines, Us)):
                got[i].append(fetch(e, U, limiters=i != 1))
    finally:
        for e in engines:
            e.close()
    for i in range(3):
        compare(got[i], want[i], tag=f"pool {i}")


def check_forms(make_engine, algo, form, U=65, k=64, seed=381):
    """the limiters only move the filter: the same cycles under another placement form give the oracle's results"""
    pool = make_pool(seed, U)
    cycles = seeded_cycles(seed, U, k)
    got, want = check(make_engine, P1(match_algo=algo), pool, cycles, U, expect_form=form)
    assert_exercised(want)


def check_edges(make_engine, U=64, k=65, seed=391):
    """a rate whose product with the elapsed time is above 2^62 (clamped: the bucket fills), bucket = 0 (never a token: every job
    limited), a bucket of 2^53 with tokens at both ends of the range"""
    pool = make_pool(seed, U)
    lim = random_limiters(seed, U)
    by_jobs = np.argsort(-np.bincount(pool.pending_jobs.user, minlength=U))
    a, b, c3, d = (int(x) for x in by_jobs[:4])
    lim.per_minute[a], lim.bucket[a], lim.tokens[a], lim.last_update_ms[a] = 1e300, 7, -(2 ** 53), -(2 ** 62)
    lim.per_minute[b], lim.bucket[b], lim.tokens[b] = 600.0, 0, 0
    lim.per_minute[c3], lim.bucket[c3], lim.tokens[c3] = 1e-300, 2 ** 53, -(2 ** 53)
    lim.per_minute[d], lim.bucket[d], lim.tokens[d] = 60000.0, 2 ** 53, 2 ** 53
    cycles = seeded_cycles(seed, U, k, lim=lim)
    want = O.oracle(P1(), pool, cycles)
    assert want[0].view[a] == 7 and all(w.passed[b] == 0 and w.rate_limited[b] > 0 for w in want)
    assert want[0].until[c3] == 2 ** 62 and all(w.rate_limited[d] == 0 for w in want)
    compare(run_engine(make_engine, P1(), pool, cycles, U), want)


# ---- refusals and orders (the ABI test drives these on the emulator build) -----------------------------------------------------------------------
def code(fn):
    with pytest.raises(CookError) as ex:
        fn()
    return ex.value.code


def check_refusals(make_engine, U=65, k=64, seed=401):
    pool = make_pool(seed, U)
    lim = random_limiters(seed, U)
    L = lambda **kw: A.Limiters(**{**dict(per_minute=lim.per_minute, bucket=lim.bucket, tokens=lim.tokens, last_update_ms=lim.last_update_ms), **kw})
    one = lambda **kw: A.Limiters(**{**dict(per_minute=[60.0], bucket=[5], tokens=[1], last_update_ms=[0], user=[3]), **kw})
    with make_engine(P1()) as e:
        assert code(lambda: e.cycle_set_limiters(lim)) == COOK_E_STATE  # before cook_cycle_stage
        assert code(lambda: e.cycle_limiters_spend(0)) == COOK_E_STATE
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        e.cycle_set_considerable(open_state(U), None)
        assert code(lambda: e.fetch_limiters(U)) == COOK_E_STATE  # none held
        assert code(lambda: e.cycle_limiters_spend(0)) == COOK_E_STATE
        assert code(lambda: e.cycle_set_limiters(one())) == COOK_E_INVALID  # the first call must cover every user
        assert code(lambda: e.cycle_set_limiters(random_limiters(seed, U - 1))) == COOK_E_INVALID
        assert code(lambda: e.fetch_limiters(U)) == COOK_E_STATE  # (still none)
        e.cycle_set_limiters(lim)
        before = e.fetch_limiters(U)
        bad = [one(user=[U]), A.Limiters([60.0, 60.0], [5, 5], [1, 1], [0, 0], user=[3, 3]), one(per_minute=[0.0]), one(per_minute=[-1.0]),
               one(per_minute=[np.inf]), one(per_minute=[np.nan]), one(bucket=[-1]), one(bucket=[2 ** 53 + 1]), one(tokens=[2 ** 53 + 1]),
               one(tokens=[-(2 ** 53) - 1]), one(last_update_ms=[2 ** 62 + 1]), random_limiters(seed, U + 1)]
        for x in bad:
            assert code(lambda: e.cycle_set_limiters(x)) == COOK_E_INVALID
        assert code(lambda: e.cycle_set_clock(2 ** 62 + 1, 0)) == COOK_E_INVALID
        assert code(lambda: e.cycle_set_considerable(open_state(U, tokens=np.zeros(U, np.int64)), None)) == COOK_E_INVALID
        assert code(lambda: e.cycle_set_considerable(open_state(U + 1), None)) == COOK_E_INVALID
        assert code(lambda: e.cycle_limiters_spend(0)) == COOK_E_STATE  # no completed cycle yet
        assert all(np.array_equal(x, y) for x, y in zip(before, e.fetch_limiters(U)))
        e.cycle_set_clock(1500, 1500)
        e.cycle_run(k)
        ref = fetch(e, U)
        assert (ref.j2o >= 0).any()
        # a refused step changes nothing and leaves the clock staged
        e.cycle_set_clock(2500, 2400)
        assert code(lambda: e.cycle_run_queue_carry(k, A.QueueCarry(offers=True, usage=True, tokens_left=np.zeros(U, np.int64)))) == COOK_E_INVALID
        assert code(lambda: e.cycle_run_queue(k, remove_mode=2)) == COOK_E_INVALID
        assert code(lambda: e.cycle_limiters_spend(0, offer_skipped=np.zeros(pool.offers.n + 1, np.uint8))) == COOK_E_INVALID
        now = fetch(e, U)
        for f in ("Q", "pos", "j2o", "tokens", "last", "until"):
            assert np.array_equal(getattr(now, f), getattr(ref, f)), f
        # between a deferred set-up and cook_cycle_match_multi
        e.cycle_run_queue_rank(k)
        assert code(lambda: e.cycle_set_limiters(one())) == COOK_E_STATE
        assert code(lambda: e.cycle_set_limiters(None)) == COOK_E_STATE
        cycle_match_multi([e])
        e.cycle_set_limiters(one())
        # the refused steps left the clock staged: the deferred cycle ran with it — the same cycles on a fresh engine
        cycles = [O.cycle(k, state=open_state(U), now=1500, set_limiters=lim), O.cycle(k, now=2500, spend_ms=2400)]
        want = O.oracle(P1(), pool, cycles)
        got = fetch(e, U)
        w1 = want[1]
        tok = w1.tokens.copy()
        tok[3] = 1
        assert np.array_equal(got.j2o, w1.j2o) and np.array_equal(got.tokens, tok) and np.array_equal(got.rate_limited, w1.rate_limited)
        # an explicit spend, a second one, and the advance behind them
        e.cycle_limiters_spend(2600)
        assert e.limiter_info()["spent"] == int((w1.j2o >= 0).sum())
        assert code(lambda: e.cycle_limiters_spend(2600)) == COOK_E_STATE
        after = e.fetch_limiters(U)
        e.cycle_run_queue(0)  # (considers nothing: nothing earns)
        assert all(np.array_equal(x, y) for x, y in zip(after, e.fetch_limiters(U)))  # (spent once)


def struct_layout_sources():
    """-> (a C program that prints sizes and offsets of the new structs and the ABI version, the same numbers from cook_amd._abi)"""
    structs = [("cook_limiters", A.CookLimiters), ("cook_clock", A.CookClock), ("cook_limiter_info", A.CookLimiterInfo)]
    lines, want = ['#include <stdio.h>', '#include <stddef.h>', '#include "cookmatch.h"', "int main(void) {"], []
    for cname, cls in structs:
        lines.append(f'  printf("%zu\\n", sizeof({cname}));')
        want.append(__import__("ctypes").sizeof(cls))
        for fname, _ in cls._fields_:
            lines.append(f'  printf("%zu\\n", offsetof({cname}, {fname}));')
            want.append(getattr(cls, fname).offset)
    lines += ['  printf("%d\\n", COOK_ABI_VERSION);', "  return 0;", "}"]
    want.append(A.ABI_VERSION)
    return "\n".join(lines) + "\n", want
