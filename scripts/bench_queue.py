"""Measures a queue cycle (cook_cycle_run_queue / cook_cycle_run_queue_multi + cook_cycle_match_multi: a match cycle on the standing
ranked queue, without a re-rank) beside the full resident cycle (cook_cycle_run / cook_cycle_run_rank_multi + cook_cycle_match_multi) of
the SAME build in the SAME process: one C4 pool and the eight C4 pools of the timed configuration at K = 1000 (--k-all: also K = every
pending job).  Both are timed against offer sets of the SAME size and make (Q_OFFERS seeded offers per pool: the pools are staged with
the first set, the full cycle places against it, the queue cycles against two such sets in turns), so the difference is the rank against
the advance and not the size of the placement.  Median host wall time per call over --steps cycles after --warmup; the fetches that keep
every timed queue cycle's result are outside the timed region, and afterwards every one of those results is compared with the oracle of
tests/queue_cases.py (the engine's job_to_offer as given for the removal: the placement itself is the parity suites' business).  The
advance alone: the host's wall time in it, its one synchronisation included (cook_match_stats_ex [31], median over the timed cycles,
summed over the pools), and the sum of its kernels from cook_kernel_timings in a profiled pass of its own.  One JSON line per
configuration.
The carry (cook_cycle_run_queue_carry*), --carry: two legs of the same content on the same build in the same process.
Leg one is a queue cycle with offers = usage = 1 and no upload.  Leg two is a queue cycle whose host reads job_to_offer and the
considered positions back and supplies the same next offers through step->offers and the same user state through
cook_cycle_set_considerable (the host's own arithmetic between the two — here tests/carry_oracle.py, from leg one's results — is NOT
timed: a JVM host would do it faster than Python does).  Episodes of one rank cycle and CARRY_CYCLES queue cycles from the same staged
state, the queue cycles timed; both legs must place every job identically, cycle for cycle, or the run fails.
The release (cook_cycle_run_queue_release*), --release: the same two legs with a list of finished tasks per queue cycle
(RELEASE_FRAC of the placements of the episode so far that have not ended yet, drawn from leg one's own results).  Leg one is a queue
cycle with carry + release and no upload; leg two's host supplies the same offers, user state and groups' table through step->offers,
cook_cycle_set_considerable and step->groups (its arithmetic — tests/carry_oracle.py and tests/release_oracle.py — is NOT timed).  Both
legs must place every job identically in every cycle, or the run fails.  The row also has the device time of the release's kernels
beside the carry's for the same cycles, from a profiled episode of its own.
The host churn (cook_cycle_run_queue_hosts*), --churn: the release's two legs with, per queue cycle, CHURN_FRAC of the
staged hosts leaving and as many rows joining (hosts that return, new hosts; anchored at random old rows or at the end).  Leg one is a
queue cycle with carry + release + churn and no table upload; leg two's host supplies the same table through step->offers (its
arithmetic — the oracles of tests/ — is NOT timed).  Both legs must place every job identically in every cycle, or the run fails.
The host reservations (cook_cycle_run_queue_reserve*), --reserve: leg one of --churn through the new entry point, once
with reservations = NULL and once with, per queue cycle, release_matched = 1 and a replacement list of RESERVE_LIST random entries
(the two legs place differently: hosts are reserved); the row has both cycle times and the device time of the reserve kernels beside
the carry's, the release's and the churn's.
--limiters: the churn's first leg under an enforcing launch-rate limit, twice each in turns: a host that uploads
tokens_left per pool per cycle (the counts come from the other leg: its arithmetic is not timed) against limiters kept on the device with
cook_cycle_set_clock per cycle; identical placements asserted; the row has the four medians, the spread of the host's two runs and the
limiter kernels' device time per cycle.
    python scripts/bench_queue.py [--steps 50] [--warmup 5] [--k-all] [--carry | --carry-only] [--release | --release-only] [--churn | --churn-only] [--reserve] [--limiters]
                                  [--out results/queue.json]"""
import argparse
import copy
import dataclasses
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cook_amd import _abi as A  # noqa: E402
from cook_amd import workload  # noqa: E402
from cook_amd.engine import (Engine, cycle_match_multi, cycle_run_queue_carry_multi, cycle_run_queue_hosts_multi, cycle_run_queue_multi, cycle_run_queue_reserve_multi,  # noqa: E402
                             cycle_run_queue_release_multi, cycle_run_rank_multi)
from tests import autoscale_cases as AS  # noqa: E402
from tests import carry_oracle as CO  # noqa: E402
from tests import churn_oracle as HO  # noqa: E402
from tests import queue_cases as S  # noqa: E402
from tests import release_oracle as RO  # noqa: E402

Q_OFFERS = 120  # offers of a queue cycle: well below K, so that every cycle keeps matches and leaves considered jobs unmatched
CARRY_CYCLES = 4  # queue cycles per episode of the carry legs (K = all: 1, the first cycle places whatever fits)
CARRY = ("carry_keys", "carry_seg_bounds", "carry_fold_offers", "carry_fold_users", "carry_fold_pool")
RELEASE = ("release_host_rows", "release_keys", "release_fold_offers", "release_fold_users", "release_fold_pool", "release_group_mark",
           "release_group_scan", "release_group_offsets", "release_group_compact")
RELEASE_FRAC = 0.3  # of the episode's placements that have not ended yet, per queue cycle
CHURN = ("churn_mark", "churn_scan", "churn_source", "churn_gather")
RESERVE = ("resv_release", "resv_retire", "resv_install", "resv_bits")
RESERVE_LIST = 128  # entries of a cycle's replacement list: max-preemption of the reference's rebalancer tests
CHURN_FRAC = 0.01  # of the staged hosts leave per queue cycle, and as many rows join
ADVANCE = ("q_mark_removed", "q_queue_scan", "q_compact_ranked", "q_group_scan", "q_fold_offsets", "q_fold_copy_old", "q_fold_append")


def median_ms(ts):
    return round(sorted(ts)[len(ts) // 2] * 1e3, 4)


def run(name, pools, k, steps, warmup):
    params = A.default_params()
    n = len(pools)
    states = [AS.random_state(pl, 40 + i) for i, pl in enumerate(pools)]
    offers = [[S.fresh_offers(7000 + 10 * i + c, Q_OFFERS, gpus=True, constraints=True) for c in range(2)] for i in range(n)]
    engines = [Engine(params) for _ in pools]
    ks = [k if k else pl.pending_jobs.n for pl in pools]

    def full():
        if n == 1:
            engines[0].cycle_run(ks[0])
        else:
            cycle_run_rank_multi(engines, ks)
            cycle_match_multi(engines)

    def queue(c):
        if n == 1:
            engines[0].cycle_run_queue(ks[0], offers=offers[0][c & 1])
        else:
            cycle_run_queue_multi(engines, ks, [dict(offers=offers[i][c & 1]) for i in range(n)])
            cycle_match_multi(engines)

    try:
        for e, pl, (st, el) in zip(engines, pools, states):
            e.cycle_stage(pl.tasks, pl.users, pl.pending_jobs, offers[engines.index(e)][0], pl.groups)
            e.cycle_set_considerable(st, el)
        t_full, t_queue, t_adv = [], [], []
        for s in range(warmup + steps):
            t0 = time.perf_counter()
            full()
            if s >= warmup:
                t_full.append(time.perf_counter() - t0)
        got = [[S.fetch(e, False)] for e in engines]  # the rank cycle the queue cycles start from
        for c in range(1, warmup + steps + 1):
            t0 = time.perf_counter()
            queue(c)
            if c > warmup:
                t_queue.append(time.perf_counter() - t0)
                t_adv.append(sum(e.match_stats()["queue_advance_us"] for e in engines) * 1e-6)
            for i, e in enumerate(engines):
                got[i].append(S.fetch(e, False))
        # the advance's kernels, in a profiled pass of its own (event timing serialises the launches: not part of the wall times above)
        for e in engines:
            e.set_profiling(True)
        full()
        queue(1)
        adv_us = 0.0
        for e in engines:
            adv_us += sum(ms for nm, (ms, _) in e.kernel_timings().items() if nm in ADVANCE) * 1e3
            e.set_profiling(False)
    finally:
        for e in engines:
            e.close()
    # every timed queue cycle against the oracle (removal, queue, considered positions)
    for i, (pl, (st, el)) in enumerate(zip(pools, states)):
        cycles = [SimpleNamespace(k=ks[i], state=st, eligible=el, offers=offers[i][0] if c == 0 else offers[i][c & 1], offer_skipped=None,
                                  remove_mode=0, groups=None) for c in range(len(got[i]))]
        staged = copy.copy(pl)
        staged.offers = offers[i][0]
        want = S.oracle(params, staged, cycles, given_j2o=[g.j2o for g in got[i]])
        S.assert_exercised(want)
        S.compare(got[i], want, cycles, f"pool {i}")
        assert (got[i][0].j2o >= 0).any() and (got[i][0].j2o < 0).any(), "the full cycle keeps a match and leaves a considered job unmatched"
    fm, qm = median_ms(t_full), median_ms(t_queue)
    return {"config": name, "pools": n, "K": k or "all", "steps": steps, "full_cycle_ms": fm, "queue_cycle_ms": qm,
            "queue_over_full": round(qm / fm, 3), "offers_per_pool": Q_OFFERS,
            "advance_wall_us": round(median_ms(t_adv) * 1e3, 1), "advance_kernels_us": round(adv_us, 1), "parity": "oracle (removal; placement as given)",
            "queue_len_first_last": [[int(len(g[0].Q)), int(len(g[-1].Q))] for g in got]}


def run_carry(name, pools, k, steps, warmup):
    """the two legs of the carry; -> one result row"""
    params = A.default_params()
    n = len(pools)
    states = [AS.random_state(pl, 40 + i, tokens=False, pool_quota=False) for i, pl in enumerate(pools)]
    ks = [k if k else pl.pending_jobs.n for pl in pools]
    cyc = CARRY_CYCLES if k else 1
    episodes = max(1, -(-(warmup + steps) // cyc))
    both = A.QueueCarry(offers=True, usage=True)

    def rank(engines):
        if n == 1:
            engines[0].cycle_run(ks[0])
        else:
            cycle_run_rank_multi(engines, ks)
            cycle_match_multi(engines)

    def episode(engines, step, record):
        """restage the offers and the user state, rank, cyc queue cycles through step(c); -> their wall times"""
        for e, pl, (st, el) in zip(engines, pools, states):
            e.cycle_update(offers=pl.offers)
            e.cycle_set_considerable(st, el)
        rank(engines)
        if record is not None:
            record.append([S.fetch(e, False) for e in engines])
        ts = []
        for c in range(1, cyc + 1):
            t0 = time.perf_counter()
            step(engines, c)
            ts.append(time.perf_counter() - t0)
            if record is not None:
                record.append([S.fetch(e, False) for e in engines])
        return ts

    def leg(step, want_launches=False):
        engines = [Engine(params) for _ in pools]
        try:
            for e, pl in zip(engines, pools):
                e.cycle_stage(pl.tasks, pl.users, pl.pending_jobs, pl.offers, pl.groups)
            first, ts = [], []
            for ep in range(episodes):
                ts += episode(engines, step, first if ep == 0 else None)
            launches = None
            if want_launches:  # the advance's launches, counted in a profiled episode of its own
                for e in engines:
                    e.set_profiling(True)
                episode(engines, step, None)
                launches = round(sum(nl for e in engines for nm, (_, nl) in e.kernel_timings().items() if nm in ADVANCE + CARRY) / cyc / n, 1)
            return first, ts[warmup:], launches
        finally:
            for e in engines:
                e.close()

    def step_carry(engines, c):
        if n == 1:
            engines[0].cycle_run_queue_carry(ks[0], both)
        else:
            cycle_run_queue_carry_multi(engines, ks, None, [both] * n)
            cycle_match_multi(engines)

    got1, t1, launches = leg(step_carry, want_launches=True)
    # what the host of leg two supplies: the oracle's carry of leg one's own placements (untimed)
    supply = [[None] * (cyc + 1) for _ in pools]
    for i, (pl, (st, el)) in enumerate(zip(pools, states)):
        offers, state = pl.offers, st
        jq_of = np.cumsum(pl.tasks.pending) - 1
        for c in range(1, cyc + 1):
            g = got1[c - 1][i]
            jobs = pl.pending_jobs.take(jq_of[g.Q[g.pos]])
            hit = g.j2o >= 0
            offers, state = CO.carry_offers(offers, jobs, g.j2o, hit), CO.carry_usage(state, jobs, hit, spend=False)
            supply[i][c] = (offers, state, el)

    def step_host(engines, c):
        for i, e in enumerate(engines):  # the read-back a host needs before it can do the arithmetic
            e.cycle_fetch()
            e.cycle_fetch_considerable()
            e.cycle_set_considerable(supply[i][c][1], supply[i][c][2])
        if n == 1:
            engines[0].cycle_run_queue(ks[0], offers=supply[0][c][0])
        else:
            cycle_run_queue_multi(engines, ks, [dict(offers=supply[i][c][0]) for i in range(n)])
            cycle_match_multi(engines)

    got2, t2, _ = leg(step_host)
    for c, (a, b) in enumerate(zip(got1, got2)):
        for i in range(n):
            assert np.array_equal(a[i].Q, b[i].Q) and np.array_equal(a[i].pos, b[i].pos) and np.array_equal(a[i].j2o, b[i].j2o), \
                f"{name}: the legs differ in cycle {c}, pool {i}"
    kept = [[int((g[i].j2o >= 0).sum()) for g in got1] for i in range(n)]
    assert all(x > 0 for row in kept for x in row[:-1]), "a timed cycle has no kept placement to carry"
    cm, hm = median_ms(t1), median_ms(t2)
    return {"config": name + ", carry", "pools": n, "K": k or "all", "timed_cycles": len(t1), "carry_cycle_ms": cm, "host_supplied_cycle_ms": hm,
            "carry_over_host": round(cm / hm, 3), "advance_launches_per_pool_without_sort_passes": launches, "advance_syncs": 1,
            "identical_placements": True, "kept_per_cycle": kept}


def run_release(name, pools, k, steps, warmup):
    """the two legs of the release (carry + release against a host that supplies offers, user state and groups); -> one result row"""
    params = A.default_params()
    n = len(pools)
    states = [AS.random_state(pl, 40 + i, tokens=False, pool_quota=False) for i, pl in enumerate(pools)]
    ks = [k if k else pl.pending_jobs.n for pl in pools]
    cyc = CARRY_CYCLES if k else 1
    episodes = max(1, -(-(warmup + steps) // cyc))
    both = A.QueueCarry(offers=True, usage=True)
    grouped = [pl.groups is not None and pl.pending_jobs.group is not None for pl in pools]
    jq_of = [np.cumsum(pl.tasks.pending) - 1 for pl in pools]
    lists = [[None] * (cyc + 1) for _ in pools]   # lists[i][c]: what queue cycle c of pool i releases (drawn in leg one's first episode)
    history = [[] for _ in pools]
    rng = np.random.default_rng(99)
    gone = [set() for _ in pools]

    def rank(engines):
        if n == 1:
            engines[0].cycle_run(ks[0])
        else:
            cycle_run_rank_multi(engines, ks)
            cycle_match_multi(engines)

    def note(engines, c, draw):
        """after cycle c of the first episode: keep its result; draw: the next cycle's lists from the placements so far"""
        out = [S.fetch(e, False) for e in engines]
        if draw:
            for i, (g, pl) in enumerate(zip(out, pools)):
                history[i].append(SimpleNamespace(j2o=g.j2o, jobs=pl.pending_jobs.take(jq_of[i][g.Q[g.pos]]), offers=pl.offers))
                if c < cyc:
                    picks = [q for q in RO.placed_rows(history[i]) if q not in gone[i] and rng.random() < RELEASE_FRAC]
                    gone[i].update(picks)
                    lists[i][c + 1] = RO.finished_of(history[i], picks, offers=1, usage=1, groups=int(grouped[i]))
        return out

    def episode(engines, step, record, draw=False):
        for e, pl, (st, el) in zip(engines, pools, states):
            e.cycle_update(offers=pl.offers)
            e.cycle_set_considerable(st, el)
        rank(engines)
        if record is not None:
            record.append(note(engines, 0, draw))
        ts = []
        for c in range(1, cyc + 1):
            t0 = time.perf_counter()
            step(engines, c)
            ts.append(time.perf_counter() - t0)
            if record is not None:
                record.append(note(engines, c, draw))
        return ts

    def leg(step, first_leg=False):
        engines = [Engine(params) for _ in pools]
        try:
            for e, pl in zip(engines, pools):
                e.cycle_stage(pl.tasks, pl.users, pl.pending_jobs, pl.offers, pl.groups)
            first, ts = [], []
            for ep in range(episodes):
                ts += episode(engines, step, first if ep == 0 else None, draw=first_leg and ep == 0)
            prof = None
            if first_leg:  # launches and device time of the advance's parts, in a profiled episode of its own
                for e in engines:
                    e.set_profiling(True)
                episode(engines, step, None)
                kt = [e.kernel_timings() for e in engines]
                part = lambda names, x: sum(v[x] for t in kt for nm, v in t.items() if nm in names)
                prof = dict(launches=round(part(ADVANCE + CARRY + RELEASE, 1) / cyc / n, 1), release_launches=round(part(RELEASE, 1) / cyc / n, 1),
                            carry_us=round(part(CARRY, 0) * 1e3 / cyc, 1), release_us=round(part(RELEASE, 0) * 1e3 / cyc, 1))
            return first, ts[warmup:], prof
        finally:
            for e in engines:
                e.close()

    def step_release(engines, c):
        if n == 1:
            engines[0].cycle_run_queue_release(ks[0], both, lists[0][c])
        else:
            cycle_run_queue_release_multi(engines, ks, None, [both] * n, [lists[i][c] for i in range(n)])
            cycle_match_multi(engines)

    got1, t1, prof = leg(step_release, first_leg=True)
    # what the host of leg two supplies: the oracle's carry and release of leg one's own placements and lists (untimed)
    supply = [[None] * (cyc + 1) for _ in pools]
    for i, (pl, (st, el)) in enumerate(zip(pools, states)):
        offers, state, table = pl.offers, st, S.group_table(pl.groups)
        for c in range(1, cyc + 1):
            g, h = got1[c - 1][i], history[i][c - 1]
            hit = g.j2o >= 0
            offers, state = CO.carry_offers(offers, h.jobs, g.j2o, hit), CO.carry_usage(state, h.jobs, hit, spend=False)
            if grouped[i]:
                table = copy.deepcopy(table)
                for x in np.flatnonzero(hit):
                    gg = int(h.jobs.group[x])
                    if gg != A.NONE_U32:
                        table.run_hosts[gg].append(int(pl.offers.host[g.j2o[x]]))
                        table.run_attrs[gg].append(S.offer_attr(pl.offers, int(g.j2o[x]), int(table.attr_key[gg])))
            fin = lists[i][c]
            if fin is not None:
                offers, state = RO.release_offers(offers, fin)[0], RO.release_usage(state, fin)
                if grouped[i]:
                    table = RO.release_groups(table, fin)[0]
            supply[i][c] = (offers, state, el, S.build_groups(table) if grouped[i] else None)

    def step_host(engines, c):
        for i, e in enumerate(engines):  # the read-back a host needs before it can do the arithmetic
            e.cycle_fetch()
            e.cycle_fetch_considerable()
            e.cycle_set_considerable(supply[i][c][1], supply[i][c][2])
        if n == 1:
            engines[0].cycle_run_queue(ks[0], offers=supply[0][c][0], groups=supply[0][c][3])
        else:
            cycle_run_queue_multi(engines, ks, [dict(offers=supply[i][c][0], groups=supply[i][c][3]) for i in range(n)])
            cycle_match_multi(engines)

    got2, t2, _ = leg(step_host)
    for c, (a, b) in enumerate(zip(got1, got2)):
        for i in range(n):
            assert np.array_equal(a[i].Q, b[i].Q) and np.array_equal(a[i].pos, b[i].pos) and np.array_equal(a[i].j2o, b[i].j2o), \
                f"{name}: the legs differ in cycle {c}, pool {i}"
    released = [[0 if f is None else int(f.n) for f in row[1:]] for row in lists]
    assert all(x > 0 for row in released for x in row), "a timed cycle has nothing to release"
    rm, hm = median_ms(t1), median_ms(t2)
    return {"config": name + ", carry + release", "pools": n, "K": k or "all", "timed_cycles": len(t1), "release_cycle_ms": rm,
            "host_supplied_cycle_ms": hm, "release_over_host": round(rm / hm, 3), "advance_launches_per_pool_without_sort_passes": prof["launches"],
            "of_them_release": prof["release_launches"], "carry_kernels_us_per_cycle": prof["carry_us"], "release_kernels_us_per_cycle": prof["release_us"],
            "advance_syncs": 1, "identical_placements": True, "released_per_cycle": released, "groups": grouped}


def run_churn(name, pools, k, steps, warmup, reserve=False, limiters=False):
    """the two legs of the host churn (carry + release + churn against a host that supplies the table, the user state and the groups);
    -> one result row.  reserve: instead of the host's leg, the same carry + release + churn cycles through
    cook_cycle_run_queue_reserve* with reservations = NULL (leg one) and with, per queue cycle, release_matched = 1 and a replacement
    list of RESERVE_LIST entries (leg two; its placements differ: hosts are reserved).  limiters: the same first leg
    under an enforcing launch-rate limit, twice each in turns: (b) with the limiters on the device and cook_cycle_set_clock per cycle,
    (a) as a host drives it, uploading tokens_left per pool per cycle (its own arithmetic is not counted: the counts are leg (b)'s)"""
    params = A.default_params()
    n = len(pools)
    states = [AS.random_state(pl, 40 + i, tokens=False, pool_quota=False) for i, pl in enumerate(pools)]
    ks = [k if k else pl.pending_jobs.n for pl in pools]
    cyc = CARRY_CYCLES if k else 1
    episodes = max(1, -(-(warmup + steps) // cyc))
    both = A.QueueCarry(offers=True, usage=True)
    grouped = [pl.groups is not None and pl.pending_jobs.group is not None for pl in pools]
    jq_of = [np.cumsum(pl.tasks.pending) - 1 for pl in pools]
    lists = [[None] * (cyc + 1) for _ in pools]   # what queue cycle c of pool i releases (drawn in leg one's first episode)
    history = [[] for _ in pools]
    rng = np.random.default_rng(99)
    gone = [set() for _ in pools]
    # the churns: drawn up front over the hosts alone (every episode starts from the pool's own offers again)
    churns = [[None] * (cyc + 1) for _ in pools]
    for i, pl in enumerate(pools):
        assert len(set(pl.offers.host.tolist())) == pl.offers.n, "one offer per host"
        draw = HO.churner(500 + i, CHURN_FRAC, fresh_from=int(pl.offers.host.max()) + 1)  # (new hosts get the next ids: host ids are dense hostname ranks)
        hosts = pl.offers.host
        for c in range(1, cyc + 1):
            h = churns[i][c] = draw([SimpleNamespace(offers=pl.offers)], SimpleNamespace(n=len(hosts), host=hosts))
            src = HO.new_order(hosts, h)[0]
            hosts = np.array([hosts[x] if kind == "old" else h.join.host[x] for kind, x in src], np.uint32)

    def rank(engines):
        if n == 1:
            engines[0].cycle_run(ks[0])
        else:
            cycle_run_rank_multi(engines, ks)
            cycle_match_multi(engines)

    def note(engines, c, draw):
        out = [S.fetch(e, False) for e in engines]
        if draw:
            for i, (g, pl, e) in enumerate(zip(out, pools, engines)):
                g.churn = e.churn_info()
                if limiters:
                    tokens[i][c] = e.fetch_limiters(states[i][0].n)[0]
                    limited[0] += int(e.fetch_rate_limit(states[i][0].n)[0].sum())
                history[i].append(SimpleNamespace(j2o=g.j2o, jobs=pl.pending_jobs.take(jq_of[i][g.Q[g.pos]]), offers=e.fetch_offers().offers()))
                if c < cyc:
                    picks = [q for q in RO.placed_rows(history[i]) if q not in gone[i] and rng.random() < RELEASE_FRAC]
                    gone[i].update(picks)
                    lists[i][c + 1] = RO.finished_of(history[i], picks, offers=1, usage=1, groups=int(grouped[i]))
        return out

    def episode(engines, step, record, draw=False, begin=None):
        for e, pl, (st, el) in zip(engines, pools, states):
            e.cycle_update(offers=pl.offers)
            e.cycle_set_considerable(st, el)
        if begin is not None:
            begin(engines)
        rank(engines)
        if record is not None:
            record.append(note(engines, 0, draw))
        ts = []
        for c in range(1, cyc + 1):
            t0 = time.perf_counter()
            step(engines, c)
            ts.append(time.perf_counter() - t0)
            if record is not None:
                record.append(note(engines, c, draw))
        return ts

    def leg(step, first_leg=False, profile=None):
        profile = first_leg if profile is None else profile
        engines = [Engine(params) for _ in pools]
        try:
            for e, pl in zip(engines, pools):
                e.cycle_stage(pl.tasks, pl.users, pl.pending_jobs, pl.offers, pl.groups)
            first, ts = [], []
            for ep in range(episodes):
                ts += episode(engines, step, first if ep == 0 else None, draw=first_leg and ep == 0)
            prof = None
            if profile:  # launches and device time of the advance's parts, in a profiled episode of its own
                for e in engines:
                    e.set_profiling(True)
                episode(engines, step, None)
                kt = [e.kernel_timings() for e in engines]
                part = lambda names, x: sum(v[x] for t in kt for nm, v in t.items() if nm in names)
                prof = dict(launches=round(part(ADVANCE + CARRY + RELEASE + CHURN, 1) / cyc / n, 1), churn_launches=round(part(CHURN, 1) / cyc / n, 1),
                            carry_us=round(part(CARRY, 0) * 1e3 / cyc, 1), release_us=round(part(RELEASE, 0) * 1e3 / cyc, 1),
                            churn_us=round(part(CHURN, 0) * 1e3 / cyc, 1), reserve_us=round(part(RESERVE, 0) * 1e3 / cyc, 1),
                            reserve_launches=round(part(RESERVE, 1) / cyc / n, 1))
            return first, ts[warmup:], prof
        finally:
            for e in engines:
                e.close()

    def step_churn(engines, c):
        if n == 1:
            engines[0].cycle_run_queue_hosts(ks[0], both, lists[0][c], churns[0][c])
        else:
            cycle_run_queue_hosts_multi(engines, ks, None, [both] * n, [lists[i][c] for i in range(n)], [churns[i][c] for i in range(n)])
            cycle_match_multi(engines)

    if limiters:
        lr = np.random.default_rng(4242)
        lims = []
        for st, _ in states:
            bucket = lr.integers(20, 200, st.n)
            lims.append(A.Limiters(lr.choice([60.0, 600.0, 1333.0, 6000.0], size=st.n), bucket, bucket, np.zeros(st.n, np.int64)))
        states_b = [(dataclasses.replace(st, enforce_rate_limit=True), el) for st, el in states]
        tokens = [[None] * (cyc + 1) for _ in pools]  # what the filters of cycle c compared with, from leg (b)'s first episode
        limited = [0]  # jobs the rate-limit stage held back in that episode (the legs must not measure a limit that never binds)

        def limiter_leg(on_device):
            nonlocal states
            if on_device:
                states = states_b
            else:
                states = [(dataclasses.replace(st, tokens_left=tokens[i][0]), el) for i, (st, el) in enumerate(states_b)]

            def step(engines, c):
                if on_device:
                    for e in engines:
                        e.cycle_set_clock(1000 * (c + 1), 1000 * (c + 1) - 30)
                    step_churn(engines, c)
                    return
                cy = [A.QueueCarry(offers=True, usage=True, tokens_left=tokens[i][c]) for i in range(n)]
                if n == 1:
                    engines[0].cycle_run_queue_hosts(ks[0], cy[0], lists[0][c], churns[0][c])
                else:
                    cycle_run_queue_hosts_multi(engines, ks, None, cy, [lists[i][c] for i in range(n)], [churns[i][c] for i in range(n)])
                    cycle_match_multi(engines)
            return step
        LIMITER = ("lim_count_kept", "lim_spend", "lim_commit_earn")
        results = {}
        for turn, on_device in enumerate((True, False, True, False)):
            step = limiter_leg(on_device)
            engines = [Engine(params) for _ in pools]
            try:
                for e, pl in zip(engines, pools):
                    e.cycle_stage(pl.tasks, pl.users, pl.pending_jobs, pl.offers, pl.groups)
                first, ts = [], []

                def begin(engines):  # (the limiters and the rank cycle's clock go in behind the episode's cook_cycle_set_considerable)
                    if on_device:
                        for e, lm in zip(engines, lims):
                            e.cycle_set_limiters(lm)
                            e.cycle_set_clock(1000, 1000)
                for ep in range(episodes):
                    if on_device:
                        for e in engines:
                            e.cycle_set_limiters(None)  # (the episode restages the user state)
                    rec = first if ep == 0 else None
                    ts += episode(engines, step, rec, draw=(turn == 0 and ep == 0), begin=begin)
                prof_us = prof_launches = None
                if on_device:
                    for e in engines:
                        e.set_profiling(True)
                        e.cycle_set_limiters(None)
                    episode(engines, step, None, begin=begin)
                    kt = [e.kernel_timings() for e in engines]
                    prof_us = round(sum(v[0] for t in kt for nm, v in t.items() if nm in LIMITER) * 1e3 / cyc, 1)
                    prof_launches = round(sum(v[1] for t in kt for nm, v in t.items() if nm in LIMITER) / cyc, 1)
                results[turn] = (first, median_ms(ts[warmup:]), prof_us, prof_launches)
                if turn == 0:
                    assert all(t is not None for row in tokens for t in row) and limited[0] > 0, "the limit binds nowhere"
            finally:
                for e in engines:
                    e.close()
        for c, (a, b) in enumerate(zip(results[0][0], results[1][0])):
            for i in range(n):
                assert np.array_equal(a[i].Q, b[i].Q) and np.array_equal(a[i].pos, b[i].pos) and np.array_equal(a[i].j2o, b[i].j2o), \
                    f"{name}: the limiter legs differ in cycle {c}, pool {i}"
        a_ms, b_ms = [results[1][1], results[3][1]], [results[0][1], results[2][1]]
        return {"config": name + ", carry + release + churn under an enforcing launch-rate limit", "pools": n, "K": k or "all", "timed_cycles": len(ts[warmup:]),
                "host_tokens_left_cycle_ms": a_ms, "device_limiters_cycle_ms": b_ms, "host_runs_spread_ms": round(abs(a_ms[0] - a_ms[1]), 3),
                "limiter_kernels_us_per_cycle": results[2][2], "limiter_launches_per_cycle": results[2][3], "rate_limited_jobs_first_episode": limited[0],
                "identical_placements": True}
    if reserve:
        rr = np.random.default_rng(777)
        rlists = [[A.Reservations(rr.choice(pl.pending_jobs.n, min(RESERVE_LIST, pl.pending_jobs.n), replace=False),
                                  rr.choice(pl.offers.host, min(RESERVE_LIST, pl.pending_jobs.n))) for _ in range(cyc + 1)] for pl in pools]

        def step_reserve(with_lists):
            def step(engines, c):
                rv = [rlists[i][c] if with_lists else None for i in range(n)]
                if n == 1:
                    engines[0].cycle_run_queue_reserve(ks[0], both, lists[0][c], churns[0][c], rv[0])
                else:
                    cycle_run_queue_reserve_multi(engines, ks, None, [both] * n, [lists[i][c] for i in range(n)], [churns[i][c] for i in range(n)], rv)
                    cycle_match_multi(engines)
            return step
        _, t0, prof0 = leg(step_reserve(False), first_leg=True)
        _, t1, prof1 = leg(step_reserve(True), profile=True)
        return {"config": name + ", carry + release + churn through cook_cycle_run_queue_reserve", "pools": n, "K": k or "all", "timed_cycles": len(t1),
                "reservations_null_cycle_ms": median_ms(t0), "reservations_cycle_ms": median_ms(t1), "list_entries_per_cycle": RESERVE_LIST,
                "carry_kernels_us_per_cycle": prof1["carry_us"], "release_kernels_us_per_cycle": prof1["release_us"],
                "churn_kernels_us_per_cycle": prof1["churn_us"], "reserve_kernels_us_per_cycle": prof1["reserve_us"],
                "reserve_launches_per_pool": prof1["reserve_launches"], "reserve_kernels_us_per_cycle_null": prof0["reserve_us"], "advance_syncs": 1}
    got1, t1, prof = leg(step_churn, first_leg=True)
    # what the host of leg two supplies: the oracles' carry, release and churn of leg one's own placements and lists (untimed)
    supply = [[None] * (cyc + 1) for _ in pools]
    for i, (pl, (st, el)) in enumerate(zip(pools, states)):
        offers, state, table = pl.offers, st, S.group_table(pl.groups)
        for c in range(1, cyc + 1):
            g, h = got1[c - 1][i], history[i][c - 1]
            hit = g.j2o >= 0
            if grouped[i]:
                table = copy.deepcopy(table)
                for x in np.flatnonzero(hit):
                    gg = int(h.jobs.group[x])
                    if gg != A.NONE_U32:
                        table.run_hosts[gg].append(int(offers.host[g.j2o[x]]))
                        table.run_attrs[gg].append(S.offer_attr(offers, int(g.j2o[x]), int(table.attr_key[gg])))
            offers, state = CO.carry_offers(offers, h.jobs, g.j2o, hit), CO.carry_usage(state, h.jobs, hit, spend=False)
            fin = lists[i][c]
            if fin is not None:
                offers, state = RO.release_offers(offers, fin)[0], RO.release_usage(state, fin)
                if grouped[i]:
                    table = RO.release_groups(table, fin)[0]
            offers, info = HO.churn_offers(offers, churns[i][c])
            assert got1[c][i].churn == info, (name, i, c, got1[c][i].churn, info)
            supply[i][c] = (offers, state, el, S.build_groups(table) if grouped[i] else None)

    def step_host(engines, c):
        for i, e in enumerate(engines):  # the read-back a host needs before it can do the arithmetic
            e.cycle_fetch()
            e.cycle_fetch_considerable()
            e.cycle_set_considerable(supply[i][c][1], supply[i][c][2])
        if n == 1:
            engines[0].cycle_run_queue(ks[0], offers=supply[0][c][0], groups=supply[0][c][3])
        else:
            cycle_run_queue_multi(engines, ks, [dict(offers=supply[i][c][0], groups=supply[i][c][3]) for i in range(n)])
            cycle_match_multi(engines)

    got2, t2, _ = leg(step_host)
    for c, (a, b) in enumerate(zip(got1, got2)):
        for i in range(n):
            assert np.array_equal(a[i].Q, b[i].Q) and np.array_equal(a[i].pos, b[i].pos) and np.array_equal(a[i].j2o, b[i].j2o), \
                f"{name}: the legs differ in cycle {c}, pool {i}"
    churned = [[[int(len(h.leave)), int(h.join.n)] for h in row[1:]] for row in churns]
    assert all(a > 0 and b > 0 for row in churned for a, b in row), "a timed cycle has no host that leaves or joins"
    cm, hm = median_ms(t1), median_ms(t2)
    return {"config": name + ", carry + release + churn", "pools": n, "K": k or "all", "timed_cycles": len(t1), "churn_cycle_ms": cm,
            "host_supplied_cycle_ms": hm, "churn_over_host": round(cm / hm, 3), "advance_launches_per_pool_without_sort_passes": prof["launches"],
            "of_them_churn": prof["churn_launches"], "carry_kernels_us_per_cycle": prof["carry_us"], "release_kernels_us_per_cycle": prof["release_us"],
            "churn_kernels_us_per_cycle": prof["churn_us"], "advance_syncs": 1, "identical_placements": True, "offers_per_pool": [int(pl.offers.n) for pl in pools],
            "leave_join_per_cycle": churned, "groups": grouped}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--carry", action="store_true", help="also the two legs of the carry")
    ap.add_argument("--carry-only", action="store_true", help="only the two legs of the carry")
    ap.add_argument("--release", action="store_true", help="also the two legs of the release")
    ap.add_argument("--release-only", action="store_true", help="only the two legs of the release (and, with --carry, of the carry)")
    ap.add_argument("--churn", action="store_true", help="also the two legs of the host churn")
    ap.add_argument("--churn-only", action="store_true", help="only the two legs of the host churn (and, with --carry / --release, of those)")
    ap.add_argument("--reserve", action="store_true", help="only the churn's first leg through cook_cycle_run_queue_reserve*, without and with reservations")
    ap.add_argument("--limiters", action="store_true", help="only the churn's first leg under a launch-rate limit: tokens_left from the host against limiters on the device")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k-all", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    spec = workload.ClusterSpec()
    c4 = [workload.make_pool(spec, p) for p in range(spec.pools)]
    rows = []

    def add(r):  # (printed as it comes: a long run that is cut short keeps what it has measured)
        rows.append(r)
        print(json.dumps(r), flush=True)
    for k in [1000] + ([0] if args.k_all else []):
        if args.limiters:
            add(run_churn("one C4 pool", c4[:1], k, args.steps, args.warmup, limiters=True))
            add(run_churn("eight C4 pools, multi form", c4, k, args.steps, args.warmup, limiters=True))
            continue
        if args.reserve:
            add(run_churn("one C4 pool", c4[:1], k, args.steps, args.warmup, reserve=True))
            add(run_churn("eight C4 pools, multi form", c4, k, args.steps, args.warmup, reserve=True))
            continue
        if not args.carry_only and not args.release_only and not args.churn_only:
            add(run("one C4 pool", c4[:1], k, args.steps, args.warmup))
            add(run("eight C4 pools, multi form", c4, k, args.steps, args.warmup))
        if args.carry or args.carry_only:
            add(run_carry("one C4 pool", c4[:1], k, args.steps, args.warmup))
            add(run_carry("eight C4 pools, multi form", c4, k, args.steps, args.warmup))
        if args.release or args.release_only:
            add(run_release("one C4 pool", c4[:1], k, args.steps, args.warmup))
            add(run_release("eight C4 pools, multi form", c4, k, args.steps, args.warmup))
        if args.churn or args.churn_only:
            add(run_churn("one C4 pool", c4[:1], k, args.steps, args.warmup))
            add(run_churn("eight C4 pools, multi form", c4, k, args.steps, args.warmup))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
