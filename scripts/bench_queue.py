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
    python scripts/bench_queue.py [--steps 50] [--warmup 5] [--k-all] [--carry | --carry-only] [--out results/queue.json]"""
import argparse
import copy
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
from cook_amd.engine import Engine, cycle_match_multi, cycle_run_queue_carry_multi, cycle_run_queue_multi, cycle_run_rank_multi  # noqa: E402
from tests import autoscale_cases as AS  # noqa: E402
from tests import carry_oracle as CO  # noqa: E402
from tests import queue_cases as S  # noqa: E402

Q_OFFERS = 120  # offers of a queue cycle: well below K, so that every cycle keeps matches and leaves considered jobs unmatched
CARRY_CYCLES = 4  # queue cycles per episode of the carry legs (K = all: 1, the first cycle places whatever fits)
CARRY = ("carry_keys", "carry_seg_bounds", "carry_fold_offers", "carry_fold_users", "carry_fold_pool")
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--carry", action="store_true", help="also the two legs of the carry")
    ap.add_argument("--carry-only", action="store_true", help="only the two legs of the carry")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k-all", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    spec = workload.ClusterSpec()
    c4 = [workload.make_pool(spec, p) for p in range(spec.pools)]
    rows = []
    for k in [1000] + ([0] if args.k_all else []):
        if not args.carry_only:
            rows.append(run("one C4 pool", c4[:1], k, args.steps, args.warmup))
            rows.append(run("eight C4 pools, multi form", c4, k, args.steps, args.warmup))
        if args.carry or args.carry_only:
            rows.append(run_carry("one C4 pool", c4[:1], k, args.steps, args.warmup))
            rows.append(run_carry("eight C4 pools, multi form", c4, k, args.steps, args.warmup))
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
