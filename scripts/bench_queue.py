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
    python scripts/bench_queue.py [--steps 50] [--warmup 5] [--k-all] [--out results/queue.json]"""
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
from cook_amd.engine import Engine, cycle_match_multi, cycle_run_queue_multi, cycle_run_rank_multi  # noqa: E402
from tests import autoscale_cases as AS  # noqa: E402
from tests import queue_cases as S  # noqa: E402

Q_OFFERS = 120  # offers of a queue cycle: well below K, so that every cycle keeps matches and leaves considered jobs unmatched
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k-all", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    spec = workload.ClusterSpec()
    c4 = [workload.make_pool(spec, p) for p in range(spec.pools)]
    rows = []
    for k in [1000] + ([0] if args.k_all else []):
        rows.append(run("one C4 pool", c4[:1], k, args.steps, args.warmup))
        rows.append(run("eight C4 pools, multi form", c4, k, args.steps, args.warmup))
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
