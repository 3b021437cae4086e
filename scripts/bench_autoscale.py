"""Measures cook_cycle_autoscale (the pending-job candidates of handle-resource-offers-autoscaling-helper on the device) after one
cycle of a C4 pool at K = 1000, and after the eight C4 pools of the timed configuration (cook_cycle_run_rank_multi +
cook_cycle_match_multi), called one pool after another: wall-clock microseconds per call as the host sees it (median of --steps; the
call includes its readback of m, the filters' own synchronisations and the copy of the result).  Beside it the CPU leg: the oracle's
considerable over the masked queue Q' (built on the host), on one thread.  Every result is checked against the oracle of
tests/autoscale_cases.py.  One JSON line per configuration.  --multi adds the eight pools through ONE cook_cycle_autoscale_multi (the
pools' flows in one pool batch) beside the same pools one after another: same build, same process, same engines, the results compared.
    python scripts/bench_autoscale.py [--steps 50] [--multi] [--out results/autoscale.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cook_amd import _abi as A  # noqa: E402
from cook_amd import workload  # noqa: E402
from cook_amd.engine import Engine, cycle_autoscale_multi, cycle_match_multi, cycle_run_rank_multi  # noqa: E402
from oracle import pyoracle  # noqa: E402
from tests import autoscale_cases as S  # noqa: E402

K = 1000  # the reference's operating point (num-considerable)


def timed(fn, steps):
    fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2] * 1e6


def run(name, pools, steps, multi=False):
    params = A.default_params()
    states = [S.random_state(pl, 40 + i) for i, pl in enumerate(pools)]
    engines = [Engine(params) for _ in pools]
    try:
        for e, pl, (st, el) in zip(engines, pools, states):
            e.cycle_stage(pl.tasks, pl.users, pl.pending_jobs, pl.offers, pl.groups)
            e.cycle_set_considerable(st, el)
        if len(engines) == 1:
            engines[0].cycle_run(K)
        else:
            cycle_run_rank_multi(engines, [K] * len(engines))
            cycle_match_multi(engines)
        us = timed(lambda: [e.cycle_autoscale() for e in engines], steps)
        got = [e.cycle_autoscale() for e in engines]
        multi_us = stats = None
        if multi:  # the two legs alternate, so that neither has the warmer caches or the quieter moment
            none = [None] * len(engines)
            multi_us = timed(lambda: cycle_autoscale_multi(engines, none), steps)
            stats = engines[0].batch_stats()
            us = min(us, timed(lambda: [e.cycle_autoscale() for e in engines], steps))
            multi_us = min(multi_us, timed(lambda: cycle_autoscale_multi(engines, none), steps))
            for (out, info), (m_out, m_info) in zip(got, cycle_autoscale_multi(engines, none)):
                assert np.array_equal(out, m_out) and info == m_info, (info, m_info)
        cpu_us = 0.0
        for e, pl, (st, el), (out, info) in zip(engines, pools, states, got):
            _, j2o, _ = e.cycle_fetch()
            o_out, o_info, d = S.oracle(params, pl, st, K, el, j2o=j2o)
            assert np.array_equal(out, o_out) and info == o_info, (info, o_info)
            t0 = time.perf_counter()
            pyoracle.considerable(d.queue2, st, info["scaled"])
            cpu_us += (time.perf_counter() - t0) * 1e6
    finally:
        for e in engines:
            e.close()
    infos = [g[1] for g in got]
    extra = {"us_all_pools_multi": round(multi_us, 1), "multi_speedup": round(us / multi_us, 2), "batch": stats} if multi else {}
    return {**extra, "config": name, "pools": len(pools), "K": K, "pending": int(sum(pl.pending_jobs.n for pl in pools)),
            "us_per_call": round(us / len(pools), 1), "us_all_pools": round(us, 1), "cpu_leg_us": round(cpu_us / len(pools), 1),
            "cpu_leg_us_all_pools": round(cpu_us, 1), "speedup_vs_cpu": round(cpu_us / us, 1), "parity": "oracle",
            "matched": [i["matched"] for i in infos], "scaled": [i["scaled"] for i in infos], "n_out": [i["n_out"] for i in infos]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--multi", action="store_true", help="also the eight pools through one cook_cycle_autoscale_multi")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    spec = workload.ClusterSpec()
    c4 = [workload.make_pool(spec, p) for p in range(spec.pools)]
    rows = [run("C4 pool, K = 1000", c4[:1], args.steps), run("C4 x 8 after cook_cycle_match_multi, one call per pool", c4, args.steps, multi=args.multi)]
    for r in rows:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
