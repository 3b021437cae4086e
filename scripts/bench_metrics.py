"""Measures cook_match_metrics (handle-match-cycle-metrics' numbers on the device) after one cycle of a C4 pool at K = 1000, and after the
eight C4 pools of the timed configuration (cook_cycle_run_rank_multi + cook_cycle_match_multi) called one pool after another and through
ONE cook_match_metrics_multi: wall-clock microseconds as the host sees it (median of --steps; a call includes its two read-backs).  Both
legs run on the same build, in the same process, on the same engines, alternating; their results are compared, and pool 0's are checked
against pyoracle.resource_stats.  The one-pool row on this build against the same row on another build shows what the call's own
structure costs.  One JSON line per configuration.
    python scripts/bench_metrics.py [--steps 50] [--out results/metrics.json]"""
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
from cook_amd.engine import Engine, cycle_match_multi, cycle_run_rank_multi  # noqa: E402
from cook_amd import engine as E  # noqa: E402
from oracle import pyoracle  # noqa: E402

K = 1000  # the reference's operating point (num-considerable)


def timed(fn, steps):
    fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2] * 1e6


def same(a, b):
    for k in a:
        if isinstance(a[k], dict):
            same(a[k], b[k])
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), (k, a[k], b[k])


def run(name, pools, steps, n_users):
    params = A.default_params()
    engines = [Engine(params) for _ in pools]
    multi = getattr(E, "match_metrics_multi", None) if len(pools) > 1 else None  # (absent in a build without the multi call)
    try:
        for e, pl in zip(engines, pools):
            e.cycle_stage(pl.tasks, pl.users, pl.pending_jobs, pl.offers, pl.groups)
        if len(engines) == 1:
            engines[0].cycle_run(K)
        else:
            cycle_run_rank_multi(engines, [K] * len(engines))
            cycle_match_multi(engines)
        one = lambda: [e.match_metrics(n_users=n_users, n_gpu_models=2) for e in engines]  # noqa: E731
        us = timed(one, steps)
        got = one()
        extra = {}
        if multi:
            many = lambda: multi(engines, n_users=n_users, n_gpu_models=2)  # noqa: E731
            multi_us = timed(many, steps)
            stats = engines[0].batch_stats()
            us = min(us, timed(one, steps))
            multi_us = min(multi_us, timed(many, steps))
            for a, b in zip(got, many()):
                same(a, b)
            extra = {"us_all_pools_multi": round(multi_us, 1), "multi_speedup": round(us / multi_us, 2), "batch": stats}
        ranked, _, _ = engines[0].cycle_fetch()
        pl = pools[0]
        jobs = pl.pending_jobs.take((np.cumsum(pl.tasks.pending) - 1)[ranked[:got[0]["considerable"]]])
        for key, v in pyoracle.resource_stats(jobs.cpus, jobs.mem).items():
            assert got[0]["jobs"][key] == v, (key, got[0]["jobs"][key], v)
        for key, v in pyoracle.resource_stats(pl.offers.cpus, pl.offers.mem).items():
            assert got[0]["offers_stats"][key] == v, (key, got[0]["offers_stats"][key], v)
    finally:
        for e in engines:
            e.close()
    return {**extra, "config": name, "pools": len(pools), "K": K, "offers": int(sum(pl.offers.n for pl in pools)),
            "us_per_call": round(us / len(pools), 1), "us_all_pools": round(us, 1), "matched": [g["matched"] for g in got]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    spec = workload.ClusterSpec()
    c4 = [workload.make_pool(spec, p) for p in range(spec.pools)]
    rows = [run("C4 pool, K = 1000", c4[:1], args.steps, spec.users), run("C4 x 8 after cook_cycle_match_multi", c4, args.steps, spec.users)]
    for r in rows:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
