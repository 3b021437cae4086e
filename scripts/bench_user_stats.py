"""Measures cook_user_stats (set-stats-counters!'s arithmetic on the device) at one C4 pool (175k tasks, 10k users) and at the C5
table (1.5M tasks), and cook_user_stats_multi over the eight C4 pools of the timed configuration: wall-clock microseconds per call
(median of --steps, the call includes its one stream synchronisation and the copies of the results), the bytes its kernels read,
and the CPU leg — tests/user_stats_oracle.py, the numpy restatement, on one host thread.  One JSON line per configuration.
    python scripts/bench_user_stats.py [--steps 50] [--out results/user_stats.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cook_amd import _abi as A  # noqa: E402
from cook_amd import synth, workload  # noqa: E402
from cook_amd.engine import Engine, user_stats_multi  # noqa: E402
from tests import user_stats_oracle as O  # noqa: E402


def bytes_read(n_tasks, n_users, n_pools=1):
    """what the kernels read: the sorted rows (40 B SumU4) + pending flag + user id per task, twice (scan, mark; the fold-again pass
    only for rounded users), the segments / inverse map per pool and user, then 12 doubles + limits per user, three times"""
    return n_tasks * (40 + 1 + 4) + n_tasks * 52 + n_pools * n_users * 12 + n_users * (96 + 48 + 1) * 3


def timed(fn, steps):
    fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2] * 1e6


def one(name, pools, steps, cpu_reps):
    n_users = pools[0].users.n
    lim = A.UserLimits.from_users(pools[0].users)
    engines = [Engine(A.default_params()) for _ in pools]
    try:
        for e, pl in zip(engines, pools):
            e.rank_stage(pl.tasks, pl.users)
            e.rank_run()
        call = (lambda: engines[0].user_stats(lim)) if len(engines) == 1 else (lambda: user_stats_multi(engines, lim))
        us = timed(call, steps)
        got = call()
        want = None
        t0 = time.perf_counter()
        for _ in range(cpu_reps):
            want = O.user_stats([(pl.tasks, None) for pl in pools], n_users, lim)
        cpu_us = (time.perf_counter() - t0) / cpu_reps * 1e6
        O.assert_same(got, want)
    finally:
        for e in engines:
            e.close()
    n_tasks = sum(pl.tasks.n for pl in pools)
    nb = bytes_read(n_tasks, n_users, len(pools))
    return {"config": name, "pools": len(pools), "tasks": n_tasks, "users": n_users, "us_per_call": round(us, 1), "bytes_read": nb,
            "GBps": round(nb / (us * 1e-6) / 1e9, 1), "cpu_leg_us": round(cpu_us, 1), "speedup_vs_cpu": round(cpu_us / us, 1),
            "parity": "bit-identical", "counts": got["counts"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    spec = workload.ClusterSpec()
    c4 = [workload.make_pool(spec, p) for p in range(spec.pools)]
    c5 = synth.make_pool(seed=0xC00C0005, n_pending=500_000, n_running=1_000_000, n_users=10_000, n_offers=50_000)
    rows = [one("C4 pool", c4[:1], args.steps, 3), one("C5", [c5], args.steps, 1), one("C4 x 8 (quota group)", c4, args.steps, 1)]
    for r in rows:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
