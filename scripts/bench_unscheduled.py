"""Measures cook_unscheduled (the quota, share and queue-position reasons of /unscheduled_jobs on the device) for all rows of one C4
pool (175k tasks, 10k users), for all rows of the C5 table (1.5M tasks) (also with the usage rows left on the device) and for a list of 1 000 rows of the C4 pool: wall-clock
microseconds per call (median of --steps; the call includes its one stream synchronisation and the copies of the results), beside
cook_user_stats on the same C4 pool in the same process (a comparable scan over the same rows), and the CPU leg —
tests/unscheduled_oracle.py's numpy form on one host thread.  One JSON line per configuration.
    python scripts/bench_unscheduled.py [--steps 50] [--out results/unscheduled.json]"""
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
from cook_amd.engine import Engine  # noqa: E402
from tests import unscheduled_oracle as O  # noqa: E402


def timed(fn, steps):
    fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2] * 1e6


def one(name, pool, steps, rows=None, with_user_stats=False, kernels=False, total_on_device=False):
    lim = A.UnschedLimits.from_users(pool.users)
    out = {"config": name, "tasks": pool.tasks.n, "users": pool.users.n, "rows": pool.tasks.n if rows is None else len(rows)}
    with Engine(A.default_params()) as e:
        e.rank_stage(pool.tasks, pool.users)
        e.rank_run()
        dev = None
        if total_on_device:  # the usage rows stay on the device (total_is_device): 32 of the 40 bytes per row are not copied
            import torch
            dev = torch.zeros((out["rows"], 4), dtype=torch.float64, device="cuda")
        call = lambda: e.unscheduled(lim, rows=rows, total_device_ptr=dev.data_ptr() if dev is not None else None)  # noqa: E731
        out["us_per_call"] = round(timed(call, steps), 1)
        if with_user_stats:
            ulim = A.UserLimits.from_users(pool.users)
            out["user_stats_us_per_call"] = round(timed(lambda: e.user_stats(ulim), steps), 1)
        got = call()
        if kernels:  # the device time of the call's launches (HIP events around each), one more call
            e.set_profiling(True)
            call()
            out["kernel_ms"] = {k: round(v[0], 4) for k, v in e.kernel_timings().items() if k.startswith(("un_", "seg_scan"))}
            e.set_profiling(False)
    t0 = time.perf_counter()
    want = O.unscheduled(pool.tasks, pool.users.n, lim, None, rows)
    out["cpu_leg_us"] = round((time.perf_counter() - t0) * 1e6, 1)
    if dev is not None:
        got["total"] = dev.cpu().numpy()
    O.assert_same(got, want)
    out["speedup_vs_cpu"] = round(out["cpu_leg_us"] / out["us_per_call"], 1)
    out["parity"] = "bit-identical"
    out["bits_set"] = {k: int((got["reasons"] & v != 0).sum()) for k, v in (("quota", 15), ("share", 112), ("queue-position", 128), ("at-least", 256))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    c4 = workload.make_pool(workload.ClusterSpec(), 0)
    c5 = synth.make_pool(seed=0xC00C0005, n_pending=500_000, n_running=1_000_000, n_users=10_000, n_offers=50_000)
    some = np.random.default_rng(1).integers(0, c4.tasks.n, 1000).astype(np.uint32)
    rows = [one("C4 pool, all rows", c4, args.steps, with_user_stats=True, kernels=True), one("C5, all rows", c5, args.steps, kernels=True),
            one("C5, all rows, total on the device", c5, args.steps, total_on_device=True),
            one("C4 pool, 1000 rows", c4, args.steps, rows=some, kernels=True)]
    for r in rows:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
