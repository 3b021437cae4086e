"""Measures cook_usage_breakdown / cook_usage_breakdown_multi (GET /usage with its job-group breakdown on the device): all users of
one C4 pool (175k tasks, 10k users), all users of C5's table (1M running rows; also with the usage arrays left on the device), one
listed user of C5, and the eight pools of the timed configuration through the multi form.  Per configuration: wall-clock
microseconds per call (median of --steps; the call includes its synchronisations and the copies of the results), the device time of
the call's launches from a profiled call of its own (cook_kernel_timings), cook_user_stats on the same pool in the same process as
the yardstick, and the CPU leg — tests/usage_oracle.py's numpy form on one host thread, against which every result is checked.
One JSON line per configuration.
    python scripts/bench_usage.py [--steps 50] [--out results/usage.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cook_amd import _abi as A  # noqa: E402
from cook_amd import synth, workload  # noqa: E402
from cook_amd.engine import Engine, usage_breakdown_multi  # noqa: E402
from tests import usage_cases as S  # noqa: E402
from tests import usage_oracle as O  # noqa: E402

OURS = ("ub_", "seg_scan", "radix_")


def timed(fn, steps):
    fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2] * 1e6


def finish(out, engines, call, got, pools, n_users, users, multi, dev):
    lead = engines[0]
    lead.set_profiling(True)  # the device time of the call's launches (HIP events around each), one more call
    call()
    out["kernel_ms"] = {k: round(v[0], 4) for k, v in lead.kernel_timings().items() if k.startswith(OURS)}
    out["kernel_ms_sum"] = round(sum(out["kernel_ms"].values()), 4)
    lead.set_profiling(False)
    t0 = time.perf_counter()
    want = O.usage(pools, n_users, None, users, multi)
    out["cpu_leg_us"] = round((time.perf_counter() - t0) * 1e6, 1)
    if dev is not None:
        B = len(got["bucket_group"])
        got["bucket_usage"], got["total"] = dev[0].cpu().numpy()[:B], dev[1].cpu().numpy()
    O.assert_same(got, want)
    out["buckets"], out["rows"] = int(len(got["bucket_group"])), int(len(got["rows"]))
    out["speedup_vs_cpu"] = round(out["cpu_leg_us"] / out["us_per_call"], 1)
    out["parity"] = "bit-identical"
    return out


def one(name, pool, n_groups, steps, users=None, with_user_stats=False, on_device=False):
    grp = S.random_groups(1, pool.tasks, n_groups)
    out = {"config": name, "tasks": pool.tasks.n, "running": int((pool.tasks.pending == 0).sum()), "users": pool.users.n, "groups": n_groups}
    with Engine(A.default_params()) as e:
        e.rank_stage(pool.tasks, pool.users)
        e.rank_run()
        dev = None
        if on_device:  # bucket_usage and total stay on the device: 32 of the 44 bytes per bucket are not copied
            import torch
            dev = (torch.zeros((pool.tasks.n, 4), dtype=torch.float64, device="cuda"), torch.zeros((pool.users.n, 4), dtype=torch.float64, device="cuda"))
        call = lambda: e.usage_breakdown(grp, n_groups, users=users, usage_device_ptr=dev[0].data_ptr() if dev else None,  # noqa: E731
                                         total_device_ptr=dev[1].data_ptr() if dev else None)
        out["us_per_call"] = round(timed(call, steps), 1)
        if with_user_stats:
            ulim = A.UserLimits.from_users(pool.users)
            out["user_stats_us_per_call"] = round(timed(lambda: e.user_stats(ulim), steps), 1)
        return finish(out, [e], call, call(), [(pool.tasks, grp)], pool.users.n, users, False, dev)


def multi(name, pools, n_groups, steps):
    groups = [S.random_groups(10 + i, pl.tasks, n_groups) for i, pl in enumerate(pools)]
    n_users = max(pl.users.n for pl in pools)
    out = {"config": name, "tasks": sum(pl.tasks.n for pl in pools), "running": int(sum((pl.tasks.pending == 0).sum() for pl in pools)),
           "users": n_users, "groups": n_groups, "engines": len(pools)}
    engines = [Engine(A.default_params()) for _ in pools]
    try:
        for e, pl in zip(engines, pools):
            e.rank_stage(pl.tasks, pl.users)
            e.rank_run()
        call = lambda: usage_breakdown_multi(engines, n_users, groups, n_groups)  # noqa: E731
        out["us_per_call"] = round(timed(call, steps), 1)
        return finish(out, engines, call, call(), [(pl.tasks, g) for pl, g in zip(pools, groups)], n_users, None, True, None)
    finally:
        for e in engines:
            e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    spec = workload.ClusterSpec()
    c4 = workload.make_pool(spec, 0)
    c5 = synth.make_pool(seed=0xC00C0005, n_pending=500_000, n_running=1_000_000, n_users=10_000, n_offers=50_000)
    rev = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_rev.py")], capture_output=True, text=True).stdout.strip()
    rows = [one("C4 pool, all users", c4, 30_000, args.steps, with_user_stats=True),
            one("C5, all users", c5, 200_000, args.steps, with_user_stats=True),
            one("C5, all users, usage on the device", c5, 200_000, args.steps, on_device=True),
            one("C5, one listed user", c5, 200_000, args.steps, users=np.array([int(c5.tasks.user[0])], np.uint32)),
            multi("eight pools, multi form", [workload.make_pool(spec, i) for i in range(8)], 50_000, args.steps)]
    for r in rows:
        r["kernel_rev"] = rev
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
