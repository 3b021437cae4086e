"""Measures cook_sweep_running (the lingering, straggler and cancelled killers over the running set) at two sizes: the GPU test's
running set (1 000 000 rows, 100 000 groups, 4 000 000 successful instances, one group of 1 000 000) and one C4 pool's 50 000
running rows (5 000 groups, 200 000 successful instances).  Per size: the median host wall time per call (the uploads from the
caller's pageable arrays, the kernels, both synchronisations and the copies of the result), the bytes uploaded, the device time of
the call's kernels (cook_kernel_timings, a profiled call of its own), and the CPU leg: the oracle of tests/sweep_oracle.py on one
thread.  Every result is checked against the oracle.  One JSON line per size, with the kernel revision (scripts/kernel_rev.py).
    python scripts/bench_sweep.py [--steps 20] [--out results/sweep.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cook_amd import _abi as A  # noqa: E402
from cook_amd.engine import Engine  # noqa: E402
from scripts.kernel_rev import kernel_rev  # noqa: E402
from tests import sweep_cases as S  # noqa: E402


def upload_bytes(kw):
    n, g = len(kw["start_ms"]), kw["groups"]
    G, NS = len(g["type"]), len(g["succ_start_ms"])
    return n * (8 + 1 + 8 + 1 + 4) + G * (1 + 8 + 8 + 4 + 4) + 4 + NS * 16


def run(name, kw, steps):
    with Engine(A.default_params()) as e:
        got = e.sweep_running(**kw)  # (the first call allocates the device buffers)
        ts = []
        for _ in range(steps):
            t0 = time.perf_counter()
            e.sweep_running(**kw)
            ts.append(time.perf_counter() - t0)
        e.set_profiling(True)
        e.sweep_running(**kw)
        kt = e.kernel_timings()
        e.set_profiling(False)
    t0 = time.perf_counter()
    want = S.run_oracle(kw)
    cpu_us = (time.perf_counter() - t0) * 1e6
    S.same(got, want)
    us = sorted(ts)[len(ts) // 2] * 1e6
    g = kw["groups"]
    return {"config": name, "rows": len(kw["start_ms"]), "groups": len(g["type"]), "successful": len(g["succ_start_ms"]),
            "us_per_call": round(us, 1), "upload_mb": round(upload_bytes(kw) / 1e6, 2), "kernel_us": round(sum(v[0] for v in kt.values()) * 1e3, 1),
            "kernels": {k: [round(v[0] * 1e3, 1), v[1]] for k, v in sorted(kt.items())}, "cpu_leg_us": round(cpu_us, 1),
            "speedup_vs_cpu": round(cpu_us / us, 1), "parity": "oracle", "info": got["info"], "kernel_rev": kernel_rev()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = [run("1M running rows, 100k groups, 4M successful", S.random_table(11, 1_000_000, 100_000, 4_000_000, big_group=1_000_000), args.steps),
            run("C4 pool: 50k running rows, 5k groups, 200k successful", S.random_table(15, 50_000, 5_000, 200_000), args.steps)]
    for r in rows:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
