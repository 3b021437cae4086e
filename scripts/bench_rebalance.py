#!/usr/bin/env python3
"""Rebalancer preemption sweep (BASELINE.json configs[4]): R running tasks + P pending jobs examined,
one cook_rebalance_run per step with inputs resident in HBM.  Prints one JSON line (reported beside bench.py's headline,
never instead of it).  `--check` compares the decisions with the CPU oracle (bit-exact) on the same inputs and times it.

Algorithmic bytes: B_rebal(R, P) = 52·R (init: keys + resources in, order + DRU out) + P·40·R (per pending
job every scored task's dru/mem/cpus/gpus/host/user is read once).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def resident_leg(args):
    """--resident: cook_rebalance_stage (through ctypes, every array contiguous and every struct built beforehand) beside
    cook_cycle_rebalance_stage on an engine that holds the same pool as a cycle stage, in turns, `--runs` times each; behind each stage
    one cook_rebalance_run (its cook_rebalance_timing) and a fetch: the decisions of the two must be identical."""
    import ctypes as C

    import numpy as np

    from cook_amd import _abi as A
    from cook_amd.engine import Engine
    from tests import parity_cases as P
    from tests import resident_rebalance_cases as X
    from tests import resident_rebalance_oracle as O

    b = P.make_rebalance_case(seed=0xC00C0005, n_running=args.running, n_pending=args.pending, n_users=args.users,
                              n_hosts=args.hosts, max_preemption=args.pending, quota_frac=0.02, spare_frac=args.spare_frac)
    sc, sm = np.zeros(args.hosts), np.zeros(args.hosts)
    sc[b["spare"].host], sm[b["spare"].host] = b["spare"].cpus, b["spare"].mem
    m = X.embed(b, 5, offers=A.Offers(cpus=sc, mem=sm, host=np.arange(args.hosts, dtype=np.uint32)))
    rp = b["rparams"]
    med = lambda v: sorted(v)[len(v) // 2]
    with Engine(b["params"]) as ea, Engine(b["params"]) as eb:
        m.stage(eb)
        eb.cycle_run(0)
        first = eb.cycle_rebalance(rp)  # (also the warm-up of the resident leg; its selected list defines the explicit inputs)
        sel_task, sel_ord = first["selected_task_idx"].astype(np.int64), first["selected_pending_ord"].astype(np.int64)
        running = O.tasks_take(m.tasks, np.flatnonzero(m.tasks.pending == 0))
        pending = m.jobs.take(sel_ord)
        jid, pri = np.ascontiguousarray(m.tasks.job_id[sel_task]), np.ascontiguousarray(m.tasks.priority[sel_task])
        spare = O.spare_of_offers(m.offers)
        rs, ps, us, ss, hs = running.as_struct(), pending.as_struct(), m.users.as_struct(), spare.as_struct(), m.offers.as_struct()
        i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
        stage_a = lambda: ea._lib.cook_rebalance_stage(ea._h, C.byref(rs), None, C.byref(ps), jid.ctypes.data_as(i64p), pri.ctypes.data_as(i32p),
                                                       C.byref(us), C.byref(ss), C.byref(hs), None, C.byref(rp))
        req = A.CookCycleRebalance(rp, None, None, None, 0, 0)
        stage_b = lambda: eb._lib.cook_cycle_rebalance_stage(eb._h, C.byref(req))
        ea._rb_p, ea._rb_r = pending.n, running.n
        assert stage_a() == 0
        ea.rebalance_run()  # warm-up of the classic leg
        ta, tb, ra, rb, same, diff = [], [], [], [], True, None
        for _ in range(args.runs):
            t0 = time.perf_counter()
            assert stage_a() == 0
            ta.append((time.perf_counter() - t0) * 1e3)
            ea.rebalance_run()
            ra.append(ea.rebalance_timing())
            got_a = ea.rebalance_fetch()
            t0 = time.perf_counter()
            assert stage_b() == 0
            tb.append((time.perf_counter() - t0) * 1e3)
            eb.rebalance_run()
            rb.append(eb.rebalance_timing())
            got_b = eb.rebalance_fetch()  # the compacted spaces: those of the explicit call
            same = same and got_a["decisions"] == got_b["decisions"] and np.array_equal(got_a["pending_dru"], got_b["pending_dru"], equal_nan=True)
            if not same and diff is None:
                diff = {"n": [len(got_a["decisions"]), len(got_b["decisions"])], "pending_dru_len": [len(got_a["pending_dru"]), len(got_b["pending_dru"])],
                        "first": next(([i, x, y] for i, (x, y) in enumerate(zip(got_a["decisions"], got_b["decisions"])) if x != y), None)}
    print(json.dumps({"metric": "rebalancer stage from the resident cycle state", "unit": "ms", "runs": args.runs,
                      "config": {"running": args.running, "pending": args.pending, "users": args.users, "hosts": args.hosts,
                                 "decisions": len(got_b["decisions"])},
                      "cook_rebalance_stage_ms": {"median": med(ta), "min": min(ta), "max": max(ta), "samples": ta},
                      "cook_cycle_rebalance_stage_ms": {"median": med(tb), "min": min(tb), "max": max(tb), "samples": tb},
                      "run_behind_classic_ms": {"median": med(ra), "min": min(ra), "max": max(ra)},
                      "run_behind_resident_ms": {"median": med(rb), "min": min(rb), "max": max(rb)},
                      "decisions_identical": bool(same), "first_difference": diff}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resident", action="store_true", help="cook_rebalance_stage beside cook_cycle_rebalance_stage, in turns")
    ap.add_argument("--runs", type=int, default=5, help="--resident: runs of each leg")
    ap.add_argument("--running", type=int, default=1_000_000)
    ap.add_argument("--pending", type=int, default=128, help="pending jobs examined (= max-preemption)")
    ap.add_argument("--users", type=int, default=10_000)
    ap.add_argument("--hosts", type=int, default=50_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--spare-frac", type=float, default=0.0, help="hosts with spare capacity; 0 = every decision has to preempt")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--kernels", action="store_true", help="one more profiled call: per-kernel microseconds and launches")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs an MI355X (no CPU fallback)"
    if args.resident:
        return resident_leg(args)
    from cook_amd.engine import Engine
    from tests import parity_cases as P

    b = P.make_rebalance_case(seed=0xC00C0005, n_running=args.running, n_pending=args.pending, n_users=args.users,
                              n_hosts=args.hosts, max_preemption=args.pending, quota_frac=0.02, spare_frac=args.spare_frac)
    with Engine(b["params"]) as e:
        t0 = time.perf_counter()
        e.rebalance_stage(b["running"], b["pending"], b["pending_job_id"], b["pending_priority"], b["users"], b["spare"],
                          b["rparams"], host_attrs=b["host_attrs"], groups=b["groups"])
        stage_s = time.perf_counter() - t0
        for _ in range(args.warmup):
            e.rebalance_run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev = []
        for _ in range(args.steps):
            e.rebalance_run()
            ev.append(e.rebalance_timing())
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / args.steps
        got = e.rebalance_fetch()
        kern = None
        if args.kernels:
            e.set_profiling(True)
            e.rebalance_run()
            kern = {k: [round(v[0] * 1e3, 1), v[1]] for k, v in sorted(e.kernel_timings().items(), key=lambda kv: -kv[1][0])[:14]}
            e.set_profiling(False)
    nd = len(got["decisions"])
    nbytes = 52 * args.running + args.pending * 40 * args.running
    out = {"metric": "rebalancer sweep: cook_rebalance_run calls/sec", "value": 1.0 / wall, "unit": "calls/s",
           "ms_per_call": wall * 1e3, "hip_event_ms": sorted(ev)[len(ev) // 2], "n_gpus": 1, "steps": args.steps,
           "warmup": args.warmup, "dtype": "f64", "data": "synthetic",
           "config": {"workload": f"{args.running} running tasks + {args.pending} pending jobs examined, {args.users} users, "
                                  f"{args.hosts} hosts", "decisions": nd,
                      "preempted": sum(len(d["tasks"]) for d in got["decisions"])},
           "stage_s": stage_s, "kernels_us_and_launches_per_call": kern,
           "roofline": {"bound": "hbm", "achieved": nbytes / wall / 1e9, "peak": 8000.0, "unit": "GB/s",
                        "frac": nbytes / wall / 1e9 / 8000.0, "algorithmic_bytes_per_call": nbytes, "traffic": None}}
    if args.check:
        from oracle import pyoracle
        t0 = time.perf_counter()
        want = pyoracle.rebalance(b["params"], b["running"], b["pending"], b["pending_job_id"], b["pending_priority"], b["users"],
                                  b["spare"], b["rparams"], host_attrs=b["host_attrs"], groups=b["groups"])
        cpu_s = time.perf_counter() - t0
        P._rebal_equal(got, want, "C5")
        out["cpu_baseline"] = {"value": 1.0 / cpu_s, "unit": "calls/s", "cores": 1, "kind": "port",
                               "sample": "the oracle on the same inputs, whole call"}
        out["speedup_vs_cpu_baseline"] = cpu_s / wall
        out["parity"] = "decisions, preempted tasks and pending DRUs bit-identical to the oracle"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
