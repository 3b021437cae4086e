#!/usr/bin/env python3
"""Offer construction (cook_offers_run) on one MI355X: the whole 50k-node cluster of BASELINE.json's configs[3] with 400k pods
(= its running tasks), inputs resident in HBM, kernels only.  Prints one JSON line; --check compares with the oracle.
--resident: the resident pod table instead — a pool's queue cycles with a pod delta (leg b) beside the composition that
was there before (leg a: cook_offers_stage + _run + _fetch, the rows handed to cook_cycle_run_queue_reserve as step offers; the host's
own arithmetic not counted), the legs in turns, identical placements asserted in every cycle; and cook_offers_update + cook_offers_run
alone at --nodes x --pods."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cook_amd import _abi as A  # noqa: E402
from cook_amd import synth  # noqa: E402
from cook_amd.engine import Engine  # noqa: E402


def percentile_ms(xs):
    return dict(median=round(float(np.median(xs)), 4), lo=round(float(np.min(xs)), 4), hi=round(float(np.max(xs)), 4))


def draw_delta(rng, ids, next_id, frac, n_nodes, cols):
    """frac of the pods change: half of them leave, as many fresh ones join (ids from next_id on) -> (PodDelta, the ids behind it)"""
    n = max(1, int(len(ids) * frac / 2))
    gone = rng.choice(ids, n, replace=False).astype(np.uint32)
    add = A.Pods(node=rng.integers(0, n_nodes, n).astype(np.uint32), cpus=rng.integers(1, 8, n) + 0.1, mem=rng.integers(1, 16, n) * 1024.0,
                 **{c: np.zeros(n, dt) if c != "disk" else np.full(n, -1.0) for c, dt in cols})
    add_id = np.arange(next_id, next_id + n, dtype=np.uint32)
    keep = ~np.isin(ids, gone)
    return A.PodDelta(remove=gone, add=add, add_id=add_id), np.concatenate([ids[keep], add_id]), keep, add


def apply_host(pods, keep, add):
    """the host's mirror of the pod table behind a delta (leg a uploads it whole)"""
    cat = lambda c: None if getattr(pods, c) is None else np.concatenate([getattr(pods, c)[keep], getattr(add, c)])  # noqa: E731
    return A.Pods(**{c: cat(c) for c in ("node", "cpus", "mem", "gpus", "gpu_model", "disk", "disk_type", "flags")})


def resident(a):
    from cook_amd import workload
    opt = [("gpus", np.int32), ("gpu_model", np.uint32), ("disk", np.float64), ("disk_type", np.uint32), ("flags", np.uint8)]
    out = dict(what="resident pod table", frac_changed=a.frac)
    # ---- the update + rebuild alone, at the offers benchmark's shape ----------------------------------------------------------------------
    nodes, pods, op = synth.make_cluster_state(seed=0xC00C, n_nodes=a.nodes, n_pods=a.pods, disk=True, n_attr_keys=8, max_pods=110)
    rng = np.random.default_rng(5)
    with Engine(A.default_params()) as e:
        ids = np.arange(pods.n, dtype=np.uint32)
        id_cap = pods.n + (a.steps + a.warmup + 1) * (int(pods.n * a.frac / 2) + 1)
        e.offers_stage(nodes, pods, op)
        e.offers_stage_pod_ids(ids, id_cap)
        upd, run = [], []
        for it in range(a.warmup + a.steps):
            if it == a.warmup:
                e.set_profiling(True)
            d, ids, _, _ = draw_delta(rng, ids, int(ids.max()) + 1, a.frac, nodes.n, opt)
            t0 = time.perf_counter()
            e.offers_update(d)
            t1 = time.perf_counter()
            e.offers_run()
            t2 = time.perf_counter()
            if it >= a.warmup:
                upd.append((t1 - t0) * 1e3), run.append((t2 - t1) * 1e3)
        kt = e.kernel_timings()
        changed = len(d.remove) + d.add.n
        out["update_alone"] = dict(nodes=a.nodes, pods=a.pods, changed_per_cycle=changed, update_ms=percentile_ms(upd), rebuild_ms=percentile_ms(run),
                                   pod_kernels_us=round(sum(v[0] for k, v in kt.items() if k.startswith("pod_")) * 1e3 / a.steps, 2),
                                   rebuild_kernels_us=round(sum(v[0] for k, v in kt.items() if k.startswith(("offers", "radix", "iota"))) * 1e3 / a.steps, 2),
                                   bytes_uploaded_per_cycle=41 * d.add.n + 4 * len(d.remove), bytes_full_stage=77 * a.nodes + 41 * a.pods)
    # ---- the queue cycles: one C4 pool at K = 1000 over 6 250 nodes x 50 000 pods -----------------------------------------------------------
    pool = workload.make_pool(workload.ClusterSpec(), 0)
    nodes, pods0, op = synth.make_cluster_state(seed=0xC4, n_nodes=a.q_nodes, n_pods=a.q_pods, n_attr_keys=0, max_pods=110)
    K = a.k
    legs = {"a": [], "b": []}
    pod_us, reb_us = [], []
    for rnd in range(a.runs):
        for leg in ("a", "b"):
            rng = np.random.default_rng(11)
            pods, ids = pods0, np.arange(pods0.n, dtype=np.uint32)
            placed, ms = [], []
            with Engine(A.default_params(good_enough_fitness=1.0)) as e:
                e.offers_stage(nodes, pods, op)
                e.offers_stage_pod_ids(ids, pods.n + (a.steps + 2) * (int(pods.n * a.frac / 2) + 1))
                e.offers_run()
                e.cycle_stage_built_offers(pool.tasks, pool.users, pool.pending_jobs, pool.groups, with_task_limits=True)
                e.cycle_run(K)
                if leg == "b":
                    e.set_profiling(True)
                for it in range(a.steps):
                    d, ids, keep, add = draw_delta(rng, ids, int(ids.max()) + 1, a.frac, nodes.n, opt)
                    pods = apply_host(pods, keep, add)  # (the host's own arithmetic: outside both clocks)
                    t0 = time.perf_counter()
                    if leg == "b":
                        e.cycle_run_queue_pods(K, None, None, d, None, True)
                    else:
                        e.offers_stage(nodes, pods, op)
                        e.offers_run()
                        rows = e.offers_fetch()
                        e.cycle_run_queue_reserve(K, None, None, None, None, offers=rows.as_offers(
                            max_tasks=np.full(rows.n, op.max_pods_per_node, np.int32), num_tasks=rows.num_pods))
                    ms.append((time.perf_counter() - t0) * 1e3)
                    placed.append(e.cycle_fetch()[1].copy())
                if leg == "b":
                    kt = e.kernel_timings()
                    pod_us.append(sum(v[0] for k, v in kt.items() if k.startswith("pod_")) * 1e3 / a.steps)
                    reb_us.append(sum(v[0] for k, v in kt.items() if k.startswith(("offers", "radix", "iota", "fill"))) * 1e3 / a.steps)
            legs[leg].append((float(np.median(ms)), placed))
    for (_, pa), (_, pb) in zip(legs["a"], legs["b"]):
        assert len(pa) == len(pb) and all(np.array_equal(x, y) for x, y in zip(pa, pb)), "the legs place differently"
    changed = 2 * max(1, int(a.q_pods * a.frac / 2))
    out["queue_cycle"] = dict(nodes=a.q_nodes, pods=a.q_pods, K=K, runs=a.runs, cycles_per_run=a.steps, identical_placements=True,
                              leg_a_ms=[round(m, 4) for m, _ in legs["a"]], leg_b_ms=[round(m, 4) for m, _ in legs["b"]],
                              pod_kernels_us=round(float(np.median(pod_us)), 2), rebuild_kernels_us=round(float(np.median(reb_us)), 2),
                              bytes_uploaded_per_cycle=dict(leg_a=77 * a.q_nodes + 41 * a.q_pods, leg_b=41 * changed // 2 + 4 * changed // 2))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resident", action="store_true")
    ap.add_argument("--frac", type=float, default=0.01)
    ap.add_argument("--q-nodes", type=int, default=6250)
    ap.add_argument("--q-pods", type=int, default=50000)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--nodes", type=int, default=50000)
    ap.add_argument("--pods", type=int, default=400000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    if a.resident:
        return resident(a)
    nodes, pods, op = synth.make_cluster_state(seed=0xC00C, n_nodes=a.nodes, n_pods=a.pods, disk=True, n_attr_keys=8, max_pods=110)
    # algorithmic bytes: every input column once + the offer rows once (cookmatch.h cook_nodes / cook_pods / cook_node_offers)
    b_in = a.nodes * (8 + 8 + 4 + 4 + 8 + 4 + 1 + 4 + 8 * 4) + a.pods * (4 + 8 + 8 + 4 + 4 + 8 + 4 + 1)
    with Engine(A.default_params()) as e:
        e.offers_stage(nodes, pods, op)
        for _ in range(a.warmup):
            e.offers_run()
        e.set_profiling(True)
        ms = []
        for _ in range(a.steps):
            e.offers_run()
            ms.append(e.offers_timing())
        kt = e.kernel_timings()
        got = e.offers_fetch()
        b_out = got.n * (4 + 4 + 8 + 8 + 4 + 8 + 4 + 8 + 4 + 8 * 4) + a.nodes
        out = dict(what="cook_offers_run", nodes=a.nodes, pods=a.pods, offers=int(got.n), ms_per_call=float(np.median(ms)),
                   algorithmic_bytes=b_in + b_out, achieved_GBps=(b_in + b_out) / (float(np.median(ms)) * 1e-3) / 1e9,
                   peak_GBps=8000.0, kernels_us_per_call={k: round(v[0] * 1e3 / a.steps, 2) for k, v in sorted(kt.items(), key=lambda kv: -kv[1][0])
                                                          if k.startswith(("offers", "radix", "iota"))})
        if a.check:
            from oracle import k8s_offers
            t0 = time.time()
            want = k8s_offers.build_rows(nodes, pods, op)
            out["oracle_s"] = round(time.time() - t0, 2)
            ok = all(np.array_equal(getattr(got, k), v) for k, v in want["rows"].items()) and np.array_equal(got.node_status, want["status"])
            ok = ok and all(got.totals[k] == v for k, v in want["totals"].items())
            out["identical_to_oracle"] = bool(ok)
            out["speedup_vs_oracle"] = round(out["oracle_s"] * 1e3 / out["ms_per_call"], 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
