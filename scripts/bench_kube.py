"""Measures cook_kube_distribute (scheduling-capacity-constrained-job-distributor on the device) at the reference's operating point
(max-jobs-considered 500) and at 50 000 jobs, for 3 and 32 compute clusters: wall-clock microseconds per call as the host sees it
(median and min-max of --steps; the call includes its uploads, its one synchronisation and the copy of the choices and lists), the
kernel's own time from per-kernel event timing in a second pass, and, for scale only, the job-by-job oracle of tests/kube_oracle.py on
one thread (Python: it says nothing about the JVM's distributor, which is not measured).  Two capacity shapes per size: `ample` (no
cluster runs out: one pass per tile) and `tight` (capacities of about 3/4 of the jobs: every cluster runs out, the worst case of
ceil(K / tile) + n passes).  Every result is checked against the oracle.  One JSON line per configuration.
--cycles adds the pool's cycle: one C4 pool and the eight C4 pools, max-jobs-considered 500 and 50 000, 3 and 32 clusters, two legs run
in turns in one session on the same engines — (a) the composition the library offered before cook_cycle_run_kube:
cook_cycle_run_queue_release with remove_mode = 1 on a pool without offers, cook_cycle_fetch_considerable, the host's distribution
(the oracle of tests/kube_oracle.py, timed separately and reported counted and not counted), the user state after the launched jobs
uploaded through cook_cycle_set_considerable (its arithmetic not counted: the upload alone); (b) cook_cycle_run_kube with carry usage,
and for eight pools cook_cycle_run_kube_multi.  Every episode starts from a fresh rank; medians and min-max per queue cycle, the
distributor's kernel time, launches and synchronisations from cook_batch_stats.  The launched lists of both legs are compared.
    python scripts/bench_kube.py [--steps 50] [--cycles] [--small] [--out results/kube.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cook_amd import _abi as A  # noqa: E402
from cook_amd.engine import Engine  # noqa: E402
from tests import kube_cases as KC  # noqa: E402
from tests import kube_oracle as O  # noqa: E402


def timed(fn, steps):
    fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    ts.sort()
    return dict(median=round(ts[len(ts) // 2], 1), min=round(ts[0], 1), max=round(ts[-1], 1))


def spread(ts):
    ts = sorted(ts)
    return dict(median=round(ts[len(ts) // 2], 1), min=round(ts[0], 1), max=round(ts[-1], 1), n=len(ts))


def cycle_legs(pools, label, mjc, n_cl, steps, lib):
    """legs (a) and (b) in turns over the same engines; -> one row"""
    from cook_amd.engine import cycle_run_kube_multi
    from tests import autoscale_cases as S
    n = len(pools)
    no_offers = A.Offers(cpus=np.zeros(0), mem=np.zeros(0), host=np.zeros(0, np.uint32))
    es = [Engine(A.default_params(good_enough_fitness=1.0), lib_path=lib) for _ in pools]
    states = [S.open_state(p.users.n) for p in pools]
    for e, p, st in zip(es, pools, states):
        e.cycle_stage(p.tasks, p.users, p.pending_jobs, no_offers, p.groups)
        e.cycle_set_considerable(st, np.ones(p.pending_jobs.n, np.uint8))
    cl_loc, cl_cap = np.zeros(n_cl, np.uint32), np.full(n_cl, max(1, (3 * mjc) // (4 * n_cl)), np.int64)  # three quarters of the jobs find room
    mc = O.gate(cl_cap, mjc, 0)["max_considerable"]  # (the host's gate, :1767-1778: what leg (a) asks its queue cycle for)
    n_steps = max(2, min(steps, min(p.pending_jobs.n for p in pools) // mjc - 2))
    pend_ord = [np.cumsum(p.tasks.pending) - 1 for p in pools]
    t_a, t_a_host, t_b, lists_a, lists_b, kstats = [], [], [], [], [], None
    for turn in range(4):
        leg = "ab"[turn % 2]
        for e in es:
            e.cycle_run(mjc)  # a fresh rank: both legs start from the same queue (its own cycle is not timed)
        for step in range(n_steps):
            seed = 1000 + step
            if leg == "a":
                t0 = time.perf_counter()
                host = 0.0
                for i, (e, p) in enumerate(zip(es, pools)):
                    e.cycle_run_queue_release(mc, remove_mode=1)
                    pos = e.cycle_fetch_considerable()
                    h0 = time.perf_counter()
                    ranked = e.cycle_fetch()[0]
                    ck = p.pending_jobs.ckpt_location
                    loc = ck[pend_ord[i][ranked[pos]]] if ck is not None else None
                    d = O.distribute(len(pos), cl_loc, cl_cap, loc, None, seed, task=ranked[pos])
                    host += time.perf_counter() - h0
                    e.cycle_set_considerable(states[i], None)  # (the upload of the user state after the launched jobs; its arithmetic is the host's)
                    if turn == 0:
                        lists_a.append(d["lists"])
                dt = time.perf_counter() - t0
                t_a.append((dt - host) * 1e6)
                t_a_host.append(dt * 1e6)
            else:
                kw = dict(cluster_location=cl_loc, cluster_capacity=cl_cap, max_jobs_considered=mjc, seed=seed, carry=A.QueueCarry(usage=True))
                t0 = time.perf_counter()
                got = cycle_run_kube_multi(es, [kw] * n) if n > 1 else [es[0].cycle_run_kube(**kw)]
                t_b.append((time.perf_counter() - t0) * 1e6)
                if turn == 1:
                    lists_b += [[l.tolist() for l in g["lists"]] for g in got]
                    kstats = es[0].batch_stats() if n > 1 else None
    # Leg (a) re-uploads the unchanged user state where leg (b) carries the launched jobs' usage: the two legs consider the same jobs only
    # because open_state limits nobody.  Under that state the launch lists of the two first episodes must be identical.
    same = [[[int(t) for t in l] for l in a] for a in lists_a] == lists_b
    assert same, "the launch lists of the two legs differ"
    es[0].set_profiling(True)
    for e in es:
        e.cycle_run(mjc)
    kw = dict(cluster_location=cl_loc, cluster_capacity=cl_cap, max_jobs_considered=mjc, seed=1, carry=A.QueueCarry(usage=True))
    cycle_run_kube_multi(es, [kw] * n) if n > 1 else es[0].cycle_run_kube(**kw)
    kt = es[0].kernel_timings().get("kube_distribute", (0.0, 0))
    return dict(bench="kube_cycle", pools=label, max_jobs_considered=mjc, clusters=n_cl, queue_cycles_per_episode=n_steps,
                baseline_us_host_distribution_not_counted=spread(t_a), baseline_us_host_distribution_counted=spread(t_a_host),
                run_kube_us=spread(t_b), identical_lists_first_episode=same, kube_distribute_kernel_us=round(kt[0] * 1e3, 1),
                kube_distribute_launches=kt[1], batch_stats_run_kube_multi=kstats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", action="store_true")
    ap.add_argument("--small", action="store_true", help="small synthetic pools (a dry run of --cycles)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    rows = []
    if a.cycles:
        if a.small:
            from cook_amd import synth
            c4 = [synth.make_pool(seed=50 + i, n_pending=3000, n_running=300, n_users=20, n_offers=8) for i in range(3)]
            sizes = (100,)
        else:
            from cook_amd import workload
            spec = workload.ClusterSpec()
            c4 = [workload.make_pool(spec, p) for p in range(spec.pools)]
            sizes = (500, 50000)
        for label, pools in (("one C4 pool", c4[:1]), ("%d C4 pools" % len(c4), c4)):
            for mjc in sizes:
                for n_cl in (3, 32):
                    row = cycle_legs(pools, label, mjc, n_cl, a.steps, a.lib)
                    print(json.dumps(row), flush=True)
                    rows.append(row)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)
        return
    e = Engine(A.default_params(), lib_path=a.lib)
    for K in (500, 50000):
        for n in (3, 32):
            for shape in ("ample", "tight"):
                rng = np.random.default_rng(K + n)
                cl_loc = np.zeros(n, np.uint32)
                cl_cap = np.full(n, KC.BIG, np.int64) if shape == "ample" else rng.integers(1, max(2, (3 * K) // (2 * n)), n).astype(np.int64)
                loc = np.zeros(K, np.uint32)
                draw = rng.random(K)
                for source, dr in (("draws", draw), ("seed", None)):
                    call = lambda: e.kube_distribute(K, cl_loc, cl_cap, loc, dr, seed=7)  # noqa: E731
                    t0 = time.perf_counter()
                    want = O.distribute(K, cl_loc, cl_cap, loc, dr, seed=7)
                    oracle_us = (time.perf_counter() - t0) * 1e6
                    KC.compare(call(), want, (K, n, shape, source))
                    us = timed(call, a.steps)
                    e.set_profiling(True)
                    before = e.kernel_timings().get("kube_distribute", (0.0, 0))
                    for _ in range(a.steps):
                        call()
                    after = e.kernel_timings()["kube_distribute"]
                    e.set_profiling(False)
                    row = dict(bench="kube_distribute", jobs=K, clusters=n, capacities=shape, draws=source, call_us=us,
                               kernel_us=round((after[0] - before[0]) * 1e3 / max(1, after[1] - before[1]), 1), launches_per_call=(after[1] - before[1]) / a.steps,
                               exhaustions=want["info"]["exhaustions"], no_cluster=want["info"]["no_cluster"], python_oracle_us=round(oracle_us, 1))
                    print(json.dumps(row), flush=True)
                    rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
