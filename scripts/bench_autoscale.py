"""Measures cook_cycle_autoscale (the pending-job candidates of handle-resource-offers-autoscaling-helper on the device) after one
cycle of a C4 pool at K = 1000, and after the eight C4 pools of the timed configuration (cook_cycle_run_rank_multi +
cook_cycle_match_multi), called one pool after another: wall-clock microseconds per call as the host sees it (median of --steps; the
call includes its readback of m, the filters' own synchronisations and the copy of the result).  Beside it the CPU leg: the oracle's
considerable over the masked queue Q' (built on the host), on one thread.  Every result is checked against the oracle of
tests/autoscale_cases.py.  One JSON line per configuration.  --multi adds the eight pools through ONE cook_cycle_autoscale_multi (the
pools' flows in one pool batch) beside the same pools one after another: same build, same process, same engines, the results compared.
--clusters N adds cook_cycle_autoscale_clusters (the distribution to N compute clusters and the cut per cluster, an outstanding list of
about a tenth of the candidates) beside cook_cycle_autoscale on the same engines, with the sum of its kernels from per-kernel event
timing, checked against tests/distribute_oracle.py.  --max-jobs / --scale-factor / --skip-all set the call's operating point (the
low-match one: --max-jobs 50000 --scale-factor 1000 --skip-all, N in the tens of thousands).
    python scripts/bench_autoscale.py [--steps 50] [--multi] [--clusters 3] [--out results/autoscale.json]"""
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


def clusters_leg(engines, pools, got, kws, n_clusters, steps, multi):
    """cook_cycle_autoscale_clusters on the engines as they stand: -> the extra fields of the row"""
    from cook_amd.engine import cycle_autoscale_clusters_multi
    from tests import autoscale_cluster_cases as CC
    cls, hashes = [], []
    for i, (e, pl, (out, _)) in enumerate(zip(engines, pools, got)):
        rng = np.random.default_rng(900 + i)
        h = rng.integers(-2 ** 31, 2 ** 31, pl.pending_jobs.n).astype(np.int32)
        e.cycle_set_job_hashes(h)
        hashes.append(h)
        outst = [sorted(int(t) for t in rng.choice(out, size=min(len(out), max(1, len(out) // (10 * n_clusters))), replace=False)) if len(out) else [] for _ in range(n_clusters)]
        room = max(1, len(out) // (2 * n_clusters))  # half of an even share: every list is cut
        cls.append(CC.clusters_of(np.zeros(n_clusters, np.uint32), [(room, 0, CC.BIG, 0, CC.BIG, 0)] * n_clusters, outst))
    one = lambda: [e.cycle_autoscale_clusters(cl, **kw) for e, cl, kw in zip(engines, cls, kws)]  # noqa: E731
    us = timed(one, steps)
    res = one()
    for pl, h, cl, (out, info), r in zip(pools, hashes, cls, got, res):
        CC.compare(r, *CC.distribute_out(pl, h, cl, out), info)
    names = ("as_outstanding_flags", "as_choose_cluster", "as_bin_scan", "as_partition_scatter")
    ksum, reps = 0.0, 10
    for e in engines:
        e.set_profiling(True)
    before = [e.kernel_timings() for e in engines]
    for _ in range(reps):
        one()
    for e, b in zip(engines, before):
        t = e.kernel_timings()
        ksum += sum(t[n][0] - b.get(n, (0.0, 0))[0] for n in names if n in t) / reps
        e.set_profiling(False)
    extra = {"clusters": n_clusters, "clusters_us_all_pools": round(us, 1), "clusters_us_per_call": round(us / len(pools), 1),
             "clusters_kernel_sum_us_all_pools": round(ksum * 1e3, 1), "launched": [int(sum(len(x) for x in r[0])) for r in res],
             "outstanding": [int(sum(len(x) for x in cl.outstanding)) for cl in cls], "clusters_parity": "oracle"}
    if multi:
        calls = [dict(clusters=cl, **kw) for cl, kw in zip(cls, kws)]
        mus = timed(lambda: cycle_autoscale_clusters_multi(engines, calls), steps)
        for a, b in zip(res, cycle_autoscale_clusters_multi(engines, calls)):
            S._same(a, b)
        extra["clusters_us_all_pools_multi"] = round(mus, 1)
        extra["clusters_batch"] = engines[0].batch_stats()
    return extra


def run(name, pools, steps, multi=False, call=None, n_clusters=0):
    call = call or {}
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
        kws = [dict(call, offer_skipped=np.ones(pl.offers.n, np.uint8)) if call.get("offer_skipped") == "all" else call for pl in pools]
        us = timed(lambda: [e.cycle_autoscale(**kw) for e, kw in zip(engines, kws)], steps)
        got = [e.cycle_autoscale(**kw) for e, kw in zip(engines, kws)]
        multi_us = stats = None
        if multi:  # the two legs alternate, so that neither has the warmer caches or the quieter moment
            none = kws
            multi_us = timed(lambda: cycle_autoscale_multi(engines, none), steps)
            stats = engines[0].batch_stats()
            us = min(us, timed(lambda: [e.cycle_autoscale(**kw) for e, kw in zip(engines, kws)], steps))
            multi_us = min(multi_us, timed(lambda: cycle_autoscale_multi(engines, none), steps))
            for (out, info), (m_out, m_info) in zip(got, cycle_autoscale_multi(engines, none)):
                assert np.array_equal(out, m_out) and info == m_info, (info, m_info)
        cpu_us = 0.0
        for e, pl, (st, el), (out, info) in zip(engines, pools, states, got):
            _, j2o, _ = e.cycle_fetch()
            o_out, o_info, d = S.oracle(params, pl, st, K, el, j2o=j2o, **kws[engines.index(e)])
            assert np.array_equal(out, o_out) and info == o_info, (info, o_info)
            t0 = time.perf_counter()
            pyoracle.considerable(d.queue2, st, info["scaled"])
            cpu_us += (time.perf_counter() - t0) * 1e6
        cl_extra = clusters_leg(engines, pools, got, kws, n_clusters, steps, multi) if n_clusters else {}
    finally:
        for e in engines:
            e.close()
    infos = [g[1] for g in got]
    extra = {"us_all_pools_multi": round(multi_us, 1), "multi_speedup": round(us / multi_us, 2), "batch": stats} if multi else {}
    return {**extra, **cl_extra, "config": name, "pools": len(pools), "K": K, "pending": int(sum(pl.pending_jobs.n for pl in pools)),
            "us_per_call": round(us / len(pools), 1), "us_all_pools": round(us, 1), "cpu_leg_us": round(cpu_us / len(pools), 1),
            "cpu_leg_us_all_pools": round(cpu_us, 1), "speedup_vs_cpu": round(cpu_us / us, 1), "parity": "oracle",
            "matched": [i["matched"] for i in infos], "scaled": [i["scaled"] for i in infos], "n_out": [i["n_out"] for i in infos]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--multi", action="store_true", help="also the eight pools through one cook_cycle_autoscale_multi")
    ap.add_argument("--clusters", type=int, default=0, help="also cook_cycle_autoscale_clusters with this many compute clusters")
    ap.add_argument("--max-jobs", type=int, default=None)
    ap.add_argument("--scale-factor", type=float, default=None)
    ap.add_argument("--skip-all", action="store_true", help="offer_skipped all ones: no match is kept")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    call = {}
    if args.max_jobs is not None:
        call["max_jobs"] = args.max_jobs
    if args.scale_factor is not None:
        call["scale_factor"] = args.scale_factor
    if args.skip_all:
        call["offer_skipped"] = "all"
    spec = workload.ClusterSpec()
    c4 = [workload.make_pool(spec, p) for p in range(spec.pools)]
    rows = [run("C4 pool, K = 1000", c4[:1], args.steps, call=call, n_clusters=args.clusters),
            run("C4 x 8 after cook_cycle_match_multi, one call per pool", c4, args.steps, multi=args.multi, call=call, n_clusters=args.clusters)]
    for r in rows:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
