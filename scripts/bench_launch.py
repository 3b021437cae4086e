"""Measures cook_match_launch_resources (the assigned ports and the per-role takes of the last match's placed tasks, on the device)
behind a match cycle of one C4 pool at K = 1000 considered jobs and at K = all pending jobs: 2 roles ("cook", "*"), 2 slots (cpus, mem),
a tenth of the jobs asking for 1 to 3 ports, two port ranges per host.  Per configuration: wall-clock microseconds per call as the host
sees it (median and min-max of --steps; the call includes its uploads, its two synchronisations and the copies of the results), the sum
of its kernels' times from per-kernel event timing in a second pass (and of those, the chains and the ports' expansion), and, reported
apart and for scale only, the same arithmetic by tests/launch_oracle.py's numpy-free Python on one thread — which says nothing about the
JVM's compile-mesos-messages, which is not measured.  The result is compared with the oracle, bit for bit.  One JSON line per
configuration.
    python scripts/bench_launch.py [--steps 30] [--small] [--out results/launch.json]"""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cook_amd import _abi as A  # noqa: E402
from cook_amd.engine import Engine  # noqa: E402
from tests import launch_cases as LC  # noqa: E402
from tests import launch_oracle as O  # noqa: E402

ROLES, NAMES = ["cook", "*"], ["cpus", "mem"]
PORTS_PER_RANGE = 500


def timed(fn, steps):
    fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    ts.sort()
    return dict(median=round(ts[len(ts) // 2], 1), min=round(ts[0], 1), max=round(ts[-1], 1))


def with_ports(pool, seed):
    """a tenth of the pending jobs ask for 1 to 3 ports; every host offers the ports of its two ranges"""
    rng = np.random.default_rng(seed)
    J, o = pool.pending_jobs, pool.offers
    ports = np.where(rng.random(J.n) < 0.1, rng.integers(1, 4, J.n), 0).astype(np.int32)
    pool.pending_jobs = dataclasses.replace(J, ports=ports)
    pool.offers = dataclasses.replace(o, ports=np.full(o.n, 2 * PORTS_PER_RANGE, np.int32))
    return pool


def role_view(offers, seed):
    """the hosts' role view as columns, and the same as the oracle's dicts: "cook" holds 10 to 60 % of a host's cpus / mem, "*" the
    rest; the "*" range comes first and lies above the "cook" range (a slice across both is not ascending)"""
    rng = np.random.default_rng(seed)
    M = offers.n
    share = np.round(rng.uniform(0.1, 0.6, (2, M)), 2)
    total = np.stack([offers.cpus, offers.mem])
    cook = total * share
    avail = np.stack([cook, total - cook], axis=1)  # [slot, role, row]
    begin = np.stack([np.full(M, 31000), np.full(M, 2000)], axis=1).astype(np.int32)  # per row: the "*" range, then the "cook" range
    rows = A.LaunchOffers(n=M, n_roles=2, range_off=(2 * np.arange(M + 1)).astype(np.uint32), range_begin=begin.reshape(-1),
                          range_end=(begin + PORTS_PER_RANGE - 1).reshape(-1), range_role=np.tile(np.asarray([1, 0], np.uint8), M),
                          res_source=np.asarray([A.LAUNCH_CPUS, A.LAUNCH_MEM], np.uint32), avail=avail)
    hosts = []
    for v in range(M):
        lease = [{"begin": int(begin[v, 0]), "end": int(begin[v, 0]) + PORTS_PER_RANGE - 1}, {"begin": int(begin[v, 1]), "end": int(begin[v, 1]) + PORTS_PER_RANGE - 1}]
        hosts.append({"resources": {"cpus": {"cook": float(avail[0, 0, v]), "*": float(avail[0, 1, v])},
                                    "mem": {"cook": float(avail[1, 0, v]), "*": float(avail[1, 1, v])}, "ports": {"*": [lease[0]], "cook": [lease[1]]}},
                      "lease-ranges": lease})
    return rows, hosts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="a small synthetic pool (a dry run)")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.small:
        from cook_amd import synth
        pool = synth.make_pool(seed=50, n_pending=3000, n_running=300, n_users=20, n_offers=40)
        sizes = (("100", 100), ("all", 3000))
    else:
        from cook_amd import workload
        spec = workload.ClusterSpec()
        pool = workload.make_pool(spec, 0)
        sizes = (("1000", 1000), ("all", pool.pending_jobs.n))
    pool = with_ports(pool, 7)
    rows, hosts = role_view(pool.offers, 8)
    out = []
    with Engine(A.default_params(good_enough_fitness=1.0), lib_path=a.lib) as e:
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        for label, k in sizes:
            e.cycle_run(k)
            j2o, jrows = LC.cycle_rows(e, pool)
            call = lambda: e.match_launch_resources(rows)  # noqa: E731
            got = call()
            tasks = LC.oracle_tasks(pool.pending_jobs, j2o, jrows, NAMES)
            t0 = time.perf_counter()
            result, bad = O.launch(hosts, tasks)
            oracle_us = (time.perf_counter() - t0) * 1e6
            assert bad is None
            LC.compare(got, O.as_arrays(result, NAMES, ROLES), "K = " + label)
            us = timed(call, a.steps)
            e.set_profiling(True)
            for _ in range(a.steps):
                call()
            kt = e.kernel_timings()
            e.set_profiling(False)
            per = lambda names: round(sum(ms for nm, (ms, _) in kt.items() if names(nm)) * 1e3 / a.steps, 1)  # noqa: E731
            row = dict(bench="launch_resources", pool="one C4 pool", considered=len(j2o), K=label, offers=pool.offers.n, info=got["info"],
                       roles=2, slots=2, call_us=us, kernels_us=per(lambda nm: True), chains_kernel_us=per(lambda nm: nm == "lr_take_chains"),
                       ports_kernel_us=per(lambda nm: nm == "lr_emit_ports"), launches_per_call=sum(n for _, n in kt.values()) / a.steps,
                       python_oracle_us=round(oracle_us, 1))
            print(json.dumps(row), flush=True)
            out.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
