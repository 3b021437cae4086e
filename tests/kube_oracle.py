"""A job-by-job restatement of the Kubernetes-scheduler pool's gate and distributor, written from the reference's text
(handle-kubernetes-scheduler-pool, scheduler.clj:1747-1810; scheduling-capacity-constrained-job-distributor, :1110-1151), with the
draw of rand-nth as an input.  Plain Python integers and one float multiply per job; no numpy on the decision path."""
from __future__ import annotations

import math

NO_CLUSTER = 0xFF
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
MASK64 = 2 ** 64 - 1


def splitmix64(x: int) -> int:
    z = (x + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def seed_draw(seed: int, k: int) -> float:
    """u_k of a call without a draw column: the top 53 bits of splitmix64(seed + k) scaled by 2^-53 (exact, in [0, 1))"""
    return float(splitmix64((seed + k) & MASK64) >> 11) * 2.0 ** -53


def available(capacity) -> int:
    """(reduce + capacities) of :1767 over the raw values, in int64, saturating"""
    s = 0
    for c in capacity:
        s += int(c)
        if s > INT64_MAX or s < INT64_MIN:
            s = INT64_MAX if int(c) > 0 else INT64_MIN
    return s


def gate(capacity, max_jobs_considered: int, min_capacity_threshold: int) -> dict:
    """:1767-1778: available = the capacities' sum; max_considerable = min(max-jobs-considered, max(available, 0)); the cycle runs iff
    available > threshold (strict), else it is paused"""
    av = available(capacity)
    return dict(available=av, max_considerable=min(int(max_jobs_considered), max(av, 0), 2 ** 32 - 1),
                paused=0 if av > int(min_capacity_threshold) else 1)


def rand_nth_index(m: int, u: float) -> int:
    """(int (* (count coll) (Math/random))): one float64 multiply, truncated; the clamp is never reached for u < 1"""
    return min(int(math.trunc(float(m) * u)), m - 1)


def distribute(n_jobs: int, cluster_location, capacity, location=None, draw=None, seed: int = 0, task=None) -> dict:
    """the jobs 0 .. n_jobs-1 one by one.  -> choice per job, the clusters' lists (positions, or task[k]), off, cluster_info, info"""
    n = len(cluster_location)
    assert len(capacity) == n
    cap = [int(c) for c in capacity]
    name = (lambda k: int(task[k])) if task is not None else (lambda k: k)
    choice, lists, none, exhaustions = [], [[] for _ in range(n)], [], 0
    for k in range(n_jobs):
        L = int(location[k]) if location is not None else 0
        acceptable = [c for c in range(n) if L == 0 or int(cluster_location[c]) == L]   # job->acceptable-compute-clusters
        avail = [c for c in acceptable if cap[c] > 0]                                   # (pos? capacity), :1128-1139
        if not avail:
            choice.append(NO_CLUSTER)                                                   # :no-acceptable-compute-cluster
            none.append(name(k))
            continue
        u = float(draw[k]) if draw is not None else seed_draw(seed, k)
        assert 0.0 <= u < 1.0
        c = avail[rand_nth_index(len(avail), u)]                                        # rand-nth, :1142
        cap[c] -= 1                                                                     # decrement-scheduling-capacity-counter
        exhaustions += cap[c] == 0
        choice.append(c)
        lists[c].append(name(k))                                                        # group-by keeps the jobs' order
    off = [0]
    for x in lists:
        off.append(off[-1] + len(x))
    return dict(choice=choice, lists=lists, off=off,
                cluster_info=[dict(assigned=len(lists[c]), capacity=int(capacity[c])) for c in range(n)],
                info=dict(paused=0, max_considerable=n_jobs, available=available(capacity), n_considered=n_jobs, launched=off[-1],
                          no_cluster=len(none), first_tasks=none[:10], exhaustions=exhaustions))
