"""A Python restatement of what trigger-autoscaling! (scheduler.clj:1178-1202) does with the autoscaling candidates: steps 6-9 of
cook_cycle_autoscale_clusters (include/cookmatch.h).  Written from the reference's text, one job at a time and in its order, with Python
lists and dicts; it shares nothing with the engine.  Composed behind tests/autoscale_cases.oracle by tests/autoscale_cluster_cases.py.

  job->acceptable-compute-clusters (:1059-1076): the clusters whose location equals the job's last checkpoint location, in the
      collection's order; every cluster when the job has none.
  distribute-jobs-to-compute-clusters (:1078-1103): group-by of (nth acceptable (mod (hash uuid) (count acceptable))), or
      :no-acceptable-compute-cluster; group-by keeps the jobs' order; the first ten jobs without a cluster are logged.
  autoscale! (kubernetes/compute_cluster.clj:606-731): max-launchable = (min (- max-pods-outstanding num-synthetic-pods)
      (- max-total-nodes total-nodes) (- max-total-pods total-pods)); the jobs with an outstanding synthetic pod in the cluster are
      removed, (take max-launchable) of the rest are launched; not (pos? max-launchable): none."""
from __future__ import annotations

import uuid as _uuid

NO_CLUSTER = "no-acceptable-compute-cluster"


def java_uuid_hash(u: _uuid.UUID) -> int:
    """java.util.UUID.hashCode, which Clojure's (hash uuid) returns: hilo = mostSigBits ^ leastSigBits; ((int)(hilo >> 32)) ^ (int) hilo"""
    msb, lsb = u.int >> 64, u.int & (2 ** 64 - 1)
    hilo = msb ^ lsb
    v = ((hilo >> 32) ^ hilo) & 0xFFFFFFFF
    return v - 2 ** 32 if v >= 2 ** 31 else v


def acceptable_clusters(job_location, cluster_locations):
    """-> indices into the cluster collection.  job_location 0 / None: the job has no last checkpoint location; a cluster's location 0 /
    None: it has none, which equals no job's"""
    if not job_location:
        return list(range(len(cluster_locations)))
    return [c for c, loc in enumerate(cluster_locations) if loc and loc == job_location]


def choose_cluster(job_hash, acceptable):
    if not acceptable:
        return NO_CLUSTER
    return acceptable[job_hash % len(acceptable)]  # Python's % is Clojure's mod: the sign of the divisor


def distribute(jobs, cluster_locations):
    """jobs: [(task, location, hash)] in candidate order -> ({cluster: [task]}, [tasks without a cluster])"""
    by = {}
    for task, loc, h in jobs:
        by.setdefault(choose_cluster(int(h), acceptable_clusters(int(loc), cluster_locations)), []).append(int(task))
    none = by.pop(NO_CLUSTER, [])
    return by, none


def max_launchable(cl, c):
    return min(int(cl["max_pods_outstanding"][c]) - int(cl["num_synthetic_pods"][c]), int(cl["max_total_nodes"][c]) - int(cl["total_nodes"][c]),
               int(cl["max_total_pods"][c]) - int(cl["total_pods"][c]))


def autoscale_cut(tasks, outstanding, ml):
    """-> (launched, removed as outstanding)"""
    pods = set(int(t) for t in outstanding)
    new_jobs = [t for t in tasks if t not in pods]
    return (new_jobs[:ml] if ml > 0 else []), len(tasks) - len(new_jobs)


def clusters_oracle(out_tasks, location_of_task, hash_of_task, cl):
    """out_tasks: Out as task indices; location_of_task / hash_of_task: callables; cl: dict of the cluster columns (location, the six
    counts, outstanding: per cluster a list of task indices, or None).  -> (launch lists per cluster, cluster info dicts, no_cluster dict)"""
    n = len(cl["location"])
    by, none = distribute([(t, location_of_task(t), hash_of_task(t)) for t in out_tasks], [int(x) for x in cl["location"]])
    lists, info = [], []
    for c in range(n):
        tasks = by.get(c, [])
        ml = max_launchable(cl, c)
        launched, removed = autoscale_cut(tasks, cl["outstanding"][c] if cl.get("outstanding") is not None else [], ml)
        lists.append(launched)
        info.append(dict(assigned=len(tasks), outstanding_removed=removed, max_launchable=ml, launched=len(launched)))
    return lists, info, dict(no_cluster=len(none), first_tasks=none[:10])
