"""CPU restatement of the three reasons of cook.unscheduled/reasons that need the user's whole task list, for the tests of
cook_unscheduled: how-job-would-exceed-resource-limits (unscheduled.clj:37-55), check-exceeds-limit (:57-77) and check-queue-position
(:128-158), over dicts.

A task is a dict {row, user, priority, start, task, job, pending, cpus, mem, gpus}.  A user's rows are sorted HERE by
task->feature-vector (tools.clj:614-632): -priority, start time with Long.MAX_VALUE for a pending row, task id with nil first for a
pending row, job id — running and pending rows TOGETHER (a pending row of higher priority stands before a running row).  Where the
reference depends on Datomic's order the engine's oracle-defined order holds (include/cookmatch.h): running-jobs is the user's running
rows in that task order, (conj running-jobs job) puts the job last, and Python floats are added left to right.  job->usage always
carries :gpus here (0.0 where the table has no gpus column); the reference leaves the key out of a job without gpus, which adds
nothing to a sum."""
from __future__ import annotations

from typing import Optional

import numpy as np

from cook_amd import _abi as A

LONG_MAX = 2 ** 63 - 1
KEYS = A.UNSCHED_RESOURCES  # ("count", "cpus", "mem", "gpus")
QUOTA_BIT = {"count": A.UNSCHED_QUOTA_COUNT, "cpus": A.UNSCHED_QUOTA_CPUS, "mem": A.UNSCHED_QUOTA_MEM, "gpus": A.UNSCHED_QUOTA_GPUS}
SHARE_BIT = {"cpus": A.UNSCHED_SHARE_CPUS, "mem": A.UNSCHED_SHARE_MEM, "gpus": A.UNSCHED_SHARE_GPUS}


def feature_vector(t):
    """task->feature-vector as a Python sort key (nil sorts first: (False, 0) < (True, id))"""
    return (-t["priority"], LONG_MAX if t["pending"] else t["start"], (False, 0) if t["pending"] else (True, t["task"]), t["job"])


def job_usage(job):
    """tools.clj:883-889 job->usage"""
    return {"count": 1, "cpus": job["cpus"], "mem": job["mem"], "gpus": job["gpus"]}


def merge_with_plus(a, b):
    out = dict(a)
    for k, v in b.items():
        out[k] = out[k] + v if k in out else v
    return out


def how_job_would_exceed_resource_limits(limits, running_jobs, job):
    """unscheduled.clj:37-55 -> ({k {limit, usage}} of the exceeded keys, the total usage)"""
    jobs_with_new = list(running_jobs) + [job]  # (conj running-jobs job) of a vector
    usages = [job_usage(j) for j in jobs_with_new]
    total = usages[0]
    for u in usages[1:]:  # (reduce (partial merge-with +) usages): no initial value, left to right
        total = merge_with_plus(total, u)
    ways = {k: {"limit": v, "usage": total.get(k)} for k, v in limits.items() if (total.get(k) or 0) > v}
    return ways, total


def check_exceeds_limit(limits, job, running_jobs):
    """unscheduled.clj:57-77: waiting jobs only"""
    if not job["pending"]:
        return None, None
    return how_job_would_exceed_resource_limits(limits, running_jobs, job)


def check_queue_position(job, running_tasks, pending_tasks):
    """unscheduled.clj:128-158 -> (queue_pos, at_least, tasks_ahead, len(all_tasks)); the reason exists iff tasks_ahead is non-empty"""
    all_tasks = list(running_tasks) + list(pending_tasks)
    sorted_tasks = sorted(all_tasks, key=feature_vector)
    pos = next((i for i, t in enumerate(sorted_tasks) if t["row"] == job["row"]), None)
    queue_pos = pos if pos is not None else len(all_tasks)
    return queue_pos, queue_pos == len(all_tasks), sorted_tasks[:min(queue_pos, 10)], len(all_tasks)


def task_dicts(tasks: A.Tasks):
    g = tasks.gpus if tasks.gpus is not None and len(tasks.gpus) == tasks.n else None
    return [dict(row=i, user=int(tasks.user[i]), priority=int(tasks.priority[i]), start=int(tasks.start_ms[i]), task=int(tasks.task_id[i]),
                 job=int(tasks.job_id[i]), pending=bool(tasks.pending[i]), cpus=float(tasks.cpus[i]), mem=float(tasks.mem[i]),
                 gpus=float(g[i]) if g is not None else 0.0) for i in range(tasks.n)]


def unscheduled_literal(tasks: A.Tasks, n_users: int, lim: A.UnschedLimits, in_window: Optional[np.ndarray] = None, rows=None) -> dict:
    """what Engine.unscheduled returns, computed job by job the way the reference answers one request (small tables: every job sorts
    its user's list and sums its user's running jobs again)"""
    ts = task_dicts(tasks)
    by_user = {}
    for t in ts:
        by_user.setdefault(t["user"], []).append(t)
    running, waiting = {}, {}
    for u, l in by_user.items():
        l.sort(key=feature_vector)
        running[u] = [t for t in l if not t["pending"]]
        waiting[u] = [t for t in l if t["pending"] and (in_window is None or in_window[t["row"]])]
    ask = list(range(tasks.n)) if rows is None else [int(r) for r in rows]
    n = len(ask)
    reasons, qpos, total = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros((n, 4))
    ahead = np.full((n_users, A.UNSCHED_AHEAD), A.NONE_U32, np.uint32)
    list_len = np.zeros(n_users, np.uint32)
    for u in by_user:
        _, _, first, length = check_queue_position({"row": -1}, running[u], waiting[u])  # (a job outside the list sees its head)
        list_len[u] = length
        ahead[u, :len(first)] = [t["row"] for t in first]
    for k, r in enumerate(ask):
        job = ts[r]
        u = job["user"]
        bits = 0
        quota = {"count": lim.quota_count[u], "cpus": lim.quota_cpus[u], "mem": lim.quota_mem[u], "gpus": lim.quota_gpus[u]}
        share = {"cpus": lim.share_cpus[u], "mem": lim.share_mem[u], "gpus": lim.share_gpus[u]}
        ways, tot = check_exceeds_limit(quota, job, running[u])
        if tot is not None:
            total[k] = [float(tot[x]) for x in KEYS]
            for x in ways:
                bits |= QUOTA_BIT[x]
            for x in check_exceeds_limit(share, job, running[u])[0]:
                bits |= SHARE_BIT[x]
        p, at_least, tasks_ahead, _ = check_queue_position(job, running[u], waiting[u])
        assert [t["row"] for t in tasks_ahead] == [int(x) for x in ahead[u, :min(p, 10)]]  # the tasks ahead are a prefix of the user's list
        bits |= (A.UNSCHED_QUEUE_POSITION if tasks_ahead else 0) | (A.UNSCHED_AT_LEAST if at_least else 0)
        reasons[k], qpos[k] = bits, p
    return dict(reasons=reasons, queue_pos=qpos, total=total, ahead=ahead, list_len=list_len)


def unscheduled(tasks: A.Tasks, n_users: int, lim: A.UnschedLimits, in_window: Optional[np.ndarray] = None, rows=None) -> dict:
    """the same numbers for tables of any size: every user's list is sorted once and its running usage summed once (np.cumsum adds
    left to right, and the reduce's last step, + the job, is one more addition).  The cases compare it with unscheduled_literal on
    every small table."""
    n = tasks.n
    pend = tasks.pending.astype(bool)
    g = tasks.gpus if tasks.gpus is not None and len(tasks.gpus) == n else np.zeros(n)
    start = np.where(pend, LONG_MAX, tasks.start_ms)
    task = np.where(pend, 0, tasks.task_id)  # (nil first: the third key is (is-running, id))
    order = np.lexsort((tasks.job_id, task, ~pend, start, -tasks.priority.astype(np.int64), tasks.user))
    listed = ~pend | (np.ones(n, bool) if in_window is None else np.asarray(in_window).astype(bool))
    pos = np.zeros(n, np.int64)       # row -> list entries in front of it
    base = np.zeros((n_users, 4))     # the user's running usage, left to right
    ahead = np.full((n_users, A.UNSCHED_AHEAD), A.NONE_U32, np.uint32)
    list_len = np.zeros(n_users, np.uint32)
    su = tasks.user[order]
    bounds = np.flatnonzero(np.r_[True, su[1:] != su[:-1], True]) if n else np.zeros(1, np.int64)
    for a, b in zip(bounds[:-1], bounds[1:]):
        u, seg = int(su[a]), order[a:b]
        l = listed[seg]
        c = np.cumsum(l)
        pos[seg] = np.where(l, c - 1, c[-1])
        list_len[u] = c[-1]
        head = seg[l][:A.UNSCHED_AHEAD]
        ahead[u, :len(head)] = head
        run = seg[~pend[seg]]
        if len(run):
            base[u] = [len(run), np.cumsum(tasks.cpus[run])[-1], np.cumsum(tasks.mem[run])[-1], np.cumsum(g[run])[-1]]
    ask = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    u = tasks.user[ask].astype(np.int64)
    own = np.stack([np.ones(len(ask)), tasks.cpus[ask], tasks.mem[ask], g[ask]], axis=1) if len(ask) else np.zeros((0, 4))
    has_run = (base[u, 0] > 0)[:, None] if len(ask) else np.zeros((0, 1), bool)
    total = np.where(has_run, base[u] + own, own)
    p = pend[ask]
    total[~p] = 0.0
    quota = np.stack([lim.quota_count, lim.quota_cpus, lim.quota_mem, lim.quota_gpus], axis=1)[u] if len(ask) else np.zeros((0, 4))
    share = np.stack([lim.share_cpus, lim.share_mem, lim.share_gpus], axis=1)[u] if len(ask) else np.zeros((0, 3))
    reasons = np.zeros(len(ask), np.uint32)
    for k, x in enumerate(KEYS):
        reasons |= np.where(p & (total[:, k] > quota[:, k]), QUOTA_BIT[x], 0).astype(np.uint32)
        if x in SHARE_BIT:
            reasons |= np.where(p & (total[:, k] > share[:, k - 1]), SHARE_BIT[x], 0).astype(np.uint32)
    qpos = pos[ask].astype(np.uint32)
    reasons |= np.where(qpos > 0, A.UNSCHED_QUEUE_POSITION, 0).astype(np.uint32)
    reasons |= np.where(~listed[ask], A.UNSCHED_AT_LEAST, 0).astype(np.uint32)
    return dict(reasons=reasons, queue_pos=qpos, total=total, ahead=ahead, list_len=list_len)


def assert_same(got: dict, want: dict):
    """every output with == on the bit patterns: there is no tolerance anywhere"""
    for k in ("reasons", "queue_pos", "ahead", "list_len"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (k, np.flatnonzero((got[k] != want[k]).reshape(len(want[k]), -1).any(axis=1))[:8])
    g, w = np.ascontiguousarray(got["total"]).view(np.uint64), np.ascontiguousarray(want["total"]).view(np.uint64)
    assert g.shape == w.shape and np.array_equal(g, w), ("total", np.flatnonzero((g != w).any(axis=1))[:8])


def pairwise_sum(xs):
    """a tree sum (halves), the order a parallel reduction would use"""
    if len(xs) <= 2:
        return sum(xs[1:], xs[0]) if xs else 0.0
    h = len(xs) // 2
    return pairwise_sum(xs[:h]) + pairwise_sum(xs[h:])


def users_whose_cpus_sum_depends_on_order(tasks: A.Tasks):
    """the users whose running cpus give another sum as a tree than left to right in the user's task order: such a user's prefixes
    cannot all be exact, so the engine has to take its fold path for it"""
    by_user = {}
    for t in task_dicts(tasks):
        if not t["pending"]:
            by_user.setdefault(t["user"], []).append(t)
    out = []
    for u, l in by_user.items():
        xs = [t["cpus"] for t in sorted(l, key=feature_vector)]
        seq = xs[0]
        for x in xs[1:]:
            seq = seq + x
        if pairwise_sum(xs) != seq:
            out.append(u)
    return out
