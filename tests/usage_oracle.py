"""CPU restatement of GET /usage with its job-group breakdown for the tests of cook_usage_breakdown / cook_usage_breakdown_multi:
user-usage (rest/api.clj:2894-2915), no-usage-map (:2917-2923) and tools/total-resources-of-jobs (tools.clj:294-306), over dicts
(usage_literal), and a numpy form of the same numbers for the large tables (usage).

A job is a dict {engine, row, user, group, priority, start, task, job, cpus, mem, gpus}: a RUNNING row of a task table.  A user's jobs
are sorted HERE by task->feature-vector (tools.clj:614-632), engine by engine in the order of the engines.  Where the reference's
order is a hash map's or a Datomic query's the engine's oracle-defined order holds (include/cookmatch.h): users in id order, the
ungrouped bucket first, then the grouped ones in ascending group id, Python floats added left to right from 0.0."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from cook_amd import _abi as A

LONG_MAX = 2 ** 63 - 1
NONE = A.NONE_U32


def feature_vector(t):
    """task->feature-vector of a running row as a Python sort key"""
    return (-t["priority"], t["start"], t["task"], t["job"])


def total_resources_of_jobs(jobs):
    """tools.clj:294-306: (reduce (fn [acc job] (merge-with + acc (select-keys (job-ent->resources job) [:cpus :mem :gpus])))
    {:cpus 0.0 :mem 0.0 :gpus 0.0 :jobs (count jobs)} jobs)"""
    acc = {"cpus": 0.0, "mem": 0.0, "gpus": 0.0, "jobs": len(jobs)}
    for j in jobs:
        for k in ("cpus", "mem", "gpus"):
            acc[k] = acc[k] + j[k]
    return acc


def group_by(f, xs):
    out = {}
    for x in xs:
        out.setdefault(f(x), []).append(x)
    return out


def user_usage(jobs):
    """api.clj:2894-2915 with group_breakdown -> {total-usage, grouped: [(group id, rows, usage)] ascending, ungrouped: (rows, usage)}"""
    breakdowns = {g: ([(j["engine"], j["row"]) for j in js], total_resources_of_jobs(js)) for g, js in group_by(lambda j: j["group"], jobs).items()}
    grouped = [(g, rows, usage) for g, (rows, usage) in sorted((kv for kv in breakdowns.items() if kv[0] is not None), key=lambda kv: kv[0])]
    rows, usage = breakdowns.get(None, ([], None))
    return {"total-usage": total_resources_of_jobs(jobs), "grouped": grouped, "ungrouped": (rows, usage or total_resources_of_jobs([]))}


def jobs_of_users(pools, user_maps=None):
    """{user of the call: its running jobs}, the engines' parts one after the other, each sorted by the feature vector"""
    by_user = {}
    for e, (t, grp) in enumerate(pools):
        g = t.gpus if t.gpus is not None and len(t.gpus) == t.n else None
        mine = {}
        for i in range(t.n):
            if t.pending[i]:
                continue
            u = int(t.user[i])
            if user_maps is not None and user_maps[e] is not None:
                u = int(user_maps[e][u])
            gid = None if grp is None or int(grp[i]) == NONE else int(grp[i])
            mine.setdefault(u, []).append(dict(engine=e, row=i, user=u, group=gid, priority=int(t.priority[i]), start=int(t.start_ms[i]),
                                               task=int(t.task_id[i]), job=int(t.job_id[i]), cpus=float(t.cpus[i]), mem=float(t.mem[i]),
                                               gpus=float(g[i]) if g is not None else 0.0))
        for u, js in mine.items():
            by_user.setdefault(u, []).extend(sorted(js, key=feature_vector))
    return by_user


def _vec(u):
    return [u["cpus"], u["mem"], u["gpus"], float(u["jobs"])]


def usage_literal(pools: Sequence, n_users: int, user_maps=None, users=None, multi: bool = False) -> dict:
    """what Engine.usage_breakdown / usage_breakdown_multi return, user by user the way the reference answers a request.
    pools: [(Tasks, group_of_row or None)]."""
    by_user = jobs_of_users(pools, user_maps)
    ask = range(n_users) if users is None else [int(u) for u in users]
    boff, bgroup, busage, roff, rows, total = [0], [], [], [0], [], []
    for u in ask:
        r = user_usage(by_user.get(u, []))  # (no jobs: the no-usage-map, and user-usage of nothing is the same numbers)
        total.append(_vec(r["total-usage"]))
        buckets = ([(NONE,) + r["ungrouped"]] if r["ungrouped"][0] else []) + r["grouped"]
        for g, rs, us in buckets:
            bgroup.append(g)
            busage.append(_vec(us))
            rows.extend(rs)
            roff.append(len(rows))
        boff.append(len(bgroup))
    rw = np.array(rows, dtype=np.uint32).reshape(-1, 2)
    return dict(bucket_off=np.array(boff, np.uint32), bucket_group=np.array(bgroup, np.uint32),
                bucket_usage=np.array(busage, np.float64).reshape(-1, 4), row_off=np.array(roff, np.uint32),
                rows=rw if multi else rw[:, 1].copy(), total=np.array(total, np.float64).reshape(-1, 4))


def _seg_sums(vals, starts, ends):
    """per segment: 0.0 + v0 + v1 + ... left to right (np.add.accumulate is sequential; a trailing + 0.0 is the leading one: the two
    differ only when every value is -0.0)"""
    out = np.zeros(len(starts))
    ln = ends - starts
    one = ln == 1
    out[one] = vals[starts[one]]
    for i in np.flatnonzero(ln > 1):
        out[i] = np.add.accumulate(vals[starts[i]:ends[i]])[-1]
    return out + 0.0


def _concat(pools, user_maps):
    us, ks, es, rs, cs, ms, gs = [], [], [], [], [], [], []
    for e, (t, grp) in enumerate(pools):
        n = t.n
        pend = t.pending.astype(bool)
        order = np.lexsort((t.job_id, t.task_id, t.start_ms, -t.priority.astype(np.int64), t.user))
        order = order[~pend[order]]
        u = t.user[order].astype(np.int64)
        if user_maps is not None and user_maps[e] is not None:
            u = np.asarray(user_maps[e], dtype=np.int64)[u]
        g = np.full(n, NONE, np.uint32) if grp is None else np.asarray(grp, np.uint32)
        k = np.where(g[order] == NONE, 0, g[order].astype(np.int64) + 1)
        gp = t.gpus if t.gpus is not None and len(t.gpus) == n else np.zeros(n)
        us.append(u), ks.append(k), es.append(np.full(len(order), e, np.int64)), rs.append(order.astype(np.int64))
        cs.append(t.cpus[order]), ms.append(t.mem[order]), gs.append(gp[order])
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)  # noqa: E731
    return cat(us, np.int64), cat(ks, np.int64), cat(es, np.int64), cat(rs, np.int64), cat(cs, np.float64), cat(ms, np.float64), cat(gs, np.float64)


def usage(pools: Sequence, n_users: int, user_maps=None, users=None, multi: bool = False) -> dict:
    """the same numbers for tables of any size.  The cases compare it with usage_literal on every small table."""
    U, K, E, Rw, c, m, g = _concat(pools, user_maps)
    R = len(U)
    oT = np.argsort(U, kind="stable")  # (user, engine, task order): the order of the per-user total
    total = np.zeros((n_users, 4))
    if R:
        ut = U[oT]
        st = np.flatnonzero(np.r_[True, ut[1:] != ut[:-1]])
        en = np.r_[st[1:], R]
        for col, v in enumerate((c, m, g)):
            total[ut[st], col] = _seg_sums(v[oT], st, en)
        total[ut[st], 3] = en - st
    oS = np.lexsort((K, U))  # stable: (user, bucket key, engine, task order)
    us, ks = U[oS], K[oS]
    st = np.flatnonzero(np.r_[True, (us[1:] != us[:-1]) | (ks[1:] != ks[:-1])]) if R else np.zeros(0, np.int64)
    en = np.r_[st[1:], R] if R else np.zeros(0, np.int64)
    busage = np.zeros((len(st), 4))
    for col, v in enumerate((c, m, g)):
        busage[:, col] = _seg_sums(v[oS], st, en)
    busage[:, 3] = en - st
    bgroup = np.where(ks[st] == 0, NONE, ks[st] - 1).astype(np.uint32)
    boff = np.searchsorted(us[st], np.arange(n_users + 1), side="left").astype(np.uint32)
    roff = np.r_[st, R].astype(np.uint32)
    rows = np.stack([E[oS], Rw[oS]], axis=1).astype(np.uint32)
    if users is not None:
        ul = np.asarray(users, dtype=np.int64)
        bsel = np.concatenate([np.arange(boff[u], boff[u + 1]) for u in ul]).astype(np.int64) if len(ul) else np.zeros(0, np.int64)
        rsel = np.concatenate([np.arange(roff[boff[u]], roff[boff[u + 1]]) for u in ul]).astype(np.int64) if len(ul) else np.zeros(0, np.int64)
        nb = (boff[ul + 1] - boff[ul]).astype(np.int64) if len(ul) else np.zeros(0, np.int64)
        ln = (roff[1:] - roff[:-1]).astype(np.int64)[bsel]
        boff, roff = np.r_[0, np.cumsum(nb)].astype(np.uint32), np.r_[0, np.cumsum(ln)].astype(np.uint32)
        bgroup, busage, rows, total = bgroup[bsel], busage[bsel], rows[rsel], total[ul]
    return dict(bucket_off=boff, bucket_group=bgroup, bucket_usage=busage, row_off=roff, rows=rows if multi else rows[:, 1].copy(), total=total)


def assert_same(got: dict, want: dict, what=""):
    """every output with == on the bit patterns: there is no tolerance anywhere (-0.0 against 0.0 fails)"""
    for k in ("bucket_off", "bucket_group", "row_off", "rows"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k, got[k][:12], want[k][:12])
    for k in ("bucket_usage", "total"):
        g, w = np.ascontiguousarray(got[k]).view(np.uint64), np.ascontiguousarray(want[k]).view(np.uint64)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.flatnonzero((g != w).any(axis=1))
        assert len(bad) == 0, (what, k, bad[:8], np.asarray(got[k])[bad[:3]].tolist(), np.asarray(want[k])[bad[:3]].tolist())


def pairwise_sum(xs):
    """a tree sum (halves), the order a parallel reduction would use"""
    if len(xs) <= 2:
        return sum(xs[1:], xs[0]) if len(xs) else 0.0
    h = len(xs) // 2
    return pairwise_sum(xs[:h]) + pairwise_sum(xs[h:])


def _depends(vals):
    xs = [float(v) for v in vals]
    seq = 0.0
    for x in xs:
        seq = seq + x
    return np.float64(pairwise_sum(xs)).view(np.uint64) != np.float64(seq).view(np.uint64)


def sums_that_depend_on_order(pools, n_users, user_maps=None, limit=4):
    """-> (buckets, users) whose cpus, mem or gpus give another sum as a tree than left to right in the bucket's (the user's) order:
    such a bucket's prefixes cannot all be exact, so the engine has to take its fold path for it (at most `limit` of each are looked
    for)"""
    by_user = jobs_of_users(pools, user_maps)
    buckets, users = [], []
    for u in sorted(by_user):
        js = by_user[u]
        if len(users) < limit and any(_depends([j[k] for j in js]) for k in ("cpus", "mem", "gpus")):
            users.append(u)
        for gid, bj in group_by(lambda j: j["group"], js).items():
            if len(buckets) < limit and len(bj) > 2 and any(_depends([j[k] for j in bj]) for k in ("cpus", "mem", "gpus")):
                buckets.append((u, gid))
        if len(users) >= limit and len(buckets) >= limit:
            break
    return buckets, users
