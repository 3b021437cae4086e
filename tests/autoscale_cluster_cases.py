"""The cases of cook_cycle_set_job_hashes / cook_cycle_autoscale_clusters(_multi), shared by the emulator (test_autoscale_clusters_emu.py)
and GPU (test_autoscale_clusters_gpu.py) suites.  The oracle is tests/distribute_oracle.py composed behind tests/autoscale_cases.oracle:
that one gives Out, this one distributes and cuts it.  Every launch list, offset, cluster info and no-cluster field is compared element
for element.  Shapes are the smallest that can go wrong: candidate counts around a wave (63, 64, 65) and a block of the partition
(AS_THREADS = 256: 257, and 513 for a third block), cluster counts 1, 2, 3 and COOK_MAX_CLUSTERS."""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from cook_amd import _abi as A
from cook_amd import synth
from cook_amd.engine import CookError, _ClusterCall, cycle_autoscale_clusters_multi, cycle_autoscale_multi, cycle_match_multi, cycle_run_queue_multi
from tests import autoscale_cases as S
from tests import distribute_oracle as D
from tests import followup_cases as F
from tests.parity_cases import _concat_jobs

COOK_E_INVALID, COOK_E_STATE = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
BIG = 10 ** 6


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def clusters_of(location, caps=None, outstanding=None):
    """caps: per cluster (max_pods_outstanding, num_synthetic_pods, max_total_nodes, total_nodes, max_total_pods, total_pods); None: no cut"""
    n = len(location)
    caps = np.asarray(caps if caps is not None else [(BIG, 0, BIG, 0, BIG, 0)] * n, dtype=np.int64).reshape(n, 6)
    return A.AutoscaleClusters(np.asarray(location, np.uint32), *[caps[:, i].copy() for i in range(6)], outstanding=outstanding)


def as_dict(cl):
    d = {c: getattr(cl, c) for c in ("location",) + A.CLUSTER_COLUMNS}
    d["outstanding"] = cl.outstanding
    return d


def make_case(seed, n_pending, n_running, n_users, n_offers, n_locations=3):
    """a synthetic pool whose jobs carry last checkpoint locations (0 = none for a third), and one hash per pending job with the int32
    extremes among them"""
    pool = synth.make_pool(seed=seed, n_pending=n_pending, n_running=n_running, n_users=n_users, n_offers=n_offers)
    rng = np.random.default_rng(seed + 7)
    loc = rng.integers(1, n_locations + 1, n_pending).astype(np.uint32)
    loc[rng.random(n_pending) < 0.34] = 0
    pool.pending_jobs.ckpt_location = loc
    pool.offers.location = rng.integers(1, n_locations + 1, n_offers).astype(np.uint32)
    h = rng.integers(INT32_MIN, INT32_MAX + 1, n_pending).astype(np.int32)
    h[: min(n_pending, 4)] = [-1, 0, INT32_MIN, INT32_MAX][: min(n_pending, 4)]
    return pool, h


def random_clusters(pool, seed, n, n_locations=3, cut=True, frac_outstanding=0.1, max_room=40):
    rng = np.random.default_rng(seed + 11)
    loc = rng.integers(0, n_locations + 1, n)  # (0: a cluster without a location takes only jobs without one)
    caps = [(BIG, 0, BIG, 0, BIG, 0)] * n
    if cut:
        caps = []
        for c in range(n):
            which, room = int(rng.integers(0, 4)), int(rng.integers(0, max_room))
            row = [BIG, int(rng.integers(0, 50)), BIG, int(rng.integers(0, 50)), BIG, int(rng.integers(0, 50))]
            if which < 3:
                row[2 * which] = row[2 * which + 1] + room  # that cap binds: max_launchable = room
            caps.append(tuple(row))
    pend = np.flatnonzero(pool.tasks.pending == 1)
    outstanding = [sorted(int(t) for t in rng.choice(pend, size=int(len(pend) * frac_outstanding), replace=False)) if len(pend) else []
                   for _ in range(n)]
    if pool.tasks.n > len(pend):  # an in-range index that is no candidate (a running task): ignored
        outstanding[0].append(int(np.flatnonzero(pool.tasks.pending == 0)[0]))
    return clusters_of(loc, caps, outstanding)


# ---- the oracle, composed ---------------------------------------------------------------------------------------------------------
def distribute_out(pool, hashes, cl, out):
    pend_ord = np.cumsum(pool.tasks.pending) - 1
    loc = pool.pending_jobs.ckpt_location
    return D.clusters_oracle([int(t) for t in out], (lambda t: int(loc[pend_ord[t]])) if loc is not None else (lambda t: 0),
                             lambda t: int(hashes[pend_ord[t]]), as_dict(cl))


def expected(params, pool, st, k, eligible, hashes, cl, j2o, **kw):
    out, info, _ = S.oracle(params, pool, st, k, eligible, **kw, j2o=j2o)
    return (*distribute_out(pool, hashes, cl, out), info, out)


def compare(got, want_lists, want_cinfo, want_none, want_info, tag=""):
    lists, info, cinfo, none = got
    assert len(lists) == len(want_lists), tag
    for c, (g, w) in enumerate(zip(lists, want_lists)):
        assert g.dtype == np.uint32 and g.tolist() == w, (tag, "cluster", c, g.tolist()[:8], w[:8])
    assert cinfo == want_cinfo, (tag, cinfo, want_cinfo)
    assert none == want_none, (tag, none, want_none)
    assert info == want_info, (tag, info, want_info)


def open_cycle(e, pool, k, hashes=None):
    """a cycle under no limit at all: with every match dropped (offer_skipped all ones) and scale_factor 0, Out is the first k jobs of the queue"""
    e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
    e.cycle_set_considerable(S.open_state(pool.users.n), np.ones(pool.pending_jobs.n, np.uint8))
    if hashes is not None:
        e.cycle_set_job_hashes(hashes)
    e.cycle_run(k)


def open_kw(pool):
    return dict(max_jobs=1, scale_factor=0.0, offer_skipped=np.ones(pool.offers.n, np.uint8))


def check_call(e, params, pool, st, eligible, k, hashes, cl, kw, tag=""):
    _, j2o, _ = e.cycle_fetch()
    lists, cinfo, none, info, out = expected(params, pool, st, k, eligible, hashes, cl, j2o, **kw)
    compare(e.cycle_autoscale_clusters(cl, **kw), lists, cinfo, none, info, tag)
    return lists, cinfo, none, out


# ---- golden cases (tests/golden/autoscale_clusters.json) -------------------------------------------------------------------------------
def load_golden():
    with open(os.path.join(ROOT, "tests", "golden", "autoscale_clusters.json")) as f:
        return json.load(f)["cases"]


def golden_clusters(case):
    cs = case["clusters"]
    caps = [[c.get(k, d) for k, d in zip(A.CLUSTER_COLUMNS, (BIG, 0, BIG, 0, BIG, 0))] for c in cs]
    return [c["name"] for c in cs], [c["location"] for c in cs], caps


def check_golden_oracle():
    """the oracle alone against the hand-encoded expectations"""
    cases = load_golden()
    assert len(cases) >= 15
    for case in cases:
        cnames, loc, caps = golden_clusters(case)
        jobs = case["jobs"]
        if "accepts" in case:
            for j in jobs:
                assert [cnames[c] for c in D.acceptable_clusters(j["location"], loc)] == case["accepts"][j["name"]], case["name"]
        outstanding = [[i for i, j in enumerate(jobs) if j["name"] in c.get("outstanding", [])] for c in case["clusters"]]
        cl = as_dict(clusters_of(loc, caps, outstanding))
        lists, cinfo, none = D.clusters_oracle(range(len(jobs)), lambda t: jobs[t]["location"], lambda t: jobs[t]["hash"], cl)
        got = {cnames[c]: [jobs[t]["name"] for t in lists[c]] for c in range(len(cnames))}
        if "expect" in case:
            assert got == case["expect"], (case["name"], got)
        if "expect_non_empty_lists" in case:
            assert sum(1 for v in got.values() if v) == case["expect_non_empty_lists"], (case["name"], got)
            assert sorted(x for v in got.values() for x in v) == sorted(j["name"] for j in jobs), case["name"]
        assert none["no_cluster"] == case.get("expect_no_cluster", 0), case["name"]
        if "expect_max_launchable" in case:
            assert [i["max_launchable"] for i in cinfo] == case["expect_max_launchable"], case["name"]


def check_golden(make_engine):
    """the same cases through the engine: a pool of as many pending jobs as the case has, nothing matches, Out is the whole queue; golden
    job i is the i-th job of Out (the queue's order is read from a first cycle)"""
    params = A.default_params()
    for case in load_golden():
        cnames, loc, caps = golden_clusters(case)
        jobs = case["jobs"]
        n = len(jobs)
        pool = synth.make_pool(seed=700, n_pending=n, n_running=3, n_users=2, n_offers=2)
        pend_ord = np.cumsum(pool.tasks.pending) - 1
        with make_engine(params) as e:
            open_cycle(e, pool, n)
            order, _ = e.cycle_autoscale(**open_kw(pool))
            assert len(order) == n
            ckpt, hashes = np.zeros(n, np.uint32), np.zeros(n, np.int32)
            for i, t in enumerate(order):
                ckpt[pend_ord[t]], hashes[pend_ord[t]] = jobs[i]["location"], jobs[i]["hash"]
            pool.pending_jobs.ckpt_location = ckpt
            outstanding = [[int(order[i]) for i, j in enumerate(jobs) if j["name"] in c.get("outstanding", [])] for c in case["clusters"]]
            cl = clusters_of(loc, caps, outstanding)
            open_cycle(e, pool, n, hashes)
            name_of = {int(t): jobs[i]["name"] for i, t in enumerate(order)}
            lists, _, cinfo, none = e.cycle_autoscale_clusters(cl, **open_kw(pool))
            w_lists, w_cinfo, w_none = distribute_out(pool, hashes, cl, order)
            assert [x.tolist() for x in lists] == w_lists and cinfo == w_cinfo and none == w_none, case["name"]
            got = {cnames[c]: [name_of[int(t)] for t in lists[c]] for c in range(len(cnames))}
            if "expect" in case:
                assert got == case["expect"], (case["name"], got)
            assert none["no_cluster"] == case.get("expect_no_cluster", 0), case["name"]
            assert [name_of[t] for t in none["first_tasks"]] == [j["name"] for j in jobs if j["name"] in case.get("expect_first", [])][:10]


# ---- candidate counts x cluster counts ---------------------------------------------------------------------------------------------------
COUNTS = (1, 63, 64, 65, 257, 513)  # a wave, a block of the partition (256 candidates), a third block


def check_counts(make_engine):
    params = A.default_params()
    pool, hashes = make_case(710, n_pending=600, n_running=40, n_users=9, n_offers=6)
    st, el = S.open_state(pool.users.n), np.ones(pool.pending_jobs.n, np.uint8)
    with make_engine(params) as e:
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        e.cycle_set_considerable(st, el)
        e.cycle_set_job_hashes(hashes)
        for i, k in enumerate(COUNTS):
            e.cycle_run(k)
            for n_cl in ((1, 2, 3, 32) if k in (65, 257) else ((1, 2, 3, 32)[i % 4],)):
                cl = random_clusters(pool, 720 + k + n_cl, n_cl)
                lists, cinfo, none, out = check_call(e, params, pool, st, el, k, hashes, cl, open_kw(pool), tag=(k, n_cl))
                assert len(out) == k
            # every candidate excluded: Out is empty on the device only
            cl = random_clusters(pool, 730 + k, 3)
            got = e.cycle_autoscale_clusters(cl, exclude_tasks=out, **open_kw(pool))
            assert [len(x) for x in got[0]] == [0, 0, 0] and got[1]["n_out"] == 0 and got[1]["autoscalable"] == k
            assert all(i["assigned"] == 0 and i["launched"] == 0 for i in got[2]) and got[3] == dict(no_cluster=0, first_tasks=[])
            # ... and every second one
            kw = dict(open_kw(pool), exclude_tasks=out[::2])
            check_call(e, params, pool, st, el, k, hashes, cl, kw, tag=(k, "excluded"))
    # no candidate at all: a pool without pending jobs
    empty, _ = make_case(711, n_pending=0, n_running=20, n_users=4, n_offers=4)
    with make_engine(params) as e:
        open_cycle(e, empty, 10, np.zeros(0, np.int32))
        cl = random_clusters(empty, 712, 3)
        lists, info, cinfo, none = e.cycle_autoscale_clusters(cl)
        assert [len(x) for x in lists] == [0, 0, 0] and info["n_out"] == 0 and none == dict(no_cluster=0, first_tasks=[])
        assert [i["max_launchable"] for i in cinfo] == [D.max_launchable(as_dict(cl), c) for c in range(3)]


def check_simple_shapes(make_engine):
    """one cluster gets every job in candidate order; two clusters of one location with hashes that send every job to the second"""
    params = A.default_params()
    pool, hashes = make_case(740, n_pending=300, n_running=10, n_users=5, n_offers=4)
    k = 270
    with make_engine(params) as e:
        open_cycle(e, pool, k, hashes)
        out, _ = e.cycle_autoscale(**open_kw(pool))
        lists, _, cinfo, none = e.cycle_autoscale_clusters(clusters_of([0]), **open_kw(pool))
        no_loc = [int(t) for t in out if pool.pending_jobs.ckpt_location[(np.cumsum(pool.tasks.pending) - 1)[t]] == 0]
        assert lists[0].tolist() == no_loc and none["no_cluster"] == k - len(no_loc)  # (a cluster without a location: the jobs without one)
        pool.pending_jobs.ckpt_location = None
        odd = (hashes | 1).astype(np.int32)
        open_cycle(e, pool, k, odd)
        lists, _, cinfo, none = e.cycle_autoscale_clusters(clusters_of([5]), **open_kw(pool))
        assert lists[0].tolist() == out.tolist() and cinfo[0]["assigned"] == k and none["no_cluster"] == 0
        lists, _, cinfo, none = e.cycle_autoscale_clusters(clusters_of([5, 5]), **open_kw(pool))
        assert len(lists[0]) == 0 and lists[1].tolist() == out.tolist() and [i["assigned"] for i in cinfo] == [0, k]


# ---- random pools: the full filter chain in front, three calls each ---------------------------------------------------------------------
RANDOM_CASES = [(811, 2, 40), (812, 3, 40), (813, 32, 3)]  # (seed, clusters, room of a binding cap): seeds that meet the precondition below


def check_random(make_engine, seed, n_clusters, n_pending=700, n_running=300, n_users=20, n_offers=30, k=250, max_room=40):
    params = A.default_params(good_enough_fitness=1.0)
    pool, hashes = make_case(seed, n_pending, n_running, n_users, n_offers)
    st, el = S.random_state(pool, seed)
    cl = random_clusters(pool, seed, n_clusters, max_room=max_room)
    with make_engine(params) as e:
        S.run_cycle(e, pool, st, k, el)
        e.cycle_set_job_hashes(hashes)
        for kw in S.random_calls(pool, seed, k, 3):
            lists, cinfo, none, out = check_call(e, params, pool, st, el, k, hashes, cl, kw, tag=(seed, n_clusters))
            if kw.get("exclude_tasks") is None and kw["max_jobs"] == 1000:
                # the precondition of a random case, on the oracle alone: it is a case that cuts, removes and spreads
                assert sum(1 for i in cinfo if i["assigned"] >= 2) >= min(2, n_clusters), (seed, cinfo)
                assert any(i["launched"] < i["assigned"] - i["outstanding_removed"] for i in cinfo), (seed, cinfo)
                assert any(i["outstanding_removed"] > 0 for i in cinfo), (seed, cinfo)


# ---- the hash column: refusals, cook_cycle_update, a stage ---------------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(CookError) as ex:
        fn()
    return ex.value.code


def check_hash_column(make_engine):
    params = A.default_params()
    pool, hashes = make_case(750, n_pending=200, n_running=60, n_users=6, n_offers=5)
    st, el = S.open_state(pool.users.n), np.ones(pool.pending_jobs.n, np.uint8)
    P, k = pool.pending_jobs.n, 150
    cl = random_clusters(pool, 751, 3)
    kw = open_kw(pool)
    with make_engine(params) as e:
        assert _code(lambda: e.cycle_set_job_hashes(hashes)) == COOK_E_STATE  # in front of any stage
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        e.cycle_set_considerable(st, el)
        e.cycle_run(k)
        assert _code(lambda: e.cycle_autoscale_clusters(cl, **kw)) == COOK_E_STATE  # no hashes yet
        e.cycle_set_job_hashes(hashes[:120])
        assert _code(lambda: e.cycle_autoscale_clusters(cl, **kw)) == COOK_E_STATE  # 120 of 200 rows
        # each refusal leaves the column as it was: the full column written afterwards from row 120 gives the oracle's result
        assert _code(lambda: e.cycle_set_job_hashes(hashes[:10], first=P - 5)) == COOK_E_INVALID   # past the pending count
        assert _code(lambda: e.cycle_set_job_hashes(hashes[:1], first=P + 1)) == COOK_E_INVALID
        assert _code(lambda: e.cycle_set_job_hashes(hashes[121:], first=121)) == COOK_E_INVALID    # a gap behind the set prefix
        assert _code(lambda: e.cycle_autoscale_clusters(cl, **kw)) == COOK_E_STATE
        e.cycle_set_job_hashes(hashes[120:], first=120)
        first = e.cycle_autoscale_clusters(cl, **kw)
        check_call(e, params, pool, st, el, k, hashes, cl, kw, tag="set in two parts")
        e.cycle_set_job_hashes(hashes[50:60], first=50)  # rows inside the prefix may be written again
        assert _code(lambda: e.cycle_set_job_hashes(hashes[:3], first=P - 2)) == COOK_E_INVALID
        S._same(e.cycle_autoscale_clusters(cl, **kw), first)
        # ---- a delta: pending rows removed in front, running and pending rows appended ------------------------------------------------
        pend = np.flatnonzero(pool.tasks.pending == 1)
        removed = [int(pend[0]), int(pend[1]), int(pend[7]), int(np.flatnonzero(pool.tasks.pending == 0)[0])]
        extra, xh = make_case(752, n_pending=9, n_running=2, n_users=6, n_offers=1)
        e.cycle_update(remove_task=removed, add_tasks=extra.tasks, add_pending=extra.pending_jobs)
        e.cycle_run(k)
        assert _code(lambda: e.cycle_autoscale_clusters(cl, **kw)) == COOK_E_STATE  # the appended rows are unset
        kept = P - 3
        assert _code(lambda: e.cycle_set_job_hashes(xh, first=kept + 1)) == COOK_E_INVALID
        e.cycle_set_job_hashes(xh, first=kept)
        after = e.cycle_autoscale_clusters(cl, **kw)
        # ... equal to a full restage of the pool the delta leaves
        keep_t = np.setdiff1d(np.arange(pool.tasks.n), removed)
        keep_p = np.setdiff1d(np.arange(P), (np.cumsum(pool.tasks.pending) - 1)[removed[:3]])
        T, X = pool.tasks, extra.tasks
        cols = ("cpus", "mem", "user", "priority", "start_ms", "task_id", "job_id", "pending")
        merged = SimpleNamespace(tasks=A.Tasks(**{c: np.concatenate([getattr(T, c)[keep_t], getattr(X, c)]) for c in cols}), users=pool.users,
                                 pending_jobs=_concat_jobs(pool.pending_jobs.take(keep_p), extra.pending_jobs), offers=pool.offers,
                                 groups=pool.groups)
        h2 = np.concatenate([hashes[keep_p], xh]).astype(np.int32)
        with make_engine(params) as e2:
            open_cycle(e2, merged, k, h2)
            S._same(e2.cycle_autoscale_clusters(cl, **kw), after)
            check_call(e2, params, merged, st, np.ones(merged.pending_jobs.n, np.uint8), k, h2, cl, kw, tag="restaged")
        # ---- a stage drops the column ---------------------------------------------------------------------------------------------------
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        e.cycle_set_considerable(st, el)
        e.cycle_run(k)
        assert _code(lambda: e.cycle_autoscale_clusters(cl, **kw)) == COOK_E_STATE
        assert _code(lambda: e.cycle_set_job_hashes(hashes[1:], first=1)) == COOK_E_INVALID  # nothing is set: row 0 would be a gap
        e.cycle_set_job_hashes(hashes)
        S._same(e.cycle_autoscale_clusters(cl, **kw), first)


def raw_call(e, call):
    return e._lib.cook_cycle_autoscale_clusters(e._h, C.byref(call.p), C.byref(call.cl), call.out.ctypes.data_as(C.c_void_p), call.cap,
                                                call.off.ctypes.data_as(C.c_void_p), C.byref(call.info), call.cinfo, C.byref(call.none))


def check_refusals(make_engine):
    """the call's own refusals: each leaves the engine as it was (the next good call gives what the first gave)"""
    params = A.default_params()
    pool, hashes = make_case(760, n_pending=120, n_running=30, n_users=5, n_offers=4)
    cl = random_clusters(pool, 761, 3)
    kw = open_kw(pool)
    with make_engine(params) as e:
        assert _code(lambda: e.cycle_autoscale_clusters(cl)) == COOK_E_STATE  # the state rule of cook_cycle_autoscale
        open_cycle(e, pool, 100, hashes)
        first = e.cycle_autoscale_clusters(cl, **kw)
        old = e.cycle_autoscale(**kw)

        def bad(**ch):
            c2 = clusters_of(cl.location, np.stack([getattr(cl, c) for c in A.CLUSTER_COLUMNS], axis=1), [list(x) for x in cl.outstanding])
            for k_, v in ch.items():
                setattr(c2, k_, v)
            return c2
        assert _code(lambda: e.cycle_autoscale_clusters(random_clusters(pool, 1, 33), **kw)) == COOK_E_INVALID  # n out of range
        empty = A.AutoscaleClusters(*[np.zeros(0, np.int64)] * 7)
        assert _code(lambda: e.cycle_autoscale_clusters(empty, **kw)) == COOK_E_INVALID
        assert _code(lambda: e.cycle_autoscale_clusters(bad(outstanding=[[pool.tasks.n], [], []]), **kw)) == COOK_E_INVALID  # index out of range
        call = _ClusterCall(e, dict(clusters=cl, **kw))
        call.keep[-2][1] = call.keep[-2][2] + 1  # out_off[1] > out_off[2]: it decreases
        assert raw_call(e, call) == COOK_E_INVALID
        assert _code(lambda: e.cycle_autoscale_clusters(cl, scale_factor=float("nan"))) == COOK_E_INVALID   # cook_cycle_autoscale's own
        assert _code(lambda: e.cycle_autoscale_clusters(cl, exclude_tasks=[pool.tasks.n])) == COOK_E_INVALID
        # the launch lists exceed cap: refused, the info still filled
        total = sum(len(x) for x in first[0])
        assert total > 1
        with pytest.raises(CookError) as ex:
            e.cycle_autoscale_clusters(cl, cap=total - 1, **kw)
        assert ex.value.code == COOK_E_INVALID
        call = _ClusterCall(e, dict(clusters=cl, cap=total - 1, **kw))
        rc = raw_call(e, call)
        assert rc == COOK_E_INVALID and call.info.as_dict() == first[1] and [call.cinfo[c].as_dict() for c in range(3)] == first[2]
        # cap = the lists' length suffices although |Out| is larger
        assert first[1]["n_out"] > total
        S._same(e.cycle_autoscale_clusters(cl, cap=total, **kw), first)
        S._same(e.cycle_autoscale(**kw), old)  # the old call on the same engine: exactly what it returned before


def check_cycle_undisturbed(make_engine):
    """as autoscale_cases.check_cycle_undisturbed: every fetch after the call is the one before it, the next update + cycle too"""
    pool, hashes = make_case(770, n_pending=500, n_running=300, n_users=25, n_offers=20)
    st, eligible = S.random_state(pool, 6, fractional=True)
    cl = random_clusters(pool, 771, 3)
    removed = [int(np.flatnonzero(pool.tasks.pending == 0)[0])]
    nxt = []
    for with_call in (False, True):
        with make_engine(A.default_params()) as e:
            S.run_cycle(e, pool, st, 200, eligible)
            before = S._snapshot(e, pool.users.n)
            old = e.cycle_autoscale()
            if with_call:
                e.cycle_set_job_hashes(hashes)
                e.cycle_autoscale_clusters(cl)
                e.cycle_autoscale_clusters(cl, max_jobs=5, scale_factor=0.5, offer_skipped=np.ones(pool.offers.n, np.uint8), exclude_tasks=before[0][:7])
                S._same(S._snapshot(e, pool.users.n), before)
                S._same(e.cycle_autoscale(), old)
            e.cycle_update(remove_task=removed)
            e.cycle_run(200)
            nxt.append((S._snapshot(e, pool.users.n), e.cycle_autoscale()))
    S._same(nxt[0], nxt[1])


# ---- the multi form -----------------------------------------------------------------------------------------------------------------------
MULTI_SHAPES = [(500, 300, 20, 30, 3), (300, 100, 12, 200, 32), (260, 20, 4, 8, 1)]


def multi_inputs(seed=780):
    cases = [make_case(seed + i, npd, nr, nu, no) for i, (npd, nr, nu, no, _) in enumerate(MULTI_SHAPES)]
    pools, hashes = [c[0] for c in cases], [c[1] for c in cases]
    states = [S.random_state(pl, seed + 10 + i) for i, pl in enumerate(pools)]
    cls = [random_clusters(pl, seed + 20 + i, shp[4]) for i, (pl, shp) in enumerate(zip(pools, MULTI_SHAPES))]
    cls[0].location = np.array([1, 2, 3], np.uint32)  # every location a job may have: no job without a cluster
    cls[2] = clusters_of([9], [(5, 0, BIG, 0, BIG, 0)], cls[2].outstanding)  # a location no job has: every job with one counts as no_cluster
    calls = [dict(clusters=cl, **kw) for cl, kw in zip(cls, [S.random_calls(pl, seed + 30 + i, 150, 3)[i] for i, pl in enumerate(pools)])]
    return pools, hashes, states, cls, calls


def run_multi(make_engine, queue_cycle=False, seed=780):
    """three pools with different cluster counts and different steps (a default call, a scaled one, one with exclusions and skipped offers),
    one of them with no_cluster jobs -> the multi results, each compared with the single call on the same engine and with the oracle"""
    pools, hashes, states, cls, calls = multi_inputs(seed)
    params = A.default_params(good_enough_fitness=1.0, match_algo=2)
    with F.Pools(make_engine, pools, params, states, 150) as P:
        if queue_cycle:
            cycle_run_queue_multi(P.engines, 150)
            cycle_match_multi(P.engines)
        for e, h in zip(P.engines, hashes):
            e.cycle_set_job_hashes(h)
        got = cycle_autoscale_clusters_multi(P.engines, calls)
        for i, (e, pl, h, call) in enumerate(zip(P.engines, pools, hashes, calls)):
            S._same(e.cycle_autoscale_clusters(**call), got[i])
            kw = {a: b for a, b in call.items() if a != "clusters"}
            out, info = e.cycle_autoscale(**kw)  # (a queue cycle's Out is test_queue's business; a rank cycle's is checked below)
            if not queue_cycle:
                _, j2o, _ = e.cycle_fetch()
                o_out, o_info, _ = S.oracle(params, pl, states[i][0], 150, states[i][1], **kw, j2o=j2o)
                assert np.array_equal(out, o_out) and info == o_info
            compare(got[i], *distribute_out(pl, h, call["clusters"], out), info, tag=("multi", i))
        assert got[2][3]["no_cluster"] > 0 and got[0][3]["no_cluster"] == 0
        assert len({len(g[0]) for g in got}) == 3
    return got


def check_multi_one_refused(make_engine, seed=790):
    pools, hashes, states, cls, calls = multi_inputs(seed)
    params = A.default_params(good_enough_fitness=1.0, match_algo=2)
    with F.Pools(make_engine, pools, params, states, 150) as P:
        for i, (e, h) in enumerate(zip(P.engines, hashes)):
            e.cycle_set_job_hashes(h if i != 1 else h[:-1])  # the middle engine's column misses a row
        single = [P.engines[i].cycle_autoscale_clusters(**calls[i]) for i in (0, 2)]
        got = cycle_autoscale_clusters_multi(P.engines, calls, raise_errors=False)
        assert isinstance(got[1], CookError) and got[1].code == COOK_E_STATE and "cook_cycle_set_job_hashes" in str(got[1])
        S._same([got[0], got[2]], single)
        with pytest.raises(CookError):
            cycle_autoscale_clusters_multi(P.engines, calls)
        assert cycle_autoscale_clusters_multi([], []) == []
        with pytest.raises(CookError):
            cycle_autoscale_clusters_multi([P.engines[0], P.engines[0]], calls[:2])  # an engine twice: the whole call is refused


def jsonable(got):
    return [[[x.tolist() for x in g[0]], g[1], g[2], g[3]] for g in got]


_CHILD = r'''
import json, sys
sys.path.insert(0, %r)
from tests import autoscale_cluster_cases as CC
from cook_amd.engine import Engine
so = sys.argv[1]
if so == "emu":
    from tests.simt_emu import build_emu
    so = build_emu.build()
    make = lambda p: Engine(p, lib_path=so)
else:
    make = lambda p: Engine(p)
print(json.dumps(CC.jsonable(CC.run_multi(make))))
''' % ROOT


def check_multi_unbatched_child(got, emu):
    """COOK_RANK_BATCH=0 in a fresh child process: the engines one after another, the same results"""
    env = {k: v for k, v in os.environ.items() if k not in ("COOK_SYNC_TRACE", "COOK_BATCH_TRACE")}
    r = subprocess.run([sys.executable, "-c", _CHILD, "emu" if emu else "gpu"], env={**env, "COOK_RANK_BATCH": "0"}, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == json.loads(json.dumps(jsonable(got)))


def check_sync_count(make_engine):
    """the call makes exactly the stream synchronisations cook_cycle_autoscale makes on the same inputs: the pool batches' counters
    (cook_batch_stats), every buffer brought to its size by the single calls first (test_followups_batch_structure does the same)"""
    pool, hashes = make_case(800, n_pending=400, n_running=150, n_users=12, n_offers=20)
    st = S.random_state(pool, 801, pool_quota=True)
    cl = random_clusters(pool, 802, 3)
    rng = np.random.default_rng(803)
    n = 2
    with F.Pools(make_engine, [pool] * n, A.default_params(good_enough_fitness=1.0, match_algo=2), [st] * n, 120) as P:
        for with_exclude in (True, False):
            kw = dict(max_jobs=400, scale_factor=2.0, offer_skipped=(rng.random(pool.offers.n) < 0.3).astype(np.uint8))
            if with_exclude:
                kw["exclude_tasks"] = F.exclusions(P, 0, kw)
            for e in P.engines:
                e.cycle_set_job_hashes(hashes)
                e.cycle_autoscale(**kw), e.cycle_autoscale_clusters(cl, **kw)
            old = cycle_autoscale_multi(P.engines, [kw] * n)
            s_old = P.engines[0].batch_stats()
            new = cycle_autoscale_clusters_multi(P.engines, [dict(clusters=cl, **kw)] * n)
            s_new = P.engines[0].batch_stats()
            assert old[0][1]["n_out"] > 0 and sum(len(x) for x in new[0][0]) > 0
            assert s_old["pools"] == s_new["pools"] == n and s_new["syncs"] == s_old["syncs"] > 0, (s_old, s_new)
            assert s_new["grouped_launches"] == s_new["launches"] > s_old["launches"], (s_old, s_new)  # identical flows: every kernel once for both pools
