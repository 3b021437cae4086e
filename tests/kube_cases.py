"""The cases of cook_kube_distribute and, further down, of cook_cycle_run_kube(_multi) / cook_cycle_fetch_kube, shared by the emulator (test_kube_emu.py) and GPU (test_kube_gpu.py) suites.  The oracle is
tests/kube_oracle.py, a job-by-job restatement of scheduling-capacity-constrained-job-distributor.  Every choice, list, offset, cluster
info and info field is compared element for element.  Shapes are the smallest that can go wrong: job counts around a wave (63, 64, 65)
and around the walk's tile T (T - 1, T, T + 1, 2T + 1), cluster counts 1, 2, 3 and COOK_MAX_CLUSTERS, and exhaustions at the places
where the walk changes its path (the first job, the last lane of a tile, the first lane of the next, two in one wave, all 32 in one
tile, the very last job)."""
from __future__ import annotations

import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from cook_amd import _abi as A
from cook_amd.engine import CookError
from tests import kube_oracle as O

COOK_E_INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = A.KUBE_TILE
BIG = 10 ** 6
SIZES = (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1)
CLUSTER_COUNTS = (1, 2, 3, A.MAX_CLUSTERS)


def engine(make_engine):
    return make_engine(A.default_params())


def compare(got, want, tag=""):
    assert got["choice"].dtype == np.uint8 and got["choice"].tolist() == want["choice"], (tag, got["choice"].tolist()[:16], want["choice"][:16])
    assert got["off"].tolist() == want["off"], (tag, got["off"].tolist(), want["off"])
    assert len(got["lists"]) == len(want["lists"]), tag
    for c, (g, w) in enumerate(zip(got["lists"], want["lists"])):
        assert g.dtype == np.uint32 and g.tolist() == w, (tag, "cluster", c, g.tolist()[:8], w[:8])
    assert got["cluster_info"] == want["cluster_info"], (tag, got["cluster_info"], want["cluster_info"])
    assert got["info"] == want["info"], (tag, got["info"], want["info"])


def check(e, K, cl_loc, cl_cap, loc=None, draw=None, seed=0, tag=""):
    want = O.distribute(K, cl_loc, cl_cap, loc, draw, seed)
    compare(e.kube_distribute(K, cl_loc, cl_cap, loc, draw, seed), want, tag)
    return want


# ---- golden cases (tests/golden/kube_distribute.json) -----------------------------------------------------------------------------------
def load_golden():
    with open(os.path.join(ROOT, "tests", "golden", "kube_distribute.json")) as f:
        return json.load(f)["cases"]


def golden_inputs(case):
    cl_loc = [c[0] for c in case["clusters"]]
    cl_cap = [c[1] for c in case["clusters"]]
    loc = [j[0] for j in case["jobs"]]
    draw = [float.fromhex(j[1]) if isinstance(j[1], str) else float(j[1]) for j in case["jobs"]]
    return cl_loc, cl_cap, loc, draw


def golden_expect(case):
    x, lists = case["expect"], case["expect"]["lists"]
    return dict(choice=x["choice"], lists=lists, no_cluster=x["no_cluster"], first_tasks=x["first_tasks"], exhaustions=x["exhaustions"],
                launched=sum(len(l) for l in lists))


def project(res):
    """a result (the oracle's, or the engine's as lists) onto the fields the golden file states"""
    i = res["info"]
    return dict(choice=[int(c) for c in res["choice"]], lists=[[int(t) for t in l] for l in res["lists"]], no_cluster=i["no_cluster"],
                first_tasks=i["first_tasks"], exhaustions=i["exhaustions"], launched=i["launched"])


def any_draw_holds(res, inv, tag):
    if "choice" in inv:
        assert [int(c) for c in res["choice"]] == inv["choice"], tag
    for k in ("launched", "no_cluster"):
        if k in inv:
            assert res["info"][k] == inv[k], (tag, k)


def check_golden_oracle():
    """the oracle alone against the hand-encoded expectations, the gate included, and the two draws the header derives by hand"""
    cases = load_golden()
    assert len(cases) >= 15 and sum("reference test" in c["name"] for c in cases) == 4
    for case in cases:
        cl_loc, cl_cap, loc, draw = golden_inputs(case)
        assert project(O.distribute(len(loc), cl_loc, cl_cap, loc, draw)) == golden_expect(case), case["name"]
        for seed in range(5):
            any_draw_holds(O.distribute(len(loc), cl_loc, cl_cap, loc, None, seed), case.get("any_draw", {}), case["name"])
        for (mjc, thr), (av, mc, paused) in case.get("gate", []):
            assert O.gate(cl_cap, mjc, thr) == dict(available=av, max_considerable=mc, paused=paused), (case["name"], mjc, thr)
    top = math.nextafter(1.0, 0.0)
    assert [O.rand_nth_index(m, top) for m in range(1, 33)] == list(range(32))  # no u < 1 reaches the clamp
    assert 3.0 * (1.0 / 3.0) == 1.0 and O.rand_nth_index(3, 1.0 / 3.0) == 1
    # splitmix64 against the published test vector of the generator (state 1234567: the first output is the function of 1234567)
    assert O.splitmix64(1234567) == 6457827717110365317 == A.splitmix64(1234567)
    assert all(O.seed_draw(s, k) == A.kube_seed_draw(s, k) and 0.0 <= O.seed_draw(s, k) < 1.0 for s in (0, 1, 2 ** 64 - 1) for k in range(20))


def check_golden(make_engine):
    e = engine(make_engine)
    for case in load_golden():
        cl_loc, cl_cap, loc, draw = golden_inputs(case)
        got = e.kube_distribute(len(loc), cl_loc, cl_cap, loc, draw)
        assert project(got) == golden_expect(case), case["name"]
        compare(got, O.distribute(len(loc), cl_loc, cl_cap, loc, draw), case["name"])
        for seed in range(5):
            any_draw_holds(e.kube_distribute(len(loc), cl_loc, cl_cap, loc, None, seed), case.get("any_draw", {}), case["name"])


# ---- sizes and cluster counts, both draw sources --------------------------------------------------------------------------------------
def sized_case(K, n, seed):
    """capacities that sum to about 3/4 of the jobs, a zero and a negative one among them when there is room: clusters run out on the way"""
    rng = np.random.default_rng(seed)
    cl_loc = rng.integers(0, 4, n).astype(np.uint32)
    cl_cap = rng.integers(0, max(2, (3 * K) // (2 * n) + 2), n).astype(np.int64)
    if n >= 3:
        cl_cap[1], cl_cap[2] = 0, -7
    loc = rng.integers(0, 4, K).astype(np.uint32)
    loc[rng.random(K) < 0.4] = 0
    return cl_loc, cl_cap, loc, rng.random(K)


def check_sizes(make_engine, n):
    e = engine(make_engine)
    for K in SIZES:
        cl_loc, cl_cap, loc, draw = sized_case(K, n, 1000 + 37 * K + n)
        check(e, K, cl_loc, cl_cap, loc, draw, tag=("draws", K, n))
        check(e, K, cl_loc, cl_cap, loc, None, seed=0xC0FFEE + K, tag=("seed", K, n))
        check(e, K, cl_loc, cl_cap, None, None, seed=2 ** 64 - 1 - K, tag=("no locations, seed + k wraps", K, n))


# ---- exhaustions where the walk changes its path ---------------------------------------------------------------------------------------
def check_exhaustion_places(make_engine):
    e = engine(make_engine)
    zeros = lambda K: np.zeros(K)  # u = 0: every job takes the first available cluster, so capacities place the exhaustions exactly
    # at the very first job
    w = check(e, 70, [0, 0], [1, BIG], draw=zeros(70), tag="first job")
    assert w["choice"][:2] == [0, 1] and w["info"]["exhaustions"] == 1
    # at the last lane of a tile / at the first lane of the second tile
    for cap0, tag in ((T, "last lane of a tile"), (T + 1, "first lane of the second tile")):
        w = check(e, T + 10, [0, 0], [cap0, BIG], draw=zeros(T + 10), tag=tag)
        assert w["choice"][cap0 - 1] == 0 and w["choice"][cap0] == 1 and w["info"]["exhaustions"] == 1
    # two clusters exhausting inside one wave, a third behind them
    w = check(e, 64, [0, 0, 0], [3, 5, BIG], draw=zeros(64), tag="two in a wave")
    assert w["choice"][:9] == [0] * 3 + [1] * 5 + [2] and w["info"]["exhaustions"] == 2
    # all 32 clusters (capacity 1 each) exhausting inside one tile: the pass bound ceil(K / T) + n is met exactly
    for draw, seed in ((zeros(40), 0), (np.random.default_rng(5).random(40), 0), (None, 77)):
        w = check(e, 40, [0] * 32, [1] * 32, draw=draw, seed=seed, tag="32 in a tile")
        assert w["info"]["exhaustions"] == 32 and w["info"]["no_cluster"] == 8 and sorted(w["choice"][:32]) == list(range(32))
    # ... and in the second tile, behind jobs that no cluster accepts
    loc = np.array([9] * (T + 3) + [0] * 40, np.uint32)
    w = check(e, T + 43, [0] * 32, [1] * 32, loc=loc, draw=None, seed=5, tag="32 in the second tile")
    assert w["info"]["exhaustions"] == 32 and w["info"]["no_cluster"] == T + 3 + 8 and w["info"]["first_tasks"] == list(range(10))
    # a capacity that is exactly met by the last job
    for K in (1, 100, T, T + 1):
        w = check(e, K, [0], [K], draw=None, seed=K, tag=("met by the last job", K))
        assert w["info"]["exhaustions"] == 1 and w["info"]["no_cluster"] == 0 and w["info"]["launched"] == K
    # total capacity far above n_jobs: no exhaustion occurs
    w = check(e, 2 * T + 1, [1, 2, 0], [BIG, 2 ** 40, 2 ** 62], loc=np.arange(2 * T + 1) % 3, draw=None, seed=3, tag="no exhaustion")
    assert w["info"]["exhaustions"] == 0 and w["info"]["available"] == BIG + 2 ** 40 + 2 ** 62
    # the capacities' sum saturates in int64
    w = check(e, 5, [0, 0], [2 ** 63 - 1, 2 ** 63 - 1], draw=None, seed=4, tag="the sum saturates")
    assert w["info"]["available"] == 2 ** 63 - 1
    w = check(e, 5, [0, 0, 0], [-2 ** 63, -2 ** 63, 3], draw=None, seed=4, tag="the sum saturates below")
    assert w["info"]["available"] == -2 ** 63 + 3 and w["info"]["launched"] == 3  # (every addition saturates, left to right)


# ---- seeded random cases ---------------------------------------------------------------------------------------------------------------
def random_case(seed, n):
    rng = np.random.default_rng(seed)
    K = int(rng.integers(T + 1, 3 * T))
    cl_loc = rng.integers(0, 3, n).astype(np.uint32)
    cl_cap = rng.integers(1, max(2, (3 * K) // (2 * n)), n).astype(np.int64)
    loc = rng.integers(0, 4, K).astype(np.uint32)  # (location 3: no cluster has it)
    loc[rng.random(K) < 0.5] = 0
    return K, cl_loc, cl_cap, loc, rng.random(K)


# (seed, clusters): chosen on the CPU so that the case's own oracle run meets random_precondition
RANDOM_CASES = ((9001, 3), (9002, 7), (9003, A.MAX_CLUSTERS))


def random_precondition(want):
    """at least two exhaustions, at least one job without a cluster, every cluster used"""
    return want["info"]["exhaustions"] >= 2 and want["info"]["no_cluster"] >= 1 and all(len(l) > 0 for l in want["lists"])


def check_random(make_engine, seed, n):
    K, cl_loc, cl_cap, loc, draw = random_case(seed, n)
    e = engine(make_engine)
    for dr, tag in ((draw, "draws"), (None, "seed")):
        want = check(e, K, cl_loc, cl_cap, loc, dr, seed=seed, tag=(tag, seed, n))
        assert random_precondition(want), (tag, seed, n, want["info"])


# ---- one launch ------------------------------------------------------------------------------------------------------------------------
def check_one_launch(make_engine):
    """the distribution and the lists are ONE launch of one kernel, whatever the number of exhaustions"""
    e = engine(make_engine)
    e.kube_distribute(2 * T + 1, [0] * 32, [1] * 32)  # (buffers to their size)
    e.set_profiling(True)
    before = e.kernel_timings()
    e.kube_distribute(2 * T + 1, [0] * 32, [1] * 32)
    after = e.kernel_timings()
    e.set_profiling(False)
    new = {k: v[1] - before.get(k, (0.0, 0))[1] for k, v in after.items() if v[1] != before.get(k, (0.0, 0))[1]}
    assert new == {"kube_distribute": 1}, new


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def raw_call(e, K, cl, location=None, draw=None, seed=0, choice=True, idx=True, cap=None, off=True, cinfo=True, info=True):
    """cook_kube_distribute with any argument missing -> (rc, choice, idx, off, info)"""
    cap = K if cap is None else cap
    ch = np.full(max(1, K), 0x5A, np.uint8)
    ix = np.full(max(1, cap), 0x5A5A5A5A, np.uint32)
    of = np.full(A.MAX_CLUSTERS + 2, 0x5A5A5A5A, np.uint32)
    ci = (A.CookKubeClusterInfo * (A.MAX_CLUSTERS + 1))()
    inf = A.CookKubeInfo()
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a is not None else None
    rc = e._lib.cook_kube_distribute(e._h, K, p(location, C.c_uint32), p(draw, C.c_double), C.c_uint64(seed), C.byref(cl) if cl is not None else None,
                                     p(ch, C.c_uint8) if choice else None, p(ix, C.c_uint32) if idx else None, cap, p(of, C.c_uint32) if off else None,
                                     ci if cinfo else None, C.byref(inf) if info else None)
    return rc, ch, ix, of, inf


def check_refusals(make_engine):
    e = engine(make_engine)
    K = 70
    loc3, cap3 = np.array([0, 0, 0], np.uint32), np.array([30, 30, 30], np.int64)
    locs = np.zeros(K, np.uint32)
    cl = lambda n=3, l=loc3, c=cap3: A.CookKubeClusters(n, 0, l.ctypes.data_as(C.POINTER(C.c_uint32)) if l is not None else None,
                                                         c.ctypes.data_as(C.POINTER(C.c_int64)) if c is not None else None)
    good = np.random.default_rng(1).random(K)
    reference = O.distribute(K, loc3, cap3, locs, good)

    def refused(tag, **kw):
        rc, ch, ix, of, inf = raw_call(e, K, **kw)
        assert rc == COOK_E_INVALID, (tag, rc)
        assert (ch == 0x5A).all() and (ix == 0x5A5A5A5A).all() and (of == 0x5A5A5A5A).all(), (tag, "a refused call writes nothing")
        assert e._lib.cook_last_error(e._h).decode().startswith("cook_kube_distribute:"), tag
        compare(e.kube_distribute(K, loc3, cap3, locs, good), reference, (tag, "the next call"))  # the engine is as it was

    big = np.zeros(A.MAX_CLUSTERS + 1, np.uint32), np.ones(A.MAX_CLUSTERS + 1, np.int64)
    refused("n > 32", cl=cl(A.MAX_CLUSTERS + 1, *big))
    refused("clusters NULL", cl=None)
    refused("location column NULL", cl=cl(3, None, cap3))
    refused("capacity column NULL", cl=cl(3, loc3, None))
    refused("choice NULL", cl=cl(), choice=False)
    refused("pos_idx NULL", cl=cl(), idx=False)
    refused("cluster_off NULL", cl=cl(), off=False)
    refused("cluster_info NULL", cl=cl(), cinfo=False)
    for bad, tag in ((1.0, "1.0"), (-0.25, "negative"), (float("nan"), "NaN"), (float("inf"), "inf"), (1.5, "1.5")):
        for at in (0, K - 1):
            d = good.copy()
            d[at] = bad
            refused(("draw", tag, at), cl=cl(), draw=d)
    # -0.0 is 0.0: in range
    d = good.copy()
    d[3] = -0.0
    compare(e.kube_distribute(K, loc3, cap3, locs, d), O.distribute(K, loc3, cap3, locs, d), "-0.0")
    # n_jobs > INT32_MAX is refused before any column is read
    one, off = np.zeros(1, np.uint8), np.zeros(4, np.uint32)
    rc = e._lib.cook_kube_distribute(e._h, 2 ** 31, None, None, C.c_uint64(0), C.byref(cl()), one.ctypes.data_as(C.POINTER(C.c_uint8)), None, 0,
                                     off.ctypes.data_as(C.POINTER(C.c_uint32)), (A.CookKubeClusterInfo * 3)(), None)
    assert rc == COOK_E_INVALID
    # cap too small: COOK_E_INVALID with choice, offsets, cluster info and info still filled
    with pytest.raises(CookError) as x:
        e.kube_distribute(K, loc3, cap3, locs, good, cap=K - 1)
    assert x.value.code == COOK_E_INVALID and "cap" in str(x.value)
    last = e.last_kube
    assert last["choice"].tolist() == reference["choice"] and last["off"].tolist() == reference["off"]
    assert last["cluster_info"] == reference["cluster_info"] and last["info"] == reference["info"]
    # info is optional, n = 0 needs no cluster columns and no cluster_info, n_jobs = 0 needs no job columns
    rc, ch, ix, of, inf = raw_call(e, K, cl(), draw=good, info=False)
    assert rc == 0 and ch[:K].tolist() == reference["choice"]
    rc, ch, ix, of, inf = raw_call(e, 5, cl(0, None, None), cinfo=False)
    assert rc == 0 and ch[:5].tolist() == [A.KUBE_NO_CLUSTER] * 5 and of[0] == 0 and inf.no_cluster == 5 and inf.n_first == 5
    rc, ch, ix, of, inf = raw_call(e, 0, cl(), choice=False, idx=False)
    assert rc == 0 and of[:4].tolist() == [0, 0, 0, 0] and inf.launched == 0


# ======================================================================================================================================
# The cycle form (cook_cycle_run_kube, _multi, cook_cycle_fetch_kube) against the oracle composed behind the considerable oracle:
# rank / queue with every considered job removed (tests/queue_cases._queue_of) -> pyoracle.considerable -> kube_oracle.distribute, the
# launched jobs carried into the user state by tests/carry_oracle.carry_usage.
# ======================================================================================================================================
import dataclasses  # noqa: E402
import subprocess  # noqa: E402
import sys  # noqa: E402
from types import SimpleNamespace  # noqa: E402

from cook_amd import synth  # noqa: E402
from cook_amd.engine import cycle_autoscale_clusters_multi, cycle_run_kube_multi, cycle_run_queue_release_multi  # noqa: E402
from oracle import pyoracle  # noqa: E402
from tests import carry_cases as CK  # noqa: E402
from tests import carry_oracle as CO  # noqa: E402
from tests import queue_cases as Q  # noqa: E402
from tests import release_oracle as RO  # noqa: E402

COOK_E_STATE = -4


def kube_pool(seed, n_pending=700, n_running=120, n_users=10, n_offers=16, n_locations=3):
    pool = synth.make_pool(seed=seed, n_pending=n_pending, n_running=n_running, n_users=n_users, n_offers=n_offers)
    rng = np.random.default_rng(seed + 3)
    loc = rng.integers(1, n_locations + 1, n_pending).astype(np.uint32)
    loc[rng.random(n_pending) < 0.4] = 0
    pool.pending_jobs.ckpt_location = loc
    pool.offers.location = rng.integers(1, n_locations + 1, n_offers).astype(np.uint32)
    pool.top_user = -1  # (carry_cases.base_state limits every second user but this one: none is exempt here)
    return pool


def kcycle(cl_loc, cl_cap, mjc=200, thr=0, rank_first=False, draw=None, seed=0, carry_usage=True, fenzo=False, finished=None):
    return SimpleNamespace(cl_loc=list(cl_loc), cl_cap=list(cl_cap), mjc=mjc, thr=thr, rank_first=rank_first, draw=draw, seed=seed,
                           carry_usage=carry_usage, fenzo=fenzo, finished=finished)


def cycle_oracle(params, pool, state, eligible, cycles, with_carry=True):
    """-> per cycle SimpleNamespace(paused, gate, Q, pos, jobs, d (kube_oracle.distribute with task indices), launched mask, state);
    a cycle with fenzo=True is a Fenzo queue cycle (cook_cycle_run_queue_carry) of mjc jobs behind the Kubernetes cycles"""
    J = pool.pending_jobs
    rank = lambda: pyoracle.rank(params, pool.tasks, pool.users)[0]  # noqa: E731
    Qv, last, out = rank(), None, []
    for cy in cycles:
        g = O.gate(cy.cl_cap, cy.mjc, cy.thr) if not cy.fenzo else dict(available=0, max_considerable=cy.mjc, paused=0)
        if g["paused"]:
            out.append(SimpleNamespace(paused=True, gate=g))
            continue
        if cy.rank_first:
            Qv = rank()
        elif last is not None:
            if with_carry and cy.carry_usage:
                state = CO.carry_usage(state, last.jobs, last.hit, spend=True)
            if cy.finished is not None:  # (the release comes behind the carry of the same advance)
                state = RO.release_usage(state, cy.finished)
            keep = np.ones(len(Qv), bool)
            keep[last.pos] = False  # every considered job leaves the queue (:1792-1794)
            Qv = Qv[keep]
        jq, queue = Q._queue_of(pool, Qv, eligible)
        pos = pyoracle.considerable(queue, state, g["max_considerable"])[0]
        jobs = J.take(jq[pos])
        if cy.fenzo:
            j2o, _, _ = pyoracle.match(params, jobs, pool.offers, Q.build_groups(Q.group_table(pool.groups)))
            last = SimpleNamespace(paused=False, gate=g, Q=Qv, pos=pos, jobs=jobs, j2o=j2o, hit=j2o >= 0, state=state)
        else:
            loc = J.ckpt_location[jq[pos]] if J.ckpt_location is not None else None
            d = O.distribute(len(pos), cy.cl_loc, cy.cl_cap, loc, cy.draw, cy.seed, task=Qv[pos])
            d["info"].update(available=g["available"], max_considerable=g["max_considerable"])
            last = SimpleNamespace(paused=False, gate=g, Q=Qv, pos=pos, jobs=jobs, d=d, hit=np.array(d["choice"]) != O.NO_CLUSTER, state=state)
        out.append(last)
    return out


def run_kube(e, cy, **kw):
    return e.cycle_run_kube(cy.cl_loc, cy.cl_cap, cy.mjc, cy.thr, rank_first=cy.rank_first, draw=cy.draw, seed=cy.seed,
                            carry=A.QueueCarry(usage=cy.carry_usage) if not cy.rank_first else None, finished=cy.finished, **kw)


def compare_cycle(e, got, w, tag):
    """one Kubernetes cycle: the call's outputs, and what the engine holds afterwards"""
    assert got["off"].tolist() == w.d["off"], (tag, got["off"].tolist(), w.d["off"])
    for c, (g, x) in enumerate(zip(got["lists"], w.d["lists"])):
        assert g.tolist() == [int(t) for t in x], (tag, "cluster", c)
    assert got["cluster_info"] == w.d["cluster_info"], tag
    assert got["info"] == w.d["info"], (tag, got["info"], w.d["info"])
    ranked, j2o, _ = e.cycle_fetch()
    assert np.array_equal(ranked, w.Q) and len(j2o) == len(w.pos) and (j2o == -1).all(), tag
    assert np.array_equal(e.cycle_fetch_considerable(), w.pos), tag
    assert e.cycle_fetch_kube().tolist() == w.d["choice"], tag


def paused_result(cy):
    g = O.gate(cy.cl_cap, cy.mjc, cy.thr)
    return dict(off=[0] * (len(cy.cl_loc) + 1), cluster_info=[dict(assigned=0, capacity=int(c)) for c in cy.cl_cap],
                info=dict(paused=1, max_considerable=g["max_considerable"], available=g["available"], n_considered=0, launched=0, no_cluster=0,
                          exhaustions=0, first_tasks=[]))


def check_paused(got, cy, tag):
    w = paused_result(cy)
    assert got["off"].tolist() == w["off"] and got["cluster_info"] == w["cluster_info"] and got["info"] == w["info"], (tag, got, w)
    assert all(len(l) == 0 for l in got["lists"]), tag


def cycle_case(seed, tokens=None, enforce=False):
    """a pool, a user state whose quotas (and tokens) the launched jobs of the first cycles use up, and three Kubernetes cycles:
    after a rank, then two queue steps; clusters that run out, a location no cluster has, both draw sources"""
    pool = kube_pool(seed)
    st, eligible = CK.base_state(pool, seed, tokens=tokens, enforce=enforce)
    rng = np.random.default_rng(seed + 5)
    cycles = [kcycle([1, 2, 0], [60, 50, 30], mjc=200, rank_first=True, seed=seed),
              kcycle([1, 2, 0], [80, 5, 40], mjc=150, draw=rng.random(150)),
              kcycle([1, 2, 0], [70, 60, -3], mjc=200, seed=seed + 1)]
    return pool, st, eligible, cycles


def staged(make_engine, params, pool, st, eligible):
    e = make_engine(params)
    e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
    e.cycle_set_considerable(st, eligible)
    return e


def check_cycles(make_engine, tokens=False, limiters=False, paused_between=False, release=False, stop_after=3):
    """three consecutive Kubernetes cycles with carry->usage = 1: every cycle against the oracle, and the second cycle's considerable set
    differs from the run without the carry (a user hits its quota or runs out of tokens)"""
    params = A.default_params()
    tok = None
    if tokens or limiters:
        tok = np.full(10, 10 ** 6, np.int64)
        tok[1::2] = [4, 9, 2, 30, 6]  # users that run out of tokens within the first cycles
    pool, st, eligible, cycles = cycle_case(7300 + int(tokens) + 2 * int(limiters), tokens=tok, enforce=tok is not None)
    if release:  # the first fifteen jobs the first cycle launched have ended by the third: they leave the staged user state there
        first = cycle_oracle(params, pool, st, eligible, cycles[:1])[0]
        jobs, idx = first.jobs, np.flatnonzero(first.hit)[:15]
        cycles[2].finished = A.Finished(host=np.zeros(len(idx), np.uint32), cpus=jobs.cpus[idx], mem=jobs.mem[idx], user=jobs.user[idx], usage=1)
    want = cycle_oracle(params, pool, st, eligible, cycles)
    stale = cycle_oracle(params, pool, st, eligible, cycles, with_carry=False)
    assert not np.array_equal(want[1].pos, stale[1].pos), "the carry decides the second cycle's considerable set"
    assert all(w.d["info"]["launched"] > 0 and w.d["info"]["no_cluster"] > 0 for w in want), [w.d["info"] for w in want]
    if limiters:  # the engine's own limiters in the place of the staged tokens: no clock is set, so nobody earns and they only spend
        e = staged(make_engine, params, pool, dataclasses.replace(st, tokens_left=None), eligible)
        e.cycle_set_limiters(A.Limiters(np.ones(10), np.full(10, 10 ** 7, np.int64), tok, np.zeros(10, np.int64)))
    else:
        e = staged(make_engine, params, pool, st, eligible)
    for c, (cy, w) in enumerate(zip(cycles[:stop_after], want)):
        if paused_between and c == 2:  # a paused call: nothing ran, the last cycle's record is still pending
            before = e.cycle_fetch()
            halt = kcycle(cy.cl_loc, [3, -1, 2], thr=4)
            check_paused(run_kube(e, halt), halt, "paused")
            after = e.cycle_fetch()
            assert all(np.array_equal(a, b) for a, b in zip(before[:2], after[:2])) and before[2] == after[2]
            assert e.cycle_fetch_kube().tolist() == want[1].d["choice"]
        compare_cycle(e, run_kube(e, cy), w, ("cycle", c))
    return e, pool, st, eligible, cycles, want


def check_release(make_engine):
    e, pool, st, eligible, cycles, want = check_cycles(make_engine, release=True)
    plain = cycle_oracle(A.default_params(), pool, st, eligible, cycles[:2] + [kcycle(cycles[2].cl_loc, cycles[2].cl_cap, mjc=cycles[2].mjc, seed=cycles[2].seed)])
    assert not np.array_equal(plain[2].pos, want[2].pos), "the release decides the third cycle's considerable set"


def check_fenzo_after_kube(make_engine):
    """a Fenzo queue cycle behind a Kubernetes cycle: its advance removes EVERY considered job and carries the launched ones"""
    params = A.default_params(good_enough_fitness=1.0)
    pool, st, eligible, cycles = cycle_case(7400)
    cycles = cycles[:2] + [kcycle([], [], mjc=120, fenzo=True)]
    want = cycle_oracle(params, pool, st, eligible, cycles)
    stale = cycle_oracle(params, pool, st, eligible, cycles, with_carry=False)
    assert not np.array_equal(want[2].pos, stale[2].pos)
    e = staged(make_engine, params, pool, st, eligible)
    for c in range(2):
        compare_cycle(e, run_kube(e, cycles[c]), want[c], ("cycle", c))
    e.cycle_run_queue_carry(120, A.QueueCarry(usage=True))  # (remove_mode 0: after a Kubernetes cycle every considered job leaves all the same)
    ranked, j2o, _ = e.cycle_fetch()
    assert np.array_equal(ranked, want[2].Q) and np.array_equal(e.cycle_fetch_considerable(), want[2].pos)
    assert np.array_equal(j2o, want[2].j2o) and (j2o >= 0).any()
    with pytest.raises(CookError) as x:
        e.cycle_fetch_kube()
    assert x.value.code == COOK_E_STATE
    e.match_metrics()  # (a placement ran: its readers answer again)


def check_distribute_beside_cycle(make_engine):
    """the stateless distributor on the engine of a Kubernetes cycle, with other job counts and clusters: the cycle's record stays — the
    fetches, and the next cycle's carry"""
    e, pool, st, eligible, cycles, want = check_cycles(make_engine, stop_after=2)
    for K, n in ((7, 1), (3 * T + 5, A.MAX_CLUSTERS), (0, 2)):  # smaller, larger (the scratch buffers grow) and empty
        cl_loc, cl_cap, loc, draw = sized_case(K, n, 4400 + K)
        check(e, K, cl_loc, cl_cap, loc, draw, tag=("beside a cycle", K, n))
        assert e.cycle_fetch_kube().tolist() == want[1].d["choice"], (K, n)
        ranked, j2o, _ = e.cycle_fetch()
        assert np.array_equal(ranked, want[1].Q) and (j2o == -1).all() and np.array_equal(e.cycle_fetch_considerable(), want[1].pos)
    compare_cycle(e, run_kube(e, cycles[2]), want[2], "the cycle behind the stateless calls")


def check_offer_skipped_ignored(make_engine):
    """offer_skipped behind a Kubernetes cycle is not read: all ones or all zeros, the launched jobs are carried and spend all the same"""
    params = A.default_params()
    tok = np.full(10, 10 ** 6, np.int64)
    tok[1::2] = [4, 9, 2, 30, 6]
    pool, st, eligible, cycles = cycle_case(7301, tokens=tok, enforce=True)
    want = cycle_oracle(params, pool, st, eligible, cycles)
    for fill in (1, 0):
        e = staged(make_engine, params, pool, st, eligible)
        compare_cycle(e, run_kube(e, cycles[0]), want[0], "cycle 0")
        for c in (1, 2):
            compare_cycle(e, run_kube(e, cycles[c], offer_skipped=np.full(pool.offers.n, fill, np.uint8)), want[c], ("offer_skipped", fill, c))


def check_state_answers(make_engine):
    """after a Kubernetes cycle no placement ran: explain, metrics and autoscale answer COOK_E_STATE, the cycle's record stays"""
    e, pool, st, eligible, cycles, want = check_cycles(make_engine)
    for call in (lambda: e.match_explain([0]), lambda: e.match_metrics(), lambda: e.cycle_autoscale(),
                 lambda: e.cycle_autoscale_clusters(AS_CLUSTERS())):
        with pytest.raises(CookError) as x:
            call()
        assert x.value.code == COOK_E_STATE
    assert e.cycle_fetch_kube().tolist() == want[2].d["choice"]


def AS_CLUSTERS():
    one = np.ones(1, np.int64)
    return A.AutoscaleClusters(np.zeros(1, np.uint32), one * BIG, one * 0, one * BIG, one * 0, one * BIG, one * 0)


# ---- refusals of the cycle form, each leaving the engine unchanged ------------------------------------------------------------------------
def snapshot(e):
    r, j, h = e.cycle_fetch()
    return r.tolist(), j.tolist(), h, e.cycle_fetch_considerable().tolist(), e.cycle_fetch_kube().tolist()


def check_cycle_refusals(make_engine):
    params = A.default_params()
    pool, st, eligible, cycles = cycle_case(7500)
    want = cycle_oracle(params, pool, st, eligible, cycles)
    e = make_engine(params)
    cy = cycles[1]
    for rank_first in (True, False):  # before a stage
        with pytest.raises(CookError) as x:
            e.cycle_run_kube(cy.cl_loc, cy.cl_cap, cy.mjc, rank_first=rank_first)
        assert x.value.code == COOK_E_STATE
    e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
    e.cycle_set_considerable(st, eligible)
    compare_cycle(e, run_kube(e, cycles[0]), want[0], "cycle 0")
    before = snapshot(e)
    mc = O.gate(cy.cl_cap, cy.mjc, cy.thr)["max_considerable"]  # (the draws of positions 0 .. max_considerable - 1 are the call's)
    assert 0 < mc < cy.mjc
    bad = cy.draw.copy()
    bad[mc - 1] = float("nan")
    big = [0] * (A.MAX_CLUSTERS + 1)
    for tag, code, kw in (
            ("n > 32", COOK_E_INVALID, dict(cluster_location=big, cluster_capacity=[1] * len(big))),
            ("a draw that is NaN", COOK_E_INVALID, dict(draw=bad)),
            ("a draw of 1.0", COOK_E_INVALID, dict(draw=np.ones(mc))),
            ("n_draw too small", COOK_E_INVALID, dict(draw=cy.draw[: mc - 1])),
            ("step->offers", COOK_E_INVALID, dict(offers=pool.offers)),
            ("carry->offers", COOK_E_INVALID, dict(carry=A.QueueCarry(offers=True))),
            ("finished->offers", COOK_E_INVALID, dict(finished=A.Finished(host=np.zeros(1, np.uint32), cpus=np.ones(1), mem=np.ones(1), offers=1))),
            ("a queue step's own refusal: carry usage without users in finished", COOK_E_INVALID,
             dict(finished=A.Finished(host=np.zeros(1, np.uint32), cpus=np.ones(1), mem=np.ones(1), usage=1)))):
        args = dict(cluster_location=cy.cl_loc, cluster_capacity=cy.cl_cap, max_jobs_considered=cy.mjc, draw=cy.draw, carry=A.QueueCarry(usage=True))
        args.update(kw)
        with pytest.raises(CookError) as x:
            e.cycle_run_kube(**args)
            pytest.fail("not refused: " + tag)
        assert x.value.code == code, (tag, x.value)
        assert snapshot(e) == before, tag
    # NULL columns, NULL outputs
    call = lambda c, out=True, off=True, ci=True: e._lib.cook_cycle_run_kube(  # noqa: E731
        e._h, C.byref(c.c) if c is not None else None, c0.out.ctypes.data if out else None, c0.cap, c0.off.ctypes.data if off else None,
        C.cast(c0.cinfo, C.c_void_p) if ci else None, None)
    from cook_amd.engine import _KubeCall
    c0 = _KubeCall(e, dict(cluster_location=cy.cl_loc, cluster_capacity=cy.cl_cap, max_jobs_considered=cy.mjc))
    nocol = _KubeCall(e, dict(cluster_location=cy.cl_loc, cluster_capacity=cy.cl_cap, max_jobs_considered=cy.mjc))
    nocol.cl.capacity = None
    nocl = _KubeCall(e, dict(cluster_location=cy.cl_loc, cluster_capacity=cy.cl_cap, max_jobs_considered=cy.mjc))
    nocl.c.clusters = None
    for tag, rc in (("null cycle", call(None)), ("null clusters", call(nocl)), ("null capacity column", call(nocol)),
                    ("null task_idx", call(c0, out=False)), ("null cluster_off", call(c0, off=False)), ("null cluster_info", call(c0, ci=False))):
        assert rc == COOK_E_INVALID, (tag, rc)
        assert snapshot(e) == before, tag
    # cap too small: the cycle has run, info is still filled
    with pytest.raises(CookError) as x:
        run_kube(e, cy, cap=3)
    assert x.value.code == COOK_E_INVALID and e.last_kube["info"] == want[1].d["info"] and e.last_kube["off"].tolist() == want[1].d["off"]
    compare_cycle(e, run_kube(e, cycles[2]), want[2], "the cycle after it")
    # between a deferred set-up and cook_cycle_match_multi
    e.cycle_run_rank(50)
    for rank_first in (True, False):
        with pytest.raises(CookError) as x:
            e.cycle_run_kube(cy.cl_loc, cy.cl_cap, cy.mjc, rank_first=rank_first)
        assert x.value.code == COOK_E_STATE, rank_first
    from cook_amd.engine import cycle_match_multi
    cycle_match_multi([e])
    assert (e.cycle_fetch()[1] >= 0).any()


# ---- several pools in one call ---------------------------------------------------------------------------------------------------------------
def multi_case():
    """three good pools with 3, 32 and 1 clusters, a paused one, a refused one (a draw of 1.0) and one that considers nothing"""
    params = A.default_params()
    rng = np.random.default_rng(77)
    shapes = [([1, 2, 0], [60, 50, 30]), (list(rng.integers(0, 4, 32)), list(rng.integers(0, 9, 32))), ([0], [90]),
              ([0, 0], [2, 2]), ([1, 2, 0], [60, 50, 30]), ([0, 1], [40, 40])]
    pools = [kube_pool(7600 + i, n_pending=400 + 30 * i) for i in range(6)]
    states = [CK.base_state(p, 7600 + i) for i, p in enumerate(pools)]
    first = [kcycle(l, c, mjc=150, rank_first=True, seed=i) for i, (l, c) in enumerate(shapes)]
    second = [kcycle(l, c, mjc=120, seed=10 + i) for i, (l, c) in enumerate(shapes)]
    second[3].thr = 4                      # paused: available == threshold
    second[4].draw = np.ones(120)          # refused
    second[5].mjc = 0                      # considers nothing
    return params, pools, states, first, second


def kube_kw(cy):
    return dict(cluster_location=cy.cl_loc, cluster_capacity=cy.cl_cap, max_jobs_considered=cy.mjc, min_capacity_threshold=cy.thr,
                rank_first=cy.rank_first, draw=cy.draw, seed=cy.seed, carry=A.QueueCarry(usage=True) if not cy.rank_first else None)


def run_multi(make_engine):
    params, pools, states, first, second = multi_case()
    es = [staged(make_engine, params, p, st, el) for p, (st, el) in zip(pools, states)]
    want = [cycle_oracle(params, p, st, el, [a, b if i != 4 else kcycle(b.cl_loc, b.cl_cap, mjc=b.mjc, seed=b.seed)])
            for i, (p, (st, el), a, b) in enumerate(zip(pools, states, first, second))]
    es[0].set_profiling(True)
    got1 = cycle_run_kube_multi(es, [kube_kw(c) for c in first])
    launches = es[0].kernel_timings().get("kube_distribute", (0.0, 0))[1]
    es[0].set_profiling(False)
    for i, (e, g) in enumerate(zip(es, got1)):
        compare_cycle(e, g, want[i][0], ("multi, first", i))
    stats = dict(es[0].batch_stats(), kube_distribute_launches=launches)
    got2, rcs = cycle_run_kube_multi(es, [kube_kw(c) for c in second], raise_errors=False)
    assert rcs == [0, 0, 0, 0, COOK_E_INVALID, 0], rcs
    for i in (0, 1, 2, 5):
        compare_cycle(es[i], got2[i], want[i][1], ("multi, second", i))
    assert want[5][1].d["info"]["n_considered"] == 0
    check_paused(got2[3], second[3], "multi, paused")
    for i in (3, 4):  # the paused and the refused pool still hold their first cycle
        assert es[i].cycle_fetch_kube().tolist() == want[i][0].d["choice"], i
    return dict(stats=stats, lists=[[l.tolist() for l in g["lists"]] for g in got1 + got2], infos=[g["info"] for g in got1 + got2], rcs=rcs)


def check_multi_batched(got, emu):
    """the pools' flows ran as ONE pool batch: the distributor of the six pools is one launch (blockIdx.y = pool)"""
    s = got["stats"]
    assert s["pools"] == 6 and s["kube_distribute_launches"] == 1, s


def check_multi_unbatched_child(got, emu):
    """the same calls with COOK_RANK_BATCH=0 in a fresh child process: engine by engine, the same results"""
    code = ("import json, sys; sys.path.insert(0, %r)\n"
            "from cook_amd.engine import Engine\nfrom tests import kube_cases as KC\n"
            "%s\n"
            "r = KC.run_multi(lambda p: Engine(p, lib_path=so)); r.pop('stats'); print('RESULT' + json.dumps(r))") % (
        ROOT, "from tests.simt_emu import build_emu; so = build_emu.build()" if emu else "from cook_amd import build; so = build.build()")
    env = dict(os.environ, COOK_RANK_BATCH="0")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    child = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1][6:])
    mine = {k: v for k, v in got.items() if k != "stats"}
    assert child == json.loads(json.dumps(mine))


def check_sync_count(make_engine):
    """no more stream synchronisations than cook_cycle_run_queue_release on the same step followed by cook_cycle_autoscale_clusters: the
    pool batches' counters (cook_batch_stats), every buffer brought to its size by a first round of the same calls"""
    params = A.default_params(good_enough_fitness=1.0)
    pool = kube_pool(7700)
    st, eligible = CK.base_state(pool, 7700)
    n = 2
    es = [staged(make_engine, params, pool, st, eligible) for _ in range(n)]
    cl = AS_CLUSTERS()
    hashes = np.arange(pool.pending_jobs.n, dtype=np.int32)
    syncs = {}
    for leg in ("warm", "timed"):
        for e in es:
            e.cycle_run(100)
            e.cycle_set_job_hashes(hashes)
        cycle_run_queue_release_multi(es, [100] * n, [dict(remove_mode=1)] * n, [A.QueueCarry(usage=True)] * n)
        a = es[0].batch_stats()
        from cook_amd.engine import cycle_match_multi
        cycle_match_multi(es)
        cycle_autoscale_clusters_multi(es, [dict(clusters=cl, max_jobs=100)] * n)
        b = es[0].batch_stats()
        for e in es:
            e.cycle_run(100)
        cycle_run_kube_multi(es, [dict(cluster_location=[0, 0, 0], cluster_capacity=[40, 30, 20], max_jobs_considered=100, carry=A.QueueCarry(usage=True))] * n)
        k = es[0].batch_stats()
        syncs[leg] = (a["syncs"], b["syncs"], k["syncs"])
        assert k["pools"] == n and k["grouped_launches"] == k["launches"], k  # identical flows: every kernel once for both pools
    a, b, k = syncs["timed"]
    print("synchronisations: queue_release", a, "+ autoscale_clusters", b, "against run_kube", k)
    assert 0 < k <= a + b, syncs
