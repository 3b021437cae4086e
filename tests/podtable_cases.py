"""The cases of the resident pod table (cook_offers_stage_pod_ids, cook_offers_update, cook_offers_update_info, cook_offers_fetch_pods,
cook_cycle_set_built_offers, cook_cycle_run_queue_pods*), shared by the emulator suite, the GPU suite and the ABI suite.  Every case
is judged by tests/podtable_oracle.py: the pod table, every offer column, node_status, the totals and the per-model / per-type gauges,
the queue, rank_pos, job_to_offer, head_matched and the info counters, bit for bit in every cycle; what a case is there to show is
asserted on the oracle before the engine is called.  Every queue case is also driven the parent's way — cook_offers_build on the
mirrored tables, its rows handed to cook_cycle_run_queue_reserve as step->offers — with identical results."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np
import pytest

from cook_amd import _abi as A
from cook_amd import synth
from cook_amd.engine import CookError, cycle_match_multi, cycle_run_queue_pods_multi
from tests import carry_cases as K
from tests import churn_cases as CH
from tests import podtable_oracle as PO
from tests import queue_cases as S
from tests import release_oracle as R

COOK_E_INVALID, COOK_E_STATE = -1, -4
NONE = A.NONE_U32
P1 = K.P1
_code = K._code


# ---- comparisons ------------------------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_pods(e, tab, where=""):
    """the engine's pod table against the mirror: every column and the ids, element for element (doubles by their bits)"""
    rows = e.offers_fetch_pods()
    assert rows.n == tab.pods.n, (where, "pods", rows.n, tab.pods.n)
    for c in PO.POD_COLS:
        want = getattr(tab.pods, c)
        got = rows.column(c)
        if want is None:
            want = np.full(rows.n, PO.NULL_MEANS[c], got.dtype)
        assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want)), (where, c, got[:8], want[:8])
    assert np.array_equal(rows.column("id"), tab.ids), (where, "id", rows.column("id")[:8], tab.ids[:8])


def same_built(got: A.BuiltOffers, want: dict, tab, where=""):
    """cook_offers_fetch against the offer oracle: rows, node_status, totals, gauges"""
    for k, v in want["rows"].items():
        g = getattr(got, k)
        v = v.reshape(g.shape) if v.size == 0 else v
        assert g.dtype == v.dtype and np.array_equal(_bits(g), _bits(v)), (where, k, g[:8], v[:8])
    assert np.array_equal(got.node_status, want["status"]), (where, "node_status")
    for k, v in want["totals"].items():
        assert np.float64(got.totals[k]).tobytes() == np.float64(v).tobytes(), (where, k, got.totals[k], v)
    for k in ("gpu_capacity_by_model", "gpu_consumed_by_model", "disk_capacity_by_type", "disk_consumed_by_type"):
        assert np.array_equal(_bits(getattr(got, k)), _bits(want[k])), (where, k, getattr(got, k), want[k])
    if tab.nodes.attr is not None:
        assert np.array_equal(got.attr, tab.nodes.attr[got.node]), (where, "attr rows")


def staged(e, nodes, pods, op, ids, id_cap=None):
    e.offers_stage(nodes, pods, op)
    e.offers_stage_pod_ids(ids, int(max(ids)) + 1 if id_cap is None and len(ids) else (id_cap or 0))


def update_and_compare(e, tab, op, delta, where=""):
    """one cook_offers_update + cook_offers_run against the oracle -> the mirrored tables behind it"""
    tab2, info = PO.apply_delta(tab, delta)
    want = PO.build(tab2, op)
    e.offers_update(delta)
    same_pods(e, tab2, where)
    e.offers_run()
    same_built(e.offers_fetch(), want, tab2, where)
    assert e.offers_update_info() == dict(info, n_pods=tab2.pods.n, n_offers=len(want["rows"]["cpus"])), (where, e.offers_update_info(), info)
    return tab2


def some_pods(rng, n, n_nodes, *, fractional=True):
    node = rng.integers(0, max(1, n_nodes), n).astype(np.uint32)
    cpus = rng.integers(1, 4, n).astype(np.float64) + (0.1 if fractional else 0.0)
    mem = rng.integers(1, 9, n).astype(np.float64) * 128.0 + (rng.choice([0.0, 0.3], n) if fractional else 0.0)
    return A.Pods(node=node, cpus=cpus, mem=mem)


def some_nodes(rng, n):
    return A.Nodes(cpus=rng.choice([16.0, 32.0, 64.0], n), mem=rng.choice([16384.0, 65536.0], n), host=np.arange(n) * 3 + 2)


# ---- 1: by hand ----------------------------------------------------------------------------------------------------------------------------
def check_by_hand(make_engine):
    """three nodes.  A pod leaves a full node and the next cycle places onto it; a starting pod joins and the node is no longer offered
    (pod limit, with_task_limits); a node row flips to COOK_NODE_UNSCHEDULABLE and back."""
    params = P1(match_algo=1)
    nodes = A.Nodes(cpus=[4.0, 4.0, 4.0], mem=[4096.0] * 3, host=[10, 20, 30], flags=[0, 0, 0])
    pods = A.Pods(node=[0, 0, 1, 2], cpus=[2.0, 2.0, 1.0, 4.0], mem=[100.0] * 4)  # node 0 is full (cpus), node 2 too
    op = A.offer_params(max_pods_per_node=3)
    ids = np.arange(4, dtype=np.uint32)
    n_jobs = 6
    tasks = A.Tasks(cpus=np.full(n_jobs, 2.0), mem=np.full(n_jobs, 10.0), user=np.zeros(n_jobs, np.uint32), priority=np.full(n_jobs, 50),
                    start_ms=np.arange(n_jobs), task_id=np.arange(n_jobs), job_id=np.arange(n_jobs), pending=np.ones(n_jobs, np.uint8))
    users = A.Users(div_cpus=[100.0], div_mem=[1e6])
    jobs = A.Jobs(cpus=tasks.cpus.copy(), mem=tasks.mem.copy(), user=tasks.user.copy())
    pool = synth.Pool(tasks=tasks, users=users, pending_jobs=jobs, offers=None, groups=None, n_running=0, n_pending=n_jobs)
    flip = lambda f: A.PodDelta(node_rows=[2], node_values=A.Nodes(cpus=[4.0], mem=[4096.0], flags=[f]))
    cycles = [PO.cycle(1),
              PO.cycle(1, pods=A.PodDelta(remove=[0], add=A.Pods(node=[1], cpus=[2.1], mem=[10.0]), add_id=[4])),  # pod 0 leaves node 0; job 0's pod starts on node 1
              PO.cycle(1, pods=A.PodDelta(add=A.Pods(node=[0, 1], cpus=[2.1, 0.1], mem=[10.0, 1.0]), add_id=[0, 5])),  # node 1 reaches the pod limit
              PO.cycle(1, pods=flip(A.NODE_UNSCHEDULABLE)),
              PO.cycle(1, pods=A.PodDelta(remove=[5], node_rows=[2], node_values=A.Nodes(cpus=[4.0], mem=[4096.0], flags=[0]))),
              PO.cycle(1, pods=None)]
    tab = PO.mirror(nodes, pods, ids)
    want = PO.oracle(params, pool, tab, op, cycles)
    host_of = lambda w: [int(w.offers.host[o]) if o >= 0 else -1 for o in w.j2o]
    assert want[0].offers.host.tolist() == [10, 20, 30] and host_of(want[0]) == [20]  # only node 1 has room for 2 cpus
    assert host_of(want[1]) == [10] and want[1].offers.cpus.tolist() == [2.0, 4.0 - 1.0 - 2.1, 0.0]  # the freed node takes the next job
    assert want[2].offers.host.tolist() == [10, 30] and not want[2].built["status"][1] & A.NODE_ST_OFFER  # node 1: 3 pods = the limit
    assert host_of(want[2]) == [-1] and want[2].offers.num_tasks.tolist() == [2, 1]
    assert want[3].offers.host.tolist() == [10]  # node 2 is unschedulable ...
    assert want[4].offers.host.tolist() == [10, 20, 30]  # ... and back; node 1 is under the limit again
    assert want[5].pod_info["added"] == 0 and want[5].offers.n == 3
    run_and_compare(make_engine, params, pool, nodes, pods, op, ids, cycles, want, expect_form=1, id_cap=6)


# ---- the queue cycles' driver -----------------------------------------------------------------------------------------------------------------
def fetch(e):
    g = S.fetch(e, False)
    g.info = e.release_info()
    g.pod_info = e.offers_update_info()
    g.offers = e.fetch_offers().offers()
    return g


def compare_cycle(e, g, w, c, tag=""):
    where = f"{tag} cycle {c}"
    assert g.pod_info == w.pod_info, (where, "pod_info", g.pod_info, w.pod_info)
    assert g.info == w.info, (where, "release_info", g.info, w.info)
    same_pods(e, w.tab, where)
    same_built(e.offers_fetch(), w.built, w.tab, where)
    CH.same_table(g.offers, w.offers, where)


def run_and_compare(make_engine, params, pool, nodes, pods, op, ids, cycles, want, *, expect_form=None, id_cap=None, with_task_limits=True,
                    before_step=None):
    """the engine's way (resident table, deltas, rebuild in the advance), every cycle against the oracle; then the parent's way on a
    second engine, against the same oracle and so with identical results"""
    got = []
    with make_engine(params) as e:
        staged(e, nodes, pods, op, ids, id_cap)
        e.offers_run()
        e.cycle_stage_built_offers(pool.tasks, pool.users, pool.pending_jobs, pool.groups, with_task_limits=with_task_limits)
        for c, cy in enumerate(cycles):
            if cy.state is not None:
                e.cycle_set_considerable(cy.state, cy.eligible)
            if before_step is not None:
                before_step(e, c, cy)
            if c == 0:
                e.cycle_run(cy.k)
            else:
                kw = dict(K.step_kw(cy), offers=None)
                e.cycle_run_queue_pods(cy.k, K.carry_of(cy), getattr(cy, "finished", None), cy.pods, getattr(cy, "reservations", None),
                                       with_task_limits, **kw)
            got.append(fetch(e))
            if c:
                compare_cycle(e, got[-1], want[c], c)
            # (cycle 0 is placed on the rows of cook_cycle_stage_built_offers, whose hosts the engine does not know: no class-ordered walk there)
            if expect_form is not None and len(got[-1].j2o) and (c or expect_form != 3):
                ms = e.match_stats()
                assert ms["placement_form"] == expect_form, (c, ms["placement_form"], hex(ms["classfit_refused"]))
    S.compare(got, want, cycles, "resident")
    old = []
    with make_engine(params) as e:
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        for c, cy in enumerate(cycles):
            if cy.state is not None:
                e.cycle_set_considerable(cy.state, cy.eligible)
            if before_step is not None:
                before_step(e, c, cy)
            if c == 0:
                e.cycle_run(cy.k)
            else:
                rows = e.offers_build(want[c].tab.nodes, want[c].tab.pods, op)
                kw = {}
                if with_task_limits:
                    kw = dict(max_tasks=np.full(rows.n, op.max_pods_per_node, np.int32), num_tasks=rows.num_pods)
                e.cycle_run_queue_reserve(cy.k, K.carry_of(cy), getattr(cy, "finished", None), None, getattr(cy, "reservations", None),
                                          **dict(K.step_kw(cy), offers=rows.as_offers(**kw)))
            old.append(S.fetch(e, False))
    S.compare(old, want, cycles, "parent's way")
    for c, (g, o) in enumerate(zip(got, old)):
        assert np.array_equal(g.Q, o.Q) and np.array_equal(g.pos, o.pos) and np.array_equal(g.j2o, o.j2o) and g.head == o.head, c
    return got


# ---- 2: boundaries of the update alone ----------------------------------------------------------------------------------------------------------
BOUNDARY_PODS = (0, 1, 63, 64, 65, 255, 256, 257, 1025)
BOUNDARY_NODES = (1, 64, 257)


def check_boundary(make_engine, n_pods, n_nodes):
    """cook_offers_update + cook_offers_run at a wave / block boundary of the pod count: remove none, one, the first, the last, all; add 0,
    1 or 257; id_cap exactly the greatest id + 1; an id that leaves and rejoins in one call"""
    rng = np.random.default_rng(1000 * n_nodes + n_pods)
    nodes = some_nodes(rng, n_nodes)
    op = A.offer_params(max_pods_per_node=40)
    ids0 = rng.permutation(n_pods + 257).astype(np.uint32)  # (ids are slot numbers, not row numbers)
    with make_engine(P1()) as e:
        for mode, n_add in (("none", 1), ("one", 0), ("first", 257), ("last", 1), ("all", 0), ("all", 257), ("none", 0)):
            pods = some_pods(rng, n_pods, n_nodes)
            ids = ids0[:n_pods].copy()
            free = ids0[n_pods:]
            tab = PO.mirror(nodes, pods, ids)
            id_cap = int(ids0.max()) + 1
            assert id_cap == n_pods + 257
            staged(e, nodes, pods, op, ids, id_cap)
            rm = {"none": [], "one": ids[n_pods // 2:n_pods // 2 + 1], "first": ids[:1], "last": ids[-1:], "all": ids}[mode]
            add_id = free[:n_add].copy()
            if n_add and len(rm):
                add_id[0] = rm[0]  # leaves and rejoins in one call: it moves to the end
            if n_add:
                assert id_cap - 1 in set(int(x) for x in ids0)  # (the greatest id is used somewhere: id_cap is tight)
            d = A.PodDelta(remove=rm, add=some_pods(rng, n_add, n_nodes) if n_add else None, add_id=add_id if n_add else None)
            tab = update_and_compare(e, tab, op, d, f"{n_pods} pods, {n_nodes} nodes, remove {mode}, add {n_add}")
            if mode == "none" and n_add == 1:  # a second delta on the same table: the ids follow their rows
                d2 = A.PodDelta(remove=[int(tab.ids[-1])] + ([int(tab.ids[0])] if tab.pods.n > 1 else []))
                update_and_compare(e, tab, op, d2, "second delta")


def check_big_node(make_engine):
    """one node with 1030 pods — two LDS chunks of offers_node_eval — losing pods from both chunks"""
    rng = np.random.default_rng(77)
    nodes = A.Nodes(cpus=[4096.0, 8.0], mem=[1e7, 1e4], host=[1, 2])
    n = 1030 + 5
    node = np.zeros(n, np.uint32)
    node[rng.choice(n, 5, replace=False)] = 1
    pods = A.Pods(node=node, cpus=rng.integers(1, 3, n) + 0.1, mem=rng.integers(1, 9, n) * 10.0 + 0.3)
    ids = np.arange(n, dtype=np.uint32)[::-1].copy()
    op = A.offer_params(max_pods_per_node=5000)
    big = np.flatnonzero(node == 0)
    assert len(big) == 1030
    lose = np.concatenate([big[[0, 5, 700, 1023]], big[[1024, 1029]]])  # positions in the node's list: both chunks, and the chunk's edges
    with make_engine(P1()) as e:
        staged(e, nodes, pods, op, ids)
        tab = PO.mirror(nodes, pods, ids)
        before = PO.build(tab, op)
        tab2 = update_and_compare(e, tab, op, A.PodDelta(remove=ids[lose]), "1030 pods on one node")
        assert PO.build(tab2, op)["rows"]["cpus"][0] != before["rows"]["cpus"][0]


# ---- 3: the order rule -------------------------------------------------------------------------------------------------------------------------
def check_order_rule(make_engine):
    """non-dyadic requests on one node: the middle pod removed and re-added moves to the end, and the consumed cpus differ in the last
    bit from the unmodified order's — and equal the oracle's"""
    nodes = A.Nodes(cpus=[8.0], mem=[1000.0], host=[7])
    cpus = [0.3, 0.1, 0.1, 0.1, 0.3]
    best = None
    for mid in range(1, len(cpus) - 1):  # the middle pod whose move changes the sum's last bit
        moved = cpus[:mid] + cpus[mid + 1:] + [cpus[mid]]
        if R.seq_sum(moved) != R.seq_sum(cpus):
            best = mid
            break
    assert best is not None, "no move changes the left-to-right sum: other requests"
    pods = A.Pods(node=np.zeros(len(cpus), np.uint32), cpus=cpus, mem=[1.0] * len(cpus))
    ids = np.arange(len(cpus), dtype=np.uint32)
    op = A.offer_params(max_pods_per_node=100)
    one = lambda i: A.Pods(node=[0], cpus=[cpus[i]], mem=[1.0])
    with make_engine(P1()) as e:
        staged(e, nodes, pods, op, ids)
        e.offers_run()
        same = e.offers_fetch().totals["cpus_consumed"]
        tab = PO.mirror(nodes, pods, ids)
        tab = update_and_compare(e, tab, op, A.PodDelta(remove=[best], add=one(best), add_id=[best]), "order rule")
        moved = e.offers_fetch().totals["cpus_consumed"]
        assert tab.ids.tolist() == [i for i in range(len(cpus)) if i != best] + [best]
        assert moved != same and abs(moved - same) < 1e-12, (moved, same)
        assert moved == PO.build(tab, op)["totals"]["cpus_consumed"]


# ---- 4: every column ---------------------------------------------------------------------------------------------------------------------------
def check_columns(make_engine, slots):
    """gpus, models, disk, disk types, flags and label rows with `slots` slots; a synthetic pod under clobber_synthetic_pods; an added
    pod without a node of the pool; a column the table has and add lacks; node rows replaced in every column"""
    nodes, pods, op = synth.make_cluster_state(seed=51, n_nodes=70, n_pods=300, gpus=True, disk=True, fractional=True, n_attr_keys=3, max_pods=9,
                                               corrupt=0.2)
    assert op.clobber_synthetic_pods and (pods.flags & A.POD_SYNTHETIC).any()
    op.gpu_slots = op.disk_slots = slots
    ids = np.arange(pods.n, dtype=np.uint32) * 2
    rng = np.random.default_rng(5)
    _, more, _ = synth.make_cluster_state(seed=53, n_nodes=70, n_pods=40, gpus=True, disk=True, fractional=True, max_pods=9, corrupt=0.3)
    more.node[:3] = [NONE, 70, 1_000_000]  # no node of this pool: dropped by the rebuild, kept by the table
    more.flags[3] |= A.POD_SYNTHETIC
    with make_engine(P1()) as e:
        staged(e, nodes, pods, op, ids)
        tab = PO.mirror(nodes, pods, ids)
        d = A.PodDelta(remove=ids[rng.choice(pods.n, 30, replace=False)], add=more, add_id=np.arange(40, dtype=np.uint32) * 2 + 1)
        tab = update_and_compare(e, tab, op, d, f"every column, {slots} slots")
        bare = A.Pods(node=[5, 5], cpus=[1.1, 2.1], mem=[7.0, 9.5])  # the table has gpus / disk / flags, these rows do not: 0, absent
        tab = update_and_compare(e, tab, op, A.PodDelta(add=bare, add_id=[81, 83]), "columns add lacks")
        assert tab.pods.disk[-1] == -1.0 and tab.pods.gpus[-1] == 0
        rows = np.array([0, 33, 69], np.uint32)
        vals = A.Nodes(cpus=[128.0, 1.0, 2.5], mem=[1e6, 10.0, 100.3], gpus=[4, 0, 1], gpu_model=[2, 0, 1], disk=[9e5, -1.0, 10.5], disk_type=[1, 0, 2],
                       flags=[0, A.NODE_UNSCHEDULABLE, A.NODE_GPU_TAINT], attr=[[9, 9, 9], [0, 1, 2], [4, 4, 4]])
        tab = update_and_compare(e, tab, op, A.PodDelta(node_rows=rows, node_values=vals), "node rows, every column")
        assert tab.nodes.host.tolist() == nodes.host.tolist()
        only = A.Nodes(cpus=[3.0], mem=[5.0])  # the table has gpus / disk / flags / labels, this row does not: 0, absent
        tab = update_and_compare(e, tab, op, A.PodDelta(node_rows=[33], node_values=only, node_host=[12345]), "node row, bare")
        assert tab.nodes.host[33] == 12345 and tab.nodes.disk[33] == -1.0 and not tab.nodes.attr[33].any()
    # the reverse: a table without the optional columns refuses rows that carry one
    plain_n, plain_p = A.Nodes(cpus=[4.0], mem=[8.0], host=[1]), A.Pods(node=[0], cpus=[1.0], mem=[1.0])
    with make_engine(P1()) as e:
        staged(e, plain_n, plain_p, op, [0])
        for col, val in (("gpus", [1]), ("gpu_model", [1]), ("disk", [5.0]), ("disk_type", [1]), ("flags", [1])):
            add = A.Pods(node=[0], cpus=[1.0], mem=[1.0], **{col: val})
            assert _code(lambda: e.offers_update(A.PodDelta(add=add, add_id=[1]))) == COOK_E_INVALID, col
        for col, val in (("gpus", [1]), ("flags", [1]), ("attr", [[1]])):
            nv = A.Nodes(cpus=[1.0], mem=[1.0], **{col: val})
            assert _code(lambda: e.offers_update(A.PodDelta(node_rows=[0], node_values=nv))) == COOK_E_INVALID, col
        same_pods(e, PO.mirror(plain_n, plain_p, [0]), "refused: unchanged")


# ---- 5: queue cycles ---------------------------------------------------------------------------------------------------------------------------
QUEUE_CASES = ((3, 1), (6, 64), (11, 65))  # users x K


def cluster_for(seed, n_nodes=48, n_pods=170, fractional=True, **kw):
    nodes, pods, op = synth.make_cluster_state(seed=seed, n_nodes=n_nodes, n_pods=n_pods, fractional=fractional, max_pods=8, gpus=fractional, **kw)
    if fractional:
        nodes.cpus[:] = np.minimum(nodes.cpus, 32.0)  # (small nodes: the launched pods fill them within the case's cycles)
    else:  # (the class-ordered walk refuses a table with a row that has nothing left: roomy nodes, the unmatched jobs are the huge ones)
        nodes.cpus[:], nodes.mem[:] = 512.0, 4194304.0
    return nodes, pods, op, np.arange(pods.n, dtype=np.uint32)[::-1].copy()


def queue_pool(seed, users, k, n_cycles, *, groups=False, fractional=True):
    n_pending = max(40, 3 * k * n_cycles // 2)
    pool = synth.make_pool(seed=seed, n_pending=n_pending, n_running=10, n_users=users, n_offers=4, gpus=True, fractional=fractional)
    rng = np.random.default_rng(seed + 7)
    if groups:  # six unique-placement groups over a third of the jobs: the fold adds the kept matches' hosts, read from the OLD rows
        group = np.where(rng.random(n_pending) < 0.33, rng.integers(0, 6, n_pending), NONE).astype(np.uint32)
        pool.pending_jobs = dataclasses.replace(pool.pending_jobs, group=group)
        pool.groups = A.Groups(type=np.ones(6, np.uint8))
    J, T = pool.pending_jobs, pool.tasks
    pidx = np.flatnonzero(T.pending)
    huge = rng.random(J.n) < 0.3 if k == 1 else rng.random(J.n) < 0.1
    J.mem[huge] = 1e9
    T.mem[pidx[huge]] = 1e9
    return pool


def watcher(seed, id_base, *, frac=0.03, strangers=2, fractional=True):
    """a function for cycle(pods=...): the last cycle's kept matches start as pods on their offers' nodes (add-starting-pods), a few
    pods the watch saw end leave, a few foreign pods appear, and now and then a pod is modified (leaves and rejoins: to the end)"""
    rng = np.random.default_rng(seed)
    nxt = [id_base]

    def draw(history, tab):
        last = history[-1]
        add = PO.launched_pods(last, last.built["rows"]["node"], sidecar=0.1 if fractional else 0.0)
        extra = some_pods(rng, strangers, tab.nodes.n, fractional=fractional)
        parts = [p for p in (add, extra) if p is not None]
        cols = {}
        for c in PO.POD_COLS:
            have = getattr(tab.pods, c)
            if have is None:
                continue
            cols[c] = np.concatenate([getattr(p, c) if getattr(p, c) is not None else np.full(p.n, PO.NULL_MEANS[c], have.dtype) for p in parts])
        add = A.Pods(**cols)
        gone = tab.ids[rng.random(len(tab.ids)) < frac]
        if not len(gone):
            gone = tab.ids[:1]
        add_id = np.arange(nxt[0], nxt[0] + add.n, dtype=np.uint32)
        nxt[0] += add.n
        add_id[-1] = gone[0]  # the watch modified this pod
        missing = np.array([nxt[0] + 5], np.uint32)  # an id that is not live: counted, no error
        return A.PodDelta(remove=np.concatenate([gone, missing]), add=add, add_id=add_id)
    return draw


def queue_case(users, k, *, n_cycles=6, seed=None, groups=False, fractional=True):
    seed = seed if seed is not None else (600 if k == 1 else 600 + 10 * users + k)
    nodes, pods, op, ids = cluster_for(seed, n_attr_keys=2 if groups else 0, fractional=fractional)
    pool = queue_pool(seed + 1, users, k, n_cycles, groups=groups, fractional=fractional)
    state, eligible = K.base_state(pool_with_top(pool), seed, fractional=fractional, pool_slack=1e9)
    draw = watcher(seed + 2, id_base=pods.n, fractional=fractional)
    ends = R.finisher(seed + 3, 0.3, offers=0, usage=1, groups=1 if groups else 0)
    cycles = [PO.cycle(k, state=state, eligible=eligible)]
    for c in range(1, n_cycles):
        cycles.append(PO.cycle(k, pods=None if c == 3 else draw, carry_usage=True, finished=ends))
    id_cap = pods.n + n_cycles * (k + 4) + 16
    return pool, nodes, pods, op, ids, id_cap, cycles


def pool_with_top(pool):
    pool.top_user = int(np.bincount(pool.pending_jobs.user, minlength=pool.users.n).argmax())
    return pool


def queue_oracle(params, pool, nodes, pods, op, ids, cycles):
    want = PO.oracle(params, pool, PO.mirror(nodes, pods, ids), op, cycles)
    if cycles[0].k > 1:
        K.assert_every_cycle_mixed(want)
    else:  # (one considered job per cycle cannot be both: some cycle keeps its match, another leaves its job unmatched)
        assert any((w.j2o >= 0).all() for w in want[1:]) and any((w.j2o < 0).all() for w in want[1:]), "K = 1: re-seed the case"
    for c, (w, cy) in enumerate(zip(want, cycles)):
        if c and cy.pods is not None:
            assert w.pod_info["removed"] >= 1 and w.pod_info["added"] >= 1, f"cycle {c} removes or adds no pod: re-seed the case"
    assert sum(w.pod_info["remove_missing"] for w in want[1:]) >= 1
    assert len(set(w.offers.n for w in want)) > 1, "the rebuilds never change the row count: re-seed the case"
    assert any(cy.pods is None for cy in cycles[1:])
    return want


def check_queue(make_engine, users, k, *, algo=2, expect_form=None):
    """five queue cycles with pod deltas: carry.usage and finished (usage) in the same advance, a cycle with pods = NULL.  The
    class-ordered walk (form 3) takes dyadic resources and offers without a task limit only: that case has no sidecar fraction and
    runs without the task limits"""
    params = P1(match_algo=algo)
    walk = expect_form == 3
    pool, nodes, pods, op, ids, id_cap, cycles = queue_case(users, k, fractional=not walk)
    want = PO.oracle(params, pool, PO.mirror(nodes, pods, ids), op, cycles, with_task_limits=not walk) if walk else \
        queue_oracle(params, pool, nodes, pods, op, ids, cycles)
    if walk:
        K.assert_every_cycle_mixed(want)
    return run_and_compare(make_engine, params, pool, nodes, pods, op, ids, cycles, want, id_cap=id_cap, expect_form=expect_form,
                           with_task_limits=not walk)


def check_queue_groups(make_engine):
    """groups whose fold reads the OLD rows' hosts and attributes while the rebuild changes the row count; finished.groups in the same advance"""
    params = P1()
    pool, nodes, pods, op, ids, id_cap, cycles = queue_case(6, 64, groups=True, seed=733)
    assert pool.groups is not None and pool.pending_jobs.group is not None
    want = queue_oracle(params, pool, nodes, pods, op, ids, cycles)
    folded = sum(int((w.jobs.group[w.j2o >= 0] != NONE).sum()) for w in want[:-1])
    assert folded >= 2, "no grouped job is placed: the fold reads nothing: re-seed the case"
    return run_and_compare(make_engine, params, pool, nodes, pods, op, ids, cycles, want, id_cap=id_cap)


def check_queue_edges(make_engine):
    """an empty queue; a cycle whose last cycle considered nothing; no pods at all"""
    params = P1()
    pool, nodes, pods, op, ids, id_cap, cycles = queue_case(3, 1, n_cycles=3)
    with make_engine(params) as e:
        staged(e, nodes, pods, op, ids, id_cap)
        e.offers_run()
        e.cycle_stage_built_offers(pool.tasks, pool.users, pool.pending_jobs, None, with_task_limits=True)
        e.cycle_run(0)  # considers nothing
        tab = PO.mirror(nodes, pods, ids)
        d = A.PodDelta(remove=ids[:3], add=some_pods(np.random.default_rng(1), 2, nodes.n), add_id=[int(ids[0]), id_cap - 1])
        d.add = A.Pods(**{c: (getattr(d.add, c) if getattr(d.add, c) is not None else np.full(2, PO.NULL_MEANS[c], getattr(pods, c).dtype))
                          for c in PO.POD_COLS})
        tab, info = PO.apply_delta(tab, d)
        e.cycle_run_queue_pods(0, None, None, d, None, True)
        built = PO.build(tab, op)
        same_pods(e, tab, "no advance")
        same_built(e.offers_fetch(), built, tab, "no advance")
        assert e.offers_update_info() == dict(info, n_pods=tab.pods.n, n_offers=len(built["rows"]["cpus"]))
        CH.same_table(e.fetch_offers().offers(), PO.as_offers(built, tab, op, True), "no advance")
        big = pool.pending_jobs.n + 10
        e.cycle_run_queue_pods(big, None, None, None, None, True)  # everything is considered ...
        e.cycle_run_queue_pods(big, None, None, None, None, True, remove_mode=1)  # ... and leaves: the queue is empty
        Q, j2o, _ = e.cycle_fetch()
        e.cycle_run_queue_pods(big, None, None, None, None, True, remove_mode=1)
        Q, j2o, _ = e.cycle_fetch()
        assert len(Q) == 0 and len(j2o) == 0
        same_pods(e, tab, "empty queue")


def check_rank_between(make_engine):
    """a rank cycle in between: cook_offers_update + cook_offers_run + cook_cycle_set_built_offers + cook_cycle_run places what a fresh
    stage of the same rows places, and the queue cycles go on behind it"""
    params = P1()
    pool, nodes, pods, op, ids, id_cap, cycles = queue_case(6, 64, n_cycles=2)
    k = cycles[0].k
    tab = PO.mirror(nodes, pods, ids)
    want = PO.oracle(params, pool, tab, op, cycles)
    with make_engine(params) as e:
        staged(e, nodes, pods, op, ids, id_cap)
        e.offers_run()
        e.cycle_stage_built_offers(pool.tasks, pool.users, pool.pending_jobs, None, with_task_limits=True)
        e.cycle_set_considerable(cycles[0].state, cycles[0].eligible)
        e.cycle_run(k)
        e.cycle_run_queue_pods(k, K.carry_of(cycles[1]), cycles[1].finished, cycles[1].pods, None, True)
        S.compare([S.fetch(e, False)], want[1:], cycles[1:], "before the rank")
        d = A.PodDelta(remove=want[1].tab.ids[:40])
        tab2 = update_and_compare(e, want[1].tab, op, d, "between")
        built = PO.build(tab2, op)
        assert len(built["rows"]["cpus"]) != want[1].offers.n or not np.array_equal(built["rows"]["cpus"], want[1].offers.cpus)
        e.cycle_set_built_offers(True)
        CH.same_table(e.fetch_offers().offers(), PO.as_offers(built, tab2, op, True), "set_built_offers")
        assert _code(lambda: e.cycle_run_queue_pods(k, None, None, None, None, True)) == COOK_E_STATE  # the standing queue ended: rank first
        e.cycle_run(k)
        got = S.fetch(e, False)
    with make_engine(params) as e:  # the same rows through a fresh stage
        e.offers_stage(tab2.nodes, tab2.pods, op)
        e.offers_run()
        e.cycle_stage_built_offers(pool.tasks, pool.users, pool.pending_jobs, None, with_task_limits=True)
        e.cycle_set_considerable(want[1].state, cycles[0].eligible)
        e.cycle_run(k)
        ref = S.fetch(e, False)
    assert np.array_equal(got.Q, ref.Q) and np.array_equal(got.pos, ref.pos) and np.array_equal(got.j2o, ref.j2o) and (got.j2o >= 0).any()


def check_reserve_limiters(make_engine):
    """reservations released and replaced, and limiters with a clock, in the same advance as the pod delta: the queue cycle beside the
    composition that was there before (cook_offers_build on the mirrored tables, the rows as step offers of
    cook_cycle_run_queue_reserve) — identical queue, rank_pos, job_to_offer, head, limiters, reservations and their counters in
    every cycle; the pod table and the built rows against the oracle"""
    from tests import limiter_cases as LC
    params = P1()
    pool, nodes, pods, op, ids, id_cap, cycles = queue_case(6, 64, n_cycles=5)
    k, U = cycles[0].k, pool.users.n
    rng = np.random.default_rng(44)
    tabs, deltas = [PO.mirror(nodes, pods, ids)], [None]
    nxt = pods.n
    for c in range(1, 5):  # (deltas that do not depend on the placements: both ways take the same lists)
        tab = tabs[-1]
        add = some_pods(rng, 3, nodes.n)
        add = A.Pods(**{col: (getattr(add, col) if getattr(add, col) is not None else np.full(3, PO.NULL_MEANS[col], getattr(pods, col).dtype))
                        for col in PO.POD_COLS})
        d = A.PodDelta(remove=rng.choice(tab.ids, 6, replace=False), add=add, add_id=np.arange(nxt, nxt + 3, dtype=np.uint32))
        nxt += 3
        deltas.append(d)
        tabs.append(PO.apply_delta(tab, d)[0])
    lim = LC.random_limiters(5, U)
    resv = [None] + [A.Reservations(pending=rng.choice(pool.pending_jobs.n, 4, replace=False), host=rng.choice(nodes.host, 4, replace=False))
                     for _ in range(4)]

    def drive(resident):
        out = []
        with make_engine(params) as e:
            if resident:
                staged(e, nodes, pods, op, ids, id_cap)
                e.offers_run()
                e.cycle_stage_built_offers(pool.tasks, pool.users, pool.pending_jobs, None, with_task_limits=True)
            else:
                rows = e.offers_build(nodes, pods, op)
                e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs,
                              rows.as_offers(max_tasks=np.full(rows.n, op.max_pods_per_node, np.int32), num_tasks=rows.num_pods), None)
            e.cycle_set_considerable(cycles[0].state, cycles[0].eligible)
            e.cycle_set_limiters(lim)
            for c in range(5):
                e.cycle_set_clock(1000 + 900 * c, 1000 + 900 * c - (40 if c else 0))
                carry = A.QueueCarry(usage=True) if c else None
                if c == 0:
                    e.cycle_run(k)
                elif resident:
                    e.cycle_run_queue_pods(k, carry, None, deltas[c], resv[c], True)
                    same_pods(e, tabs[c], f"cycle {c}")
                    same_built(e.offers_fetch(), PO.build(tabs[c], op), tabs[c], f"cycle {c}")
                else:
                    rows = e.offers_build(tabs[c].nodes, tabs[c].pods, op)
                    e.cycle_run_queue_reserve(k, carry, None, None, resv[c], offers=rows.as_offers(
                        max_tasks=np.full(rows.n, op.max_pods_per_node, np.int32), num_tasks=rows.num_pods))
                g = S.fetch(e, False)
                g.lim, g.lim_info, g.resv_info, g.resv = e.fetch_limiters(U), e.limiter_info(), e.reserve_info(), e.fetch_reservations()
                g.rate = e.fetch_rate_limit(U)
                g.autoscale, g.why = e.cycle_autoscale(), e.match_explain(np.arange(min(8, len(g.j2o)), dtype=np.uint32))  # (they read this cycle's rows)
                out.append(g)
        return out
    new, old = drive(True), drive(False)
    assert sum(g.lim_info["spent"] for g in old) > 0 and sum(g.resv_info["installed"] for g in old) > 0, "nothing spent or reserved: re-seed the case"
    assert any(g.rate[0].any() for g in old), "the limiters stop nobody: re-seed the case"
    for c, (g, o) in enumerate(zip(new, old)):
        assert np.array_equal(g.Q, o.Q) and np.array_equal(g.pos, o.pos) and np.array_equal(g.j2o, o.j2o) and g.head == o.head, c
        assert all(np.array_equal(a, b) for a, b in zip(g.lim, o.lim)) and g.lim_info == o.lim_info, (c, g.lim_info, o.lim_info)
        assert all(np.array_equal(a, b) for a, b in zip(g.rate, o.rate)), c
        assert g.resv_info == o.resv_info and all(np.array_equal(a, b) for a, b in zip(g.resv, o.resv)), (c, g.resv_info, o.resv_info)
        assert (g.j2o >= 0).any() and (g.j2o < 0).any(), c
        assert np.array_equal(g.autoscale[0], o.autoscale[0]) and g.autoscale[1] == o.autoscale[1] and np.array_equal(g.why, o.why), c


# ---- 6: several pools ---------------------------------------------------------------------------------------------------------------------------
def check_multi(make_engine):
    """three pools in one call: one with a delta, one with pods = NULL, one that is refused; the others go on, the refused one is unchanged"""
    params = P1()
    cases = [queue_case(u, k, n_cycles=3, seed=900 + i) for i, (u, k) in enumerate(((3, 1), (6, 64), (11, 65)))]
    wants = [PO.oracle(params, c[0], PO.mirror(c[1], c[2], c[4]), c[3], c[6]) for c in cases]
    engines = [make_engine(params) for _ in cases]
    try:
        for e, (pool, nodes, pods, op, ids, id_cap, cycles) in zip(engines, cases):
            staged(e, nodes, pods, op, ids, id_cap)
            e.offers_run()
            e.cycle_stage_built_offers(pool.tasks, pool.users, pool.pending_jobs, None, with_task_limits=True)
            e.cycle_set_considerable(cycles[0].state, cycles[0].eligible)
            e.cycle_run(cycles[0].k)
        before = fetch(engines[2])
        pods_before = engines[2].offers_fetch_pods()
        bad = A.PodDelta(remove=[cases[2][5] + 1])  # an id at or above id_cap
        ks = [c[6][1].k for c in cases]
        with pytest.raises(CookError) as ex:
            cycle_run_queue_pods_multi(engines, ks, None, [K.carry_of(c[6][1]) for c in cases], [c[6][1].finished for c in cases],
                                       [cases[0][6][1].pods, None, bad], None, True)
        assert ex.value.code == COOK_E_INVALID
        cycle_match_multi(engines[:2])
        after = fetch(engines[2])
        CH._same_fetch(after, before)
        same_pods(engines[2], PO.mirror(cases[2][1], cases[2][2], pods_before.column("id")), "refused pool")
        S.compare([S.fetch(engines[0], False)], wants[0][1:2], cases[0][6][1:2], "pool 0")
        compare_cycle(engines[0], fetch(engines[0]), wants[0][1], 1, "pool 0")
        # pool 1 ran with pods = NULL: its table is the staged one, its rows are rebuilt from it
        tab1 = PO.mirror(cases[1][1], cases[1][2], cases[1][4])
        same_pods(engines[1], tab1, "pool 1")
        same_built(engines[1].offers_fetch(), PO.build(tab1, cases[1][3]), tab1, "pool 1")
        engines[2].cycle_run_queue_pods(ks[2], K.carry_of(cases[2][6][1]), cases[2][6][1].finished, cases[2][6][1].pods, None, True)  # the refused pool goes on alone
        S.compare([S.fetch(engines[2], False)], wants[2][1:2], cases[2][6][1:2], "pool 2")
    finally:
        for e in engines:
            e.close()


# ---- 7: refusals and state ------------------------------------------------------------------------------------------------------------------------
def check_refusals(make_engine):
    """every COOK_E_INVALID and COOK_E_STATE of the contract; the pod table, the id state, the queue and the staged offers before and after"""
    params = P1()
    pool, nodes, pods, op, ids, id_cap, cycles = queue_case(6, 64, n_cycles=3)
    k = cycles[0].k
    tab = PO.mirror(nodes, pods, ids)
    want = PO.oracle(params, pool, tab, op, cycles)
    live, dead = int(ids[3]), id_cap - 1
    one = A.Pods(**{c: np.array([v], getattr(pods, c).dtype) for c, v in dict(node=0, cpus=1.0, mem=1.0, gpus=0, gpu_model=0, disk=-1.0, disk_type=0, flags=0).items()})
    two = A.Pods(**{c: np.repeat(getattr(one, c), 2) for c in PO.POD_COLS})
    nv = A.Nodes(cpus=[1.0], mem=[1.0])
    invalid = [A.PodDelta(remove=[id_cap]), A.PodDelta(remove=[live, live]), A.PodDelta(add=one, add_id=[id_cap]),
               A.PodDelta(add=two, add_id=[dead, dead]), A.PodDelta(add=one, add_id=[live]), A.PodDelta(node_rows=[nodes.n], node_values=nv),
               A.PodDelta(node_rows=[1, 1], node_values=A.Nodes(cpus=[1.0, 1.0], mem=[1.0, 1.0])),
               A.PodDelta(node_rows=[1, 2], node_values=nv), A.PodDelta(node_rows=[1], node_values=A.Nodes(cpus=[1.0], mem=[1.0], attr=[[1, 2, 3, 4, 5]])),
               A.PodDelta(add=one, add_id=None)]
    with make_engine(params) as e:
        assert _code(lambda: e.offers_stage_pod_ids(ids, id_cap)) == COOK_E_STATE  # before cook_offers_stage
        assert _code(lambda: e.offers_update(A.PodDelta(remove=[1]))) == COOK_E_STATE
        e.offers_stage(nodes, pods, op)
        assert _code(lambda: e.offers_update(A.PodDelta(remove=[1]))) == COOK_E_STATE  # staged, but no ids
        assert _code(lambda: e.offers_stage_pod_ids(ids[:-1], id_cap)) == COOK_E_INVALID  # another row count
        assert _code(lambda: e.offers_stage_pod_ids(np.where(np.arange(len(ids)) == 1, ids[0], ids), id_cap)) == COOK_E_INVALID  # an id twice
        assert _code(lambda: e.offers_stage_pod_ids(ids, int(ids.max()))) == COOK_E_INVALID  # an id at id_cap
        assert _code(lambda: e.offers_update(A.PodDelta(remove=[1]))) == COOK_E_STATE  # a refused id list leaves no ids
        e.offers_stage_pod_ids(ids, id_cap)
        assert _code(lambda: e.cycle_set_built_offers(True)) == COOK_E_STATE  # before a cycle stage / cook_offers_run
        e.offers_run()
        built0 = e.offers_fetch()
        for d in invalid:
            assert _code(lambda: e.offers_update(d)) == COOK_E_INVALID, vars(d)
            same_pods(e, tab, "refused update")
        assert dataclasses.asdict(e.offers_fetch()).keys() == dataclasses.asdict(built0).keys()
        # offers staged from the host: the pods' queue cycle has nothing to rebuild into
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, None)
        e.cycle_set_considerable(cycles[0].state, cycles[0].eligible)
        e.cycle_run(k)
        assert _code(lambda: e.cycle_run_queue_pods(k, None, None, None, None, True)) == COOK_E_STATE
        e.cycle_stage_built_offers(pool.tasks, pool.users, pool.pending_jobs, None, with_task_limits=True)
        e.cycle_set_considerable(cycles[0].state, cycles[0].eligible)
        assert _code(lambda: e.cycle_run_queue_pods(k, None, None, None, None, True)) == COOK_E_STATE  # no completed cycle yet
        e.cycle_run(k)
        before = fetch(e)
        fin = A.Finished(cpus=[1.0], mem=[1.0], user=[0], host=[int(before.offers.host[0])], offers=True)
        refused = [lambda: e.cycle_run_queue_pods(k, None, None, None, None, True, offers=before.offers),
                   lambda: e.cycle_run_queue_pods(k, A.QueueCarry(offers=True, usage=True), None, None, None, True),
                   lambda: e.cycle_run_queue_pods(k, None, fin, None, None, True)]
        refused += [(lambda d=d: e.cycle_run_queue_pods(k, None, None, d, None, True)) for d in invalid]
        for x, fn in enumerate(refused):
            assert _code(fn) == COOK_E_INVALID, x
            CH._same_fetch(fetch(e), before)
            same_pods(e, tab, "refused queue cycle")
        assert _code(lambda: e.cycle_run_queue_hosts(k, None, None, A.HostChurn(leave=[int(before.offers.host[0])]))) == COOK_E_STATE  # the churn stays refused
        CH._same_fetch(fetch(e), before)
        # ... and after all that the case runs as if nothing had been asked
        e.cycle_run_queue_pods(k, K.carry_of(cycles[1]), getattr(cycles[1], "finished", None), cycles[1].pods, None, True)
        S.compare([S.fetch(e, False)], want[1:2], cycles[1:2], "after the refusals")
        compare_cycle(e, fetch(e), want[1], 1, "after the refusals")
        e.offers_stage(nodes, pods, op)  # a fresh stage drops the ids
        assert _code(lambda: e.offers_update(A.PodDelta(remove=[1]))) == COOK_E_STATE
        assert (e.offers_fetch_pods().column("id") == NONE).all()


# ---- 8: layouts ---------------------------------------------------------------------------------------------------------------------------------
def struct_layout_sources():
    """-> (a C program that prints size and field offsets of the new structs, then COOK_ABI_VERSION; the same numbers from the ctypes mirrors)"""
    structs = (("cook_pod_delta", A.CookPodDelta), ("cook_pod_delta_info", A.CookPodDeltaInfo), ("cook_pod_rows", A.CookPodRows))
    lines, want = [], []
    for cname, mirror in structs:
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        want.append(C.sizeof(mirror))
        for field, _ in mirror._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {field}));')
            want.append(getattr(mirror, field).offset)
    lines.append('printf("%d\\n", COOK_ABI_VERSION);')
    want.append(A.ABI_VERSION)
    return '#include <stddef.h>\n#include <stdio.h>\n#include "cookmatch.h"\nint main(void){' + "".join(lines) + "return 0;}", want
