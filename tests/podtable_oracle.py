"""Oracle of the resident pod table (cook_offers_stage_pod_ids, cook_offers_update, cook_cycle_run_queue_pods): a pod delta
applied to mirrored numpy tables by THE ORDER RULE of include/cookmatch.h — survivors keep their relative order, added rows go behind the
last survivor in list order, removes apply before adds —, then the existing offer oracle (oracle/k8s_offers.py, unchanged) over the
mirrored tables and the existing queue-cycle oracle (tests/churn_oracle.py, unchanged) with the built rows as every cycle's offers."""
from __future__ import annotations

import copy
from types import SimpleNamespace

import numpy as np

from cook_amd import _abi as A
from oracle import k8s_offers
from tests import churn_oracle as H

NONE = A.NONE_U32
POD_COLS = ("node", "cpus", "mem", "gpus", "gpu_model", "disk", "disk_type", "flags")
NODE_COLS = ("host", "cpus", "mem", "gpus", "gpu_model", "disk", "disk_type", "flags")
NULL_MEANS = dict(node=NONE, cpus=0.0, mem=0.0, gpus=0, gpu_model=0, disk=-1.0, disk_type=0, flags=0, host=0)
NO_INFO = dict(removed=0, remove_missing=0, added=0, node_rows=0)


def mirror(nodes: A.Nodes, pods: A.Pods, ids) -> SimpleNamespace:
    """the engine's tables as the host would keep them: copies (the deltas never edit the caller's)"""
    return SimpleNamespace(nodes=copy.deepcopy(nodes), pods=copy.deepcopy(pods), ids=np.array(ids, np.uint32))


def apply_delta(tab: SimpleNamespace, d: A.PodDelta):
    """-> (the tables behind the delta, the info counters)"""
    keep = ~np.isin(tab.ids, d.remove)
    removed = int((~keep).sum())
    n_add = d.add.n if d.add is not None else 0
    cols = {}
    for c in POD_COLS:
        old = getattr(tab.pods, c)
        if old is None:
            assert d.add is None or getattr(d.add, c) is None, f"add carries {c}, the table lacks it: the engine refuses"
            cols[c] = None
            continue
        new = getattr(d.add, c) if d.add is not None else None
        tail = new if new is not None else np.full(n_add, NULL_MEANS[c], old.dtype)
        cols[c] = np.concatenate([old[keep], tail.astype(old.dtype)])
    ids = np.concatenate([tab.ids[keep], d.add_id if n_add else np.zeros(0, np.uint32)]).astype(np.uint32)
    assert len(set(int(x) for x in ids)) == len(ids), "an id twice: the engine refuses"
    nodes = copy.deepcopy(tab.nodes)
    if len(d.node_rows):
        v = d.node_values
        for c in NODE_COLS:
            old = getattr(nodes, c)
            new = d.node_host if c == "host" else getattr(v, c)
            if old is None or (c == "host" and new is None):
                continue
            old[d.node_rows] = new if new is not None else NULL_MEANS[c]
        if nodes.attr is not None:
            nodes.attr[d.node_rows] = v.attr if v.attr is not None else 0
    info = dict(removed=removed, remove_missing=len(d.remove) - removed, added=n_add, node_rows=len(d.node_rows))
    return SimpleNamespace(nodes=nodes, pods=A.Pods(**cols), ids=ids), info


def build(tab: SimpleNamespace, op) -> dict:
    return k8s_offers.build_rows(tab.nodes, tab.pods, op)


def as_offers(built: dict, tab: SimpleNamespace, op, with_task_limits: bool) -> A.Offers:
    """the built rows as the offers of a match: the columns of cook_cycle_stage_built_offers"""
    r = built["rows"]
    M = len(r["cpus"])
    kw = dict(cpus=r["cpus"], mem=r["mem"], host=r["host"], k8s=np.ones(M, np.uint8), gpu_model=r["gpu_model"], gpu_count=r["gpu_count"],
              disk_type=r["disk_type"], disk_space=r["disk_space"])
    if tab.nodes.attr is not None:
        kw["attr"] = tab.nodes.attr[r["node"]]
    if with_task_limits:
        kw.update(max_tasks=np.full(M, op.max_pods_per_node, np.int32), num_tasks=r["num_pods"])
    return A.Offers(**kw)


def cycle(k, *, pods=None, rank=False, **kw):
    """churn_oracle.cycle (no churn) with the step's pod delta: an A.PodDelta, None (a rebuild from the table as it stands), or a function
    of (the results of the cycles so far, the mirrored tables) -> A.PodDelta or None that the oracle calls ONCE and replaces by what it
    returned.  rank: the cycle is a rank cycle behind cook_offers_update + cook_offers_run + cook_cycle_set_built_offers."""
    cy = H.cycle(k, **kw)
    cy.pods = pods
    cy.rank = rank
    return cy


def oracle(params, pool, tab0: SimpleNamespace, op, cycles, *, with_task_limits=True):
    """-> per cycle what churn_oracle.oracle gives, plus tab (the mirrored tables behind the cycle's delta), built (the offer oracle's
    answer over them) and pod_info.  pool.offers is set to the rows built from tab0: cycle 0 is the rank cycle on them.  Every later
    cycle's offers are the rows rebuilt behind its delta, handed to the queue-cycle oracle as the step's offers."""
    assert not any(cy.rank for cy in cycles), "a rank cycle in between restarts the queue: drive the parts apart (podtable_cases.check_rank_between)"
    tab, out = tab0, []
    built = build(tab, op)
    pool.offers = as_offers(built, tab, op, with_task_limits)
    extra = [SimpleNamespace(tab=tab, built=built, pod_info=dict(NO_INFO, n_pods=tab.pods.n, n_offers=pool.offers.n))]
    for c, cy in enumerate(cycles):
        if c:
            if callable(cy.pods):
                cy.pods = cy.pods(out, tab)
            info = dict(NO_INFO)
            if cy.pods is not None:
                tab, info = apply_delta(tab, cy.pods)
            built = build(tab, op)
            cy.offers = as_offers(built, tab, op, with_task_limits)
            extra.append(SimpleNamespace(tab=tab, built=built, pod_info=dict(info, n_pods=tab.pods.n, n_offers=cy.offers.n)))
        out = H.oracle(params, pool, cycles[:c + 1], with_churn=False)
        for w, x in zip(out, extra):
            w.tab, w.built, w.pod_info = x.tab, x.built, x.pod_info
    return out


def launched_pods(last, node_of_row, sidecar=0.1):
    """add-starting-pods: one pod per kept match of the last cycle, on its offer's node, with the job's requests plus the sidecar's cpus,
    in considered order -> (A.Pods or None)"""
    hit = np.flatnonzero(last.j2o >= 0)
    if not len(hit):
        return None
    J = last.jobs
    gp = J.gpus[hit].astype(np.int32) if J.gpus is not None else None
    gm = J.gpu_model[hit] if J.gpu_model is not None else None
    return A.Pods(node=node_of_row[last.j2o[hit]], cpus=J.cpus[hit] + sidecar, mem=J.mem[hit], gpus=gp, gpu_model=gm)
