"""The oracle of the release (cook_cycle_run_queue_release*): tests/carry_oracle.oracle's composition of the frozen
oracle.pyoracle calls — pyoracle.rank ONCE, then per cycle pyoracle.considerable over the current queue and pyoracle.match of the
considered jobs — with, between two cycles and behind the carry and the groups' fold, the release rules of include/cookmatch.h applied
to numpy copies of the offers, of the user state and of the groups' table with plain sequential Python loops (never np.sum): every sum
runs over the entries of its segment in LIST order, left to right, one IEEE-754 double add after another.  Nothing of the engine
produces an expected value."""
from __future__ import annotations

import copy
import dataclasses
from types import SimpleNamespace

import numpy as np

from cook_amd import _abi as A
from oracle import pyoracle
from tests import carry_oracle as O
from tests import queue_cases as S

_cp = O._cp
OFFER_COLS = ("cpus", "mem", "run_cpus", "run_mem", "run_count", "num_tasks", "ports", "scalars", "gpu_count", "disk_space")
STATE_COLS = ("usage_count", "usage_cpus", "usage_mem", "usage_gpus", "pool_usage")
NO_INFO = dict(with_row=0, without_row=0, counts_clamped=0, cotasks_removed=0, cotasks_missing=0)


def active(fin) -> bool:
    return fin is not None and fin.n > 0 and bool(fin.offers or fin.usage or fin.groups)


def rows_of(offers: A.Offers, fin: A.Finished):
    """per entry the row of the staged offers on its host, or -1"""
    row = {}
    for v in range(offers.n):
        assert int(offers.host[v]) not in row, "two offers on one host: the engine refuses the release"
        row[int(offers.host[v])] = v
    return [row.get(int(h), -1) for h in fin.host]


def release_offers(offers: A.Offers, fin: A.Finished):
    """-> (the staged offers after the entries came back, with_row, without_row, counts_clamped)"""
    M = offers.n
    ns_off = offers.n_scalars if offers.scalars is not None else 0
    ns_fin = fin.scalars.shape[1] if fin.scalars is not None else 0
    R_c, R_m, R_n, R_p = [0.0] * M, [0.0] * M, [0] * M, [0] * M
    R_s = [[0.0] * A.MAX_SCALARS for _ in range(M)]
    gm = None if offers.gpu_model is None else offers.gpu_model.reshape(M, -1)
    gc = None if offers.gpu_count is None else _cp(offers.gpu_count).reshape(M, -1)
    dt = None if offers.disk_type is None else offers.disk_type.reshape(M, -1)
    dsp = None if offers.disk_space is None else _cp(offers.disk_space).reshape(M, -1)
    rows = rows_of(offers, fin)
    without = 0
    for t, v in enumerate(rows):
        if v < 0:
            without += 1
            continue
        R_c[v] = R_c[v] + float(fin.cpus[t])
        R_m[v] = R_m[v] + float(fin.mem[t])
        R_n[v] += 1
        if fin.ports is not None and int(fin.ports[t]) > 0:
            R_p[v] += int(fin.ports[t])
        for s in range(ns_fin):
            r = float(fin.scalars[t, s])
            if r == r:
                R_s[v][s] = R_s[v][s] + r
        if offers.k8s is not None and offers.k8s[v]:
            g = float(fin.gpus[t]) if fin.gpus is not None else 0.0
            model = int(fin.gpu_model[t]) if fin.gpu_model is not None else 0
            if g > 0 and model != 0 and gc is not None and gm is not None:
                for s in range(gm.shape[1]):
                    if int(gm[v, s]) == model:
                        gc[v, s] = float(gc[v, s]) + g
            d = float(fin.disk_request[t]) if fin.disk_request is not None else -1.0
            typ = int(fin.disk_type[t]) if fin.disk_type is not None else 0
            if d >= 0 and typ != 0 and dsp is not None and dt is not None:
                for s in range(dt.shape[1]):
                    if int(dt[v, s]) == typ:
                        dsp[v, s] = float(dsp[v, s]) + d
    cpus, mem = _cp(offers.cpus), _cp(offers.mem)
    run_cpus = _cp(offers.run_cpus) if offers.run_cpus is not None else np.zeros(M)
    run_mem = _cp(offers.run_mem) if offers.run_mem is not None else np.zeros(M)
    run_count = _cp(offers.run_count) if offers.run_count is not None else np.zeros(M, np.int32)
    num_tasks = _cp(offers.num_tasks) if offers.num_tasks is not None else np.zeros(M, np.int32)
    ports = _cp(offers.ports) if offers.ports is not None else np.zeros(M, np.int32)
    scal = _cp(offers.scalars)
    clamped = 0
    for v in range(M):
        if R_n[v] == 0:
            continue
        cpus[v] = float(cpus[v]) + R_c[v]
        mem[v] = float(mem[v]) + R_m[v]
        run_cpus[v] = float(run_cpus[v]) - R_c[v]
        run_mem[v] = float(run_mem[v]) - R_m[v]
        rc, nt = int(run_count[v]) - R_n[v], int(num_tasks[v]) - R_n[v]
        run_count[v], num_tasks[v] = max(0, rc), max(0, nt)
        clamped += 1 if (rc < 0 or nt < 0) else 0
        ports[v] = int(ports[v]) + R_p[v]
        for s in range(ns_off):
            scal[v, s] = float(scal[v, s]) + R_s[v][s]
    new = A.Offers(cpus=cpus, mem=mem, host=_cp(offers.host), k8s=_cp(offers.k8s), gpu_model=_cp(offers.gpu_model),
                   gpu_count=None if gc is None else gc.reshape(offers.gpu_count.shape), disk_type=_cp(offers.disk_type),
                   disk_space=None if dsp is None else dsp.reshape(offers.disk_space.shape), attr=_cp(offers.attr),
                   max_tasks=_cp(offers.max_tasks), num_tasks=num_tasks, location=_cp(offers.location), host_start_s=_cp(offers.host_start_s),
                   run_cpus=run_cpus, run_mem=run_mem, run_count=run_count, ports=ports, scalars=scal)
    return new, len(rows) - without, without, clamped


def release_usage(state: A.UserState, fin: A.Finished) -> A.UserState:
    U = state.n
    S_c, S_m, S_g, N = [0.0] * U, [0.0] * U, [0.0] * U, [0] * U
    P_c = P_m = P_g = 0.0
    for t in range(fin.n):
        u = int(fin.user[t])
        c, m = float(fin.cpus[t]), float(fin.mem[t])
        g = float(fin.gpus[t]) if fin.gpus is not None else 0.0
        S_c[u] = S_c[u] + c
        S_m[u] = S_m[u] + m
        S_g[u] = S_g[u] + g
        N[u] += 1
        P_c = P_c + c
        P_m = P_m + m
        P_g = P_g + g
    st = dataclasses.replace(state, usage_count=_cp(state.usage_count), usage_cpus=_cp(state.usage_cpus), usage_mem=_cp(state.usage_mem),
                             usage_gpus=_cp(state.usage_gpus), tokens_left=_cp(state.tokens_left))
    for u in range(U):
        if N[u] == 0:
            continue
        st.usage_count[u] = float(st.usage_count[u]) - float(N[u])
        st.usage_cpus[u] = float(st.usage_cpus[u]) - S_c[u]
        st.usage_mem[u] = float(st.usage_mem[u]) - S_m[u]
        st.usage_gpus[u] = float(st.usage_gpus[u]) - S_g[u]
    if state.pool_usage is not None:
        p = state.pool_usage
        st.pool_usage = A.usage(p.count - float(fin.n), p.cpus - P_c, p.mem - P_m, p.gpus - P_g)
    return st


def release_groups(table, fin: A.Finished):
    """-> (the table without the first row on the entry's host per entry with a group, cotasks_removed, cotasks_missing)"""
    removed = missing = 0
    if fin.group is None:
        return table, 0, 0
    t2 = copy.deepcopy(table) if table is not None else None
    for t in range(fin.n):
        g = int(fin.group[t])
        if g == A.NONE_U32:
            continue
        h = int(fin.host[t])
        if t2 is not None and h in t2.run_hosts[g]:
            x = t2.run_hosts[g].index(h)
            del t2.run_hosts[g][x]
            del t2.run_attrs[g][x]
            removed += 1
        else:
            missing += 1
    return t2, removed, missing


def cycle(k, *, finished=None, **kw):
    """carry_oracle.cycle with the step's list of finished tasks: an A.Finished, None, or a function of the results of the cycles so far
    (-> A.Finished or None) that the oracle calls ONCE and replaces by what it returned, so that every later run of the same cycles
    (the engine's, and the oracle's runs with something left out) releases the same list"""
    cy = O.cycle(k, **kw)
    cy.finished = finished
    return cy


def oracle(params, pool, cycles, *, with_release=True, stale=()):
    """-> per cycle SimpleNamespace(Q, pos, j2o, head, offers, state, jobs, table, info, finished).  cycles[0] is the rank cycle on the
    pool's staged offers.  with_release=False: the same cycles with every release left out.  stale: names of OFFER_COLS / STATE_COLS /
    "groups" that the release leaves as they were (everything else released)."""
    J = pool.pending_jobs
    Q, _ = pyoracle.rank(params, pool.tasks, pool.users)
    table = S.group_table(pool.groups)
    offers, state, eligible, last, out = pool.offers, None, None, None, []
    for c, cy in enumerate(cycles):
        if cy.state is not None:
            state, eligible = cy.state, cy.eligible
        info = dict(NO_INFO)
        fin = None
        if c:
            hit = O.kept(last.j2o, cy.offer_skipped)
            if cy.carry:
                if cy.carry_offers:
                    offers = O.carry_offers(offers, last.jobs, last.j2o, hit)
                if cy.carry_usage:
                    state = O.carry_usage(state, last.jobs, hit, spend=cy.tokens_left is None)
                if cy.tokens_left is not None:
                    state = dataclasses.replace(state, tokens_left=_cp(cy.tokens_left))
            if cy.groups is not None:
                table = S.group_table(cy.groups)
            elif table is not None and J.group is not None:
                table = copy.deepcopy(table)
                for i in np.flatnonzero(hit):
                    g = int(last.jobs.group[i])
                    if g != A.NONE_U32:
                        o = int(last.j2o[i])
                        table.run_hosts[g].append(int(last.offers_matched.host[o]))
                        table.run_attrs[g].append(S.offer_attr(last.offers_matched, o, int(table.attr_key[g])))
            if callable(getattr(cy, "finished", None)):
                cy.finished = cy.finished(out)
            fin = getattr(cy, "finished", None)
            if with_release and active(fin):
                if fin.offers:
                    new, info["with_row"], info["without_row"], info["counts_clamped"] = release_offers(offers, fin)
                    offers = dataclasses.replace(new, **{x: getattr(offers, x) for x in stale if x in OFFER_COLS})
                if fin.usage:
                    new = release_usage(state, fin)
                    state = dataclasses.replace(new, **{x: getattr(state, x) for x in stale if x in STATE_COLS})
                if fin.groups:
                    new, info["cotasks_removed"], info["cotasks_missing"] = release_groups(table, fin)
                    table = table if "groups" in stale else new
            keep = np.ones(len(Q), bool)
            keep[last.pos[np.ones(len(hit), bool) if cy.remove_mode else hit]] = False
            Q = Q[keep]
            if cy.offers is not None:
                offers = cy.offers
        jq, queue = S._queue_of(pool, Q, eligible if state is not None else None)
        pos = pyoracle.considerable(queue, state, cy.k)[0] if state is not None else np.arange(min(cy.k, len(Q)), dtype=np.uint32)
        jobs = J.take(jq[pos])
        j2o, fail, head = pyoracle.match(params, jobs, offers, S.build_groups(table))
        last = SimpleNamespace(Q=Q, jq=jq, pos=pos, j2o=j2o, head=head, fail=fail, offers=offers, offers_matched=offers, state=state, jobs=jobs,
                               queue=queue, table=table, info=info, finished=fin)
        out.append(last)
    return out


# ---- lists of finished tasks ---------------------------------------------------------------------------------------------------------
def placed_rows(history):
    """(cycle, considered position) of every placement of the cycles so far"""
    return [(c, int(i)) for c, w in enumerate(history) for i in np.flatnonzero(w.j2o >= 0)]


def finished_of(history, picks, *, offers=0, usage=0, groups=0):
    """the list of finished tasks that are the placements `picks` ((cycle, considered position) pairs), in that order, with every
    column the pool's jobs carry"""
    if not picks:
        return None
    j0 = history[0].jobs
    col = lambda name, dt: None if getattr(j0, name) is None else np.array([getattr(history[c].jobs, name)[i] for c, i in picks], dt)
    host = np.array([history[c].offers.host[history[c].j2o[i]] for c, i in picks], np.uint32)
    return A.Finished(host=host, cpus=col("cpus", np.float64), mem=col("mem", np.float64), user=col("user", np.uint32), gpus=col("gpus", np.float64),
                      ports=col("ports", np.int32), scalars=col("scalars", np.float64), gpu_model=col("gpu_model", np.uint32),
                      disk_request=col("disk_request", np.float64), disk_type=col("disk_type", np.uint32), group=col("group", np.uint32),
                      offers=offers, usage=usage, groups=groups)


def finisher(seed, frac, **flags):
    """a function for cycle(finished=...): every placement of the cycles so far that no earlier step of this finisher released ends
    with probability `frac`, in a shuffled order (so: the last cycle's placements too — carried, folded and released in one advance)"""
    rng = np.random.default_rng(seed)
    gone = set()

    def draw(history):
        cand = [p for p in placed_rows(history) if p not in gone]
        picks = [p for p in cand if rng.random() < frac]
        picks = [picks[x] for x in rng.permutation(len(picks))]
        gone.update(picks)
        return finished_of(history, picks, **flags)
    return draw


def seq_sum(xs):
    s = 0.0
    for x in xs:
        s = s + float(x)
    return s


def pairwise_sum(xs):
    if len(xs) <= 1:
        return float(xs[0]) if len(xs) else 0.0
    m = len(xs) // 2
    return pairwise_sum(xs[:m]) + pairwise_sum(xs[m:])
