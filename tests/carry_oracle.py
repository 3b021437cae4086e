"""The oracle of the carry (cook_cycle_run_queue_carry*): the composition of the frozen oracle.pyoracle calls that
tests/queue_cases.oracle makes — pyoracle.rank ONCE, then per cycle pyoracle.considerable over the current queue and pyoracle.match of the
considered jobs — and, between two cycles, the carry rules of include/cookmatch.h applied to numpy copies of the offers and of the user
state with plain sequential Python loops (never np.sum): every sum runs over the kept placements in considered order, left to right,
one IEEE-754 double add after another.  Nothing of the engine produces an expected value."""
from __future__ import annotations

import copy
import dataclasses
from types import SimpleNamespace

import numpy as np

from cook_amd import _abi as A
from oracle import pyoracle
from tests import queue_cases as S


def _cp(a):
    return None if a is None else np.array(a, copy=True)


def kept(j2o, offer_skipped):
    hit = np.asarray(j2o) >= 0
    if offer_skipped is not None:
        hit &= np.asarray(offer_skipped, np.uint8)[np.maximum(j2o, 0)] == 0
    return hit


def carry_offers(offers: A.Offers, jobs: A.Jobs, j2o, hit) -> A.Offers:
    """the staged offers after the kept placements (jobs: the considered jobs in considered order, j2o their offers)"""
    M = offers.n
    ns_off = offers.n_scalars if offers.scalars is not None else 0
    ns_job = jobs.n_scalars if jobs.scalars is not None else 0
    A_c, A_m, A_n, A_p = [0.0] * M, [0.0] * M, [0] * M, [0] * M
    A_s = [[0.0] * A.MAX_SCALARS for _ in range(M)]
    gm = None if offers.gpu_model is None else offers.gpu_model.reshape(M, -1)
    gc = None if offers.gpu_count is None else _cp(offers.gpu_count).reshape(M, -1)
    dt = None if offers.disk_type is None else offers.disk_type.reshape(M, -1)
    dsp = None if offers.disk_space is None else _cp(offers.disk_space).reshape(M, -1)
    for i in range(len(j2o)):
        if not hit[i]:
            continue
        v = int(j2o[i])
        A_c[v] = A_c[v] + float(jobs.cpus[i])
        A_m[v] = A_m[v] + float(jobs.mem[i])
        A_n[v] += 1
        if jobs.ports is not None and int(jobs.ports[i]) > 0:
            A_p[v] += int(jobs.ports[i])
        for s in range(ns_job):
            r = float(jobs.scalars[i, s])
            if r == r:
                A_s[v][s] = A_s[v][s] + r
        if offers.k8s is not None and offers.k8s[v]:
            g = float(jobs.gpus[i]) if jobs.gpus is not None else 0.0
            model = int(jobs.gpu_model[i]) if jobs.gpu_model is not None else 0
            if g > 0 and model != 0 and gc is not None and gm is not None:
                for s in range(gm.shape[1]):
                    if int(gm[v, s]) == model:
                        gc[v, s] = float(gc[v, s]) - g
            d = float(jobs.disk_request[i]) if jobs.disk_request is not None else -1.0
            typ = int(jobs.disk_type[i]) if jobs.disk_type is not None else 0
            if d >= 0 and typ != 0 and dsp is not None:
                for s in range(dt.shape[1]):
                    if int(dt[v, s]) == typ:
                        dsp[v, s] = float(dsp[v, s]) - d
    cpus, mem = _cp(offers.cpus), _cp(offers.mem)
    run_cpus = _cp(offers.run_cpus) if offers.run_cpus is not None else np.zeros(M)
    run_mem = _cp(offers.run_mem) if offers.run_mem is not None else np.zeros(M)
    run_count = _cp(offers.run_count) if offers.run_count is not None else np.zeros(M, np.int32)
    num_tasks = _cp(offers.num_tasks) if offers.num_tasks is not None else np.zeros(M, np.int32)
    ports = _cp(offers.ports) if offers.ports is not None else np.zeros(M, np.int32)
    scal = _cp(offers.scalars)
    for v in range(M):
        cpus[v] = float(cpus[v]) - A_c[v]
        mem[v] = float(mem[v]) - A_m[v]
        run_cpus[v] = float(run_cpus[v]) + A_c[v]
        run_mem[v] = float(run_mem[v]) + A_m[v]
        run_count[v] = int(run_count[v]) + A_n[v]
        num_tasks[v] = int(num_tasks[v]) + A_n[v]
        ports[v] = int(ports[v]) - A_p[v]
        for s in range(ns_off):
            scal[v, s] = float(scal[v, s]) - A_s[v][s]
    return A.Offers(cpus=cpus, mem=mem, host=_cp(offers.host), k8s=_cp(offers.k8s), gpu_model=_cp(offers.gpu_model),
                    gpu_count=None if gc is None else gc.reshape(offers.gpu_count.shape), disk_type=_cp(offers.disk_type),
                    disk_space=None if dsp is None else dsp.reshape(offers.disk_space.shape), attr=_cp(offers.attr),
                    max_tasks=_cp(offers.max_tasks), num_tasks=num_tasks, location=_cp(offers.location), host_start_s=_cp(offers.host_start_s),
                    run_cpus=run_cpus, run_mem=run_mem, run_count=run_count, ports=ports, scalars=scal)


def carry_usage(state: A.UserState, jobs: A.Jobs, hit, spend: bool) -> A.UserState:
    """the staged user state after the kept placements; spend: one token per kept job of a user"""
    U = state.n
    S_c, S_m, S_g, N = [0.0] * U, [0.0] * U, [0.0] * U, [0] * U
    P_c = P_m = P_g = 0.0
    P_n = 0
    for i in range(len(hit)):
        if not hit[i]:
            continue
        u = int(jobs.user[i])
        c, m = float(jobs.cpus[i]), float(jobs.mem[i])
        g = float(jobs.gpus[i]) if jobs.gpus is not None else 0.0
        S_c[u] = S_c[u] + c
        S_m[u] = S_m[u] + m
        S_g[u] = S_g[u] + g
        N[u] += 1
        P_c = P_c + c
        P_m = P_m + m
        P_g = P_g + g
        P_n += 1
    st = dataclasses.replace(state, usage_count=_cp(state.usage_count), usage_cpus=_cp(state.usage_cpus), usage_mem=_cp(state.usage_mem),
                             usage_gpus=_cp(state.usage_gpus), tokens_left=_cp(state.tokens_left))
    for u in range(U):
        if N[u] == 0:
            continue
        st.usage_count[u] = float(st.usage_count[u]) + float(N[u])
        st.usage_cpus[u] = float(st.usage_cpus[u]) + S_c[u]
        st.usage_mem[u] = float(st.usage_mem[u]) + S_m[u]
        st.usage_gpus[u] = float(st.usage_gpus[u]) + S_g[u]
        if spend and st.tokens_left is not None:
            st.tokens_left[u] = int(st.tokens_left[u]) - N[u]
    if state.pool_usage is not None:
        p = state.pool_usage
        st.pool_usage = A.usage(p.count + float(P_n), p.cpus + P_c, p.mem + P_m, p.gpus + P_g)
    return st


def cycle(k, *, state=None, eligible=None, offers=None, offer_skipped=None, remove_mode=0, carry_offers=False, carry_usage=False,
          tokens_left=None, carry=True, groups=None):
    """one cycle of a case.  state / eligible: cook_cycle_set_considerable in front of the cycle (None: what is staged stays);
    offers: the step's replacement; carry=False: the step goes through cook_cycle_run_queue (no carry struct at all)"""
    return SimpleNamespace(k=k, state=state, eligible=eligible, offers=offers, offer_skipped=offer_skipped, remove_mode=remove_mode,
                           carry_offers=carry_offers, carry_usage=carry_usage, tokens_left=_cp(tokens_left), carry=carry, groups=groups)


def oracle(params, pool, cycles, *, with_carry=True, start=None):
    """-> per cycle SimpleNamespace(Q, pos, j2o, head, offers, state, jobs, fail).  cycles[0] is the rank cycle on the pool's staged offers.
    with_carry=False: the same cycles with every carry switched off (stale offers, stale usage)."""
    J = pool.pending_jobs
    Q, _ = pyoracle.rank(params, pool.tasks, pool.users)
    table = S.group_table(pool.groups)
    offers, state, eligible, last, out = pool.offers, None, None, None, []
    for c, cy in enumerate(cycles):
        if cy.state is not None:
            state, eligible = cy.state, cy.eligible
        if c:
            hit = kept(last.j2o, cy.offer_skipped)
            if with_carry and cy.carry:
                if cy.carry_offers:
                    offers = carry_offers(offers, last.jobs, last.j2o, hit)
                if cy.carry_usage:
                    state = carry_usage(state, last.jobs, hit, spend=cy.tokens_left is None)
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
                        table.run_hosts[g].append(int(last.offers.host[o]))
                        table.run_attrs[g].append(S.offer_attr(last.offers, o, int(table.attr_key[g])))
            keep = np.ones(len(Q), bool)
            keep[last.pos[np.ones(len(hit), bool) if cy.remove_mode else hit]] = False
            Q = Q[keep]
            if cy.offers is not None:
                offers = cy.offers
        jq, queue = S._queue_of(pool, Q, eligible if state is not None else None)
        pos = pyoracle.considerable(queue, state, cy.k)[0] if state is not None else np.arange(min(cy.k, len(Q)), dtype=np.uint32)
        jobs = J.take(jq[pos])
        j2o, fail, head = pyoracle.match(params, jobs, offers, S.build_groups(table))
        last = SimpleNamespace(Q=Q, jq=jq, pos=pos, j2o=j2o, head=head, fail=fail, offers=offers, state=state, jobs=jobs, queue=queue)
        out.append(last)
    return out


def quota_rejected(queue: A.Queue, state: A.UserState):
    """queue positions the per-user quota filter rejects (tools.clj:903-915: the running state advances on rejected jobs too), by a
    sequential walk of its own"""
    U = state.n
    use = [[float(state.usage_count[u]), float(state.usage_cpus[u]), float(state.usage_mem[u]), float(state.usage_gpus[u])] for u in range(U)]
    out = []
    for q in range(queue.n):
        u = int(queue.user[q])
        x = use[u]
        x[0] = x[0] + 1.0
        x[1] = x[1] + float(queue.cpus[q])
        x[2] = x[2] + float(queue.mem[q])
        x[3] = x[3] + float(queue.gpus[q])
        if not (x[0] <= state.quota_count[u] and x[1] <= state.quota_cpus[u] and x[2] <= state.quota_mem[u] and x[3] <= state.quota_gpus[u]):
            out.append(q)
    return np.asarray(out, dtype=np.int64)
