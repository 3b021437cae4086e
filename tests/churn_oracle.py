"""The oracle of the host churn (cook_cycle_run_queue_hosts*): tests/release_oracle.oracle's composition of the frozen
oracle.pyoracle calls — pyoracle.rank ONCE, then per cycle pyoracle.considerable over the current queue and pyoracle.match of the
considered jobs — with, between two cycles and behind the carry, the groups' fold and the release, the churn rules of
include/cookmatch.h applied to the offer table as plain Python list edits: the rows of the leaving hosts go, the survivors keep their
order, every joining row goes directly in front of its anchor's OLD position, rows of one anchor in list order.  Nothing of the engine
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
from tests import release_oracle as R

NONE = A.NONE_U32
NO_CHURN = dict(left=0, leave_missing=0, joined=0)  # (+ n_offers)
# every column of a table besides cpus, mem and host, with what a NULL column means for every row (the loads of match_kernels.hpp)
NULLS = dict(k8s=0, gpu_model=0, gpu_count=0.0, disk_type=0, disk_space=0.0, attr=0, max_tasks=-1, num_tasks=0, location=0, host_start_s=-1,
             run_cpus=0.0, run_mem=0.0, run_count=0, ports=0, scalars=0.0)
COLS = ("cpus", "mem", "host") + tuple(NULLS)


def active(hosts) -> bool:
    return hosts is not None and (len(hosts.leave) > 0 or (hosts.join is not None and hosts.join.n > 0))


def new_order(old_hosts, hosts: A.HostChurn, *, leave=True):
    """-> (src, left, leave_missing): src[d] = ("old", r) or ("join", i) for row d of the new table"""
    M = len(old_hosts)
    row = {}
    for r, h in enumerate(old_hosts):
        assert int(h) not in row, "two offers on one host: the engine refuses the churn"
        row[int(h)] = r
    leaving, missing = set(), 0
    for h in hosts.leave:
        if int(h) in row:
            leaving.add(row[int(h)])
        else:
            missing += 1
    at = [[] for _ in range(M + 1)]  # joins per anchor position, list order
    nj = hosts.join.n if hosts.join is not None else 0
    for i in range(nj):
        b = NONE if hosts.before is None else int(hosts.before[i])
        if b != NONE:
            assert b in row, "join_before names a host that is not an OLD row: the engine refuses the churn"
        if not leave and int(hosts.join.host[i]) in row:
            continue  # (the variant without the leaves: a host that would have been replaced stays as it is)
        at[M if b == NONE else row[b]].append(i)
    src = []
    for r in range(M + 1):
        src += [("join", i) for i in at[r]]
        if r < M and not (leave and r in leaving):
            src.append(("old", r))
    return src, len(leaving), missing


def churn_offers(offers: A.Offers, hosts: A.HostChurn, *, leave=True):
    """-> (the staged offers behind the churn, cook_churn_info as a dict)"""
    M = offers.n
    join = hosts.join
    src, left, missing = new_order(offers.host, hosts, leave=leave)
    cols = {}
    for name in COLS:
        old = getattr(offers, name)
        if old is None:
            assert join is None or getattr(join, name) is None, f"join carries {name}, the staged offers lack it: the engine refuses the churn"
            cols[name] = None
            continue
        jn = getattr(join, name) if join is not None else None
        shape = old.shape[1:]
        assert jn is None or jn.shape[1:] == shape, (name, jn.shape, old.shape)
        rows = []
        for kind, x in src:
            if kind == "old":
                rows.append(np.array(old[x], copy=True))
            elif jn is not None:
                rows.append(np.array(jn[x], copy=True))
            else:
                rows.append(np.full(shape, NULLS[name], old.dtype))
        cols[name] = np.array(rows, old.dtype).reshape((len(rows),) + shape)
    new = A.Offers(**cols)
    joined = sum(1 for kind, _ in src if kind == "join")
    return new, dict(left=left if leave else 0, leave_missing=missing if leave else 0, joined=joined, n_offers=new.n)


def cycle(k, *, hosts=None, **kw):
    """release_oracle.cycle with the step's host churn: an A.HostChurn, None, or a function of (the results of the cycles so far, the
    offers behind the release) -> A.HostChurn or None that the oracle calls ONCE and replaces by what it returned"""
    cy = R.cycle(k, **kw)
    cy.hosts = hosts
    return cy


def oracle(params, pool, cycles, *, with_churn=True, leave=True, with_release=True):
    """-> per cycle SimpleNamespace(Q, pos, j2o, head, offers (the WHOLE table the cycle's match saw), state, jobs, table, info, finished,
    churn, hosts).  with_churn=False: the same cycles with every churn left out; leave=False: with the joins but without the leaves."""
    J = pool.pending_jobs
    Q, _ = pyoracle.rank(params, pool.tasks, pool.users)
    table = S.group_table(pool.groups)
    offers, state, eligible, last, out = pool.offers, None, None, None, []
    for c, cy in enumerate(cycles):
        if cy.state is not None:
            state, eligible = cy.state, cy.eligible
        info = dict(R.NO_INFO)
        churn = dict(NO_CHURN, n_offers=offers.n)
        fin = hosts = None
        if c:
            hit = O.kept(last.j2o, cy.offer_skipped)
            if cy.carry:
                if cy.carry_offers:
                    offers = O.carry_offers(offers, last.jobs, last.j2o, hit)
                if cy.carry_usage:
                    state = O.carry_usage(state, last.jobs, hit, spend=cy.tokens_left is None)
                if cy.tokens_left is not None:
                    state = dataclasses.replace(state, tokens_left=O._cp(cy.tokens_left))
            if cy.groups is not None:
                table = S.group_table(cy.groups)
            elif table is not None and J.group is not None:
                table = copy.deepcopy(table)
                for i in np.flatnonzero(hit):
                    g = int(last.jobs.group[i])
                    if g != NONE:
                        o = int(last.j2o[i])
                        table.run_hosts[g].append(int(last.offers.host[o]))
                        table.run_attrs[g].append(S.offer_attr(last.offers, o, int(table.attr_key[g])))
            if callable(getattr(cy, "finished", None)):
                cy.finished = cy.finished(out)
            fin = getattr(cy, "finished", None)
            if with_release and R.active(fin):
                if fin.offers:
                    offers, info["with_row"], info["without_row"], info["counts_clamped"] = R.release_offers(offers, fin)
                if fin.usage:
                    state = R.release_usage(state, fin)
                if fin.groups:
                    table, info["cotasks_removed"], info["cotasks_missing"] = R.release_groups(table, fin)
            if callable(getattr(cy, "hosts", None)):
                cy.hosts = cy.hosts(out, offers)
            hosts = getattr(cy, "hosts", None)
            churn = dict(NO_CHURN, n_offers=offers.n)
            if with_churn and active(hosts):
                offers, churn = churn_offers(offers, hosts, leave=leave)
            keep = np.ones(len(Q), bool)
            keep[last.pos[np.ones(len(hit), bool) if cy.remove_mode else hit]] = False
            Q = Q[keep]
            if cy.offers is not None:
                offers = cy.offers
                churn = dict(NO_CHURN, n_offers=offers.n)
        jq, queue = S._queue_of(pool, Q, eligible if state is not None else None)
        pos = pyoracle.considerable(queue, state, cy.k)[0] if state is not None else np.arange(min(cy.k, len(Q)), dtype=np.uint32)
        jobs = J.take(jq[pos])
        j2o, fail, head = pyoracle.match(params, jobs, offers, S.build_groups(table))
        last = SimpleNamespace(Q=Q, jq=jq, pos=pos, j2o=j2o, head=head, fail=fail, offers=offers, state=state, jobs=jobs, queue=queue,
                               table=table, info=info, finished=fin, churn=churn, hosts=hosts)
        out.append(last)
    return out


def table_columns(offers: A.Offers, like: A.Offers = None):
    """name -> the column as [n, width]; a column the table lacks: filled with its NULL meaning at the width of `like`'s (or 1)"""
    n = offers.n
    out = {}
    for name in COLS:
        a = getattr(offers, name)
        if a is None:
            ref = getattr(like, name) if like is not None else None
            if ref is None and name in ("attr", "scalars"):
                out[name] = None
                continue
            w = 1 if ref is None else int(np.asarray(ref).reshape(n, -1).shape[1]) if n else 1
            dt = np.float64 if isinstance(NULLS[name], float) else (ref.dtype if ref is not None else np.int64)
            a = np.full((n, w), NULLS[name], dt)
        a = np.asarray(a)
        out[name] = a.reshape(n, -1) if n else np.zeros((0, 1), a.dtype)  # (no rows: the widths say nothing)
    return out


# ---- lists of hosts --------------------------------------------------------------------------------------------------------------------
def rows_like(offers: A.Offers, idx, host):
    """joining rows with the columns of `offers`: copies of its rows idx under the host ids `host`"""
    d = {}
    for name in COLS:
        a = getattr(offers, name)
        d[name] = None if a is None else np.array(a[np.asarray(idx, np.int64)], copy=True)
    d["host"] = np.asarray(host, np.uint32)
    return A.Offers(**d)


def churner(seed, frac, *, fresh_from=1_000_000, template=None, extra=0):
    """a function for cycle(hosts=...): a fraction `frac` of the staged hosts leaves (at least one) and as many rows join: about half of
    them (+ extra) are hosts that left in an earlier step and return, the others new host ids; each in front of a random old row or at the end.
    A joining row is a copy of a random row of `template` (the pool's first offers: a free host) under its own host id."""
    rng = np.random.default_rng(seed)
    away, nxt = [], [fresh_from]

    def draw(history, offers):
        M = offers.n
        tpl = offers if isinstance(template, str) else template if template is not None else history[0].offers  # ("current": the table as it stands)
        if tpl.n == 0:
            return None
        n = max(1, int(round(frac * M)))
        leave = [int(h) for h in rng.choice(offers.host, min(n, M), replace=False)] if M else []
        hosts = []
        staged = set(int(h) for h in offers.host)
        away[:] = [h for h in away if h not in staged]  # (a step that replaced the offers may have brought a host back)
        for _ in range(n + extra):
            if away and rng.random() < 0.5:
                hosts.append(away.pop(int(rng.integers(len(away)))))
            else:
                hosts.append(nxt[0])
                nxt[0] += 1
        before = [int(offers.host[int(rng.integers(M))]) if (M and rng.random() < 0.8) else NONE for _ in range(n + extra)]
        away.extend(leave)
        join = rows_like(tpl, rng.integers(0, tpl.n, n + extra), hosts)
        # a host that is not staged once in a while: leave_missing
        if rng.random() < 0.5:
            leave.append(nxt[0] + 500_000)
        return A.HostChurn(leave=leave, join=join, before=before)
    return draw
