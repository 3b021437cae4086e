"""The oracle of the host reservations (cook_cycle_set_reservations, cook_cycle_run_queue_reserve*):
tests/churn_oracle.oracle's composition of the frozen oracle.pyoracle calls — pyoracle.rank ONCE, then per cycle pyoracle.considerable
over the current queue and pyoracle.match of the considered jobs — with the reference's atom kept as a Python dict (pending row ->
host; a job outside the pool under a key of its own) plus a set (`launched`).  Between two cycles, behind the carry, the groups' fold,
the release and the churn, the two Clojure functions are applied as they read: update-host-reservations! (scheduler.clj:1050-1057)
over the last cycle's kept matches, reserve-hosts! (rebalancer.clj:419-432) with the step's list.  The match gets
reserved_hosts = set(map.values()) and the considered jobs a reserved_host column made from the map (scheduler.clj:645-653,
constraints.clj:242-252).  Nothing of the engine produces an expected value."""
from __future__ import annotations

import copy
import dataclasses
from types import SimpleNamespace

import numpy as np

from cook_amd import _abi as A
from oracle import pyoracle
from tests import carry_oracle as O
from tests import churn_oracle as H
from tests import queue_cases as S
from tests import release_oracle as R

NONE = A.NONE_U32
NO_RESERVE = dict(released=0, installed=0, dropped_launched=0)  # (+ alive)


class Atom:
    """{:job-uuid->reserved-host {} :launched-job-uuids #{}} of one pool: rows are pending ordinals; own: the engine holds a map"""

    def __init__(self):
        self.map, self.launched, self.own = {}, set(), False

    def update_host_reservations(self, matched_rows):
        """-> reservations released"""
        released = sum(1 for r in matched_rows if r in self.map)
        self.map = {k: v for k, v in self.map.items() if k not in set(matched_rows)}  # (apply dissoc job-uuid->reserved-host matched)
        self.launched = self.launched | set(matched_rows)                                # (into launched-job-uuids matched)
        return released

    def reserve_hosts(self, pending, host):
        """-> (installed, dropped_launched)"""
        new = {}
        for i, (p, h) in enumerate(zip(pending, host)):
            key = ("outside", i) if int(p) == NONE else int(p)
            assert key not in new, "a pending row twice: the engine refuses the list"
            new[key] = int(h)
        dropped = sum(1 for k in new if k in self.launched)
        self.map = {k: v for k, v in new.items() if k not in self.launched}  # (apply dissoc reservations launched-job-uuids)
        self.launched = set()                                                 # :launched-job-uuids #{}
        self.own = True
        return len(self.map), dropped

    def pairs(self):
        """the map as cook_cycle_fetch_reservations shows it: a set of (pending or NONE, host)"""
        return {(NONE if isinstance(k, tuple) else k, v) for k, v in self.map.items()}

    def reserved_hosts(self):
        return sorted(set(self.map.values()))

    def column(self, rows):
        return np.array([self.map.get(int(r), -1) for r in rows], np.int32)


def cycle(k, *, reservations=None, set_reservations=None, **kw):
    """churn_oracle.cycle with the step's cook_reservations: an A.Reservations, None, or a function of (the results of the cycles so
    far, the atom in front of the step) -> A.Reservations or None that the oracle calls ONCE and replaces by what it returned.
    set_reservations: an A.Reservations handed to cook_cycle_set_reservations in front of the cycle (a rank cycle too)."""
    cy = H.cycle(k, **kw)
    cy.reservations, cy.set_reservations = reservations, set_reservations
    return cy


def oracle(params, pool, cycles, *, frozen=False, staged_reserved=(), staged_column=None):
    """-> per cycle SimpleNamespace(... of churn_oracle.oracle ..., reserve (cook_reserve_info as a dict), pairs (the atom as a set of
    pairs), reserved (the hosts the match kept jobs off), rows (the considered jobs' pending ordinals)).  frozen=True: today's
    behaviour — the first list that is installed stays for good (no release, no later replacement, nothing dropped).
    staged_reserved / staged_column: what cook_cycle_stage was given, read until the engine holds a map of its own."""
    J = pool.pending_jobs
    Q, _ = pyoracle.rank(params, pool.tasks, pool.users)
    table = S.group_table(pool.groups)
    offers, state, eligible, last, out = pool.offers, None, None, None, []
    atom = Atom()
    for c, cy in enumerate(cycles):
        if cy.state is not None:
            state, eligible = cy.state, cy.eligible
        info = dict(R.NO_INFO)
        churn = dict(H.NO_CHURN, n_offers=offers.n)
        reserve = dict(NO_RESERVE, alive=len(atom.map))
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
            if R.active(fin):
                if fin.offers:
                    offers, info["with_row"], info["without_row"], info["counts_clamped"] = R.release_offers(offers, fin)
                if fin.usage:
                    state = R.release_usage(state, fin)
                if fin.groups:
                    table, info["cotasks_removed"], info["cotasks_missing"] = R.release_groups(table, fin)
            if callable(getattr(cy, "hosts", None)):
                cy.hosts = cy.hosts(out, offers)
            hosts = getattr(cy, "hosts", None)
            churn = dict(H.NO_CHURN, n_offers=offers.n)
            if H.active(hosts):
                offers, churn = H.churn_offers(offers, hosts)
            # ---- the atom: update-host-reservations!, then reserve-hosts! ---------------------------------------------------------------
            if callable(getattr(cy, "reservations", None)):
                cy.reservations = cy.reservations(out, atom)
            rv = getattr(cy, "reservations", None)
            if rv is not None and (rv.release_matched or rv.replace):
                if frozen:
                    if rv.replace and not atom.own:
                        atom.reserve_hosts(rv.pending, rv.host)
                else:
                    if rv.release_matched:
                        assert atom.own or rv.replace, "release_matched without a map: the engine refuses the step"
                        reserve["released"] = atom.update_host_reservations([int(last.rows[i]) for i in np.flatnonzero(hit)])
                    if rv.replace:
                        reserve["installed"], reserve["dropped_launched"] = atom.reserve_hosts(rv.pending, rv.host)
                reserve["alive"] = len(atom.map)
            keep = np.ones(len(Q), bool)
            keep[last.pos[np.ones(len(hit), bool) if cy.remove_mode else hit]] = False
            Q = Q[keep]
            if cy.offers is not None:
                offers = cy.offers
                churn = dict(H.NO_CHURN, n_offers=offers.n)
        sr = getattr(cy, "set_reservations", None)
        if sr is not None and not (frozen and atom.own):
            inst, drop = atom.reserve_hosts(sr.pending, sr.host) if sr.replace else (0, 0)  # (replace = 0: nothing changes)
            reserve = dict(released=0, installed=inst, dropped_launched=drop, alive=len(atom.map))
        jq, queue = S._queue_of(pool, Q, eligible if state is not None else None)
        pos = pyoracle.considerable(queue, state, cy.k)[0] if state is not None else np.arange(min(cy.k, len(Q)), dtype=np.uint32)
        rows = np.asarray(jq[pos], np.int64)
        jobs = J.take(rows)
        if atom.own:
            reserved = atom.reserved_hosts()
            jobs = dataclasses.replace(jobs, reserved_host=atom.column(rows))
        else:
            reserved = sorted(set(int(h) for h in staged_reserved))
            if staged_column is not None:
                jobs = dataclasses.replace(jobs, reserved_host=np.asarray(staged_column, np.int32)[rows])
        j2o, fail, head = pyoracle.match(params, jobs, offers, S.build_groups(table), reserved_hosts=reserved)
        last = SimpleNamespace(Q=Q, jq=jq, pos=pos, j2o=j2o, head=head, fail=fail, offers=offers, state=state, jobs=jobs, queue=queue,
                               table=table, info=info, finished=fin, churn=churn, hosts=hosts, reserve=reserve, pairs=atom.pairs(),
                               reserved=reserved, rows=rows, reservations=getattr(cy, "reservations", None))
        out.append(last)
    return out


def refused_by_reservation(w, params, table_groups=None):
    """considered positions of cycle result w that are unmatched or placed elsewhere with the reservations, and that the same match
    WITHOUT any reservation places on a host that is reserved for another job: -> [(position, pending row, host)]"""
    if not w.reserved:
        return []
    free = dataclasses.replace(w.jobs, reserved_host=None)
    j2o, _, _ = pyoracle.match(params, free, w.offers, S.build_groups(w.table))
    res = set(w.reserved)
    out = []
    for i in range(len(j2o)):
        o = int(j2o[i])
        if o >= 0 and int(w.offers.host[o]) in res and int(w.j2o[i]) != o and int(w.jobs.reserved_host[i]) != int(w.offers.host[o]):
            out.append((i, int(w.rows[i]), int(w.offers.host[o])))
    return out
