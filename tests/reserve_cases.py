"""The cases of the host reservations (cook_cycle_set_reservations, cook_cycle_run_queue_reserve*: the rebalancer's reserved hosts kept
on the device across match cycles), shared by the emulator (test_reserve_emu.py) and GPU (test_reserve_gpu.py) suites.  Expected values
come from tests/reserve_oracle.py alone.  Per cycle the queue, rank_pos, job_to_offer, head_matched, the considered count,
cook_reserve_info and cook_cycle_fetch_reservations (as a set of pairs) are compared with the oracle; all integers, so exactly.  The
conditions that make a case mean something are asserted on the oracle alone, before the engine is called."""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest

from cook_amd import _abi as A
from cook_amd.engine import CookError, cycle_match_multi, cycle_run_queue_reserve_multi, cycle_run_rank_multi, reservations_of
from tests import carry_cases as K
from tests import carry_oracle as O
from tests import churn_cases as CH
from tests import queue_cases as S
from tests import release_cases as X
from tests import reserve_oracle as V

COOK_E_INVALID, COOK_E_STATE = -1, -4
WHY_RESERVATION = 10
NONE = A.NONE_U32
P1 = K.P1
_code = X._code
Rsv = A.Reservations
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reservations.json")


# ---- engine side -------------------------------------------------------------------------------------------------------------------
def pairs_of(e):
    pend, host = e.fetch_reservations()
    got = {(int(p), int(h)) for p, h in zip(pend, host)}
    assert len(got) == len(pend) or NONE in pend.tolist()  # (rows are unique; several jobs outside the pool may share a host)
    return got, len(pend)


def fetch(e):
    g = S.fetch(e, False)
    g.info, g.churn, g.reserve = e.release_info(), e.churn_info(), e.reserve_info()
    g.pairs, g.n_pairs = pairs_of(e)
    return g


def run_step(e, cy):
    fin, hosts, rv = getattr(cy, "finished", None), getattr(cy, "hosts", None), getattr(cy, "reservations", None)
    assert not callable(fin) and not callable(hosts) and not callable(rv), "run the oracle first: it draws the lists"
    e.cycle_run_queue_reserve(cy.k, K.carry_of(cy), fin, hosts, rv, **K.step_kw(cy))


def run_engine(make_engine, params, pool, cycles, *, forms=None, between=None, stage=None):
    """forms: per cycle the expected placement_form (None: not looked at)"""
    got = []
    with make_engine(params) as e:
        (stage or (lambda e: e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)))(e)
        for c, cy in enumerate(cycles):
            if cy.state is not None:
                e.cycle_set_considerable(cy.state, cy.eligible)
            sr = getattr(cy, "set_reservations", None)
            if c == 0:
                if sr is not None:
                    e.cycle_set_reservations(sr)
                e.cycle_run(cy.k)
            else:
                run_step(e, cy)
                assert sr is None, "set_reservations in front of a queue cycle: hand the list to the step"
            got.append(fetch(e))
            if forms is not None and forms[c] is not None and len(got[-1].j2o):
                ms = e.match_stats()
                assert ms["placement_form"] == forms[c], (c, ms["placement_form"], hex(ms["classfit_refused"]))
                got[-1].refused = ms["classfit_refused"]
            if between is not None:
                between(e, c)
    return got


def compare(got, want, cycles, tag=""):
    S.compare(got, want, cycles, tag)
    for c, (g, w) in enumerate(zip(got, want)):
        where = f"{tag} cycle {c}"
        assert g.info == w.info, (where, "release_info", g.info, w.info)
        assert g.churn == w.churn, (where, "churn_info", g.churn, w.churn)
        if c or getattr(cycles[c], "set_reservations", None) is not None:
            assert g.reserve == w.reserve, (where, "reserve_info", g.reserve, w.reserve)
        assert g.pairs == w.pairs and g.n_pairs == w.reserve["alive"], (where, "reservations", sorted(g.pairs)[:8], sorted(w.pairs)[:8])


def check(make_engine, params, pool, cycles, want, **kw):
    got = run_engine(make_engine, params, pool, cycles, **kw)
    compare(got, want, cycles)
    return got


# ---- 1: base ---------------------------------------------------------------------------------------------------------------------------
def reserver(seed, *, n_hosts=8, per_host=1, replace_in=(1, 3)):
    """a function for cycle(reservations=...): every step releases; the steps `replace_in` replace the map by a list drawn from the
    last cycle: the hosts with the most cpus left (the only ones the large jobs fit on), each for a job the last cycle left
    unmatched (it is at the head of the queue, so considered again), and — from the second list on — a few rows the last cycle has just
    launched (dropped) and one job outside the pool"""
    rng = np.random.default_rng(seed)
    step = [0]

    def draw(history, atom):
        step[0] += 1
        if step[0] not in replace_in:
            return Rsv(release_matched=True, replace=False)
        w = history[-1]
        hosts = [int(h) for h in w.offers.host[np.argsort(-w.offers.cpus, kind="stable")[:n_hosts]]]  # the hosts with the most room
        # half of the jobs the last cycle left unmatched (the head of the queue: considered again), half the first rows of the queue
        # that it did not consider at all (the next to be)
        waiting = [int(r) for r in w.rows[w.j2o < 0]]
        seen = set(int(r) for r in w.rows)
        nxt = [int(r) for r in w.jq if int(r) not in seen][:4 * n_hosts * per_host]
        want_n = n_hosts * per_host
        rows = [int(r) for r in rng.choice(waiting, min(len(waiting), want_n // 2), replace=False)]
        rows += [int(r) for r in rng.choice(nxt, min(len(nxt), want_n - len(rows)), replace=False)]
        pend = rows
        host = [hosts[i % len(hosts)] for i in range(len(rows))]
        if step[0] != replace_in[0]:
            gone = [int(r) for r in w.rows[w.j2o >= 0][:3]]
            pend, host = pend + gone + [NONE], host + [hosts[0]] * len(gone) + [int(w.offers.host[0])]
        return Rsv(pend, host, release_matched=True, replace=True)
    return draw


def base_case(seed=511, *, scale=0.8, n_cycles=6, shrink=0.2, **kw):
    """the churn's base case (carry, release and churn on) on a cluster with `shrink` of its cpus — room is scarce, so a job kept off
    the roomiest hosts stays unmatched and is still in the queue when they are released — with the lists of reserver()"""
    pool, cycles = CH.base_case(seed, scale=scale, n_cycles=n_cycles)
    pool.offers = dataclasses.replace(pool.offers, cpus=np.floor(pool.offers.cpus * shrink))
    draw = reserver(seed, **kw)
    for c in range(1, n_cycles):
        cycles[c].reservations = draw
    return pool, cycles


def base_facts(params, pool, cycles, want):
    """the four oracle-only conditions of the base case -> a dict of counts"""
    released = sum(w.reserve["released"] for w in want)
    dropped = sum(w.reserve["dropped_launched"] for w in want)
    # a job that a reservation alone keeps off a host it fits on, and that lands on that host in a later cycle, the host free again
    # (the pool's jobs ask for cpus and mem alone: a job the cycle leaves unmatched that still fits on a host at the END of the cycle
    #  fitted there at its turn too — room only shrinks within a cycle — so, the host being another job's, the reservation alone kept it off)
    J = pool.pending_jobs
    assert J.eq_off is None and J.novel_off is None and J.group is None and (J.gpus is None or not (J.gpus > 0).any()) and J.ports is None
    later = 0
    for c, w in enumerate(want):
        if not w.reserved:
            continue
        end = O.carry_offers(w.offers, w.jobs, w.j2o, w.j2o >= 0)
        kept_off = set()
        for i in np.flatnonzero(w.j2o < 0):
            for r in np.flatnonzero(np.isin(end.host, w.reserved)):
                if int(end.host[r]) != int(w.jobs.reserved_host[i]) and end.cpus[r] >= w.jobs.cpus[i] and end.mem[r] >= w.jobs.mem[i]:
                    kept_off.add((int(w.rows[i]), int(end.host[r])))
        for w2 in want[c + 1:]:
            for i in np.flatnonzero(w2.j2o >= 0):
                host = int(w2.offers.host[int(w2.j2o[i])])
                later += (int(w2.rows[i]), host) in kept_off and host not in w2.reserved
    frozen = V.oracle(params, pool, cycles, frozen=True)
    return dict(released=released, dropped=dropped, later=later, frozen_differs=K.differs(want[1:], frozen[1:]))


def base_oracle(params, pool, cycles):
    want = V.oracle(params, pool, cycles)
    K.assert_every_cycle_mixed(want)
    f = base_facts(params, pool, cycles, want)
    assert sum(1 for w in want if w.reserve["installed"]) >= 2, "the list is not replaced in two cycles"
    assert f["released"] >= 1, "no reservation is released by a kept match: re-seed the case"
    assert f["dropped"] >= 1, "no list entry is dropped as launched: re-seed the case"
    assert f["later"] >= 1, "no job is kept off a host by a reservation alone and placed there after the release: re-seed the case"
    assert f["frozen_differs"], "the reservations frozen as first installed place the same: re-seed the case"
    return want


def check_base(make_engine, *, seed=511):
    params = P1(match_algo=2)
    pool, cycles = base_case(seed)
    want = base_oracle(params, pool, cycles)
    return check(make_engine, params, pool, cycles, want)


# ---- 2: by hand ------------------------------------------------------------------------------------------------------------------------
_hosts = CH._hosts


def check_by_hand(make_engine):
    params = P1()
    rel = Rsv(release_matched=True, replace=False)
    # -- one host, reserved for job A (row 1); B (row 0) ranks ahead of it and fits: B is refused, A lands, in the next cycle B lands
    pool = X.tiny_pool(2, _hosts([10], cpus=8.0), cpus=3.0)
    cycles = [V.cycle(0), V.cycle(2, carry_offers=True, reservations=Rsv([1], [10])), V.cycle(2, carry_offers=True, reservations=rel)]
    want = V.oracle(params, pool, cycles)
    assert [w.j2o.tolist() for w in want] == [[], [-1, 0], [0]] and [w.rows.tolist() for w in want[1:]] == [[0, 1], [0]]
    assert want[1].reserve == dict(released=0, installed=1, dropped_launched=0, alive=1) and want[2].reserve == dict(released=1, installed=0, dropped_launched=0, alive=0)
    assert V.refused_by_reservation(want[1], params) == [(0, 0, 10)]
    check(make_engine, params, pool, cycles, want)
    # -- two jobs reserved on ONE host: row 0 launches, the host stays reserved for row 1 (too big for it until the host is replaced by
    #    a larger one) and row 2 is kept off; row 1 launches; only then row 2 lands
    pool = X.tiny_pool(3, _hosts([10], cpus=8.0), cpus=[1.0, 20.0, 1.0])
    grown = A.HostChurn(leave=[10], join=_hosts([10], cpus=40.0), before=[10])
    cycles = [V.cycle(0), V.cycle(3, carry_offers=True, reservations=Rsv([0, 1], [10, 10])), V.cycle(3, carry_offers=True, reservations=rel),
              V.cycle(3, carry_offers=True, reservations=rel, hosts=grown), V.cycle(3, carry_offers=True, reservations=rel)]
    want = V.oracle(params, pool, cycles)
    assert [w.j2o.tolist() for w in want] == [[], [0, -1, -1], [-1, -1], [0, -1], [0]], [w.j2o.tolist() for w in want]
    assert [w.reserve["alive"] for w in want] == [0, 2, 1, 1, 0] and want[3].pairs == {(1, 10)}
    check(make_engine, params, pool, cycles, want)
    # -- a job outside the pool: its entry survives every match and goes only with a replacement
    pool = X.tiny_pool(4, _hosts([10, 11], cpus=8.0), cpus=3.0)
    cycles = [V.cycle(0), V.cycle(4, carry_offers=True, reservations=Rsv([NONE, 0], [10, 11])), V.cycle(4, carry_offers=True, reservations=rel),
              V.cycle(4, carry_offers=True, reservations=rel), V.cycle(4, carry_offers=True, reservations=Rsv([], []))]
    want = V.oracle(params, pool, cycles)
    assert [w.j2o.tolist() for w in want] == [[], [1, -1, -1, -1], [1, -1, -1], [-1, -1], [0, 0]], [w.j2o.tolist() for w in want]
    assert [sorted(w.pairs) for w in want] == [[], [(0, 11), (NONE, 10)], [(NONE, 10)], [(NONE, 10)], []]
    check(make_engine, params, pool, cycles, want)
    # -- a replacement naming a launched row is dropped; the same list once more is installed (launched was cleared)
    pool = X.tiny_pool(3, _hosts([10], cpus=8.0), cpus=1.0)
    same = lambda: Rsv([0], [10])
    cycles = [V.cycle(0), V.cycle(1, carry_offers=True, reservations=same()), V.cycle(1, carry_offers=True, reservations=same()),
              V.cycle(1, carry_offers=True, reservations=same()), V.cycle(1, carry_offers=True, reservations=rel)]
    want = V.oracle(params, pool, cycles)
    assert [w.reserve for w in want[1:]] == [dict(released=0, installed=1, dropped_launched=0, alive=1), dict(released=1, installed=0, dropped_launched=1, alive=0),
                                             dict(released=0, installed=1, dropped_launched=0, alive=1), dict(released=0, installed=0, dropped_launched=0, alive=1)]
    assert [w.j2o.tolist() for w in want] == [[], [0], [0], [-1], [-1]], [w.j2o.tolist() for w in want]
    check(make_engine, params, pool, cycles, want)


# ---- 3: kernel boundaries ----------------------------------------------------------------------------------------------------------------
def check_list_length(make_engine, n):
    """a list of n entries (distinct rows, hosts drawn with repeats, every 7th a job outside the pool), released over, replaced by
    another of the same length that names launched rows too"""
    params = P1()
    pool = CH.wide_pool(300, n_jobs=max(80, 2 * n + 20))
    rng = np.random.default_rng(900 + n)
    P = pool.pending_jobs.n

    def lst(first):
        rows = (first + np.arange(n)) % P
        pend = [NONE if i % 7 == 6 else int(rows[i]) for i in range(n)]
        return Rsv(pend, [int(h) for h in rng.choice(pool.offers.host, n)] if n else [])
    k = 16
    cycles = [V.cycle(k), V.cycle(k, carry_offers=True, reservations=lst(8)), V.cycle(k, carry_offers=True, reservations=Rsv(release_matched=True, replace=False)),
              V.cycle(k, carry_offers=True, reservations=lst(0))]
    want = V.oracle(params, pool, cycles)
    assert all(w.reserve["installed"] + w.reserve["dropped_launched"] == n for w in (want[1], want[3])) and all((w.j2o >= 0).any() for w in want)
    if n >= 63:  # (rows the rank cycle has just launched are named by the first list, rows of all three cycles by the second)
        assert want[1].reserve["dropped_launched"] >= 1 and want[3].reserve["dropped_launched"] >= 16 and sum(w.reserve["released"] for w in want) >= 1
    return check(make_engine, params, pool, cycles, want)


def check_considered(make_engine, k):
    """k considered jobs, every one a kept match that holds a reservation: all k are released in one advance"""
    params = P1()
    pool = X.tiny_pool(k + 40, _hosts(list(range(100)), cpus=1000.0), cpus=1.0)
    first = Rsv(list(range(k)), [i % 100 for i in range(k)])
    cycles = [V.cycle(k, set_reservations=first), V.cycle(k, carry_offers=True, reservations=Rsv(release_matched=True, replace=False))]
    want = V.oracle(params, pool, cycles)
    assert (want[0].j2o >= 0).all() and len(want[0].j2o) == k and want[0].reserve["installed"] == k
    assert want[1].reserve == dict(released=k, installed=0, dropped_launched=0, alive=0)
    return check(make_engine, params, pool, cycles, want)


def check_host_ids(make_engine):
    """reserved host ids at the bitmap's word boundaries; an id far above every offer's; an offer whose id lies above 32 x
    reserved_words (the guard of the static pass); a list whose every entry shares one host"""
    params = P1()
    ids = [31, 32, 63, 64, 5000]
    pool = X.tiny_pool(90, _hosts(ids, cpus=6.0), cpus=1.0)
    rel = Rsv(release_matched=True, replace=False)
    cycles = [V.cycle(0),
              V.cycle(8, carry_offers=True, reservations=Rsv([80, 81, 82, 83], [31, 32, 63, 64])),   # only host 5000 is free: 3 words, id 5000 past them
              V.cycle(8, carry_offers=True, reservations=Rsv([80, 81], [64, 1 << 20])),              # a far id: 32 769 words
              V.cycle(8, carry_offers=True, reservations=Rsv([NONE], [5000])),
              V.cycle(80, carry_offers=True, reservations=Rsv(list(range(20, 90)), [32] * 70)),      # 70 entries on one host
              V.cycle(80, carry_offers=True, reservations=rel)]
    want = V.oracle(params, pool, cycles)
    hosts_used = [sorted(set(int(w.offers.host[o]) for o in w.j2o[w.j2o >= 0])) for w in want]
    assert hosts_used[1] == [5000] and 64 not in hosts_used[2] and hosts_used[2] and 5000 not in hosts_used[3] and hosts_used[3]
    assert want[4].reserve["installed"] + want[4].reserve["dropped_launched"] == 70 and want[4].reserve["dropped_launched"] >= 1
    assert want[5].reserve["released"] >= 1 and len(set(h for _, h in want[5].pairs)) == 1
    return check(make_engine, params, pool, cycles, want)


# ---- 4: release details ------------------------------------------------------------------------------------------------------------------
def check_skipped_and_removal(make_engine):
    params = P1()
    rel = Rsv(release_matched=True, replace=False)
    # a skipped match releases nothing: the rank cycle matches row 0 to host 10 and the host skips that offer (the step's offer_skipped
    # speaks of the LAST cycle's offers): row 0 stays in the queue with its reservation, is matched again and released one step later
    pool = X.tiny_pool(3, _hosts([10, 11], cpus=[8.0, 2.0]), cpus=[3.0, 3.0, 1.0])
    cycles = [V.cycle(1, set_reservations=Rsv([0], [10])), V.cycle(2, reservations=rel, offer_skipped=np.array([1, 0], np.uint8)),
              V.cycle(2, carry_offers=True, reservations=rel)]
    want = V.oracle(params, pool, cycles)
    assert want[0].j2o.tolist() == [0] and want[1].reserve == dict(released=0, installed=0, dropped_launched=0, alive=1)
    assert want[1].rows.tolist() == [0, 1] and want[1].j2o.tolist() == [0, -1] and want[2].reserve["released"] == 1 and want[2].rows.tolist() == [1, 2]
    check(make_engine, params, pool, cycles, want)
    # remove_mode = 1: every considered job leaves the queue, only the kept matches release (row 1 is unmatched and keeps its host)
    pool = X.tiny_pool(4, _hosts([10, 11], cpus=[3.0, 50.0]), cpus=[3.0, 100.0, 3.0, 3.0])
    cycles = [V.cycle(2, set_reservations=Rsv([0, 1], [10, 11])), V.cycle(2, carry_offers=True, reservations=rel, remove_mode=1)]
    want = V.oracle(params, pool, cycles)
    assert want[0].j2o.tolist() == [0, -1] and want[1].rows.tolist() == [2, 3] and want[1].pairs == {(1, 11)} and want[1].j2o.tolist() == [-1, -1]
    check(make_engine, params, pool, cycles, want)


def check_no_advance(make_engine):
    """the last cycle considered nothing, and the queue is empty: the step still runs"""
    params = P1()
    pool = X.tiny_pool(2, _hosts([10, 11], cpus=8.0), cpus=3.0)
    cycles = [V.cycle(0), V.cycle(0, reservations=Rsv([1, NONE], [10, 11])), V.cycle(2, reservations=Rsv([0], [11])),
              V.cycle(2, carry_offers=True, reservations=Rsv(release_matched=True, replace=False)), V.cycle(2, reservations=Rsv([NONE], [10]))]
    want = V.oracle(params, pool, cycles)
    assert want[1].reserve == dict(released=0, installed=2, dropped_launched=0, alive=2) and want[2].pairs == {(0, 11)}
    assert want[2].j2o.tolist() == [0, 0] and [len(w.Q) for w in want] == [2, 2, 2, 0, 0] and want[4].pairs == {(NONE, 10)}
    check(make_engine, params, pool, cycles, want)


# ---- 5: a rank cycle; cook_cycle_update puts the staged reservations back -------------------------------------------------------------
def check_rank_cycle(make_engine):
    params = P1()
    pool = X.tiny_pool(3, _hosts([10, 11], cpus=[8.0, 9.0]), cpus=3.0)
    staged_col = np.array([-1, -1, 10], np.int32)
    pool.pending_jobs.reserved_host = staged_col
    stage = lambda e: e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups, reserved_hosts=[10])
    staged = V.oracle(params, pool, [V.cycle(3)], staged_reserved=[10], staged_column=staged_col)
    own = V.oracle(params, pool, [V.cycle(3, set_reservations=Rsv([1], [11]))], staged_reserved=[10], staged_column=staged_col)
    # staged: host 10 is row 2's, all three end up on host 11.  own map: host 11 is row 1's; rows 0 and 1 fill host 10, row 2 has none.
    # no reservations at all: rows 0 and 1 on host 10, row 2 on host 11
    assert staged[0].j2o.tolist() == [1, 1, 1] and own[0].j2o.tolist() == [0, 0, -1], (staged[0].j2o, own[0].j2o)
    with make_engine(params) as e:
        assert _code(lambda: e.cycle_set_reservations(Rsv([1], [11]))) == COOK_E_STATE  # before cook_cycle_stage
        stage(e)
        e.cycle_run(3)
        assert np.array_equal(S.fetch(e, False).j2o, staged[0].j2o) and pairs_of(e) == (set(), 0)
        e.cycle_set_reservations(Rsv([1], [11]))
        assert e.reserve_info() == dict(released=0, installed=1, dropped_launched=0, alive=1)
        e.cycle_run(3)
        assert np.array_equal(S.fetch(e, False).j2o, own[0].j2o) and pairs_of(e) == ({(1, 11)}, 1)
        e.cycle_run(3)  # a rank keeps the map
        assert np.array_equal(S.fetch(e, False).j2o, own[0].j2o) and pairs_of(e) == ({(1, 11)}, 1)
        e.cycle_update()  # drops it: the staged reservations are read again
        assert pairs_of(e) == (set(), 0) and e.reserve_info() == dict(released=0, installed=0, dropped_launched=0, alive=0)
        e.cycle_run(3)
        assert np.array_equal(S.fetch(e, False).j2o, staged[0].j2o)
        e.cycle_set_reservations(None)  # no reservations at all
        e.cycle_run(3)
        assert S.fetch(e, False).j2o.tolist() == [0, 0, 1]
        stage(e)  # a stage drops it too
        e.cycle_run(3)
        assert np.array_equal(S.fetch(e, False).j2o, staged[0].j2o)


def check_last_match_described(make_engine):
    """cook_cycle_set_reservations between a match and the calls that describe it: cook_match_explain and cook_match_metrics still
    answer from the map that match read, also when the new list's greatest host id makes the bitmap grow, twice in a row, and when
    the new map is empty; the NEXT match reads the new map.  A placement that is set up and has not run refuses the call.
    replace = 0 changes nothing, with or without a map of the engine's own."""
    params = P1()
    pool = X.tiny_pool(3, _hosts([10, 11], cpus=[8.0, 9.0]), cpus=3.0)
    own = V.oracle(params, pool, [V.cycle(3, set_reservations=Rsv([1], [11]))])
    free = V.oracle(params, pool, [V.cycle(3)])
    assert own[0].j2o.tolist() == [0, 0, -1] and free[0].j2o.tolist() == [0, 0, 1]
    described = lambda e: (e.match_explain(np.arange(3)), e.match_metrics(n_users=pool.users.n), vars(S.fetch(e, False)))
    with make_engine(params) as e:
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        e.cycle_set_reservations(Rsv([1], [11]))
        e.cycle_run(3)
        first = described(e)
        assert first[0][2, WHY_RESERVATION] == 1 and first[0][2].sum() == 2  # row 2: host 10 has 2 cpus left, host 11 is row 1's
        for lst, pairs in ((Rsv([0], [1 << 22]), {(0, 1 << 22)}), (Rsv([0, NONE], [1 << 23, 5]), {(0, 1 << 23), (NONE, 5)}), (Rsv([], []), set()),
                           (Rsv([2], [10]), {(2, 10)}), (Rsv([1], [3], replace=False), {(2, 10)})):
            e.cycle_set_reservations(lst)
            assert pairs_of(e)[0] == pairs
            X._same(described(e), first)
        e.cycle_set_reservations(None)
        X._same(described(e), first)
        e.cycle_run(3)  # the next match reads the new map: none
        assert np.array_equal(S.fetch(e, False).j2o, free[0].j2o) and e.match_explain(np.arange(3))[:, WHY_RESERVATION].sum() == 0
        # a placement that is set up and has not run
        cycle_run_rank_multi([e], [3])
        assert _code(lambda: e.cycle_set_reservations(Rsv([1], [11]))) == COOK_E_STATE and pairs_of(e) == (set(), 0)
        cycle_match_multi([e])
        assert np.array_equal(S.fetch(e, False).j2o, free[0].j2o)
        e.cycle_set_reservations(Rsv([1], [11]))
        e.cycle_run(3)
        assert np.array_equal(S.fetch(e, False).j2o, own[0].j2o)
    # replace = 0 on an engine without a map of its own: the staged reservations keep being read
    staged_col = np.array([-1, -1, 10], np.int32)
    pool.pending_jobs.reserved_host = staged_col
    staged = V.oracle(params, pool, [V.cycle(3)], staged_reserved=[10], staged_column=staged_col)
    assert staged[0].j2o.tolist() == [1, 1, 1]
    with make_engine(params) as e:
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups, reserved_hosts=[10])
        e.cycle_set_reservations(Rsv([1], [11], replace=False))
        assert e.reserve_info() == dict(released=0, installed=0, dropped_launched=0, alive=0) and pairs_of(e) == (set(), 0)
        e.cycle_run(3)
        assert np.array_equal(S.fetch(e, False).j2o, staged[0].j2o)


# ---- 6: the class-ordered walk ---------------------------------------------------------------------------------------------------------
def check_classfit(make_engine):
    """a pool the walk takes but for its one reservation: refused while it is alive, placing again in the cycle after the release"""
    params = P1(match_algo=3)
    pool, cycles = X.classfit_case(n_cycles=4)
    free = V.oracle(params, pool, cycles[:1])[0]
    i = int(np.flatnonzero(free.j2o >= 0)[5])
    first = Rsv([int(free.rows[i])], [int(free.offers.host[int(free.j2o[i])])])
    cycles[0].set_reservations = first
    rel = Rsv(release_matched=True, replace=False)
    for cy in cycles[1:]:
        cy.reservations = rel
    want = V.oracle(params, pool, cycles)
    K.assert_every_cycle_mixed(want)
    assert [w.reserve["alive"] for w in want] == [1, 0, 0, 0] and want[1].reserve["released"] == 1
    assert K.differs(want[:1], [free]), "the reservation changes no placement: pick another job"
    got = check(make_engine, params, pool, cycles, want, forms=[0, 3, 3, 3])
    assert got[0].refused != 0
    return got


# ---- 7: multi --------------------------------------------------------------------------------------------------------------------------
def check_multi(make_engine, *, scale=0.4):
    """three ragged pools through cook_cycle_run_queue_reserve_multi: pool 0 with reservations, pool 1 without any, pool 2 with
    reservations and its list refused in round 2 (a row twice): it stays untouched (the same step runs next), the others go on"""
    params = P1(match_algo=2)
    shapes = [(1.0, 541, 5), (0.5, 542, 5), (0.7, 543, 4)]
    cases = [base_case(seed, scale=s * scale, n_cycles=n, replace_in=(1, 2, 3)) for s, seed, n in shapes]
    for cy in cases[1][1][1:]:
        cy.reservations = None
    want = [V.oracle(params, pl, cs) for pl, cs in cases]
    for w in want:
        K.assert_every_cycle_mixed(w)
    assert all(sum(x.reserve["installed"] for x in want[i]) >= 2 for i in (0, 2)) and all(not w.pairs for w in want[1])
    assert sum(x.reserve["released"] for i in (0, 2) for x in want[i]) >= 1
    engines = [make_engine(params) for _ in cases]
    got = [[] for _ in cases]
    try:
        for e, (pl, cs) in zip(engines, cases):
            e.cycle_stage(pl.tasks, pl.users, pl.pending_jobs, pl.offers, pl.groups)
            e.cycle_set_considerable(cs[0].state, cs[0].eligible)
        cycle_run_rank_multi(engines, [cs[0].k for _, cs in cases])
        cycle_match_multi(engines)
        for i in range(3):
            got[i].append(fetch(engines[i]))
        nxt = [1, 1, 1]
        for rnd in range(1, 6):
            cur = [cs[min(nxt[i], len(cs) - 1)] for i, (_, cs) in enumerate(cases)]
            steps, carries, ks = [K.step_kw(cy) for cy in cur], [K.carry_of(cy) for cy in cur], [cy.k for cy in cur]
            fins, hosts, rvs = [cy.finished for cy in cur], [cy.hosts for cy in cur], [cy.reservations for cy in cur]
            if rnd == 2:
                r = rvs[2]
                assert r.replace and len(r.pending) and int(r.pending[0]) != NONE
                rvs[2] = Rsv(list(r.pending) + [int(r.pending[0])], list(r.host) + [int(r.host[0])])
                with pytest.raises(CookError) as ex:
                    cycle_run_queue_reserve_multi(engines, ks, steps, carries, fins, hosts, rvs)
                assert ex.value.code == COOK_E_INVALID
                live = [0, 1]
            else:
                live = [0, 1, 2]
                if any(nxt[i] >= len(cases[i][1]) for i in live):
                    break
                cycle_run_queue_reserve_multi(engines, ks, steps, carries, fins, hosts, rvs)
            cycle_match_multi([engines[i] for i in live])
            for i in live:
                got[i].append(fetch(engines[i]))
                nxt[i] += 1
    finally:
        for e in engines:
            e.close()
    for i, (pl, cs) in enumerate(cases):
        assert len(got[i]) >= 3
        compare(got[i], want[i][:len(got[i])], cs, f"pool {i}")
    return got


# ---- 8: refusals -------------------------------------------------------------------------------------------------------------------------
def check_refusals(make_engine):
    params = P1()
    pool = X.tiny_pool(6, _hosts([10, 11, 12], cpus=8.0), cpus=3.0)
    P = pool.pending_jobs.n
    with make_engine(params) as e:
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        e.cycle_run(2)
        # release_matched without a map of the engine's own
        assert _code(lambda: e.cycle_run_queue_reserve(2, reservations=Rsv(release_matched=True, replace=False))) == COOK_E_STATE
        assert pairs_of(e) == (set(), 0)
        e.cycle_run_queue_reserve(2, reservations=Rsv([4, NONE], [11, 12]))
        before = fetch(e)
        assert before.pairs == {(4, 11), (NONE, 12)}

        def raw(release, replace, n, pending, host):
            keep = (np.asarray(pending if pending is not None else [], np.uint32), np.asarray(host if host is not None else [], np.uint32))
            ptr = lambda a, given: a.ctypes.data_as(C.POINTER(C.c_uint32)) if given else None
            return A.CookReservations(release, replace, n, ptr(keep[0], pending is not None), ptr(keep[1], host is not None)), keep
        bad = [raw(2, 1, 0, [], []), raw(1, 2, 0, [], []), raw(0, 1, 2, None, [10, 11]), raw(0, 1, 2, [0, 1], None), raw(1, 1, 1, [P], [10]),
               raw(1, 1, 3, [3, 5, 3], [10, 11, 12]), raw(0, 1, 1, [0], [0x80000000])]
        for st, keep in bad:
            qs, keep2 = e._queue_step()
            assert e._lib.cook_cycle_run_queue_reserve(e._h, C.byref(qs), None, None, None, C.byref(st), 2) == COOK_E_INVALID, (st.release_matched, st.replace, st.n)
            if st.release_matched <= 1:  # (set_reservations ignores release_matched)
                assert e._lib.cook_cycle_set_reservations(e._h, C.byref(st)) == COOK_E_INVALID
            after = fetch(e)
            X._same({k: v for k, v in vars(after).items()}, {k: v for k, v in vars(before).items()})
        # a step refused for another reason leaves the reservations as they were
        assert _code(lambda: e.cycle_run_queue_reserve(2, reservations=Rsv([1], [10]), remove_mode=2)) == COOK_E_INVALID
        assert pairs_of(e) == ({(4, 11), (NONE, 12)}, 2)
        # the older entry points leave the map as it stands, and their matches read it
        e.cycle_run_queue_hosts(2, A.QueueCarry(offers=True, usage=False), None, None)
        assert pairs_of(e) == ({(4, 11), (NONE, 12)}, 2) and e.reserve_info() == dict(released=0, installed=0, dropped_launched=0, alive=2)
        assert S.fetch(e, False).j2o.tolist() == [1, -1]  # row 4 goes to its own host 11; row 5 is kept off 11 and 12, and host 10 has 2 cpus left
        # the fetch with too little room
        n = C.c_uint32(0)
        buf = (C.c_uint32 * 1)()
        assert e._lib.cook_cycle_fetch_reservations(e._h, buf, buf, 1, C.byref(n)) == COOK_E_INVALID and n.value == 2
    # reservations = NULL and both flags 0 are cook_cycle_run_queue_hosts, byte for byte
    pool, cycles = CH.base_case(405, scale=0.3, n_cycles=3)
    V.oracle(params, pool, cycles)  # (draws the lists)
    outs = []
    for mode in ("hosts", "null", "flags0"):
        with make_engine(params) as e:
            e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
            e.cycle_set_considerable(cycles[0].state, cycles[0].eligible)
            e.cycle_run(cycles[0].k)
            for cy in cycles[1:]:
                if mode == "hosts":
                    CH.run_step(e, cy)
                else:
                    cy.reservations = None if mode == "null" else Rsv([1], [2], release_matched=False, replace=False)
                    run_step(e, cy)
                    assert pairs_of(e) == (set(), 0)
            outs.append((vars(S.fetch(e, False)), e.match_metrics(n_users=pool.users.n), e.match_explain(np.arange(30)), e.release_info(), e.churn_info()))
    for x in outs[1:]:
        X._same(x, outs[0])


# ---- 9: explain ------------------------------------------------------------------------------------------------------------------------
def check_explain(make_engine):
    params = P1()
    pool = X.tiny_pool(2, _hosts([10], cpus=8.0), cpus=3.0)
    cycles = [V.cycle(0), V.cycle(2, carry_offers=True, reservations=Rsv([1], [10])),
              V.cycle(2, reservations=Rsv(release_matched=True, replace=False), offers=_hosts([10], cpus=2.0))]
    want = V.oracle(params, pool, cycles)
    assert want[1].j2o.tolist() == [-1, 0] and want[2].j2o.tolist() == [-1]
    seen = []
    compare(run_engine(make_engine, params, pool, cycles, between=lambda e, c: seen.append(e.match_explain(np.arange(len(want[c].pos))))), want, cycles)
    assert seen[1][0, WHY_RESERVATION] == 1 and seen[1][1, WHY_RESERVATION] == 0  # row 0 is kept off host 10 by the reservation ...
    assert seen[2][0, WHY_RESERVATION] == 0 and seen[2][0].sum() == 1               # ... and after the release by its cpus alone


# ---- 10: the reference's own tests (tests/golden/reservations.json) -------------------------------------------------------------------------
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _rsv_of(step, jobs):
    """a step's decision list through reservations_of (reserve-hosts!'s filter)"""
    row = lambda name: jobs.index(name) if name in jobs else NONE
    pend, host = reservations_of([dict(pending_index=row(d["job"]), host=d["host"], tasks=[NONE] * d["tasks"]) for d in step["decisions"]])
    return Rsv(pend, host, release_matched=False, replace=True)


def check_golden_atom(case):
    """the cases that only move the atom (rebalancer.clj's tests): the oracle's Atom against the recorded maps"""
    jobs = case["jobs"]
    atom = V.Atom()
    for step in case["steps"]:
        if "launch" in step:
            atom.update_host_reservations([jobs.index(j) for j in step["launch"]])
        else:
            r = _rsv_of(step, jobs)
            atom.reserve_hosts(r.pending, r.host)
        assert {jobs[k]: v for k, v in atom.map.items()} == step["map"], (case["name"], step)
        assert sorted(jobs[k] for k in atom.launched) == sorted(step["launched"]), (case["name"], step)


def check_golden_engine(make_engine, case):
    """the same steps on the engine: decisions -> cook_cycle_set_reservations; launch -> a rank cycle that considers exactly those jobs
    (the eligible mask) and places them, then a _reserve step with release_matched = 1 that considers nothing"""
    params = P1()
    jobs = case["jobs"]
    n = len(jobs)
    pool = X.tiny_pool(n, _hosts([1, 2, 3], cpus=1000.0), cpus=1.0)
    with make_engine(params) as e:
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        e.cycle_set_reservations(None)
        for step in case["steps"]:
            if "launch" in step:
                elig = np.zeros(n, np.uint8)
                elig[[jobs.index(j) for j in step["launch"]]] = 1
                e.cycle_set_considerable(X.tiny_state(), elig)
                e.cycle_run(n)
                j2o = S.fetch(e, False).j2o
                assert (j2o >= 0).all() and len(j2o) == len(step["launch"])
                e.cycle_run_queue_reserve(0, reservations=Rsv(release_matched=True, replace=False))
            else:
                e.cycle_set_reservations(_rsv_of(step, jobs))
            got, _ = pairs_of(e)
            assert {jobs[p]: h for p, h in got} == step["map"], (case["name"], step, got)


def check_golden_match(make_engine, case):
    """scheduler.clj's two reservation tests: which of the jobs launch on the one host, and the atom afterwards"""
    params = P1()
    jobs = case["jobs"]
    name = lambda p: jobs[p] if p != NONE else "(a job outside the pool)"
    offers = A.Offers(cpus=np.array([float(case["host_cpus"])]), mem=np.array([float(case["host_mem"])]), host=np.array([case["host"]], np.uint32))
    pool = X.tiny_pool(len(jobs), offers, cpus=[float(c) for c in case["job_cpus"]], mem=[float(m) for m in case["job_mem"]])
    first = Rsv([jobs.index(j) if j in jobs else NONE for j, _ in case["reserve"]], [h for _, h in case["reserve"]])
    cycles = [V.cycle(len(jobs), set_reservations=first), V.cycle(len(jobs), carry_offers=True, reservations=Rsv(release_matched=True, replace=False))]
    want = V.oracle(params, pool, cycles)
    assert [jobs[r] for r, o in zip(want[0].rows, want[0].j2o) if o >= 0] == case["launched"], (case["name"], want[0].j2o)
    assert {name(p): h for p, h in want[1].pairs} == case["map_after"] and want[1].reserve["released"] == case["released"]
    check(make_engine, params, pool, cycles, want)


# ---- 11: ABI -------------------------------------------------------------------------------------------------------------------------------
def struct_layout_sources():
    structs = [("cook_reservations", A.CookReservations), ("cook_reserve_info", A.CookReserveInfo)]
    fields = [(s, f, cls) for s, cls in structs for f, _ in cls._fields_]
    prints = "".join(f'printf("%zu ", offsetof({s}, {f}));' for s, f, _ in fields)
    sizes = "".join(f'printf("%zu ", sizeof({s}));' for s, _ in structs)
    text = ('#include <stdio.h>\n#include <stddef.h>\n#include "cookmatch.h"\nint main(){' + sizes + prints +
            'printf("%d\\n", COOK_ABI_VERSION);return 0;}')
    want = [C.sizeof(cls) for _, cls in structs] + [getattr(cls, f).offset for _, f, cls in fields]
    return text, want + [A.ABI_VERSION]
