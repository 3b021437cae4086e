"""The cases of the host churn (cook_cycle_run_queue_hosts*: a queue cycle takes the rows of hosts that leave out of the staged offers
and puts rows that join in, on the device) and of cook_cycle_fetch_offers, shared by the emulator (test_churn_emu.py) and GPU
(test_churn_gpu.py) suites.  Expected values come from tests/churn_oracle.py alone.  Per cycle the queue, rank_pos, job_to_offer,
head_matched, the considered count, cook_churn_info and — through cook_cycle_fetch_offers — every column of the staged table are compared
element for element, fp64 bit for bit.  The conditions that make a case mean something are asserted on the oracle alone, before the
engine is called."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np
import pytest

from cook_amd import _abi as A
from cook_amd.engine import CookError, cycle_match_multi, cycle_run_queue_hosts_multi, cycle_run_rank_multi
from tests import carry_cases as K
from tests import churn_oracle as H
from tests import queue_cases as S
from tests import release_cases as X
from tests import release_oracle as R

COOK_E_INVALID, COOK_E_STATE = -1, -4
NONE = A.NONE_U32
P1 = K.P1
_code = X._code


# ---- engine side -------------------------------------------------------------------------------------------------------------------
def same_table(got: A.Offers, want: A.Offers, where=""):
    """every column, element for element; doubles by their bits.  `got` comes from a fetch: it has every column, a column the oracle's
    table lacks must hold what NULL means for it"""
    assert got.n == want.n, (where, "rows", got.n, want.n)
    g, w = H.table_columns(got), H.table_columns(want, like=got)
    for name in H.COLS:
        a, b = g[name], w[name]
        if a is None or b is None:
            assert a is None and b is None, (where, name, "one side has no such column")
            continue
        assert a.shape == b.shape, (where, name, a.shape, b.shape)
        if a.dtype == np.float64:
            assert np.array_equal(a.view(np.uint64), b.astype(np.float64).view(np.uint64)), (where, name, a[:8], b[:8])
        else:
            assert np.array_equal(a.astype(np.int64), b.astype(np.int64)), (where, name, a[:8], b[:8])


def fetch(e):
    g = S.fetch(e, False)
    g.info = e.release_info()
    g.churn = e.churn_info()
    g.offers = e.fetch_offers().offers()
    return g


def run_step(e, cy):
    fin, hosts = getattr(cy, "finished", None), getattr(cy, "hosts", None)
    assert not callable(fin) and not callable(hosts), "run the oracle first: it draws the lists"
    e.cycle_run_queue_hosts(cy.k, K.carry_of(cy), fin, hosts, **K.step_kw(cy))


def run_engine(make_engine, params, pool, cycles, *, expect_form=None, between=None):
    got = []
    with make_engine(params) as e:
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        for c, cy in enumerate(cycles):
            if cy.state is not None:
                e.cycle_set_considerable(cy.state, cy.eligible)
            if c == 0:
                e.cycle_run(cy.k)
            else:
                run_step(e, cy)
            got.append(fetch(e))
            if expect_form is not None and len(got[-1].j2o):
                ms = e.match_stats()
                assert ms["placement_form"] == expect_form, (c, ms["placement_form"], hex(ms["classfit_refused"]))
            if between is not None:
                between(e, c)
    return got


def compare(got, want, cycles, tag=""):
    S.compare(got, want, cycles, tag)
    for c, (g, w) in enumerate(zip(got, want)):
        assert g.info == w.info, (f"{tag} cycle {c}", "release_info", g.info, w.info)
        assert g.churn == w.churn, (f"{tag} cycle {c}", "churn_info", g.churn, w.churn)
        same_table(g.offers, w.offers, f"{tag} cycle {c}")


def check(make_engine, params, pool, cycles, want, **kw):
    got = run_engine(make_engine, params, pool, cycles, **kw)
    compare(got, want, cycles)
    return got


# ---- 1: base ---------------------------------------------------------------------------------------------------------------------------
def base_case(seed=401, *, fractional=False, scale=1.0, n_cycles=5, frac=0.35, churn=0.15, extra=0):
    pool, cycles = X.base_case(seed, fractional=fractional, scale=scale, n_cycles=n_cycles, frac=frac)
    draw = H.churner(seed, churn, extra=extra)
    for c in range(1, n_cycles):
        cycles[c].hosts = draw
    return pool, cycles


def base_oracle(params, pool, cycles):
    want = H.oracle(params, pool, cycles)
    K.assert_every_cycle_mixed(want)
    assert all(w.hosts is not None and w.churn["left"] >= 1 and w.churn["joined"] >= 1 for w in want[1:]), "a queue cycle churns nothing: re-seed"
    assert sum(w.churn["leave_missing"] for w in want) >= 1, "no leave_host without a row: re-seed"
    # a joined host receives a placement in the cycle it joins, in at least two cycles
    took = 0
    for w in want[1:]:
        new = set(int(h) for h in w.hosts.join.host)
        took += any(int(w.offers.host[o]) in new for o in w.j2o[w.j2o >= 0])
    assert took >= 2, f"a joined host takes a job in the cycle it joins in {took} cycles only: re-seed the case"
    # with the leaves left out, some job goes to a host that has in fact left (so: it lands elsewhere or stays unmatched)
    stay = H.oracle(params, pool, cycles, leave=False)
    moved = 0
    for w, s in zip(want[1:], stay[1:]):
        gone = set(int(h) for h in w.hosts.leave)
        moved += any(int(s.offers.host[o]) in gone for o in s.j2o[s.j2o >= 0])
        if K.differs([w], [s]):
            break  # (from here on the two histories are different pools)
    assert moved >= 1, "no job would have gone to a host that left: re-seed the case"
    assert K.differs(want[1:], H.oracle(params, pool, cycles, with_churn=False)[1:]), "the churns change no result: re-seed the case"
    return want


def check_base(make_engine, *, fractional=False, scale=1.0, algo=2, expect_form=0, seed=401):
    params = P1(match_algo=algo)
    pool, cycles = base_case(seed, fractional=fractional, scale=scale)
    want = base_oracle(params, pool, cycles)
    return check(make_engine, params, pool, cycles, want, expect_form=expect_form)


# ---- 2: the order rule, by hand -----------------------------------------------------------------------------------------------------------
def _hosts(ids, cpus=4.0, **kw):
    m = len(ids)
    cp = np.full(m, float(cpus)) if np.isscalar(cpus) else np.asarray(cpus, float)
    return A.Offers(cpus=cp, mem=np.full(m, 1000.0), host=np.asarray(ids, np.uint32), **kw)


def check_order(make_engine):
    params = P1()
    # -- two hosts of equal fitness for the one job: the lowest row wins.  Joined in front of the old one the new host takes it, joined
    #    at the end the old one does
    for before, winner in ((10, 20), (NONE, 10), (None, 10)):
        pool = X.tiny_pool(2, _hosts([10]), cpus=3.0)
        churn = A.HostChurn(join=_hosts([20]), before=None if before is None else [before])
        cycles = [H.cycle(0), H.cycle(1, hosts=churn)]
        want = H.oracle(params, pool, cycles)
        assert want[1].j2o.tolist() == [0] and int(want[1].offers.host[0]) == winner, (before, want[1].offers.host)
        assert want[1].churn == dict(left=0, leave_missing=0, joined=1, n_offers=2)
        check(make_engine, params, pool, cycles, want)
    # -- a host replaced in place keeps its row; two joins on one anchor keep list order; an anchor that itself leaves; a row anchored
    #    at a leaving row and one at the end, in one list
    pool = X.tiny_pool(3, _hosts([1, 2, 3], cpus=[4.0, 5.0, 6.0]), cpus=3.0)
    steps = [
        A.HostChurn(leave=[2], join=_hosts([2], cpus=7.5), before=[2]),
        A.HostChurn(join=_hosts([30, 31], cpus=[8.0, 9.0]), before=[2, 2]),
        A.HostChurn(leave=[2], join=_hosts([40], cpus=10.0), before=[2]),
        A.HostChurn(leave=[1, 77], join=_hosts([50, 51, 52], cpus=[1.0, 2.0, 11.0]), before=[NONE, 1, 31]),
    ]
    cycles = [H.cycle(0)] + [H.cycle(1, carry_offers=True, hosts=h) for h in steps]
    want = H.oracle(params, pool, cycles)
    assert [w.offers.host.tolist() for w in want] == [[1, 2, 3], [1, 2, 3], [1, 30, 31, 2, 3], [1, 30, 31, 40, 3], [51, 30, 52, 31, 40, 3, 50]]
    assert want[1].offers.cpus.tolist() == [4.0, 7.5, 6.0] and want[4].churn == dict(left=1, leave_missing=1, joined=3, n_offers=7)
    assert [w.j2o.tolist() for w in want] == [[], [0], [4], [4], []], [w.j2o.tolist() for w in want]
    check(make_engine, params, pool, cycles, want)


# ---- 3: every column ----------------------------------------------------------------------------------------------------------------------
def full_row(host, slots, *, run=True, **over):
    """one k8s host with every column and room for everything; slots: entries of the gpu / disk maps (the first entries are other
    models / types, the LAST one is model / type 2)"""
    pad = lambda last, fill: np.array([list(fill[:slots - 1]) + [last]])
    d = dict(cpus=np.array([64.0]), mem=np.array([65536.0]), host=np.array([host], np.uint32), k8s=np.ones(1, np.uint8),
             gpu_model=pad(0, [0, 0, 0]).astype(np.uint32), gpu_count=pad(0.0, [8.0, 4.0, 2.0]),  # (no gpus: a plain job may run here)
             disk_type=pad(2, [1, 3, 4]).astype(np.uint32), disk_space=pad(1000.5, [900.0, 800.0, 700.0]),
             attr=np.array([[3, 7, 5]], np.uint32), max_tasks=np.array([-1], np.int32), num_tasks=np.array([0], np.int32),
             location=np.array([5], np.uint32), host_start_s=np.array([-1], np.int64), ports=np.array([50], np.int32),
             scalars=np.array([[9.0, 9.0, 9.0]]))
    if run:
        d.update(run_cpus=np.array([0.0]), run_mem=np.array([0.0]), run_count=np.array([0], np.int32))
    d.update(over)
    return A.Offers(**d)


def stack(*rows):
    """several one-row tables with the same columns as one"""
    d = {}
    for name in H.COLS:
        cols = [getattr(r, name) for r in rows]
        assert all((c is None) == (cols[0] is None) for c in cols), name
        d[name] = None if cols[0] is None else np.concatenate(cols)
    return A.Offers(**d)


def column_cases(slots):
    """name -> (the special job's columns as [plain job, special job] arrays, the joining host's columns that let the special job in,
    the same columns with a value that keeps it out or sends it elsewhere).  The joining row is full_row(9, slots) with the overrides;
    "two": two joining rows (hosts 9, 10), the overrides go to host 10."""
    nan = np.nan
    last = lambda v, fill: np.array([list(fill[:slots - 1]) + [v]])
    gpu_job = dict(gpus=np.array([0.0, 1.0]), gpu_model=np.array([0, 2], np.uint32))
    gpu_map = dict(gpu_model=last(2, [1, 3, 4]).astype(np.uint32))
    return {
        "cpus": (dict(cpus=[1.0, 3.0]), dict(cpus=np.array([4.0])), dict(cpus=np.array([2.5])), False),
        "mem": (dict(mem=[100.0, 200.0]), dict(mem=np.array([250.0])), dict(mem=np.array([150.0])), False),
        "ports": (dict(ports=np.array([0, 2], np.int32)), dict(ports=np.array([3], np.int32)), dict(ports=np.array([1], np.int32)), False),
        "scalars": (dict(scalars=np.array([[nan, nan, nan], [nan, 3.0, nan]])), dict(scalars=np.array([[9.0, 5.0, 9.0]])),
                    dict(scalars=np.array([[9.0, 2.0, 9.0]])), False),
        "gpu_count": (gpu_job, dict(gpu_count=last(1.0, [8.0, 4.0, 2.0]), **gpu_map), dict(gpu_count=last(2.0, [8.0, 4.0, 2.0]), **gpu_map), False),
        "gpu_model": (gpu_job, dict(gpu_count=last(1.0, [8.0, 4.0, 2.0]), **gpu_map),
                      dict(gpu_count=last(1.0, [8.0, 4.0, 2.0]), gpu_model=last(6, [1, 3, 4]).astype(np.uint32)), False),
        "k8s": (gpu_job, dict(gpu_count=last(1.0, [8.0, 4.0, 2.0]), **gpu_map),
                dict(gpu_count=last(1.0, [8.0, 4.0, 2.0]), k8s=np.zeros(1, np.uint8), **gpu_map), False),
        "run_count": (gpu_job, dict(gpu_count=last(1.0, [8.0, 4.0, 2.0]), **gpu_map),
                      dict(gpu_count=last(1.0, [8.0, 4.0, 2.0]), run_count=np.array([1], np.int32), **gpu_map), False),
        "disk_space": (dict(disk_request=np.array([-1.0, 80.25]), disk_type=np.array([0, 2], np.uint32)), dict(disk_space=last(100.5, [900.0, 800.0, 700.0])),
                       dict(disk_space=last(80.0, [900.0, 800.0, 700.0])), False),
        "disk_type": (dict(disk_request=np.array([-1.0, 80.25]), disk_type=np.array([0, 2], np.uint32)), dict(),
                      dict(disk_type=last(6, [1, 3, 4]).astype(np.uint32)), False),
        "attr": (dict(eq_off=np.array([0, 0, 1], np.uint32), eq_key=np.array([1], np.uint32), eq_val=np.array([8], np.uint32)),
                 dict(attr=np.array([[3, 8, 5]], np.uint32)), dict(attr=np.array([[8, 3, 8]], np.uint32)), False),
        "max_tasks": (dict(), dict(max_tasks=np.array([3], np.int32), num_tasks=np.array([2], np.int32)),
                      dict(max_tasks=np.array([2], np.int32), num_tasks=np.array([2], np.int32)), False),
        "num_tasks": (dict(), dict(max_tasks=np.array([3], np.int32), num_tasks=np.array([2], np.int32)),
                      dict(max_tasks=np.array([3], np.int32), num_tasks=np.array([3], np.int32)), False),
        "location": (dict(ckpt_location=np.array([0, 6], np.uint32)), dict(location=np.array([6], np.uint32)), dict(location=np.array([4], np.uint32)), False),
        "host_start_s": (dict(est_end_ms=np.array([0, 700_000], np.int64)), dict(host_start_s=np.array([1000], np.int64)),
                         dict(host_start_s=np.array([0], np.int64)), False),
        # the fuller host is the better fit: of two joining hosts that differ in nothing else the second one wins
        "run_cpus": (dict(), dict(run_cpus=np.array([10.0])), dict(), True),
        "run_mem": (dict(), dict(run_mem=np.array([5000.0])), dict(), True),
    }


def check_columns(make_engine, *, slots):
    """Two jobs, K = 1.  The staged host 7 (every column staged but run_*, which the carry of cycle 1 brings into existence) takes the
    plain job 0 in cycle 0 and has no cpus left for job 1.  Cycle 1 carries and joins host 9 (and 10): job 1 goes there only because of
    the one column, as the same cycles with that column's value changed show on the oracle."""
    params = P1(host_lifetime_mins=10)
    for name, (job_cols, good, bad, two) in column_cases(slots).items():
        jc = dict(job_cols)
        cpus, mem = jc.pop("cpus", [1.0, 1.0]), jc.pop("mem", [100.0, 100.0])
        staged = full_row(7, slots, run=False, cpus=np.array([1.5]), host_start_s=np.array([0], np.int64))
        pool = X.tiny_pool(2, staged, cpus=cpus, mem=mem, **jc)

        def cycles_with(over):
            rows = [full_row(9, slots), full_row(10, slots, **over)] if two else [full_row(9, slots, **over)]
            return [H.cycle(1), H.cycle(1, carry_offers=True, hosts=A.HostChurn(join=stack(*rows), before=[7] * len(rows)))]
        cycles = cycles_with(good)
        want, other = H.oracle(params, pool, cycles), H.oracle(params, pool, cycles_with(bad))
        assert want[0].j2o.tolist() == [0] and want[1].offers.run_cpus is not None, name
        assert want[1].j2o.tolist() == [1 if two else 0], (name, want[1].j2o)
        assert other[1].j2o.tolist() == [0 if two else -1], (name, other[1].j2o)
        compare(run_engine(make_engine, params, pool, cycles), want, cycles, f"{name} x{slots}:")


def check_null_columns(make_engine):
    """(a) the optional columns staged as NULL (no attributes, no named scalars, no maps) and absent from join: the table gains only
    what the carry brings into existence, and the joining rows get 0 there; (b) every column staged, join with cpus / mem / host alone:
    the joining rows get what NULL means for every column, -1 for max_tasks and host_start_s"""
    params = P1()
    bare = lambda ids, cpus: A.Offers(cpus=np.asarray(cpus, float), mem=np.full(len(ids), 1000.0), host=np.asarray(ids, np.uint32))
    # (a)
    pool = X.tiny_pool(3, bare([7], [1.5]), cpus=[1.0, 3.0, 3.0])
    cycles = [H.cycle(1), H.cycle(1, carry_offers=True, hosts=A.HostChurn(join=bare([9, 10], [4.0, 4.0]), before=[7, NONE])),
              H.cycle(1, carry_offers=True, hosts=A.HostChurn(leave=[9], join=bare([11], [5.0])))]
    want = H.oracle(params, pool, cycles)
    assert [w.j2o.tolist() for w in want] == [[0], [0], [1]] and want[2].offers.host.tolist() == [7, 10, 11]
    assert want[2].offers.run_count.tolist() == [1, 0, 0] and want[2].offers.attr is None and want[2].offers.scalars is None
    check(make_engine, params, pool, cycles, want)
    # (b)
    for slots in (1, 4):
        staged = stack(full_row(7, slots, cpus=np.array([1.5]), max_tasks=np.array([5], np.int32)), full_row(8, slots, cpus=np.array([2.0])))
        pool = X.tiny_pool(3, staged, cpus=[1.0, 3.0, 3.0])
        cycles = [H.cycle(1), H.cycle(1, carry_offers=True, hosts=A.HostChurn(leave=[8], join=bare([9], [4.0]), before=[8]))]
        want = H.oracle(params, pool, cycles)
        t = want[1].offers
        assert t.host.tolist() == [7, 9] and t.max_tasks.tolist() == [5, -1] and t.host_start_s.tolist() == [-1, -1] and t.k8s.tolist() == [1, 0]
        assert t.attr[1].tolist() == [0, 0, 0] and t.scalars[1].tolist() == [0.0, 0.0, 0.0] and t.ports.tolist() == [50, 0]
        assert want[1].j2o.tolist() == [1]
        check(make_engine, params, pool, cycles, want)


# ---- 4: kernel boundaries -----------------------------------------------------------------------------------------------------------------
def wide_pool(M, n_jobs=24, seed=7):
    """M hosts (ids 3 r + 1) with a few of the columns, non-dyadic amounts; n_jobs jobs of one user"""
    rng = np.random.default_rng(seed + M)
    offers = A.Offers(cpus=rng.choice([2.1, 4.3, 8.7], M), mem=rng.choice([1000.5, 2000.25, 4000.75], M), host=(3 * np.arange(M) + 1).astype(np.uint32),
                      attr=rng.integers(1, 5, (M, 2)).astype(np.uint32), run_cpus=rng.choice([0.0, 0.3, 1.7], M), run_mem=np.zeros(M),
                      run_count=np.zeros(M, np.int32))
    return X.tiny_pool(n_jobs, offers, cpus=rng.choice([0.7, 1.1, 2.9], n_jobs), mem=rng.choice([100.5, 300.25], n_jobs))


def fresh_rows(pool, n, first_host, seed=3):
    rng = np.random.default_rng(seed + n)
    return H.rows_like(pool.offers, rng.integers(0, pool.offers.n, n), first_host + np.arange(n))


def boundary_churn(pool, M):
    """the leaves and joins of one boundary shape, over the table [3 r + 1]"""
    host = lambda r: 3 * r + 1
    leave = [host(0), host(M - 1)]
    before = []
    if M >= 200:
        leave += [host(r) for r in range(100, 165)]  # a run of 65 adjacent rows
    before += [host(10)] * 65                         # 65 joins on one anchor
    if M >= 1000:
        before += [host(r) for r in range(500, 800)]  # 300 joins over 300 anchors
    before += [NONE, host(M - 1), host(0), NONE]
    return A.HostChurn(leave=leave, join=fresh_rows(pool, len(before), 100_000), before=before)


def check_boundary(make_engine, M):
    params = P1()
    pool = wide_pool(M)
    k = 8
    cycles = [H.cycle(k), H.cycle(k, carry_offers=True, hosts=boundary_churn(pool, M)), H.cycle(k, carry_offers=True)]
    want = H.oracle(params, pool, cycles)
    ch = want[1].churn
    assert ch["left"] == (67 if M >= 200 else 2) and ch["joined"] == 69 + (300 if M >= 1000 else 0) and ch["n_offers"] == M - ch["left"] + ch["joined"]
    assert all((w.j2o >= 0).any() for w in want)
    return check(make_engine, params, pool, cycles, want)


def check_empty_tables(make_engine):
    """all rows leave with joins (no old row survives); all rows leave with none (no offers: nothing matches, no launch fails); a
    churn onto the empty table"""
    params = P1()
    pool = wide_pool(65, n_jobs=12)
    all_of = lambda w: [int(h) for h in w.host]
    steps = [lambda hist, o: A.HostChurn(leave=all_of(o), join=fresh_rows(pool, 3, 500), before=[int(o.host[64]), int(o.host[0]), NONE]),
             lambda hist, o: A.HostChurn(leave=all_of(o) + [9]),
             lambda hist, o: A.HostChurn(leave=[500], join=fresh_rows(pool, 5, 600), before=None),
             lambda hist, o: A.HostChurn(join=fresh_rows(pool, 2, 700), before=[602, NONE])]
    cycles = [H.cycle(2)] + [H.cycle(2, carry_offers=True, hosts=s) for s in steps]
    want = H.oracle(params, pool, cycles)
    assert [w.offers.n for w in want] == [65, 3, 0, 5, 7] and want[1].offers.host.tolist() == [501, 500, 502]
    assert want[2].j2o.tolist() == [-1, -1] and want[2].churn == dict(left=3, leave_missing=1, joined=0, n_offers=0)
    assert want[3].churn == dict(left=0, leave_missing=1, joined=5, n_offers=5) and (want[3].j2o >= 0).all()
    assert want[4].offers.host.tolist() == [600, 601, 700, 602, 603, 604, 701]
    return check(make_engine, params, pool, cycles, want)


# ---- 5: without an advance ------------------------------------------------------------------------------------------------------------------
def check_no_advance(make_engine, hosts=(0, 2, 5)):
    """the last cycle considered nothing: the churn still runs — behind a release of the same call on the host that leaves, with a
    leave_host that has no row.  hosts: the staged ids; sparse ones go past the host-indexed table (the rows are looked up in o_host)"""
    params = P1()
    pool = X.tiny_pool(3, X._offers([4.0, 9.0, 9.5], host=hosts), cpus=3.0)
    first = lambda h: R.finished_of(h, [(0, 0)], offers=1)
    churn = A.HostChurn(leave=[hosts[0], hosts[2] + 3], join=_hosts([hosts[2] + 1, hosts[2] + 2], cpus=[3.5, 3.25]), before=[hosts[0], hosts[1]])
    cycles = [H.cycle(1), H.cycle(0, carry_offers=True), H.cycle(2, carry_offers=True, finished=first, hosts=churn)]
    want = H.oracle(params, pool, cycles)
    assert [w.j2o.tolist() for w in want] == [[0], [], [1, 0]], [w.j2o.tolist() for w in want]
    assert want[2].info["with_row"] == 1 and want[2].churn == dict(left=1, leave_missing=1, joined=2, n_offers=4)
    assert want[2].offers.host.tolist() == [hosts[2] + 1, hosts[2] + 2, hosts[1], hosts[2]]
    check(make_engine, params, pool, cycles, want)
    # an empty queue: the one job is placed and leaves; the churn still runs and a rank sees the churned table
    pool = X.tiny_pool(1, X._offers([4.0, 9.0, 9.5], host=hosts), cpus=3.0)
    cycles = [H.cycle(1), H.cycle(1, carry_offers=True), H.cycle(1, carry_offers=True, hosts=churn)]
    want = H.oracle(params, pool, cycles)
    assert [len(w.Q) for w in want] == [1, 0, 0] and want[2].churn["joined"] == 2
    check(make_engine, params, pool, cycles, want)


# ---- 6: groups -----------------------------------------------------------------------------------------------------------------------------
def check_groups(make_engine):
    params = P1()
    # -- unique: job 0 runs on host 0, which leaves and returns: the cotask is kept by host id and still blocks the group there
    pool = X.tiny_pool(4, X._offers([3.0, 8.0]), groups=A.Groups(type=np.array([1], np.uint8)), group=np.array([0, 0, 0, NONE], np.uint32), cpus=2.0)
    cycles = [H.cycle(1), H.cycle(1, hosts=A.HostChurn(leave=[0])), H.cycle(2, hosts=A.HostChurn(join=X._offers([3.0], host=[0]), before=[1]))]
    want = H.oracle(params, pool, cycles)
    # cycle 2: the group's member finds host 0 (the tighter fit, row 0) and host 1 taken; the job without a group goes to host 0
    assert [w.j2o.tolist() for w in want] == [[0], [0], [-1, 0]], [w.j2o.tolist() for w in want]
    assert want[2].offers.host.tolist() == [0, 1] and want[2].table.run_hosts == [[0, 1]]
    check(make_engine, params, pool, cycles, want)
    # -- attribute-equals: the first member goes to the JOINED host 9 (attribute 9) in the cycle it joins; the next advance folds the
    #    cotask in with that row's attribute, and the second member must go to host 2 (attribute 9) though host 0 fits tighter, where
    #    the job without a group goes
    g = A.Groups(type=np.array([3], np.uint8), attr_key=np.array([0], np.uint32), minimum=np.array([0], np.int32))
    pool = X.tiny_pool(3, X._offers([2.5, 9.0, 8.0], attr=[1, 1, 9]), groups=g, group=np.array([0, 0, NONE], np.uint32), cpus=2.0)
    cycles = [H.cycle(0), H.cycle(1, hosts=A.HostChurn(join=X._offers([2.0], attr=[9], host=[9]), before=[1])), H.cycle(2, carry_offers=True)]
    want = H.oracle(params, pool, cycles)
    assert want[1].offers.host.tolist() == [0, 9, 1, 2] and want[1].j2o.tolist() == [1]
    assert want[2].table.run_hosts == [[9]] and want[2].table.run_attrs == [[9]] and want[2].j2o.tolist() == [3, 0], want[2].j2o
    check(make_engine, params, pool, cycles, want)


# ---- 7: the class-ordered walk ----------------------------------------------------------------------------------------------------------------
def check_classfit(make_engine):
    """the form stays eligible across churns that raise the greatest host id (a host far above joins), lower it (it leaves again) and
    raise it again"""
    params = P1(match_algo=3)
    pool, cycles = X.classfit_case()
    top = int(pool.offers.host.max())
    tpl = pool.offers
    far = lambda host, row: H.rows_like(tpl, [row], [host])
    steps = [A.HostChurn(leave=[int(tpl.host[3])], join=far(top + 5000, 3), before=[int(tpl.host[0])]),
             A.HostChurn(leave=[top + 5000, int(tpl.host[4])], join=far(int(tpl.host[3]), 4)),
             A.HostChurn(leave=[top], join=far(top + 70, 5), before=[int(tpl.host[7])]),
             A.HostChurn(leave=[top + 70])]
    for cy, h in zip(cycles[1:], steps):
        cy.hosts = h
    want = H.oracle(params, pool, cycles)
    K.assert_every_cycle_mixed(want)
    assert [int(w.offers.host.max()) for w in want[1:3]] == [top + 5000, top] and int(want[4].offers.host.max()) < top
    assert K.differs(want[1:], H.oracle(params, pool, cycles, with_churn=False)[1:])
    return check(make_engine, params, pool, cycles, want, expect_form=3)


# ---- 8: multi ------------------------------------------------------------------------------------------------------------------------------
def check_multi(make_engine, *, scale=0.5):
    """three ragged pools through cook_cycle_run_queue_hosts_multi: pool 0 carries, releases and churns, pool 1 carries and releases only
    (no churn), pool 2 carries and churns and has its churn refused in round 2: it stays untouched (the same step runs next), the
    others go on; cook_cycle_match_multi places them"""
    params = P1(match_algo=2)
    shapes = [(1.0, 441, 5), (0.5, 442, 5), (0.7, 443, 4)]
    cases = [base_case(seed, scale=s * scale, n_cycles=n, fractional=(seed == 443)) for s, seed, n in shapes]
    for cy in cases[1][1][1:]:
        cy.hosts = None
    for cy in cases[2][1][1:]:
        cy.finished = None
    want = [H.oracle(params, pl, cs) for pl, cs in cases]
    for w in want:
        K.assert_every_cycle_mixed(w)
    assert all(w.churn["joined"] for i in (0, 2) for w in want[i][1:]) and all(w.hosts is None for w in want[1])
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
            fins, hosts = [cy.finished for cy in cur], [cy.hosts for cy in cur]
            if rnd == 2:  # pool 2's list names a host twice: refused for pool 2 alone
                h = hosts[2]
                hosts[2] = A.HostChurn(leave=list(h.leave) + [int(h.leave[0])], join=h.join, before=h.before)
                with pytest.raises(CookError) as ex:
                    cycle_run_queue_hosts_multi(engines, ks, steps, carries, fins, hosts)
                assert ex.value.code == COOK_E_INVALID
                live = [0, 1]
            else:
                live = [0, 1, 2]
                if any(nxt[i] >= len(cases[i][1]) for i in live):
                    break
                cycle_run_queue_hosts_multi(engines, ks, steps, carries, fins, hosts)
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


# ---- 9: refusals and persistence -----------------------------------------------------------------------------------------------------------
def check_refusals(make_engine, *, scale=0.5):
    params = P1()
    pool, cycles = base_case(405, scale=scale, n_cycles=4, extra=2)
    k, state, eligible = cycles[0].k, cycles[0].state, cycles[0].eligible
    want = H.oracle(params, pool, cycles)
    ok = want[1].hosts
    o = pool.offers
    staged = [int(h) for h in o.host]
    stay = next(h for h in staged if h not in set(int(x) for x in ok.leave))
    one = lambda host, **kw: H.rows_like(o, [0], [host]) if not kw else dataclasses.replace(H.rows_like(o, [0], [host]), **kw)
    both = A.QueueCarry(offers=True, usage=True)
    assert o.attr is None or o.attr.shape[1] != 7
    with make_engine(params) as e:
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, o, pool.groups)
        e.cycle_set_considerable(state, eligible)
        e.cycle_run(k)
        got = [fetch(e)]
        bad = [
            (A.HostChurn(leave=[staged[0], staged[1], staged[0]]), {}),                     # a host twice in leave_host
            (A.HostChurn(join=H.rows_like(o, [0, 1], [900_000, 900_000])), {}),               # ... twice in join
            (A.HostChurn(join=one(stay)), {}),                                                # joins, is staged and does not leave
            (A.HostChurn(join=one(900_000), before=[900_001]), {}),                           # the anchor is no OLD row
            (A.HostChurn(join=one(900_000), before=[900_000]), {}),                           # ... not even the joining host itself
            (ok, dict(offers=o)),                                                             # step->offers together with a churn
            (A.HostChurn(join=one(900_000, attr=np.ones((1, 7), np.uint32))), {}),            # another n_attr_keys (or: a column the table lacks)
            (A.HostChurn(join=one(900_000, scalars=np.ones((1, 2)))), {}),                    # named scalars the table lacks
            (A.HostChurn(join=one(900_000, location=np.ones(1, np.uint32))), {}) if o.location is None else None,
            (A.HostChurn(join=A.Offers(cpus=np.ones(400_000), mem=np.ones(400_000), host=(2_000_000 + np.arange(400_000)).astype(np.uint32))), {}),  # too many rows
        ]
        for item in bad:
            if item is None:
                continue
            hosts, step = item
            assert _code(lambda: e.cycle_run_queue_hosts(k, both, None, hosts, **step)) == COOK_E_INVALID, (vars(hosts), step)
        for miss in ("cpus", "mem", "host"):  # (the dataclass insists on them: the struct as a C caller could pass it)
            hs, keep = A.HostChurn(join=one(900_000)).as_struct()
            setattr(keep[0], miss, None)
            qs, keep2 = e._queue_step()
            assert e._lib.cook_cycle_run_queue_hosts(e._h, C.byref(qs), None, None, C.byref(hs), k) == COOK_E_INVALID, miss
        hs = A.CookHostChurn(2, None, None, None)  # n_leave without leave_host
        qs, keep2 = e._queue_step()
        assert e._lib.cook_cycle_run_queue_hosts(e._h, C.byref(qs), None, None, C.byref(hs), k) == COOK_E_INVALID
        assert e.churn_info() == dict(H.NO_CHURN, n_offers=o.n)
        again = fetch(e)
        _same_fetch(again, got[0])
        # the same steps without the offending part: the queue, the offers, the usage and the groups are as they were
        for cy in cycles[1:3]:
            run_step(e, cy)
            got.append(fetch(e))
        compare(got, want[:3], cycles[:3], "after the refusals:")
        # offer_skipped has one entry per row of the NEW table
        M_new = want[2].offers.n
        assert M_new == o.n + 4 == e.churn_info()["n_offers"]
        assert _code(lambda: e.cycle_run_queue_hosts(k, None, None, None, offer_skipped=np.zeros(o.n, np.uint8))) == COOK_E_INVALID
        e.cycle_run_queue_hosts(k, None, None, None, offer_skipped=np.zeros(M_new, np.uint8))
        assert e.churn_info() == dict(H.NO_CHURN, n_offers=M_new)  # (of the last QUEUE cycle: it had none)
        # a rank keeps the churned table ...
        e.cycle_run(k)
        same_table(e.fetch_offers().offers(), want[2].offers, "after a rank:")
        # ... two rows on one host: refused; and step->offers replaces the churned table
        dup = A.Offers(cpus=o.cpus, mem=o.mem, host=np.concatenate([o.host[:-1], o.host[:1]]).astype(np.uint32))
        e.cycle_run_queue(k, offers=dup)
        assert _code(lambda: e.cycle_run_queue_hosts(k, None, None, A.HostChurn(leave=[staged[1]]))) == COOK_E_INVALID
        e.cycle_run_queue(k, offers=o)
        same_table(e.fetch_offers().offers(), o, "replaced:")
        assert e.churn_info() == dict(H.NO_CHURN, n_offers=o.n)
    # hosts = NULL and both lists empty are cook_cycle_run_queue_release, byte for byte
    outs = []
    for mode in ("release", "null", "empty"):
        with make_engine(params) as e:
            e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, o, pool.groups)
            e.cycle_set_considerable(state, eligible)
            e.cycle_run(k)
            for cy in cycles[1:3]:
                if mode == "release":
                    e.cycle_run_queue_release(k, both, cy.finished)
                else:
                    empty = A.HostChurn(join=H.rows_like(o, [], []), before=[]) if mode == "empty" else None
                    e.cycle_run_queue_hosts(k, both, cy.finished, empty)
                    assert e.churn_info() == dict(H.NO_CHURN, n_offers=o.n)
            outs.append((vars(S.fetch(e, False)), e.match_metrics(n_users=pool.users.n), e.match_explain(np.arange(30)), e.release_info()))
    for x in outs[1:]:
        X._same(x, outs[0])


def _same_fetch(a, b):
    plain = lambda g: {k: v for k, v in vars(g).items() if k != "offers"}
    X._same(plain(a), plain(b))
    same_table(a.offers, b.offers, "unchanged:")


def check_built_offers(make_engine, n_nodes=30, n_pods=100, n_jobs=60, k=20):
    """offers built on the device: the engine holds no record of their hosts.  COOK_E_STATE, nothing changes, and the fetch still
    shows the table (the rows of cook_offers_run); with the same rows staged from the host the same churn goes through"""
    from cook_amd import synth
    params = P1()
    nodes, pods, op = synth.make_cluster_state(seed=31, n_nodes=n_nodes, n_pods=n_pods, n_attr_keys=0, fractional=True, max_pods=14)
    pool = synth.make_pool(seed=32, n_pending=n_jobs, n_running=n_jobs // 4, n_users=10, n_offers=10, gpus=True, fractional=True)
    with make_engine(params) as e:
        e.offers_stage(nodes, pods, op)
        e.offers_run()
        e.cycle_stage_built_offers(pool.tasks, pool.users, pool.pending_jobs, None, with_task_limits=True)
        e.cycle_run(k)
        before = fetch(e)
        assert before.offers.n > 2
        churn = A.HostChurn(leave=[int(before.offers.host[0])])
        assert _code(lambda: e.cycle_run_queue_hosts(k, None, None, churn)) == COOK_E_STATE
        _same_fetch(fetch(e), before)
        e.cycle_run_queue(k, offers=before.offers)  # the same rows from the host: now they can be churned
        e.cycle_run_queue_hosts(k, None, None, churn)
        assert e.churn_info() == dict(left=1, leave_missing=0, joined=0, n_offers=before.offers.n - 1)
        assert e.fetch_offers().offers().host.tolist() == before.offers.host.tolist()[1:]


# ---- 10: the fetch alone -------------------------------------------------------------------------------------------------------------------
def check_fetch(make_engine, *, scale=0.5):
    params = P1()
    # behind a plain stage: the staged columns, whatever was staged; NULL pointers are skipped; cap too small is refused
    for slots in (1, 4):
        t = stack(full_row(7, slots), full_row(8, slots, cpus=np.array([2.25])), full_row(3, slots, run_cpus=np.array([0.1])))
        pool = X.tiny_pool(2, t)
        with make_engine(params) as e:
            assert _code(lambda: e.fetch_offers()) == COOK_E_STATE
            e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, t, None)
            same_table(e.fetch_offers().offers(), t, f"staged x{slots}:")
            rows = A.OfferRows(3, n_attr_keys=3, skip=("mem", "attr", "gpu_count", "scalars", "host_start_s"))
            got = e.fetch_offers(rows)
            assert got.n == 3 and got.column("mem") is None and got.column("attr") is None and got.column("scalars") is None
            assert np.array_equal(got.column("cpus"), t.cpus) and np.array_equal(got.column("disk_space").reshape(t.disk_space.shape), t.disk_space)
            small = A.OfferRows(2, n_attr_keys=3)
            assert _code(lambda: e.fetch_offers(small)) == COOK_E_INVALID and small.n == 3 and not small.arrays["cpus"].any()
            e.cycle_run(1)
            same_table(e.fetch_offers().offers(), t, "a match changes nothing:")
    # bare columns: everything else comes back as what NULL means
    t = A.Offers(cpus=np.array([1.5, 2.5]), mem=np.array([10.0, 20.0]), host=np.array([4, 2], np.uint32))
    pool = X.tiny_pool(1, t)
    with make_engine(params) as e:
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, t, None)
        f = e.fetch_offers().offers()
        same_table(f, t, "bare:")
        assert f.max_tasks.tolist() == [-1, -1] and f.host_start_s.tolist() == [-1, -1] and f.ports.tolist() == [0, 0] and f.attr is None
    # behind carry + release (no churn at all): the columns the oracles of the carry and the release hold
    pool, cycles = X.base_case(305, scale=scale, n_cycles=4, fractional=True)
    want = R.oracle(params, pool, cycles)
    assert all(w.finished is not None for w in want[1:])
    with make_engine(params) as e:
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        for c, cy in enumerate(cycles):
            if cy.state is not None:
                e.cycle_set_considerable(cy.state, cy.eligible)
            if c == 0:
                e.cycle_run(cy.k)
            else:
                X.run_step(e, cy)
            same_table(e.fetch_offers().offers(), want[c].offers, f"carry + release, cycle {c}:")
            assert np.array_equal(S.fetch(e, False).j2o, want[c].j2o)


def distinct_table(slots, n=3, *, bare=False, first=0):
    """n rows whose values differ from column to column among the columns of one element type, and from row to row: two columns (or two
    named scalars, or two map entries) that change places show in a fetch.  Host ids do not ascend.  bare: cpus, mem and host alone"""
    counters = {np.float64: first, np.uint32: first, np.int32: first, np.int64: first}

    def take(dt, *shape, start, step):
        k = int(np.prod(shape))
        c = counters[dt]
        counters[dt] = c + k
        return (start + step * (c + np.arange(k))).astype(dt).reshape(shape)
    f64 = lambda *shape: take(np.float64, *shape, start=1.5, step=0.25)
    u32 = lambda *shape: take(np.uint32, *shape, start=11, step=1)
    i32 = lambda *shape: take(np.int32, *shape, start=3, step=1)
    d = dict(cpus=f64(n), mem=f64(n), host=np.roll(u32(n), 1))
    if not bare:
        d.update(k8s=(np.arange(n) % 3).astype(np.uint8)[::-1].copy(), gpu_model=u32(n, slots), gpu_count=f64(n, slots), disk_type=u32(n, slots),
                 disk_space=f64(n, slots), attr=u32(n, 3), max_tasks=i32(n), num_tasks=i32(n), location=u32(n),
                 host_start_s=take(np.int64, n, start=100_000, step=7), run_cpus=f64(n), run_mem=f64(n), run_count=i32(n), ports=i32(n),
                 scalars=f64(n, 3))
    t = A.Offers(**d)
    for dt in counters:  # the property the case rests on, on the table itself
        vals = np.concatenate([np.asarray(getattr(t, c)).ravel() for c in H.COLS if getattr(t, c) is not None and np.asarray(getattr(t, c)).dtype == dt] or [np.zeros(0, dt)])
        assert len(np.unique(vals)) == len(vals), dt
    assert n < 2 or not (np.diff(t.host.astype(np.int64)) > 0).all()
    return t


def check_fetch_routes(make_engine):
    """Every route that stages an offer table stages every column where the fetch (and so the next match) reads it: a table of pairwise
    distinct values comes back as it went in — through cook_match_stage, cook_cycle_stage, cook_cycle_update over another table,
    cook_cycle_run_queue's step->offers, and a churn that joins all of its rows while the one old row leaves.  The same with cpus, mem
    and host alone: every other column reads as what NULL means, attr and scalars are absent."""
    params = P1()
    for slots, bare in ((1, False), (4, False), (1, True)):
        t = distinct_table(slots, bare=bare)
        other = distinct_table(5 - slots, n=2, bare=not bare, first=200)  # (update, step->offers: what was staged before)
        old = distinct_table(slots, n=1, bare=bare, first=400)             # (the churn: the row that leaves; the columns of t)
        pool = X.tiny_pool(2, t)

        def stage(e, offers):
            e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, offers, None)

        def by_update(e):
            stage(e, other)
            e.cycle_update(offers=t)

        def by_queue_step(e):
            stage(e, other)
            e.cycle_run(1)
            e.cycle_run_queue(1, offers=t)

        def by_churn(e):
            stage(e, old)
            e.cycle_run(1)
            e.cycle_run_queue_hosts(1, None, None, A.HostChurn(leave=[int(old.host[0])], join=t))
            assert e.churn_info() == dict(left=1, leave_missing=0, joined=3, n_offers=3)
        routes = dict(match_stage=lambda e: e.match_stage(pool.pending_jobs, t), cycle_stage=lambda e: stage(e, t), cycle_update=by_update,
                      queue_step=by_queue_step, churn=by_churn)
        for name, route in routes.items():
            where = f"{name} x{slots}{' bare' if bare else ''}:"
            with make_engine(params) as e:
                route(e)
                f = e.fetch_offers().offers()
            same_table(f, t, where)
            if bare:
                assert f.attr is None and f.scalars is None, where
                assert f.max_tasks.tolist() == [-1] * 3 and f.host_start_s.tolist() == [-1] * 3, where
                for c in ("k8s", "gpu_model", "gpu_count", "disk_type", "disk_space", "num_tasks", "location", "run_cpus", "run_mem", "run_count", "ports"):
                    assert not np.asarray(getattr(f, c)).any(), (where, c)


# ---- 11: ABI -------------------------------------------------------------------------------------------------------------------------------
def struct_layout_sources():
    structs = [("cook_host_churn", A.CookHostChurn), ("cook_churn_info", A.CookChurnInfo), ("cook_offer_rows", A.CookOfferRows)]
    fields = [(s, f, cls) for s, cls in structs for f, _ in cls._fields_]
    prints = "".join(f'printf("%zu ", offsetof({s}, {f}));' for s, f, _ in fields)
    sizes = "".join(f'printf("%zu ", sizeof({s}));' for s, _ in structs)
    text = ('#include <stdio.h>\n#include <stddef.h>\n#include "cookmatch.h"\nint main(){' + sizes + prints +
            'printf("%d\\n", COOK_ABI_VERSION);return 0;}')
    want = [C.sizeof(cls) for _, cls in structs] + [getattr(cls, f).offset for _, f, cls in fields]
    return text, want + [A.ABI_VERSION]
