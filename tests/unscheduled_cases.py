"""The cases of cook_unscheduled, shared by the emulator (test_unscheduled_emu.py) and GPU (test_unscheduled_gpu.py) suites: the
reference's golden reasons and hand-derived edges (tests/golden/unscheduled.json), random pools against tests/unscheduled_oracle.py
bit for bit (all rows, a window mask, a list of rows; fractional pools whose sums round), the state rule, and that a call leaves the
cycle alone.  Every output is compared with == / array_equal: there is no tolerance anywhere."""
from __future__ import annotations

import numpy as np
import pytest

from cook_amd import _abi as A
from cook_amd import synth
from cook_amd.engine import CookError
from tests import golden_util as _G
from tests import unscheduled_oracle as O

COOK_E_INVALID, COOK_E_STATE = -1, -4
BITS = {"quota-count": A.UNSCHED_QUOTA_COUNT, "quota-cpus": A.UNSCHED_QUOTA_CPUS, "quota-mem": A.UNSCHED_QUOTA_MEM,
        "quota-gpus": A.UNSCHED_QUOTA_GPUS, "share-cpus": A.UNSCHED_SHARE_CPUS, "share-mem": A.UNSCHED_SHARE_MEM,
        "share-gpus": A.UNSCHED_SHARE_GPUS, "queue-position": A.UNSCHED_QUEUE_POSITION, "at-least": A.UNSCHED_AT_LEAST}
LITERAL_MAX = 4000  # tables up to this size are also answered job by job (unscheduled_literal)


def golden_inputs(case):
    """-> (Tasks, n_users, UnschedLimits, in_window or None, rows or None); ids and start times in creation (= listing) order"""
    names = case["users"]
    ts = case["tasks"]
    n = len(ts)
    pend = np.array([t["state"] == "waiting" for t in ts], dtype=np.uint8) if n else np.zeros(0, np.uint8)
    seq = np.arange(n, dtype=np.int64)
    tasks = A.Tasks(cpus=np.array([t["cpus"] for t in ts], dtype=np.float64), mem=np.array([t["mem"] for t in ts], dtype=np.float64),
                    gpus=None if case["no_gpus"] else np.array([t.get("gpus", 0.0) for t in ts], dtype=np.float64),
                    user=np.array([names.index(t["user"]) for t in ts], dtype=np.uint32),
                    priority=np.array([t.get("priority", 50) for t in ts], dtype=np.int32),
                    start_ms=np.where(pend == 1, 0, 1_600_000_000_000 + seq).astype(np.int64), task_id=17_592_186_050_000 + seq,
                    job_id=17_592_186_045_000 + seq, pending=pend)

    def col(table, key, default):
        return np.array([float(table.get(u, {}).get(key, default)) for u in names], dtype=np.float64)

    q, s = case["quota"], case["share"]
    lim = A.UnschedLimits(quota_count=col(q, "count", 2.0 ** 31 - 1), quota_cpus=col(q, "cpus", A.DMAX), quota_mem=col(q, "mem", A.DMAX),
                          quota_gpus=col(q, "gpus", A.DMAX), share_cpus=col(s, "cpus", A.DMAX), share_mem=col(s, "mem", A.DMAX),
                          share_gpus=col(s, "gpus", A.DMAX))
    win = None
    if case["window"] is not None:
        win = np.zeros(n, np.uint8)
        win[case["window"]] = 1
    rows = None if case["rows"] is None else np.array(case["rows"], dtype=np.uint32)
    return tasks, len(names), lim, win, rows


def _check_golden(case, got):
    names = case["users"]
    user_of = [names.index(t["user"]) for t in case["tasks"]]
    ask = list(range(len(case["tasks"]))) if case["rows"] is None else case["rows"]
    assert len(got["reasons"]) == len(got["queue_pos"]) == len(got["total"]) == len(ask), case["name"]
    for x in case["expect"]["rows"]:
        k = x["at"]
        where = (case["name"], case["ref"], k)
        assert int(got["reasons"][k]) == sum(BITS[b] for b in x["bits"]), (where, int(got["reasons"][k]), x["bits"])
        assert int(got["queue_pos"][k]) == x["queue_pos"], (where, int(got["queue_pos"][k]))
        if x["total"] is not None:
            assert got["total"][k].tolist() == [float(v) for v in x["total"]], (where, got["total"][k].tolist())
        if x["ahead"] is not None:
            u = user_of[ask[k]]
            assert got["ahead"][u, :min(x["queue_pos"], A.UNSCHED_AHEAD)].tolist() == x["ahead"], (where, got["ahead"][u].tolist())
    for u, v in case["expect"].get("list_len", {}).items():
        assert int(got["list_len"][names.index(u)]) == v, (case["name"], u, got["list_len"].tolist())
    for u, v in case["expect"].get("ahead", {}).items():
        assert got["ahead"][names.index(u)].tolist() == [A.NONE_U32 if r is None else r for r in v], (case["name"], u)


def check_golden(make_engine):
    for case in _G.load("unscheduled")["cases"]:
        tasks, n_users, lim, win, rows = golden_inputs(case)
        want = O.unscheduled_literal(tasks, n_users, lim, win, rows)
        _check_golden(case, want)  # (the restatement reproduces the reference's answers ...)
        O.assert_same(O.unscheduled(tasks, n_users, lim, win, rows), want)
        with make_engine(A.default_params()) as e:
            e.rank_stage(tasks, A.Users(div_cpus=np.full(n_users, A.DMAX), div_mem=np.full(n_users, A.DMAX)))
            e.rank_run()
            got = e.unscheduled(lim, in_window=win, rows=rows)
        _check_golden(case, got)      # (... and so does the engine)
        O.assert_same(got, want)


def random_limits(seed, n):
    rng = np.random.default_rng(seed)
    pick = lambda vals: np.asarray(vals, dtype=np.float64)[rng.integers(0, len(vals), n)]  # noqa: E731
    return A.UnschedLimits(quota_count=pick([0.0, 5.0, 50.0, 2.0 ** 31 - 1]), quota_cpus=pick([0.0, 20.0, 200.5, A.DMAX]),
                           quota_mem=pick([1.0, 1e5, 1e6, A.DMAX]), quota_gpus=pick([0.0, 10.0, A.DMAX, A.DMAX]),
                           share_cpus=pick([0.0, 8.0, 64.0, 64.1, A.DMAX]), share_mem=pick([0.0, 40960.0, 262144.0, 262144.3, A.DMAX]),
                           share_gpus=pick([0.0, 2.0, 8.0, A.DMAX]))


def _oracle(tasks, n_users, lim, win=None, rows=None):
    want = O.unscheduled(tasks, n_users, lim, win, rows)
    if tasks.n <= LITERAL_MAX:
        O.assert_same(want, O.unscheduled_literal(tasks, n_users, lim, win, rows))
    return want


def check_random(make_engine, pool: synth.Pool, seed=1, must_fold=False):
    """all rows; a random window; a random list of rows (repeats, running rows); NULL limits = the staged users.  must_fold: the pool
    is one in which some user's running cpus sum differently as a tree than left to right (checked here, on the CPU, before the
    engine is called), so that the engine's fold path is taken for at least that user."""
    n, N = pool.users.n, pool.tasks.n
    if must_fold:
        assert O.users_whose_cpus_sum_depends_on_order(pool.tasks), "choose a seed whose sums depend on the order of addition"
    rng = np.random.default_rng(seed)
    lim = random_limits(seed, n)
    win = (rng.random(N) < 0.6).astype(np.uint8)
    rows = rng.integers(0, max(N, 1), min(1000, 2 * N)).astype(np.uint32) if N else np.zeros(0, np.uint32)
    with make_engine(A.default_params()) as e:
        e.rank_stage(pool.tasks, pool.users)
        e.rank_run()
        got = e.unscheduled(lim)
        O.assert_same(got, _oracle(pool.tasks, n, lim))
        O.assert_same(e.unscheduled(lim, in_window=win), _oracle(pool.tasks, n, lim, win))
        O.assert_same(e.unscheduled(lim, in_window=win, rows=rows), _oracle(pool.tasks, n, lim, win, rows))
        O.assert_same(e.unscheduled(), _oracle(pool.tasks, n, A.UnschedLimits.from_users(pool.users)))
    return got


def one_user_pool(seed, n_running, n_pending, fractional=True):
    """one user holding every row (a segment far longer than a workgroup covers), a second user with a handful"""
    pool = synth.make_pool(seed=seed, n_pending=n_pending, n_running=n_running, n_users=2, n_offers=8, fractional=fractional)
    rng = np.random.default_rng(seed)
    pool.tasks.user[:] = (rng.random(pool.tasks.n) < 0.0005).astype(np.uint32)
    return pool


def check_state_rule(make_engine):
    """COOK_E_STATE before any rank and after a stage / cook_cycle_update no rank has followed; COOK_E_INVALID for limits of another
    size, a NULL column's stand-in (wrong n) and a row outside the table, which writes nothing"""
    pool = synth.make_pool(seed=31, n_pending=300, n_running=200, n_users=12, n_offers=16)
    lim = A.UnschedLimits.from_users(pool.users)
    with make_engine(A.default_params()) as e:
        with pytest.raises(CookError) as ex:
            e.unscheduled(lim)
        assert ex.value.code == COOK_E_STATE
        e.rank_stage(pool.tasks, pool.users)
        with pytest.raises(CookError) as ex:
            e.unscheduled(lim)
        assert ex.value.code == COOK_E_STATE
        e.rank_run()
        before = e.unscheduled(lim)
        O.assert_same(before, _oracle(pool.tasks, pool.users.n, lim))
        with pytest.raises(CookError) as ex:  # limits of another size
            e.unscheduled(A.UnschedLimits(np.ones(3)))
        assert ex.value.code == COOK_E_INVALID
        with pytest.raises(CookError) as ex:  # a row that is no row of the table
            e.unscheduled(lim, rows=[0, pool.tasks.n])
        assert ex.value.code == COOK_E_INVALID
        O.assert_same(e.unscheduled(lim), before)
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        e.cycle_run(50)
        O.assert_same(e.unscheduled(lim), before)
        # the first running task leaves: the rank's per-user order describes the old table until the next rank
        gone = int(np.flatnonzero(pool.tasks.pending == 0)[0])
        e.cycle_update(remove_task=[gone])
        with pytest.raises(CookError) as ex:
            e.unscheduled(lim)
        assert ex.value.code == COOK_E_STATE
        e.cycle_run(50)
        keep = np.ones(pool.tasks.n, bool)
        keep[gone] = False
        t = pool.tasks
        t2 = A.Tasks(cpus=t.cpus[keep], mem=t.mem[keep], user=t.user[keep], priority=t.priority[keep], start_ms=t.start_ms[keep],
                     task_id=t.task_id[keep], job_id=t.job_id[keep], pending=t.pending[keep])
        O.assert_same(e.unscheduled(lim), _oracle(t2, pool.users.n, lim))


def check_cycle_undisturbed(make_engine, pool: synth.Pool, k=200):
    """a cycle fetched after the calls (all rows, a window, a list of rows) is the one fetched without them"""
    lim = random_limits(3, pool.users.n)
    rng = np.random.default_rng(3)
    win = (rng.random(pool.tasks.n) < 0.5).astype(np.uint8)
    outs = []
    for with_calls in (False, True):
        with make_engine(A.default_params()) as e:
            e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
            e.cycle_run(k)
            if with_calls:
                e.unscheduled(lim)
                e.unscheduled(None, in_window=win, rows=np.arange(0, pool.tasks.n, 3))
            ranked, j2o, head = e.cycle_fetch()
            outs.append((ranked.copy(), j2o.copy(), head, e.cycle_fetch_considerable().copy(), e.rank_user_usage(pool.users.n).copy()))
    a, b = outs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3])
    assert np.array_equal(a[4].view(np.uint64), b[4].view(np.uint64))
