"""The cases of cook_sweep_running, shared by the emulator (test_sweep_emu.py) and GPU (test_sweep_gpu.py) suites: the golden cases of
tests/golden/sweep.json on the oracle and the engine, random running sets compared bit for bit with the oracle of tests/sweep_oracle.py
(reason bytes, the three lists, threshold bit patterns NaN included, info), and that the call leaves a staged pool's cycle as it was."""
from __future__ import annotations

import math

import numpy as np

from cook_amd import _abi as A
from cook_amd.engine import CookError
from tests import golden_util as G
from tests import sweep_oracle as O

COOK_E_INVALID = -1
LONG_MAX = 2 ** 63 - 1


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def golden_inputs(c):
    """a case of tests/golden/sweep.json -> keyword arguments of Engine.sweep_running (the oracle takes the same)"""
    rows = c["rows"]
    kw = dict(start_ms=np.array([O.START_ABSENT if r["start_ms"] is None else r["start_ms"] for r in rows], dtype=np.int64),
              unknown=np.array([r["unknown"] for r in rows], dtype=np.uint8),
              max_runtime_ms=np.array([-1 if r["max_runtime_ms"] is None else r["max_runtime_ms"] for r in rows], dtype=np.int64),
              cancelled=np.array([r["cancelled"] for r in rows], dtype=np.uint8),
              group=np.array([A.NONE_U32 if r["group"] is None else r["group"] for r in rows], dtype=np.uint32),
              now_ms=c["now_ms"], default_timeout_ms=c["default_timeout_ms"], max_timeout_ms=c["max_timeout_ms"], what=c["what"], cap=c["cap"])
    if c["groups"] is not None:
        gs = c["groups"]
        succ = [s for g in gs for s in g["succ"]]
        kw["groups"] = dict(type=np.array([g["type"] for g in gs], dtype=np.uint8), quantile=np.array([g["quantile"] for g in gs], dtype=np.float64),
                            multiplier=np.array([g["multiplier"] for g in gs], dtype=np.float64),
                            job_count=np.array([g["job_count"] for g in gs], dtype=np.uint32),
                            succ_off=np.concatenate([[0], np.cumsum([len(g["succ"]) for g in gs])]).astype(np.uint32),
                            succ_start_ms=np.array([O.START_ABSENT if s[0] is None else s[0] for s in succ], dtype=np.int64),
                            succ_end_ms=np.array([-1 if s[1] is None else s[1] for s in succ], dtype=np.int64))
    return kw


def run_oracle(kw):
    """the oracle on Engine.sweep_running's keyword arguments -> its result, or the SweepError it raised"""
    try:
        return O.sweep(kw["now_ms"], kw["start_ms"], unknown=kw.get("unknown"), max_runtime=kw.get("max_runtime_ms"),
                       cancelled=kw.get("cancelled"), group=kw.get("group"), groups=kw.get("groups"),
                       default_timeout=kw.get("default_timeout_ms", 0), max_timeout=kw.get("max_timeout_ms", 0), what=kw.get("what", 7))
    except O.SweepError as ex:
        return ex


def run_engine(e, kw):
    """-> the engine's result, or (rc, info) of the error"""
    try:
        return e.sweep_running(**kw)
    except CookError as ex:
        return ex.code, dict(e.last_sweep_info)


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def same(got, want):
    """the engine's result equals the oracle's: reason bytes, lists, thresholds bit for bit, info"""
    assert isinstance(got, dict), got
    assert np.array_equal(got["reason"], np.asarray(want["reason"], dtype=np.uint8))
    for k in ("lingering", "stragglers", "cancelled"):
        assert np.array_equal(got[k], np.asarray(want[k], dtype=np.uint32)), (k, got[k][:10], want[k][:10])
    assert np.array_equal(_bits(got["threshold_s"]), _bits(want["threshold_s"])), \
        [(g, a, b) for g, (a, b) in enumerate(zip(got["threshold_s"], want["threshold_s"])) if not (a == b or (math.isnan(a) and math.isnan(b)))][:5]
    assert got["info"] == want["info"], (got["info"], want["info"])


# ---- golden ------------------------------------------------------------------------------------------------------------------------
def _expected(c):
    x = c["expect"]
    if x["rc"] != 0:
        return None
    thr = [math.nan if t is None else t for t in x["threshold_s"]]
    n = len(c["rows"])
    reason = [0] * n
    for k, bit in (("lingering", 1), ("stragglers", 2), ("cancelled", 4)):
        for i in x[k]:
            reason[i] |= bit
    info = dict(lingering=len(x["lingering"]), stragglers=len(x["stragglers"]), cancelled=len(x["cancelled"]), groups_ready=x["groups_ready"],
                bad_row=A.NONE_U32)
    return dict(reason=reason, lingering=x["lingering"], stragglers=x["stragglers"], cancelled=x["cancelled"], threshold_s=thr, info=info)


def check_golden_oracle():
    """the oracle reproduces every expectation of the golden file"""
    for c in G.load("sweep")["cases"]:
        kw = golden_inputs(c)
        got, want = run_oracle(kw), _expected(c)
        if want is None and "lingering" in c["expect"]:  # (a cap error is the engine's alone: the oracle has the lengths)
            assert {k: got["info"][k] for k in ("lingering", "stragglers", "cancelled")} == \
                {k: c["expect"][k] for k in ("lingering", "stragglers", "cancelled")}, c["name"]
        elif want is None:
            assert isinstance(got, O.SweepError), c["name"]
            bad = c["expect"]["bad_row"]
            assert got.bad_row == (A.NONE_U32 if bad is None else bad), (c["name"], got.bad_row)
        else:
            assert not isinstance(got, O.SweepError), (c["name"], got)
            assert got["reason"] == want["reason"] and got["info"] == want["info"], (c["name"], got)
            for k in ("lingering", "stragglers", "cancelled"):
                assert got[k] == want[k], (c["name"], k)
            assert _bits(got["threshold_s"]).tolist() == _bits(want["threshold_s"]).tolist(), (c["name"], got["threshold_s"])


def check_golden(make_engine):
    """the engine reproduces every expectation of the golden file, error codes and bad_row included"""
    with make_engine(A.default_params()) as e:
        for c in G.load("sweep")["cases"]:
            kw = golden_inputs(c)
            got, want = run_engine(e, kw), _expected(c)
            if want is None:
                x = c["expect"]
                assert isinstance(got, tuple) and got[0] == COOK_E_INVALID, (c["name"], got)
                info = got[1]
                assert info["bad_row"] == (A.NONE_U32 if x["bad_row"] is None else x["bad_row"]), (c["name"], info)
                for k in ("lingering", "stragglers", "cancelled"):
                    if k in x:
                        assert info[k] == x[k], (c["name"], info)
            else:
                try:
                    same(got, want)
                except AssertionError as ex:
                    raise AssertionError(f"{c['name']}: {ex}") from ex


# ---- random running sets -----------------------------------------------------------------------------------------------------------
NOW = 1_760_000_000_000


def random_table(seed, n, n_groups, n_succ, *, big_group=0, ties=False, unknown_frac=0.05, cancel_frac=0.01, grouped_frac=0.4):
    """Engine.sweep_running keyword arguments of a valid random running set: n rows (unknown_frac unknown, cancel_frac cancelled,
    grouped_frac in a group), n_groups groups of skewed size holding n_succ successful instances (big_group of them in group 0),
    job counts around the success counts (so that some groups are not ready), a fifth of the groups of type 0.  ties: s drawn from
    a few dozen values."""
    rng = np.random.default_rng(seed)
    G_ = n_groups
    w = rng.pareto(1.2, G_) + 0.05
    rest = n_succ - big_group
    cnt = np.floor(w / w.sum() * rest).astype(np.int64) if G_ else np.zeros(0, np.int64)
    if G_:
        cnt[rng.integers(0, G_, rest - int(cnt.sum()))] += 1 if rest > cnt.sum() else 0
        cnt[0] += big_group
        cnt[0] += n_succ - int(cnt.sum())
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    typ = (rng.random(G_) < 0.8).astype(np.uint8)
    q = rng.uniform(0.02, 0.98, G_)
    mult = rng.choice([1.5, 2.0, 2.5, 3.0, 1.1, 4.0 / 3.0, 1.7], G_)
    jc = np.maximum(0, np.floor(cnt * rng.uniform(0.3, 2.5, G_))).astype(np.int64) + rng.integers(0, 3, G_)
    jc = np.minimum(jc, 2 ** 31 - 1).astype(np.uint32)
    if ties:
        dur = rng.integers(0, 40, n_succ) * 1000 + rng.integers(0, 1000, n_succ)
    else:
        dur = rng.integers(0, 4 * 3600 * 1000, n_succ)
    noend = rng.random(n_succ) < 0.05
    s_start = NOW - dur - np.where(noend, 0, rng.integers(0, 30 * 86400 * 1000, n_succ))
    s_end = np.where(noend, -1, s_start + dur)
    groups = dict(type=typ, quantile=q, multiplier=mult, job_count=jc, succ_off=off, succ_start_ms=s_start.astype(np.int64),
                  succ_end_ms=s_end.astype(np.int64))
    unknown = (rng.random(n) < unknown_frac).astype(np.uint8)
    start = NOW - (rng.integers(0, 12 * 3600 * 1000, n) if not ties else rng.integers(0, 120, n) * 1000 + rng.integers(0, 1000, n))
    grouped = (rng.random(n) < grouped_frac) & (G_ > 0)
    p = cnt + 1.0
    group = np.where(grouped, rng.choice(max(G_, 1), n, p=p / p.sum()) if G_ else 0, A.NONE_U32).astype(np.uint32)
    absent = (rng.random(n) < 0.01) & (~grouped | (unknown == 1))  # (a running grouped row without a start would fail the call)
    start = np.where(absent, O.START_ABSENT, start).astype(np.int64)
    start = np.where(rng.random(n) < 0.002, NOW + rng.integers(1, 10 ** 6, n), start).astype(np.int64)  # a clock ahead of now
    start = np.where(grouped & (unknown == 0) & (start > NOW), NOW, start).astype(np.int64)
    mrt = np.where(rng.random(n) < 0.5, -1, rng.integers(0, 8 * 3600 * 1000, n))
    mrt = np.where(rng.random(n) < 0.05, LONG_MAX, mrt).astype(np.int64)
    cancelled = (rng.random(n) < cancel_frac).astype(np.uint8)
    return dict(start_ms=start, unknown=unknown, max_runtime_ms=mrt, cancelled=cancelled, group=group, groups=groups, now_ms=NOW,
                default_timeout_ms=int(rng.integers(3600 * 1000, 6 * 3600 * 1000)), max_timeout_ms=int(rng.integers(2 * 3600 * 1000, 10 * 3600 * 1000)))


def check_random(make_engine, kw, whats=(7,)):
    """one table, every `what` of whats, engine against oracle"""
    with make_engine(A.default_params()) as e:
        for w in whats:
            k = dict(kw, what=w)
            want = run_oracle(k)
            assert not isinstance(want, O.SweepError), want
            same(run_engine(e, k), want)
    return want


def corrupt(kw, seed):
    """the same table with one interval the reference cannot take in a ready group (a running row and a successful instance):
    -> (kw, the bad_row the oracle reports)"""
    rng = np.random.default_rng(seed)
    res = run_oracle(kw)
    ready = np.flatnonzero(~np.isnan(np.asarray(res["threshold_s"])))
    assert len(ready) >= 2
    g1, g2 = int(ready[-1]), int(ready[len(ready) // 2])
    k = dict(kw, groups=dict(kw["groups"]))
    ss = kw["groups"]["succ_start_ms"].copy()
    off = kw["groups"]["succ_off"]
    j = int(off[g1] + rng.integers(0, off[g1 + 1] - off[g1]))
    ss[j] = O.START_ABSENT
    k["groups"]["succ_start_ms"] = ss
    want = run_oracle(k)
    assert isinstance(want, O.SweepError) and want.bad_row == len(kw["start_ms"]) + j
    rows = np.flatnonzero((kw["group"] == g2) & (kw["unknown"] == 0))
    if len(rows):
        st = kw["start_ms"].copy()
        st[rows[-1]] = NOW + 5
        k2 = dict(k, start_ms=st)
        want2 = run_oracle(k2)
        assert isinstance(want2, O.SweepError) and want2.bad_row == min(int(rows[-1]), want2.bad_row)
        return [(k, want.bad_row), (k2, want2.bad_row)]
    return [(k, want.bad_row)]


def check_errors(make_engine, kw, seed):
    with make_engine(A.default_params()) as e:
        for k, bad in corrupt(kw, seed):
            got = run_engine(e, k)
            assert isinstance(got, tuple) and got[0] == COOK_E_INVALID and got[1]["bad_row"] == bad, (got, bad)
        same(run_engine(e, kw), run_oracle(kw))  # (and the handle works on afterwards)


# ---- the cycle of a staged pool is left alone ----------------------------------------------------------------------------------------
def check_cycle_undisturbed(make_engine, pool, table, k=200):
    """every fetch after the call is the one before it, and the next cook_cycle_run gives what the first gave"""
    with make_engine(A.default_params()) as e:
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        e.cycle_run(k)
        before = e.cycle_fetch()
        same(run_engine(e, table), run_oracle(table))
        after = e.cycle_fetch()
        e.cycle_run(k)
        again = e.cycle_fetch()
    for x in (after, again):
        assert np.array_equal(x[0], before[0]) and np.array_equal(x[1], before[1]) and x[2] == before[2]
