"""The cases of the rebalancer over the pool's resident cycle state (cook_cycle_rebalance_stage, cook_cycle_rebalance_fetch), shared by the
emulator (test_resident_rebalance_emu.py) and GPU (test_resident_rebalance_gpu.py) suites.  The expected value never comes from the
engine: tests/resident_rebalance_oracle.py restates the header's derived inputs in numpy over what the case itself staged and the
deltas it applied, and pyoracle.rebalance runs on the result.  Decisions (fp64 ==), preempted lists, pending_dru and the two index maps
must agree exactly.  What makes a case mean something is asserted on the oracle alone, before the engine is called."""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

from cook_amd import _abi as A
from cook_amd import synth
from cook_amd.engine import CookError, cycle_match_multi, reservations_of
from oracle import pyoracle
from tests import autoscale_cases as AS
from tests import golden_util as G
from tests import parity_cases as P
from tests import resident_rebalance_oracle as O

COOK_E_INVALID, COOK_E_STATE = -1, -4
NONE = A.NONE_U32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE_SEED = 54  # (chosen on the oracle: check_base asserts what it was chosen for)
PENDING_HOST = 3_000_000_000  # the host value of pending rows is never read: one that would size a 12 GB table if it were


def _code(fn):
    with pytest.raises(CookError) as ex:
        fn()
    return ex.value.code


def scan_tile() -> int:
    """seg_scan's tile (cook_amd/csrc/scan.hpp): the running rows are compacted by one scan over the pending flags"""
    text = open(os.path.join(ROOT, "cook_amd", "csrc", "scan.hpp")).read()
    return int(re.search(r"SS_THREADS = (\d+);", text).group(1)) * int(re.search(r"SS_IPT = (\d+);", text).group(1))


# ---- a cook_rebalance case as a cycle stage --------------------------------------------------------------------------------------------
def offers_of_case(b) -> A.Offers:
    """the hosts of the case's attribute table as the staged offers, carrying the case's spare as cpus / mem"""
    ha = b["host_attrs"]
    n_hosts = int(max(int(ha.host.max()), int(b["spare"].host.max()) if len(b["spare"].host) else 0)) + 1
    sc, sm = np.zeros(n_hosts), np.zeros(n_hosts)
    sc[b["spare"].host], sm[b["spare"].host] = b["spare"].cpus, b["spare"].mem
    return dataclasses.replace(ha, cpus=sc[ha.host], mem=sm[ha.host])


def embed(b, seed, *, offers=None, order=None) -> O.Mirror:
    """running ++ one pending row per job of a make_rebalance_case / golden dict, as ONE task table in `order` (default: a random
    interleaving), the jobs by pending ordinal"""
    run, jobs = b["running"], b["pending"]
    R, Pn = run.n, jobs.n
    pend_rows = A.Tasks(cpus=jobs.cpus, mem=jobs.mem, gpus=jobs.gpus if jobs.gpus is not None else np.zeros(Pn), user=jobs.user,
                        priority=b["pending_priority"], start_ms=np.zeros(Pn, np.int64), task_id=np.zeros(Pn, np.int64),
                        job_id=b["pending_job_id"], pending=np.ones(Pn, np.uint8), host=np.full(Pn, PENDING_HOST, np.uint32))
    if run.gpus is None:
        run = dataclasses.replace(run, gpus=np.zeros(R))
    order = np.random.default_rng(seed).permutation(R + Pn) if order is None else np.asarray(order, dtype=np.int64)
    tasks = O.tasks_take(O.tasks_cat(run, pend_rows), order)
    if offers is None:
        offers = offers_of_case(b)
    return O.Mirror(b["params"], tasks, b["users"], jobs.take(order[order >= R] - R), offers, b["groups"])


def mirror_of_pool(pool, params=None) -> O.Mirror:
    return O.Mirror(params if params is not None else A.default_params(), pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)


def equal(got, want, tag):
    P._rebal_equal(got, want, tag)
    assert np.array_equal(got["selected_task_idx"], want["selected_task_idx"]), (tag, "selected_task_idx")
    assert np.array_equal(got["selected_pending_ord"], want["selected_pending_ord"]), (tag, "selected_pending_ord")
    assert got["selected_task_idx"].dtype == np.uint32 and len(got["pending_dru"]) == len(want["selected_task_idx"]), tag


def resident_parity(make_engine, m: O.Mirror, rparams, tag, *, rank="cycle", min_decisions=0, **kw):
    """stage -> rank -> resident rebalance against the oracle on the derived inputs; -> (got, want)"""
    want = O.rebalance(O.derive(m, rparams, spare=kw.get("spare"), host_attrs=kw.get("host_attrs")))
    assert len(want["decisions"]) >= min_decisions, (tag, len(want["decisions"]))
    with make_engine(m.params) as e:
        m.stage(e)
        e.cycle_run(0) if rank == "cycle" else e.rank_run()
        got = e.cycle_rebalance(rparams, **kw)
    equal(got, want, tag)
    return got, want


# ---- 1: base -----------------------------------------------------------------------------------------------------------------------------
def check_base(make_engine):
    b = P.make_rebalance_case(BASE_SEED, 500, 40, 15, 40, constraints=True, gpus=True)
    m = embed(b, BASE_SEED)
    flips = int((np.diff(m.tasks.pending.astype(np.int64)) != 0).sum())
    assert flips > 20, "running and pending rows are interleaved: the compaction is not the identity"
    d = O.derive(m, b["rparams"])
    want = O.rebalance(d)
    assert len(want["decisions"]) >= 3 and any(len(x["tasks"]) > 1 for x in want["decisions"]), [len(x["tasks"]) for x in want["decisions"]]
    assert not np.array_equal(d["sel_ord"], np.arange(len(d["sel_ord"]))), "the queue order is not the pending order"
    with make_engine(m.params) as e:
        m.stage(e)
        e.cycle_run(0)
        e.cycle_rebalance_stage(b["rparams"])
        e.rebalance_run()
        got = e.cycle_rebalance_fetch()
        compact = e.rebalance_fetch()  # cook_rebalance_fetch behind a resident stage: the compacted spaces
        e.rebalance_run()  # repeatable on the same staged inputs
        again = e.cycle_rebalance_fetch()
    equal(got, want, "base")
    equal(again, want, "base, second run")
    P._rebal_equal(compact, dict(decisions=want["compact"], pending_dru=want["pending_dru"]), "base, compacted spaces")
    with make_engine(m.params) as e2:  # cook_rebalance given the derived inputs explicitly
        explicit = e2.rebalance(d["running"], d["pending"], d["pending_job_id"], d["pending_priority"], d["users"], d["spare"], d["rparams"],
                                host_attrs=d["host_attrs"], groups=d["groups"])
    P._rebal_equal(compact, explicit, "base, cook_rebalance on a second engine")


# ---- 2: kernel boundaries --------------------------------------------------------------------------------------------------------------
def boundary_sizes():
    return [0, 1, 255, 256, 257, scan_tile() + 1]


def small_case(seed, R, Pn=6, **kw):
    return P.make_rebalance_case(seed, R, Pn, 3, 8, constraints=True, gpus=True, **kw)


def check_running_rows(make_engine, R):
    b = small_case(900 + R, R)
    resident_parity(make_engine, embed(b, R), b["rparams"], f"R={R}")


def check_row_ends(make_engine):
    b = small_case(77, 40)
    R, Pn = 40, 6
    rng = np.random.default_rng(5)
    ends = lambda first, last: np.concatenate([[first], rng.permutation(np.setdiff1d(np.arange(R + Pn), [first, last])), [last]])
    pend_ends, run_ends = ends(R, R + Pn - 1), ends(0, R - 1)  # (sources below R are running rows)
    assert pend_ends[0] >= R and pend_ends[-1] >= R and sorted(pend_ends.tolist()) == list(range(R + Pn))
    assert run_ends[0] < R and run_ends[-1] < R and sorted(run_ends.tolist()) == list(range(R + Pn))
    for tag, order in (("pending at both ends", pend_ends), ("running at both ends", run_ends)):
        resident_parity(make_engine, embed(b, 0, order=order), b["rparams"], tag, min_decisions=1)


def check_max_preemption(make_engine):
    b = small_case(78, 60, Pn=9)
    m = embed(b, 78)
    for mp in (0, 1, 1000, -3):
        rp = A.CookRebalanceParams(b["rparams"].safe_dru_threshold, b["rparams"].min_dru_diff, mp, 0)
        got, want = resident_parity(make_engine, m, rp, f"max_preemption={mp}")
        assert len(got["selected_task_idx"]) == (0 if mp <= 0 else min(mp, 9))


def open_state(n_users) -> A.UserState:
    """a user state that filters nothing: only the eligible mask of cook_cycle_set_considerable matters to the rebalancer"""
    z = np.zeros(n_users)
    return A.UserState(quota_count=np.full(n_users, 2.0 ** 31 - 1), quota_cpus=np.full(n_users, A.DMAX), quota_mem=np.full(n_users, A.DMAX),
                       quota_gpus=np.full(n_users, A.DMAX), usage_count=z, usage_cpus=z, usage_mem=z, usage_gpus=z)


def check_masks(make_engine):
    b = small_case(79, 80, Pn=12)
    m = embed(b, 79)
    ranked, _ = pyoracle.rank(m.params, m.tasks, m.users)
    ordv = m.pend_ord()
    head = np.ones(12, np.uint8)
    head[ordv[ranked[0]]] = 0
    some = (np.random.default_rng(3).random(12) < 0.6).astype(np.uint8)
    for tag, mask in (("the head removed", head), ("some removed", some), ("all removed", np.zeros(12, np.uint8))):
        want = O.rebalance(O.derive(m, b["rparams"], eligible=mask))
        assert len(want["selected_task_idx"]) == int(mask[ordv[ranked]].sum())
        if tag == "the head removed":
            assert ranked[0] not in want["selected_task_idx"].tolist() and len(want["selected_task_idx"]) == 11
        with make_engine(m.params) as e:
            m.stage(e)
            e.cycle_set_considerable(open_state(m.users.n), mask)
            e.cycle_run(0)
            equal(e.cycle_rebalance(b["rparams"]), want, tag)
            P._rebal_equal(e.rebalance_fetch(), dict(decisions=want["compact"], pending_dru=want["pending_dru"]), tag + ", compacted spaces")
            e.cycle_set_considerable(None)  # the filters switched off: no mask
            e.cycle_run(0)
            equal(e.cycle_rebalance(b["rparams"]), O.rebalance(O.derive(m, b["rparams"])), tag + ", then no mask")


# ---- 3: run paths that depend on device-computed stage values ------------------------------------------------------------------------------
def _kernels_of(make_engine, m, rparams, tag):
    want = O.rebalance(O.derive(m, rparams))
    with make_engine(m.params) as e:
        e.set_profiling(True)
        m.stage(e)
        e.cycle_run(0)
        got = e.cycle_rebalance(rparams)
        names = set(e.kernel_timings())
    equal(got, want, tag)
    return names, want


def check_fullest_host(make_engine):
    """rebal_decide_big is launched only when a host can hold more than 64 items: max_seg, computed on the device, decides (one pending
    job: the run adds the jobs placed so far to the bound)"""
    for full, expect in ((64, False), (65, True)):
        b = P.make_rebalance_case(31, 200, 1, 4, 12)
        host = b["running"].host.copy()
        host[:full] = 5
        host[full:] = np.where(host[full:] == 5, 6, host[full:])
        b["running"] = dataclasses.replace(b["running"], host=host)
        assert int(np.bincount(host).max()) == full
        rp = A.CookRebalanceParams(0.0, 0.05, 1, 0)
        offers = A.Offers(cpus=np.zeros(12), mem=np.zeros(12))
        names, _ = _kernels_of(make_engine, embed(b, 31, offers=offers), rp, f"fullest host {full}")
        assert ("rebal_decide_big" in names) == expect, (full, sorted(n for n in names if n.startswith("rebal_")))


def check_rescoring_paths(make_engine):
    """the shape of rebalance_paths: integer-valued resources re-score by rebal_rs_delta, a fractional resource by rebal_rs_local
    (user_safe from the compacted slots, spare_safe from the scattered tables)"""
    b = P.make_rebalance_case(58, 2600, 8, 2, 70, fractional=True)
    offers = A.Offers(cpus=np.zeros(70), mem=np.zeros(70))
    names, want = _kernels_of(make_engine, embed(b, 58, offers=offers), b["rparams"], "fractional")
    assert len(want["decisions"]) >= 3
    assert "rebal_rs_local" in names and "rebal_rs_delta" not in names, names
    b = P.make_rebalance_case(BASE_SEED, 500, 40, 15, 40, constraints=True, gpus=True)
    names, _ = _kernels_of(make_engine, embed(b, BASE_SEED), b["rparams"], "integer")
    assert "rebal_rs_delta" in names and "rebal_rs_local" not in names, names


# ---- 4: behind cook_cycle_update ---------------------------------------------------------------------------------------------------------
def _delta(pool, seed, n_run, n_pend, with_host=True, id_base=50_000_000):
    """rows to append, drawn like the pool's: n_run running rows (with hosts) and n_pend pending rows with their jobs"""
    extra = synth.make_pool(seed, n_pend, n_run, pool.users.n, pool.offers.n, gpus=pool.tasks.gpus is not None,
                            constraints=pool.pending_jobs.eq_off is not None, id_base=17_592_186_044_416 + id_base)
    t = extra.tasks if with_host else dataclasses.replace(extra.tasks, host=None)
    return t, extra.pending_jobs


def check_update(make_engine):
    pool = synth.make_pool(41, 60, 300, 6, 24, gpus=True, constraints=True)
    m = mirror_of_pool(pool)
    rp = A.CookRebalanceParams(0.0, 0.05, 30, 0)
    rng = np.random.default_rng(41)
    run_rows, pend_rows = np.flatnonzero(pool.tasks.pending == 0), np.flatnonzero(pool.tasks.pending != 0)
    remove = np.sort(np.concatenate([rng.choice(run_rows[20:-20], 25, replace=False), rng.choice(pend_rows[5:-5], 10, replace=False)]))
    add_t, add_j = _delta(pool, 4141, 30, 12)
    with make_engine(m.params) as e:
        m.stage(e)
        e.cycle_run(0)
        equal(e.cycle_rebalance(rp), O.rebalance(O.derive(m, rp)), "before the update")
        m.update(e, remove, add_t, add_j)
        assert _code(lambda: e.cycle_rebalance_stage(rp)) == COOK_E_STATE  # no rank has followed the update
        e.cycle_run(0)
        want = O.rebalance(O.derive(m, rp))
        assert len(want["decisions"]) >= 1 and want["selected_task_idx"].max() >= pool.tasks.n - len(remove)  # a job the delta added is selected
        equal(e.cycle_rebalance(rp), want, "behind the update")


def check_update_without_host(make_engine):
    pool = synth.make_pool(42, 40, 200, 5, 16)
    m = mirror_of_pool(pool)
    rp = A.CookRebalanceParams(0.0, 0.05, 20, 0)
    add_t, add_j = _delta(pool, 4242, 8, 4, with_host=False)
    first_t, first_j = _delta(pool, 4243, 0, 5, with_host=False, id_base=60_000_000)
    with make_engine(m.params) as e:
        m.stage(e)
        m.update(e, [3], first_t, first_j)  # pending rows without host: their host is never read, the column stays complete
        e.cycle_run(50)
        equal(e.cycle_rebalance(rp), O.rebalance(O.derive(m, rp)), "pending rows without host")
        m.update(e, [], add_t, add_j)  # running rows without host: not refused ...
        e.cycle_run(50)  # ... and the cycle still runs
        ranked, j2o, _ = e.cycle_fetch()
        want_ranked, want_j2o, _ = pyoracle.cycle(m.params, m.tasks, m.users, m.jobs, m.offers, m.groups, K=50)
        assert np.array_equal(ranked, want_ranked) and np.array_equal(j2o, want_j2o)
        assert _code(lambda: e.cycle_rebalance_stage(rp)) == COOK_E_STATE
        assert "host" in e._lib.cook_last_error(e._h).decode()
        # a fresh stage with hosts heals it
        m.tasks = dataclasses.replace(m.tasks, host=np.where(m.tasks.pending != 0, PENDING_HOST, np.arange(m.tasks.n) % 16).astype(np.uint32))
        m.stage(e)
        e.cycle_run(50)
        equal(e.cycle_rebalance(rp), O.rebalance(O.derive(m, rp)), "restaged with hosts")


# ---- 5: skip_matched -------------------------------------------------------------------------------------------------------------------------
def check_skip_matched(make_engine):
    pool = synth.make_pool(43, 80, 300, 6, 4)  # (few offers: the cycle cannot place all it considers)
    m = mirror_of_pool(pool)
    rp = A.CookRebalanceParams(0.0, 0.05, 40, 0)
    k = 30
    ranked, j2o, _ = pyoracle.cycle(m.params, m.tasks, m.users, m.jobs, m.offers, m.groups, K=k)
    placed = ranked[:len(j2o)][j2o >= 0]
    assert 3 <= len(placed) < k and j2o[0] >= 0, "the cycle places some head jobs, not all it considers"
    skipped = np.zeros(m.offers.n, np.uint8)
    skipped[j2o[j2o >= 0][::2]] = 1  # the offers of every second match did not launch
    kept = ranked[:len(j2o)][(j2o >= 0) & (skipped[np.maximum(j2o, 0)] == 0)]
    assert 0 < len(kept) < len(placed)
    w_all, w_kept, w_none = (O.rebalance(O.derive(m, rp, matched_tasks=x)) for x in (placed, kept, ()))
    sel = lambda w: set(w["selected_task_idx"].tolist())
    assert not (sel(w_all) & set(placed.tolist())) and set(placed.tolist()) - set(kept.tolist()) <= sel(w_kept) and set(placed.tolist()) <= sel(w_none)
    with make_engine(m.params) as e:
        m.stage(e)
        e.rank_run()
        equal(e.cycle_rebalance(rp, skip_matched=True), w_none, "no placement since the rank: nothing is matched")
        e.cycle_run(k)
        got_ranked, got_j2o, _ = e.cycle_fetch()
        assert np.array_equal(got_ranked, ranked) and np.array_equal(got_j2o, j2o)
        equal(e.cycle_rebalance(rp, skip_matched=True), w_all, "skip_matched")
        equal(e.cycle_rebalance(rp, skip_matched=True, offer_skipped=skipped), w_kept, "skip_matched with offer_skipped")
        equal(e.cycle_rebalance(rp), w_none, "without the flag")
        e.cycle_run_rank(k)  # a placement that is set up and has not run
        assert _code(lambda: e.cycle_rebalance_stage(rp, skip_matched=True)) == COOK_E_STATE
        cycle_match_multi([e])
        equal(e.cycle_rebalance(rp, skip_matched=True), w_all, "skip_matched behind a deferred placement")


# ---- 6: sources ------------------------------------------------------------------------------------------------------------------------------
def check_sources(make_engine):
    b = P.make_rebalance_case(BASE_SEED, 500, 40, 15, 40, constraints=True, gpus=True, gpu_slots=2)
    m = embed(b, 6)
    gc = m.offers.gpu_count
    assert gc.ndim == 2 and gc.shape[1] == 2 and np.any((gc[:, 0] > 0) & (gc[:, 1] > 0)), "two gpu slots, both filled on some host"
    sp = O.spare_of_offers(m.offers)
    assert np.array_equal(sp.gpus, gc[:, 0] + gc[:, 1])
    want = O.rebalance(O.derive(m, b["rparams"]))
    assert len(want["decisions"]) >= 3
    with make_engine(m.params) as e:
        m.stage(e)
        e.cycle_run(0)
        equal(e.cycle_rebalance(b["rparams"]), want, "from the offers")
        equal(e.cycle_rebalance(b["rparams"], spare=sp, host_attrs=m.offers), want, "the same given explicitly")
        equal(e.cycle_rebalance(b["rparams"], spare=sp), want, "spare explicit, attributes from the offers")
        equal(e.cycle_rebalance(b["rparams"], host_attrs=m.offers), want, "attributes explicit, spare from the offers")
        # other lists than the offers': the case's own spare (its gpus column included) and attribute table
        want2 = O.rebalance(O.derive(m, b["rparams"], spare=b["spare"], host_attrs=b["host_attrs"]))
        equal(e.cycle_rebalance(b["rparams"], spare=b["spare"], host_attrs=b["host_attrs"]), want2, "the case's own lists")
    # two staged offers on one host
    dup = dataclasses.replace(m.offers, host=np.where(np.arange(m.offers.n) == 1, m.offers.host[0], m.offers.host).astype(np.uint32))
    m2 = dataclasses.replace(m, offers=dup)
    with make_engine(m.params) as e:
        m2.stage(e)
        e.cycle_run(0)
        assert _code(lambda: e.cycle_rebalance_stage(b["rparams"])) == COOK_E_INVALID
        assert _code(lambda: e.cycle_rebalance_stage(b["rparams"], spare=sp)) == COOK_E_INVALID
        assert _code(lambda: e.cycle_rebalance_stage(b["rparams"], host_attrs=m.offers)) == COOK_E_INVALID
        equal(e.cycle_rebalance(b["rparams"], spare=sp, host_attrs=m.offers), want, "host_dup with both lists given")


# ---- 7: the reference's cases ------------------------------------------------------------------------------------------------------------
def golden_cases():
    """the cases of tests/golden/rebalance.json that check_rebalance_golden runs, without those that need a hook: forced decisions, a
    State that already holds preempted hosts, a running task whose slave is not in the attribute cache"""
    out = []
    for case in G.load("rebalance"):
        if "forced" in case or case.get("init_preempted_hosts"):
            continue
        if any(t.get("slave_cached") is False for t in case["running"]):
            continue
        out.append(case)
    return out


def check_golden(make_engine):
    n = 0
    for case in golden_cases():
        b = G.build_rebalance_inputs(case)
        attrs = b["host_attrs"] if b["host_attrs"] is not None else A.Offers(cpus=np.zeros(0), mem=np.zeros(0))
        m = embed(b, n, offers=A.Offers(cpus=np.zeros(1), mem=np.zeros(1)))
        resident_parity(make_engine, m, b["rparams"], case["name"], spare=b["spare"], host_attrs=attrs)
        n += 1
    assert n >= 20, n


# ---- 8: refusals and untouched state -----------------------------------------------------------------------------------------------------
def _views(e, n_users):
    Q, j2o, head = e.cycle_fetch()
    return (Q, j2o, head, e.cycle_fetch_considerable(), e.match_metrics(n_users=n_users), e.user_stats(), e.unscheduled(), e.usage_breakdown())


def check_refusals(make_engine):
    pool = synth.make_pool(44, 60, 200, 5, 16)
    m = mirror_of_pool(pool)
    rp = A.CookRebalanceParams(0.0, 0.05, 20, 0)
    nohost = dataclasses.replace(m, tasks=dataclasses.replace(m.tasks, host=None))
    with make_engine(m.params) as e:
        assert _code(lambda: e.cycle_rebalance_stage(rp)) == COOK_E_STATE  # nothing staged
        assert _code(e.cycle_rebalance_fetch) == COOK_E_STATE
        nohost.stage(e)
        e.cycle_run(30)
        assert _code(lambda: e.cycle_rebalance_stage(rp)) == COOK_E_STATE  # a stage without host has no column
        m.stage(e)
        assert _code(lambda: e.cycle_rebalance_stage(rp)) == COOK_E_STATE  # before the rank
        e.cycle_run(30)
        before = _views(e, m.users.n)
        req_bad = [dict(skip_matched=2), dict(offer_skipped=np.zeros(m.offers.n, np.uint8))]
        for kw in req_bad:
            assert _code(lambda: e.cycle_rebalance_stage(rp, **kw)) == COOK_E_INVALID, kw
        req = A.CookCycleRebalance(rp, None, None, None, 0, 1)  # reserved is 0
        assert e._lib.cook_cycle_rebalance_stage(e._h, C.byref(req)) == COOK_E_INVALID
        assert _code(e.cycle_rebalance_fetch) == COOK_E_STATE  # no resident stage yet
        want = O.rebalance(O.derive(m, rp))
        e.cycle_rebalance_stage(rp)
        assert _code(e.cycle_rebalance_fetch) == COOK_E_STATE  # staged, not run
        e.rebalance_run()
        equal(e.cycle_rebalance_fetch(), want, "refusals")
        AS._same(_views(e, m.users.n), before)
        # a refused stage leaves the staged rebalance as it was
        assert _code(lambda: e.cycle_rebalance_stage(rp, skip_matched=2)) == COOK_E_INVALID
        equal(e.cycle_rebalance_fetch(), want, "behind a refused stage")
        # cook_rebalance_stage replaces the resident stage: the resident fetch then refuses
        b = P.make_rebalance_case(3, 50, 5, 3, 6)
        e.rebalance(b["running"], b["pending"], b["pending_job_id"], b["pending_priority"], b["users"], b["spare"], b["rparams"])
        assert _code(e.cycle_rebalance_fetch) == COOK_E_STATE
        # after a queue cycle the task table no longer lists what runs
        e.cycle_run_queue(30)
        assert _code(lambda: e.cycle_rebalance_stage(rp)) == COOK_E_STATE
        e.cycle_run(30)  # a rank cycle: allowed again
        equal(e.cycle_rebalance(rp), want, "a rank cycle behind queue cycles")


def check_untouched(make_engine):
    """an engine that rebalanced and one that did not: bit-identical cycle fetch, views, next queue cycle"""
    pool = synth.make_pool(45, 80, 300, 6, 24, gpus=True, constraints=True)
    m = mirror_of_pool(pool)
    rp = A.CookRebalanceParams(0.0, 0.05, 40, 0)
    st, el = AS.random_state(pool, 5)
    snaps = []
    for rebalances in (False, True):
        with make_engine(m.params) as e:
            m.stage(e)
            e.cycle_set_considerable(st, el)
            e.cycle_run(40)
            if rebalances:
                got = e.cycle_rebalance(rp, skip_matched=True)
                assert len(got["selected_task_idx"]) > 0
            a = _views(e, m.users.n)
            e.cycle_run_queue(40)
            snaps.append((a, _views(e, m.users.n), e.cycle_autoscale()))
    AS._same(snaps[0], snaps[1])


# ---- 9: the loop closes ----------------------------------------------------------------------------------------------------------------------
def check_loop(make_engine):
    b = P.make_rebalance_case(BASE_SEED, 500, 40, 15, 40, constraints=True, gpus=True)
    m = embed(b, BASE_SEED)
    want = O.rebalance(O.derive(m, b["rparams"]))
    pairs = {(int(want["selected_pending_ord"][d["pending_index"]]), int(d["host"])) for d in want["decisions"] if len(d["tasks"]) > 1}
    assert pairs, "reserve-hosts! keeps the decisions that preempt more than one task"
    with make_engine(m.params) as e:
        m.stage(e)
        e.cycle_run(0)
        got = e.cycle_rebalance(b["rparams"])
        pend, host = reservations_of(got["decisions"], pending_ord=got["selected_pending_ord"])
        e.cycle_set_reservations(A.Reservations(pend, host, release_matched=False))
        fp, fh = e.fetch_reservations()
        assert {(int(p), int(h)) for p, h in zip(fp, fh)} == pairs and len(fp) == len(pairs)
        e.cycle_run(10)  # the next rank cycle reads the map
    idx, _ = reservations_of(got["decisions"])  # the default: indices into the selected list
    assert np.array_equal(got["selected_pending_ord"][idx], pend)


# ---- 10: the ABI ---------------------------------------------------------------------------------------------------------------------------
def struct_layout_sources():
    fields = ["params", "spare", "host_attrs", "offer_skipped", "skip_matched", "reserved"]
    body = "".join(f'printf("%zu\\n", offsetof(cook_cycle_rebalance, {f}));' for f in fields)
    text = ('#include <stddef.h>\n#include <stdio.h>\n#include "cookmatch.h"\nint main(){printf("%zu\\n", sizeof(cook_cycle_rebalance));' + body +
            'printf("%d\\n", COOK_ABI_VERSION);return 0;}')
    want = [A.C.sizeof(A.CookCycleRebalance)] + [getattr(A.CookCycleRebalance, f).offset for f in fields] + [A.ABI_VERSION]
    return text, want
