"""The cases of the queue cycles (cook_cycle_run_queue*: match cycles on the standing ranked queue, without a re-rank), shared by the
emulator (test_queue_emu.py) and GPU (test_queue_gpu.py) suites.

The oracle is a composition of the frozen oracle.pyoracle calls: pyoracle.rank ONCE; then per cycle pyoracle.considerable over the
current queue with that cycle's user state, pyoracle.match of the considered jobs against that cycle's offers and the current groups
(the oracle side appends the kept matches' cotasks to the cook_groups CSR in Python), removal per remove_mode and offer_skipped
(remove-matched-jobs-from-pending-jobs, scheduler.clj:790-795, :1506-1508, :1792-1794).  Compared per cycle, element for element: the
queue, rank_pos, job_to_offer, head_matched, n_considered, and cook_cycle_autoscale's output after the queue cycles."""
from __future__ import annotations

import copy
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from cook_amd import _abi as A
from cook_amd import synth
from cook_amd.engine import CookError, cycle_match_multi, cycle_run_queue_multi, cycle_run_rank_multi
from oracle import pyoracle
from tests import autoscale_cases as AS

COOK_E_INVALID, COOK_E_STATE = -1, -4


# ---- the groups' running-cotask table as Python lists ------------------------------------------------------------------------------
def group_table(groups):
    if groups is None:
        return None
    G = len(groups.type)
    off, host, attr = groups._run_off, groups._run_host, groups._run_attr
    return SimpleNamespace(type=groups.type.copy(), attr_key=groups.attr_key.copy(), minimum=groups.minimum.copy(),
                           run_hosts=[[int(h) for h in host[off[g]:off[g + 1]]] for g in range(G)],
                           run_attrs=[[int(a) for a in attr[off[g]:off[g + 1]]] for g in range(G)])


def build_groups(t):
    if t is None:
        return None
    return A.Groups(type=t.type, attr_key=t.attr_key, minimum=t.minimum, run_hosts=[list(x) for x in t.run_hosts],
                    run_attrs=[list(x) for x in t.run_attrs])


def offer_attr(offers, o, key):
    """the offer's value of an attribute key as a group's run_attr holds it (0 = absent)"""
    if offers.attr is None or key == A.NONE_U32 or key >= offers.attr.shape[1]:
        return 0
    return int(offers.attr[o, key])


def mix_group_types(pool, seed):
    """synth's groups are all unique-placement: turn two thirds into balanced / attribute-equals groups over low-cardinality attributes"""
    t = group_table(pool.groups)
    rng = np.random.default_rng(seed)
    G = len(t.type)
    t.type = rng.choice([1, 2, 3], size=G).astype(np.uint8)
    t.attr_key = rng.integers(0, 3, G).astype(np.uint32)
    t.minimum = rng.integers(0, 3, G).astype(np.int32)
    t.run_attrs = [[offer_attr(pool.offers, h, int(t.attr_key[g])) for h in t.run_hosts[g]] for g in range(G)]
    pool.groups = build_groups(t)
    return pool


# ---- cycles ------------------------------------------------------------------------------------------------------------------------
def fresh_offers(seed, n_offers, **kw):
    return synth.make_pool(seed=seed, n_pending=0, n_running=0, n_users=1, n_offers=n_offers, **kw).offers


def make_cycles(pool, seed, k, n_cycles, n_offers, *, states=True, fractional=False, offer_kw=None, remove_modes=None, skip_frac=0.0):
    """cycle 0 is the rank cycle (the pool's own offers); every later one a queue cycle with fresh seeded offers and a refreshed user
    state.  offer_skipped of a step describes the offers of the cycle before it."""
    rng = np.random.default_rng(seed)
    cycles = []
    for c in range(n_cycles):
        st = el = None
        if states:
            st, el = AS.random_state(pool, seed + 10 * c, fractional=fractional)
        offers = pool.offers if c == 0 else fresh_offers(seed + 1000 + c, n_offers, **(offer_kw or {}))
        prev_m = cycles[-1].offers.n if c else 0
        sk = (rng.random(prev_m) < skip_frac).astype(np.uint8) if (c and skip_frac) else None
        cycles.append(SimpleNamespace(k=k, state=st, eligible=el, offers=offers, offer_skipped=sk,
                                      remove_mode=(remove_modes[c] if remove_modes else 0), groups=None))
    return cycles


def _queue_of(pool, Q, eligible):
    J = pool.pending_jobs
    jq = (np.cumsum(pool.tasks.pending) - 1)[Q]
    gp = J.gpus[jq] if J.gpus is not None else np.zeros(len(jq))
    return jq, A.Queue(cpus=J.cpus[jq], mem=J.mem[jq], gpus=gp, user=J.user[jq],
                       eligible=np.asarray(eligible, dtype=np.uint8)[jq] if eligible is not None else None)


def oracle(params, pool, cycles, *, fold=True, given_j2o=None, considerable=None, match=None):
    """-> per cycle SimpleNamespace(Q, pos, j2o, head, groups (the table the cycle's match saw), queue, kept).  fold=False: the kept
    matches' cotasks are NOT appended (what a queue cycle would place without the fold).  given_j2o[c]: the placement as given.
    considerable / match: other implementations of the two calls (the host path of the engine)."""
    considerable = considerable or pyoracle.considerable
    match = match or (lambda jobs, offers, groups: pyoracle.match(params, jobs, offers, groups))
    J = pool.pending_jobs
    Q, _ = pyoracle.rank(params, pool.tasks, pool.users)
    table = group_table(pool.groups)
    offers, last, out = pool.offers, None, []
    for c, cy in enumerate(cycles):
        if c:
            hit = last.j2o >= 0
            if cy.offer_skipped is not None:
                hit &= np.asarray(cy.offer_skipped, np.uint8)[np.maximum(last.j2o, 0)] == 0
            if cy.groups is not None:
                table = group_table(cy.groups)
            elif fold and table is not None and J.group is not None:
                table = copy.deepcopy(table)
                for i in np.flatnonzero(hit):
                    g = int(J.group[last.jq[last.pos[i]]])
                    if g != A.NONE_U32:
                        o = int(last.j2o[i])
                        table.run_hosts[g].append(int(offers.host[o]))
                        table.run_attrs[g].append(offer_attr(offers, o, int(table.attr_key[g])))
            keep = np.ones(len(Q), bool)
            keep[last.pos[np.ones(len(hit), bool) if cy.remove_mode else hit]] = False
            Q = Q[keep]
            if cy.offers is not None:
                offers = cy.offers
        jq, queue = _queue_of(pool, Q, cy.eligible if cy.state is not None else None)
        pos = considerable(queue, cy.state, cy.k)[0] if cy.state is not None else np.arange(min(cy.k, len(Q)), dtype=np.uint32)
        if given_j2o is not None:
            j2o, head = given_j2o[c], None
        else:
            j2o, _, head = match(J.take(jq[pos]), offers, build_groups(table))
        last = SimpleNamespace(Q=Q, jq=jq, pos=pos, j2o=j2o, head=head, table=table, queue=queue, offers=offers)
        out.append(last)
    return out


def autoscale_oracle(ocy, st, max_jobs=1000, scale_factor=1.0):
    """handle-resource-offers-autoscaling-helper over the cycle's queue: Q' = the current queue without this cycle's matches"""
    hit = ocy.j2o >= 0
    kk, m = len(ocy.pos), int(hit.sum())
    N, fraction = AS.scaled_n(kk, kk - m, max_jobs, scale_factor)
    keep = np.ones(len(ocy.Q), bool)
    keep[ocy.pos[hit]] = False
    qp = np.flatnonzero(keep)
    q = ocy.queue
    q2 = A.Queue(cpus=q.cpus[qp], mem=q.mem[qp], gpus=q.gpus[qp], user=q.user[qp])
    apos = pyoracle.considerable(q2, st, N)[0] if len(qp) else np.zeros(0, np.uint32)
    cand = ocy.Q[qp[apos]]
    return cand.astype(np.uint32), dict(considered=kk, matched=m, unmatched=kk - m, scaled=N, autoscalable=len(cand), n_out=len(cand),
                                        fraction_unmatched=fraction)


def assert_exercised(want, *, min_cycles=3):
    """on the oracle alone: at least three queue cycles each keep >= 1 match and leave >= 1 considered job unmatched"""
    good = sum(1 for w in want[1:] if (w.j2o >= 0).any() and (w.j2o < 0).any())
    assert good >= min_cycles, f"only {good} queue cycles keep a match and leave a considered job unmatched: re-seed the case"


def assert_fold_matters(params, pool, cycles, want):
    """on the oracle alone: with the cotask fold switched off at least one placement of a queue cycle differs"""
    off = oracle(params, pool, cycles, fold=False)
    assert any(not np.array_equal(a.j2o, b.j2o) or not np.array_equal(a.Q, b.Q) for a, b in zip(want[1:], off[1:])), \
        "the cotask fold changes no placement: re-seed the case"


# ---- engine side -------------------------------------------------------------------------------------------------------------------
def step_kw(cy):
    return dict(offer_skipped=cy.offer_skipped, remove_mode=cy.remove_mode, offers=cy.offers, groups=cy.groups)


def fetch(e, with_autoscale):
    Q, j2o, head = e.cycle_fetch()
    pos = e.cycle_fetch_considerable()
    return SimpleNamespace(Q=Q, j2o=j2o, head=head, pos=pos, autoscale=e.cycle_autoscale() if with_autoscale else None)


def run_engine(make_engine, params, pool, cycles, expect_form=None):
    """expect_form: how every cycle that considered a job must have been placed (cook_match_stats_ex [37]: 0 window rounds, 1 serial
    sweep, 3 class-ordered best fit) — the engine falls back to the window rounds silently where a call is not eligible for form 3"""
    got = []
    with make_engine(params) as e:
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        for c, cy in enumerate(cycles):
            if cy.state is not None:
                e.cycle_set_considerable(cy.state, cy.eligible)
            if c == 0:
                e.cycle_run(cy.k)
            else:
                e.cycle_run_queue(cy.k, **step_kw(cy))
            got.append(fetch(e, cy.state is not None))
            if expect_form is not None and len(got[-1].j2o):
                ms = e.match_stats()
                assert ms["placement_form"] == expect_form, (c, ms["placement_form"], hex(ms["classfit_refused"]))
    return got


def compare(got, want, cycles, tag=""):
    for c, (g, w, cy) in enumerate(zip(got, want, cycles)):
        where = f"{tag} cycle {c}"
        assert np.array_equal(g.Q, w.Q), (where, "queue", len(g.Q), len(w.Q))
        assert np.array_equal(g.pos, w.pos), (where, "rank_pos", len(g.pos), len(w.pos))
        assert len(g.j2o) == len(w.pos), (where, "n_considered")
        assert np.array_equal(g.j2o, w.j2o), (where, "job_to_offer", int((g.j2o != w.j2o).sum()))
        if w.head is not None:
            assert g.head == w.head, (where, "head_matched")
        if g.autoscale is not None:
            o_out, o_info = autoscale_oracle(w, cy.state)
            assert np.array_equal(g.autoscale[0], o_out), (where, "autoscale", len(g.autoscale[0]), len(o_out))
            assert g.autoscale[1] == o_info, (where, g.autoscale[1], o_info)


def check_cycles(make_engine, params, pool, cycles, *, group_case=False, oracle_match=True, host_path=False, table_variant=False,
                 expect_form=None):
    """the whole comparison of one case; the feature-exercise conditions are asserted on the oracle before the engine is called"""
    if oracle_match:
        want = oracle(params, pool, cycles)
        assert_exercised(want)
        if group_case:
            assert_fold_matters(params, pool, cycles, want)
        got = run_engine(make_engine, params, pool, cycles, expect_form)
    else:  # the placement of a large K takes minutes on one core: the engine's job_to_offer as given for the REMOVAL
        got = run_engine(make_engine, params, pool, cycles)
        want = oracle(params, pool, cycles, given_j2o=[g.j2o for g in got])
        assert_exercised(want)
    compare(got, want, cycles)
    if table_variant:  # the equivalent table passed in the step instead of the fold on the device
        cy2 = [copy.copy(cy) for cy in cycles]
        for c in range(1, len(cy2)):
            cy2[c].groups = build_groups(want[c].table)
        compare(run_engine(make_engine, params, pool, cy2), want, cycles, "groups passed:")
    if host_path:  # the same cycles through cook_considerable + cook_match, queue, jobs and groups rebuilt on the host each cycle
        with make_engine(params) as e2:
            host = oracle(params, pool, cycles, considerable=e2.considerable, match=lambda j, o, g: e2.match(j, o, g))
        compare(got, host, cycles, "host path:")
    return got, want


# ---- several pools through the multi form ------------------------------------------------------------------------------------------
def check_multi(make_engine, pools, params, cycles_of):
    want = [oracle(params, pl, cs) for pl, cs in zip(pools, cycles_of)]
    for w in want:
        if len(w[0].Q):
            assert_exercised(w)
    n_cycles = len(cycles_of[0])
    engines = [make_engine(params) for _ in pools]
    got = [[] for _ in pools]
    try:
        for e, pl in zip(engines, pools):
            e.cycle_stage(pl.tasks, pl.users, pl.pending_jobs, pl.offers, pl.groups)
        for c in range(n_cycles):
            for e, cs in zip(engines, cycles_of):
                if cs[c].state is not None:
                    e.cycle_set_considerable(cs[c].state, cs[c].eligible)
            ks = [cs[c].k for cs in cycles_of]
            if c == 0:
                cycle_run_rank_multi(engines, ks)
            elif c == 2:  # a mix of engines prepared by a rank call and by a queue call: the first pool ranks again
                engines[0].cycle_run_rank(ks[0])
                cycle_run_queue_multi(engines[1:], ks[1:], [step_kw(cs[c]) for cs in cycles_of[1:]])
            else:
                cycle_run_queue_multi(engines, ks, [step_kw(cs[c]) for cs in cycles_of])
            cycle_match_multi(engines)
            for i, (e, cs) in enumerate(zip(engines, cycles_of)):
                got[i].append(fetch(e, cs[c].state is not None))
    finally:
        for e in engines:
            e.close()
    for i, (pl, cs) in enumerate(zip(pools, cycles_of)):
        if i == 0 and n_cycles > 2:  # the pool that ranked again at cycle 2: a rank cycle on the staged data, then queue cycles again
            compare(got[0][:2], want[0][:2], cs[:2], "pool 0")
            again = copy.copy(pl)
            again.offers = cs[1].offers  # (the offers the last queue step staged stay)
            cs2 = [copy.copy(x) for x in cs[2:]]
            cs2[0].offers = again.offers
            compare(got[0][2:], oracle(params, again, cs2), cs2, "pool 0 after its second rank")
        else:
            compare(got[i], want[i], cs, f"pool {i}")
    return got


# ---- hand-derived edges --------------------------------------------------------------------------------------------------------------
def _tiny_pool(n_jobs, cpus, groups=None, group_of=None, offers=None, mem=None):
    """one user, n_jobs pending jobs of `cpus` each in submit order (priority 50, ascending job ids: the rank keeps the order)"""
    n = n_jobs
    cp = np.full(n, float(cpus)) if np.isscalar(cpus) else np.asarray(cpus, float)
    mm = np.full(n, 100.0) if mem is None else np.asarray(mem, float)
    tasks = A.Tasks(cpus=cp, mem=mm, user=np.zeros(n, np.uint32), priority=np.full(n, 50, np.int32),
                    start_ms=np.zeros(n, np.int64), task_id=(10_000 + np.arange(n)).astype(np.int64),
                    job_id=(100 + np.arange(n)).astype(np.int64), pending=np.ones(n, np.uint8))
    jobs = A.Jobs(cpus=cp.copy(), mem=mm.copy(), user=np.zeros(n, np.uint32),
                  group=np.asarray(group_of, np.uint32) if group_of is not None else None)
    users = A.Users(div_cpus=np.full(1, A.DMAX), div_mem=np.full(1, A.DMAX))
    return SimpleNamespace(tasks=tasks, users=users, pending_jobs=jobs, offers=offers, groups=groups)


def _offers(cpus, attr=None):
    m = len(cpus)
    return A.Offers(cpus=np.asarray(cpus, float), mem=np.full(m, 1000.0), host=np.arange(m, dtype=np.uint32),
                    attr=np.asarray(attr, np.uint32).reshape(m, -1) if attr is not None else None)


def _cy(k, offers, **kw):
    d = dict(k=k, state=None, eligible=None, offers=offers, offer_skipped=None, remove_mode=0, groups=None)
    d.update(kw)
    return SimpleNamespace(**d)


def check_edges(make_engine):
    params = A.default_params(good_enough_fitness=1.0)
    NONE = A.NONE_U32
    # -- unique: the group's second member is considered one cycle after the first was launched and must avoid that host.  Host 0 fits
    #    best in both cycles (the tighter host wins the bin-pack); without the fold job 1 would go to host 0 again.
    pool = _tiny_pool(3, 2.0, groups=A.Groups(type=np.array([1], np.uint8)), group_of=[0, 0, NONE], offers=_offers([2.0, 8.0]))
    cycles = [_cy(1, pool.offers), _cy(1, _offers([2.0, 8.0])), _cy(1, _offers([2.0, 8.0]))]
    got, want = check_cycles_small(make_engine, params, pool, cycles)
    assert [int(x.j2o[0]) for x in got] == [0, 1, 0] and [len(x.Q) for x in got] == [3, 2, 1]
    assert_fold_matters(params, pool, cycles, want)
    # -- balanced with a minimum: three members, attribute 0 takes the values 1, 1, 2 on hosts 0, 1, 2.  After the first launch on a
    #    host of value 1 the second must go to value 2 (minimum 2 distinct values not reached: the least frequent counts as 0).
    g = A.Groups(type=np.array([2], np.uint8), attr_key=np.array([0], np.uint32), minimum=np.array([2], np.int32))
    pool = _tiny_pool(3, 2.0, groups=g, group_of=[0, 0, 0], offers=_offers([2.0, 3.0, 8.0], attr=[1, 1, 2]))
    cycles = [_cy(1, pool.offers)] + [_cy(1, _offers([2.0, 3.0, 8.0], attr=[1, 1, 2])) for _ in range(2)]
    got, want = check_cycles_small(make_engine, params, pool, cycles)
    assert [int(x.j2o[0]) for x in got[:2]] == [0, 2]
    assert_fold_matters(params, pool, cycles, want)
    # -- attribute-equals pinned by the first launch: the first member lands on value 7 (host 0, the tightest); afterwards host 0 is
    #    too small and the tighter of the two others has value 9: the second member must take the value-7 host 2.
    g = A.Groups(type=np.array([3], np.uint8), attr_key=np.array([0], np.uint32))
    pool = _tiny_pool(2, 2.0, groups=g, group_of=[0, 0], offers=_offers([2.0, 3.0, 8.0], attr=[7, 9, 7]))
    cycles = [_cy(1, pool.offers), _cy(1, _offers([1.0, 3.0, 8.0], attr=[7, 9, 7]))]
    got, want = check_cycles_small(make_engine, params, pool, cycles)
    assert [int(x.j2o[0]) for x in got] == [0, 2]
    assert_fold_matters(params, pool, cycles, want)
    # -- offer_skipped keeps a matched job in the queue; remove_mode 1 removes every considered job, matched or not
    pool = _tiny_pool(4, [2.0, 50.0, 2.0, 2.0], offers=_offers([2.0, 2.0]))
    cycles = [_cy(2, pool.offers), _cy(2, _offers([2.0, 2.0]), offer_skipped=np.array([1, 0], np.uint8)),
              _cy(2, _offers([2.0, 2.0]), remove_mode=1), _cy(2, _offers([2.0, 2.0]))]
    got, want = check_cycles_small(make_engine, params, pool, cycles)
    assert [x.Q.tolist() for x in got] == [[0, 1, 2, 3], [0, 1, 2, 3], [2, 3], []]
    assert got[0].j2o.tolist() == [0, -1] and got[1].j2o.tolist() == [0, -1] and got[2].j2o.tolist() == [0, 1]


def check_cycles_small(make_engine, params, pool, cycles):
    want = oracle(params, pool, cycles)
    got = run_engine(make_engine, params, pool, cycles)
    compare(got, want, cycles)
    tab = [copy.copy(cy) for cy in cycles]  # ... and with the equivalent table passed
    if pool.groups is not None:
        for c in range(1, len(tab)):
            tab[c].groups = build_groups(want[c].table)
        compare(run_engine(make_engine, params, pool, tab), want, cycles, "groups passed:")
    return got, want


# ---- the five cases of test-remove-matched-jobs-from-pending-jobs, driven through the engine -----------------------------------------
def check_golden(make_engine):
    """tests/golden/queue_cycles.json: two pools ("normal" with the nine jobs 1-9, "gpu" with the five jobs 10-14); the matches are forced by offers that fit exactly
    the named jobs; afterwards each pool's queue is the reference's expected atom"""
    from tests import golden_util as G
    cases = G.load("queue_cycles")
    assert [c["name"] for c in cases] == ["empty", "unknown", "normal", "gpu", "both"]
    params = A.default_params(good_enough_fitness=1.0)
    for case in cases:
        for pname in ("normal", "gpu"):
            names = case["pending"][pname]
            matched = [nm for nm in case["matched"][pname] if nm in names]
            # job i asks for i + 1 cpus; one offer of exactly that size per matched job: best fit pairs them off; the jobs that are
            # not to match ask for more memory than any offer has
            cp = np.arange(1, len(names) + 1, dtype=float)
            offers = _offers([float(names.index(nm) + 1) for nm in matched] or [0.5])
            pool = _tiny_pool(len(names), cp, offers=offers, mem=[100.0 if nm in matched else 5000.0 for nm in names])
            cycles = [_cy(len(names), offers), _cy(len(names), _offers([0.5]))]
            got, _ = check_cycles_small(make_engine, params, pool, cycles)
            assert [names[t] for t in got[0].Q] == names
            assert [names[t] for t, o in zip(got[0].Q[got[0].pos], got[0].j2o) if o >= 0] == matched, (case["name"], pname)
            assert [names[t] for t in got[1].Q] == case["expect"][pname], (case["name"], pname)


# ---- the state rule and isolation ------------------------------------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(CookError) as ex:
        fn()
    return ex.value.code


def _snap(e, n_users):
    Q, j2o, head = e.cycle_fetch()
    return (Q, j2o, head, e.cycle_fetch_considerable(), e.match_metrics(n_users=n_users), e.match_explain(np.arange(min(len(j2o), 30))))


def check_state_rule(make_engine, pool, k=60):
    st, el = AS.random_state(pool, 5)
    offers2 = fresh_offers(4242, pool.offers.n, constraints=pool.offers.attr is not None)
    nu = pool.users.n
    with make_engine(A.default_params()) as e:
        assert _code(lambda: e.cycle_run_queue(k)) == COOK_E_STATE  # before anything
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        assert _code(lambda: e.cycle_run_queue(k)) == COOK_E_STATE  # staged, no cycle
        e.cycle_set_considerable(st, el)
        e.cycle_run_rank(k)
        assert _code(lambda: e.cycle_run_queue(k)) == COOK_E_STATE  # the placement has not run
        cycle_match_multi([e])
        e.cycle_run_queue(k, offers=offers2)
        e.cycle_set_considerable(st, el)  # refreshing the user state does not invalidate the queue
        e.cycle_run_queue(k, offers=offers2)
        # ---- a refused step changes nothing
        before = _snap(e, nu)
        bad_groups = A.Groups(type=np.zeros((len(pool.groups.type) if pool.groups is not None else 0) + 1, np.uint8))
        assert _code(lambda: e.cycle_run_queue(k, groups=bad_groups)) == COOK_E_INVALID
        assert _code(lambda: e.cycle_run_queue(k, remove_mode=2)) == COOK_E_INVALID
        assert _code(lambda: e.cycle_run_queue(k, offer_skipped=np.zeros(offers2.n + 1, np.uint8))) == COOK_E_INVALID
        if pool.groups is not None:
            t = group_table(pool.groups)
            t.type = (t.type + 1).astype(np.uint8) % 4
            assert _code(lambda: e.cycle_run_queue(k, groups=build_groups(t))) == COOK_E_INVALID
        AS._same(_snap(e, nu), before)
        e.cycle_run_queue(k, offers=offers2)
        after_refusals = _snap(e, nu)
        # ---- the last-rank views are the same before and after a queue cycle
        rows = np.flatnonzero(pool.tasks.pending)[:50]
        gor = (np.arange(pool.tasks.n) % 7).astype(np.uint32)
        last_rank = lambda: (e.user_stats(), e.unscheduled(rows=rows), e.usage_breakdown(), e.usage_breakdown(group_of_row=gor, n_groups=7))
        views = last_rank()
        e.cycle_run_queue(k, offers=offers2)
        AS._same(last_rank(), views)
        # ---- cook_match_run places the STAGED jobs: job_to_offer is no longer the last cycle's, so neither a queue cycle nor the
        #      autoscale pass may go on from it
        e.match_run()
        assert _code(lambda: e.cycle_run_queue(k)) == COOK_E_STATE
        assert _code(e.cycle_autoscale) == COOK_E_STATE
        e.cycle_run(k)
        e.cycle_run_queue(k, offers=offers2)
        # ---- what shifts or drops the rows the queue points at
        e.cycle_update(remove_task=[int(np.flatnonzero(pool.tasks.pending == 0)[0])])
        assert _code(lambda: e.cycle_run_queue(k)) == COOK_E_STATE
        e.cycle_run(k)
        e.cycle_run_queue(k, offers=offers2)
        from tests.parity_cases import make_considerable_case
        q, st2 = make_considerable_case(9, n=20, n_users=4)
        e.considerable(q, st2, 10)
        assert _code(lambda: e.cycle_run_queue(k)) == COOK_E_STATE
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        assert _code(lambda: e.cycle_run_queue(k)) == COOK_E_STATE
        # ---- a rank call after queue cycles gives exactly what it gives on a fresh engine with the same staged data
        e.cycle_set_considerable(st, el)
        e.cycle_run(k)
        e.cycle_run_queue(k, offers=offers2)
        e.cycle_run_queue(k, offers=pool.offers)
        e.cycle_run(k)
        again = _snap(e, nu)
    with make_engine(A.default_params()) as f:
        f.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        f.cycle_set_considerable(st, el)
        f.cycle_run(k)
        AS._same(_snap(f, nu), again)
        # the refusals above did not disturb the run they interrupted: the same three queue cycles without them
        f.cycle_run_queue(k, offers=offers2)
        f.cycle_run_queue(k, offers=offers2)
        f.cycle_run_queue(k, offers=offers2)
        AS._same(_snap(f, nu), after_refusals)


def struct_size_sources():
    return ('#include <stdio.h>\n#include "cookmatch.h"\nint main(){printf("%zu\\n", sizeof(cook_queue_step));return 0;}',
            [C.sizeof(A.CookQueueStep)])
