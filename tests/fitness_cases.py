"""Inputs and checks of cook_params.fitness (Fenzo's other fitness calculators), shared by the emulator build
(tests/test_fitness_emu.py) and the HIP build (tests/test_fitness_gpu.py, -m gpu).  The reference of every placement is
tests/fitness_oracle.py, which test_fitness_emu.py::test_oracle_gate_* hold to the frozen oracle at fitness 0."""
import functools

import numpy as np

from cook_amd import _abi as A
from cook_amd import synth
from cook_amd.engine import CookError, cycle_match_multi, cycle_run_queue_multi, cycle_run_rank_multi
from oracle import pyoracle
from tests import fitness_oracle as FO
from tests import parity_cases as P

ALGOS = (1, 2, 0, 3)       # serial sweep, window rounds, the engine's choice, class-ordered best fit (refuses every fitness but 0)
GOOD_ENOUGH = (1.0, 0.8)
# (jobs, offers) of the parity pools: the emulator's shapes are MV_WSEG 96 / MV_WEVAL 256 with lists of 64 / 32 entries, the shipped
# ones MV_WSEG 384 / MV_WEVAL 960 / MV_WLONG 10 240: several rounds, several segments per round, a 65th touched offer and a truncated
# list occur at these sizes
SIZES = {"emu": (600, 150), "gpu": (4000, 400)}


# ---- 1. known answer -------------------------------------------------------------------------------------------------------------------
def known_answer():
    """cf = (4 + 1) / 8 = 0.625 | (0 + 1) / 4 = 0.25; mf = 10 / 100 = 0.1 | (100 + 10) / 200 = 0.55"""
    jobs = A.Jobs(cpus=np.array([1.0]), mem=np.array([10.0]))
    offers = A.Offers(cpus=np.array([4.0, 4.0]), mem=np.array([100.0, 100.0]), run_cpus=np.array([4.0, 0.0]), run_mem=np.array([0.0, 100.0]))
    return jobs, offers, (1, 0, 1, 0, 1, 0)  # the offer that fitness 0..5 picks


def check_known_answer(make_engine):
    jobs, offers, want = known_answer()
    for f, w in enumerate(want):
        assert FO.match(A.default_params(fitness=f, good_enough_fitness=1.0), jobs, offers)[0][0] == w, f
        for algo in ALGOS:
            with make_engine(A.default_params(fitness=f, good_enough_fitness=1.0, match_algo=algo)) as e:
                j2o, fail, head = e.match(jobs, offers)
            assert j2o[0] == w and fail[0] == 0 and head, (f, algo, j2o)


# ---- 2. invalid values -----------------------------------------------------------------------------------------------------------------
def check_invalid(make_engine):
    for bad in (6, -1):
        try:
            make_engine(A.default_params(fitness=bad)).close()
        except CookError as ex:
            assert ex.code == -1 and "cook_params.fitness" in str(ex), ex
        else:
            raise AssertionError(f"cook_engine_create took fitness {bad}")
        with make_engine(A.default_params(fitness=2)) as e:
            try:
                e.set_params(A.default_params(fitness=bad))
            except CookError as ex:
                assert ex.code == -1 and "cook_params.fitness" in str(ex), ex
            else:
                raise AssertionError(f"cook_engine_set_params took fitness {bad}")
            # the engine kept the params it had: memoryBinPacker picks offer 1 of the known answer
            jobs, offers, want = known_answer()
            assert e.match(jobs, offers)[0][0] == want[2]


# ---- 4. parity pools -------------------------------------------------------------------------------------------------------------------
def _shrink(offers, jobs, fill):
    """the offers scaled so that the pool's free cpus are `fill` times what the jobs ask for: part of the queue stays unplaced"""
    s = fill * jobs.cpus.sum() / offers.cpus.sum()
    tot_c, tot_m = offers.cpus + offers.run_cpus, offers.mem + offers.run_mem
    oc, om = np.floor(offers.cpus * s), np.floor(offers.mem * s)
    return A.Offers(cpus=oc, mem=om, run_cpus=tot_c - oc, run_mem=tot_m - om)


@functools.lru_cache(maxsize=None)
def parity_pool(name, size):
    """-> (jobs, offers).  synth: the seeded pool of the benchmark's shapes, over-subscribed; empty: identical EMPTY offers (a spreader
    rotates over all of them, every tie goes to the lowest index, a round touches 64 offers within 64 jobs); frac: non-dyadic cpus
    (0.1, 0.5, 12 among them) and mem, offers off the integer grid; ports: see below"""
    K, M = SIZES[size]
    pool = synth.make_pool(seed={"synth": 101, "empty": 102, "frac": 103, "ports": 104}[name], n_pending=K, n_running=0, n_users=20, n_offers=M)
    jobs = A.Jobs(cpus=pool.pending_jobs.cpus, mem=pool.pending_jobs.mem)
    if name == "synth":
        return jobs, _shrink(pool.offers, jobs, 0.7)
    rng = np.random.default_rng(7)
    if name in ("empty", "ports"):
        per = np.ceil(0.7 * jobs.cpus.sum() / M)
        if name == "empty":
            return jobs, A.Offers(cpus=np.full(M, per), mem=np.full(M, per * 4096.0))
        # ... the same with ports and a named scalar asked for (Fenzo's other additive resources)
        jobs = A.Jobs(cpus=jobs.cpus, mem=jobs.mem, ports=rng.integers(0, 3, K).astype(np.int32),
                      scalars=np.where(rng.random(K) < 0.5, jobs.cpus, np.nan).reshape(K, 1))
        return jobs, A.Offers(cpus=np.full(M, per), mem=np.full(M, per * 4096.0), ports=np.full(M, 5, np.int32), scalars=np.full((M, 1), per - 2.0))
    cpus = rng.choice([0.1, 0.5, 12.0, 1.3, 2.7, 3.0], size=K, p=[.2, .2, .05, .2, .2, .15])
    jobs = A.Jobs(cpus=cpus, mem=jobs.mem + rng.integers(0, 10, K) / 10.0)
    o = _shrink(pool.offers, jobs, 0.7)
    return jobs, A.Offers(cpus=o.cpus + 0.3, mem=o.mem + 0.7, run_cpus=o.run_cpus + 0.1, run_mem=o.run_mem)


POOLS = ("synth", "empty", "frac")


@functools.lru_cache(maxsize=None)
def want_of(name, size, fitness, ge, constraint=None):
    """the oracle's placement, computed once per case and shared (read-only)"""
    jobs, offers, groups = case_inputs(name, size, constraint)
    out = FO.match(A.default_params(fitness=fitness, good_enough_fitness=ge), jobs, offers, groups)
    for a in out[:2]:
        a.setflags(write=False)
    return out


def case_inputs(name, size, constraint=None):
    if constraint is None:
        return parity_pool(name, size) + (None,)
    return constraint_case(constraint)


def assert_meaningful(name, size, fitness, ge, constraint=None):
    """on the oracle alone: the fitness moves the assignment, at least a quarter of the jobs are placed, at least one is not"""
    j2o = want_of(name, size, fitness, ge, constraint)[0]
    base = want_of(name, size, 0, ge, constraint)[0]
    assert not np.array_equal(j2o, base), "the assignment equals cpuMemBinPacker's"
    assert (j2o >= 0).sum() * 4 >= len(j2o), "fewer than a quarter of the jobs placed"
    assert (j2o < 0).any(), "every job placed"


def check_parity(make_engine, name, size, fitness, ge, algo, constraint=None, stats=None):
    assert_meaningful(name, size, fitness, ge, constraint)
    jobs, offers, groups = case_inputs(name, size, constraint)
    w_j2o, w_fail, w_head = want_of(name, size, fitness, ge, constraint)
    with make_engine(A.default_params(fitness=fitness, good_enough_fitness=ge, match_algo=algo)) as e:
        j2o, fail, head = e.match(jobs, offers, groups)
        st = e.match_stats()
    bad = np.nonzero(j2o != w_j2o)[0]
    assert len(bad) == 0, f"assignment differs first at job {bad[:5]}: {j2o[bad[:5]]} vs {w_j2o[bad[:5]]}"
    assert np.array_equal(fail, w_fail) and head == w_head
    # how it was placed: the spreaders by the sweep whatever match_algo says, the packers as asked; class-ordered best fit refuses both
    assert st["placement_form"] == (1 if (algo == 1 or fitness >= 3) else 0), st["placement_form"]
    if algo == 3:
        assert st["classfit_refused"] == 0x20000, hex(st["classfit_refused"])
    assert st["spreader_serial_calls"] == (1 if (fitness >= 3 and algo != 1) else 0)
    if stats is not None:
        stats.append(st)
    return st


def check_rounds_end_every_way(make_engine, size):
    """the packers' window rounds at these sizes: several rounds, more segments than rounds, rounds ended by an exhausted list and by the
    window's end, truncated lists.  (On these pools a packer returns to the offers it has touched and a job's list runs out before a
    65th offer is touched: that end of a round is check_touched_set_full's.)"""
    tot = {}
    for name, fitness in (("synth", 1), ("ports", 2)):
        st = check_parity(make_engine, name, size, fitness, 1.0, 2)
        for k in ("rounds", "segments", "stop_list", "stop_full", "stop_window", "trunc_lists"):
            tot[k] = tot.get(k, 0) + st[k]
    print(tot)
    assert tot["rounds"] > 6 and tot["segments"] > tot["rounds"], tot
    assert tot["stop_list"] and tot["stop_window"] and tot["trunc_lists"], tot


@functools.lru_cache(maxsize=None)
def pinned_case():
    """every job pinned to one host by an EQUALS attribute (the case of tests/test_parity_emu.py's touched-set test): each placement touches
    an offer of its own, so a round ends when its 64 lanes are taken.  -> (jobs, offers)"""
    return P.pinned_jobs_case(8, 300, 400, 0)


def check_touched_set_full(make_engine, fitness):
    """a packer's window rounds ended by the touched set (the 65th touch): parity, and the round end itself.  The pins leave a job one
    host, so the calculator decides nothing here but whether the host's fitness is > 0 — the case is about the round end under the
    one-resource terms, not about the assignment (check_parity's pools are about that)."""
    jobs, offers = pinned_case()
    p = A.default_params(fitness=fitness, good_enough_fitness=1.0, match_algo=2)
    w_j2o, w_fail, w_head = FO.match(p, jobs, offers)
    assert (w_j2o >= 0).sum() > 64 and len(np.unique(w_j2o[w_j2o >= 0])) > 64  # more hosts to touch than the walk has lanes
    with make_engine(p) as e:
        j2o, fail, head = e.match(jobs, offers)
        st = e.match_stats()
    assert np.array_equal(j2o, w_j2o) and np.array_equal(fail, w_fail) and head == w_head
    assert st["placement_form"] == 0 and st["stop_full"] > 0, st


# ---- cook_match_explain under a spreader ---------------------------------------------------------------------------------------------------
def check_explain_spreader(make_engine):
    """cpuSpreader (1.0 - cf), offers {cpus 4} and {cpus 2}, both with mem to spare:
      job 0 {cpus 4}: offer 0 would be filled to the brim, cf = 4 / 4, fitness 0.0 — not > 0.0; offer 1 is short of cpus.  Unplaced.
      job 1 {cpus 1}: 1 - 1/4 = 0.75 on offer 0, 1 - 1/2 = 0.5 on offer 1.  Offer 0.
      job 2 {cpus 3}: offer 0 holds job 1: cf = (1 + 3) / 4, fitness 0.0 again; offer 1 is short of cpus.  Unplaced.
    So jobs 0 and 2 each have one host under "cpus" and one under "fitness" — under cpuMemBinPacker job 0 would simply be placed."""
    jobs = A.Jobs(cpus=np.array([4.0, 1.0, 3.0]), mem=np.array([10.0, 10.0, 10.0]))
    offers = A.Offers(cpus=np.array([4.0, 2.0]), mem=np.array([100.0, 100.0]))
    want = np.zeros((2, A.WHY_SLOTS), np.uint32)
    want[:, 0] = 1  # cpus
    want[:, 2] = 1  # fitness
    for algo in ALGOS:
        with make_engine(A.default_params(fitness=4, good_enough_fitness=1.0, match_algo=algo)) as e:
            j2o, fail, _ = e.match(jobs, offers)
            assert list(j2o) == [-1, 0, -1] and list(fail) == [5, 0, 5], (algo, j2o, fail)
            assert np.array_equal(e.match_explain([0, 2]), want), algo
            assert A.why_summary(e.match_explain([2])[0]) == {":resources": {"cpus": 1, "fitness": 1}}
        with make_engine(A.default_params(fitness=0, good_enough_fitness=1.0, match_algo=algo)) as e:
            assert e.match(jobs, offers)[0][0] == 0


# ---- 5. constraints under another fitness (emulator size) ---------------------------------------------------------------------------------
CONSTRAINTS = ("max_tasks", "equals", "unique", "balanced")


@functools.lru_cache(maxsize=None)
def constraint_case(kind):
    jobs, offers = parity_pool("synth", "emu")
    K, M = jobs.n, offers.n
    rng = np.random.default_rng(11)
    okw = dict(cpus=offers.cpus, mem=offers.mem, run_cpus=offers.run_cpus, run_mem=offers.run_mem)
    if kind == "max_tasks":
        return jobs, A.Offers(max_tasks=rng.integers(1, 5, M).astype(np.int32), num_tasks=rng.integers(0, 2, M).astype(np.int32), **okw), None
    attr = np.stack([rng.integers(1, 4, M), rng.integers(1, 5, M)], axis=1).astype(np.uint32)
    if kind == "equals":
        eq = [[(0, int(rng.integers(1, 4)))] if rng.random() < 0.4 else [] for _ in range(K)]
        return A.Jobs.with_constraints(jobs.cpus, jobs.mem, equals=eq), A.Offers(attr=attr, **okw), None
    grp = np.full(K, A.NONE_U32, np.uint32)
    if kind == "unique":
        members = rng.permutation(K)[:120]
        for g in range(12):
            grp[members[g * 10:(g + 1) * 10]] = g
        groups = A.Groups(type=np.ones(12, np.uint8), run_hosts=[[int(h) for h in rng.integers(0, M, int(rng.integers(0, 3)))] for _ in range(12)])
        return A.Jobs(cpus=jobs.cpus, mem=jobs.mem, group=grp), A.Offers(**okw), groups
    members = rng.permutation(K)[:48]
    for g in range(4):
        grp[members[g * 12:(g + 1) * 12]] = g
    run_hosts = [[int(h) for h in rng.integers(0, M, 2)] for _ in range(4)]
    groups = A.Groups(type=np.full(4, 2, np.uint8), attr_key=np.ones(4, np.uint32), minimum=np.full(4, 2, np.int32), run_hosts=run_hosts,
                      run_attrs=[[int(attr[h, 1]) for h in hs] for hs in run_hosts])
    return A.Jobs(cpus=jobs.cpus, mem=jobs.mem, group=grp), A.Offers(attr=attr, **okw), groups


# ---- 6. mixed pools ----------------------------------------------------------------------------------------------------------------------
MIXED = (0, 1, 3, 5)


def check_mixed_pools(make_engine, size):
    """four engines of fitness 0, 1, 3, 5 through the multi-pool calls — a rank cycle, then a queue cycle — each against a run of its own
    through the single-pool calls; the fitness-0 engine also against the frozen oracle"""
    K, M = SIZES[size]
    pools = [synth.make_pool(seed=201 + i, n_pending=K // 2, n_running=K // 8, n_users=15, n_offers=M // 4) for i in range(len(MIXED))]
    for pl in pools:
        pl.offers = _shrink(pl.offers, pl.pending_jobs, 0.7)
    ks = [K // 5] * len(MIXED)
    params = [A.default_params(fitness=f, good_enough_fitness=1.0) for f in MIXED]
    own = []
    for p, pl, k in zip(params, pools, ks):
        with make_engine(p) as e:
            e.cycle_stage(pl.tasks, pl.users, pl.pending_jobs, pl.offers)
            e.cycle_run(k)
            first = e.cycle_fetch()
            e.cycle_run_queue(k)
            own.append((first, e.cycle_fetch()))
    engines = [make_engine(p) for p in params]
    try:
        for e, pl in zip(engines, pools):
            e.cycle_stage(pl.tasks, pl.users, pl.pending_jobs, pl.offers)
        cycle_run_rank_multi(engines, ks)
        cycle_match_multi(engines)
        got1 = [e.cycle_fetch() for e in engines]
        cycle_run_queue_multi(engines, ks)
        cycle_match_multi(engines)
        got2 = [e.cycle_fetch() for e in engines]
    finally:
        for e in engines:
            e.close()
    for i, f in enumerate(MIXED):
        for got, want in ((got1[i], own[i][0]), (got2[i], own[i][1])):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], f"fitness {f}"
    for i in range(1, len(MIXED)):  # the engines did not all compute the same thing
        assert not np.array_equal(got1[i][1], FO.match(params[0], _considerable(pools[i], got1[i][0], ks[i]), pools[i].offers)[0]), MIXED[i]
    # fitness 0 against the frozen oracle: the rank cycle, and the queue cycle on what it left (kept matches leave the queue, the offers stay)
    pl, p = pools[0], params[0]
    o_ranked, _ = pyoracle.rank(p, pl.tasks, pl.users)
    o_j2o, _, o_head = pyoracle.match(p, _considerable(pl, o_ranked, ks[0]), pl.offers)
    assert np.array_equal(got1[0][0], o_ranked) and np.array_equal(got1[0][1], o_j2o) and got1[0][2] == o_head
    keep = np.ones(len(o_ranked), bool)
    keep[:len(o_j2o)] = o_j2o < 0
    q2 = o_ranked[keep]
    o_j2o2, _, o_head2 = pyoracle.match(p, _considerable(pl, q2, ks[0]), pl.offers)
    assert np.array_equal(got2[0][0], q2) and np.array_equal(got2[0][1], o_j2o2) and got2[0][2] == o_head2
    # ... and the others against the parametrised oracle
    for i in range(1, len(MIXED)):
        w = FO.match(params[i], _considerable(pools[i], got1[i][0], ks[i]), pools[i].offers)
        assert np.array_equal(got1[i][1], w[0]) and got1[i][2] == w[2], MIXED[i]


def _considerable(pool, ranked, k):
    pend_ord = np.cumsum(pool.tasks.pending) - 1
    j = pool.pending_jobs.take(pend_ord[ranked[:k]])
    return A.Jobs(cpus=j.cpus, mem=j.mem)
