"""Cases for the decider's RUN of plain steps in the class-ordered walk (classfit_asm.hpp, CF_ASM_DECIDER_RUN), shared by the emulated and the GPU
test files.  Not a test module.

On the GPU the decider takes the plain steps of a batch one behind the other inside one hand-placed loop: the walk's state (the jobs not decided
yet, the walked ordinal, the board's row, the log address, the minima) stays in registers from step to step, and so do the attribute bytes of the
offer an overlay lane holds — loaded at the head of a run and where a lane opens.  A step that is not plain (a gpu kind, novel hosts, a group, a
missing answer, two candidates inside the guard band, the placement that fills the overlay) leaves the loop; the C++ step takes it and the loop is
entered again.  The emulated build has the C++ step only: there the cases show that they ARE the cases they mean to be (form 3, the oracle's
placements, the events counted); on the GPU the same assertions hold for the loop.

What each case aims at:
  long_run               64 walked plain jobs in one batch, all placed: the row offset wraps five times on the 12-row board, batch slots 0 and 63
                         are walked and placed (the `-2 << slot` mask at 63), overlay wins and class wins alternate; K = 3 * 64 + 1, so the last
                         batch is one job.
  reentry_phases         13 batches; in batch r the one job that is not plain — a gpu kind, novel hosts, a group in turn — is the walked job of
                         ordinal r (r = 0 .. 12): the loop leaves and is entered again at every row of the board, and once exactly at the wrap.
                         (13 batches are 12 * 64 + 20 jobs; 44 jobs of every batch ask for more mem than any host has and are not walked.)
  equals_fresh_lane      an EQUALS job directly behind the placement that opens an overlay lane; the new lane is the best fit and its offer's
                         attribute byte decides.  Offer 0 — whose bytes a lane that never opened would hold — carries the opposite value.
  equals_reopened_lane   a lane opens on offer A and dies two steps later (or: A dies at once and nothing opens), the lane opens again on offer B
                         whose byte differs from A's, and the EQUALS job behind it is decided by B's byte: stale bytes give a wrong offer.
  nobody_in_run          EQUALS jobs whose value no offer has: the tables promise room, they are walked, nobody takes them; they stand between
                         placed jobs, first and last of a batch included.
  epoch_in_run           every job opens a lane of its own until the overlay is full (58 live lanes in the shipped shape, 8 in the emulated one);
                         the placement that ends the epoch is the C++ step's, plain steps follow in the same batch.
  tie_in_run             two offers of one class with equal free values are the best fit of a job in the middle of a batch: an exact turn, plain
                         steps on both sides; the lower offer wins.

Resources are integers on the eight cpus levels and dyadic mem; free mem is distinct from offer to offer (no ties but the one tie_in_run builds), so
every case is placed by the class-ordered form (placement_form 3) and the best fit of every job is unique.
"""
import numpy as np

from cook_amd import _abi as A
from oracle import pyoracle

BIG_MEM = 1048576.0  # more than any offer holds: such a job is not walked


def _offers(n, tot_c=64.0, free_c=8.0, mem0=10240.0, step=16.0, attr0=None, gpu_at=(), seed=0):
    """n offers of one class (two with gpu hosts): free cpus `free_c`, free mem distinct (mem0 + step * a permutation), optional attribute byte 0"""
    rng = np.random.default_rng(1000 + seed)
    tot_c = np.full(n, tot_c)
    tot_m = tot_c * 4096.0
    fc = np.full(n, free_c)
    fm = mem0 + step * rng.permutation(n).astype(np.float64)
    kw = {}
    if attr0 is not None:
        a = np.zeros((n, 8), dtype=np.uint32)
        a[:, 0] = attr0
        a[:, 7] = 1 + np.arange(n) % 200
        kw["attr"] = a
    run_n = np.maximum(1, np.rint((tot_c - fc) / 3.0)).astype(np.int32)
    if len(gpu_at):
        gm, gc = np.zeros(n, dtype=np.uint32), np.zeros(n)
        gm[list(gpu_at)], gc[list(gpu_at)] = 1, 4.0
        run_n[list(gpu_at)] = 0
        kw.update(gpu_model=gm, gpu_count=gc)
    return dict(cpus=fc, mem=fm, host=np.arange(n, dtype=np.uint32), k8s=np.ones(n, dtype=np.uint8), run_cpus=tot_c - fc, run_mem=tot_m - fm, run_count=run_n, **kw)


def _jobs(cpus, mem, equals=None, gpus=None, novel=None, group=None):
    cpus, mem = np.asarray(cpus, dtype=np.float64), np.asarray(mem, dtype=np.float64)
    kw = {}
    if equals is not None and any(len(x) for x in equals):
        kw["equals"] = equals
    if novel is not None and any(len(x) for x in novel):
        kw["novel"] = novel
    if gpus is not None and (np.asarray(gpus) > 0).any():
        g = np.asarray(gpus, dtype=np.float64)
        kw.update(gpus=g, gpu_model=(g > 0).astype(np.uint32))
    if group is not None:
        kw["group"] = group
    return A.Jobs.with_constraints(cpus, mem, **kw) if kw else A.Jobs(cpus=cpus, mem=mem)


def case_long_run():
    rng = np.random.default_rng(51)
    k = 3 * 64 + 1
    cpus = rng.integers(1, 5, k).astype(np.float64)  # an offer of 8 takes two to eight of them: its first job opens a lane, the next ones win on it
    mem = 512.0 * rng.integers(1, 4, k)
    cpus[5], cpus[-1] = 8.0, 1.0  # (the levels span 1..8; a whole offer: dead at once, nothing opens)
    return dict(jobs=_jobs(cpus, mem), offers=A.Offers(**_offers(160, seed=1)), groups=None)


N_PH = 13     # batches of reentry_phases
PH_WALK = 20  # walked jobs at the head of each


def case_reentry_phases():
    rng = np.random.default_rng(52)
    k = (N_PH - 1) * 64 + PH_WALK
    n = 220
    gpu_at = np.arange(3, n, 11)
    cpus = rng.integers(1, 4, k).astype(np.float64)
    mem = 512.0 * rng.integers(1, 4, k)
    gpus = np.zeros(k)
    novel = [[] for _ in range(k)]
    group = np.full(k, A.NONE_U32, dtype=np.uint32)
    special = []
    for r in range(N_PH):
        b = 64 * r
        mem[b + PH_WALK:b + 64] = BIG_MEM
        cpus[b + PH_WALK:b + 64] = 2.0
        q = b + r
        special.append(q)
        if r % 3 == 0:
            gpus[q], cpus[q], mem[q] = 4.0, 2.0, 1024.0
        elif r % 3 == 1:
            pass  # novel hosts, filled below: the host the job would get without the constraint
        else:
            group[q] = r // 3
            group[q + 1 if r + 1 < PH_WALK else q - 1] = r // 3  # (a second member: the group's placements must not share a host)
    cpus[0 + 15], cpus[64 + 15] = 8.0, 1.0
    o = _offers(n, gpu_at=gpu_at, seed=2)
    groups = A.Groups(type=np.ones(5, dtype=np.uint8), run_hosts=[[7], [], [30, 31], [], []])
    p3 = A.default_params(good_enough_fitness=1.0, match_algo=3)
    for r, q in enumerate(special):  # a novel-host job has run before on the host it would get otherwise, and on one without an offer: the constraint moves it
        if r % 3 == 1:
            base = pyoracle.match(p3, _jobs(cpus, mem, gpus=gpus, novel=novel, group=group), A.Offers(**o), groups, ())[0]
            novel[q] = [int(o["host"][base[q]]), 100000 + q] if base[q] >= 0 else [100000 + q]
    return dict(jobs=_jobs(cpus, mem, gpus=gpus, novel=novel, group=group), offers=A.Offers(**o), groups=groups, special=np.array(special), novel=novel)


EQ_V, EQ_W = 5, 9  # the value the EQUALS jobs ask for under key 0, and the other one


def _lane_case(reopen, take, dies_at_once=False):
    """one batch: two plain jobs that fill the least-mem offer, then four times the pattern.  A small job's best fit among untouched offers is the one
    with the least free mem, and an offer with a job on it beats every untouched one: so the patterns take the offers in the order of their free mem.
    fresh:    [opener 2 cpus -> X, a lane opens] [EQUALS 2 cpus: X's lane is the best fit]
    reopened: [2 cpus -> A, a lane opens] [2 cpus -> A] [4 cpus -> A: nothing is left, the lane dies] [opener -> B: the lane opens again] [EQUALS]
              dies_at_once: [8 cpus -> A: nothing opens] instead of the first three.
    The EQUALS job asks for (0, EQ_V).  take: X / B carries EQ_V and the job must go there; else X / B carries EQ_W and it must go to Y, the next
    untouched offer.  A, and offer 0 (the bytes a lane that never opened would hold), carry the opposite of X / B; every other offer EQ_V.
    Behind the EQUALS job the offers with a lane are filled up (jobs of 4, or of 6 and 6): the overlay is empty before the next pattern."""
    n = 120
    o = _offers(n, attr0=np.full(n, EQ_V), step=64.0, seed=3)
    order = [int(x) for x in np.argsort(o["mem"]) if x != 0]  # (offer 0 holds the most free mem of all: no job of the case gets that far)
    o["mem"][0] = 10240.0 + 64.0 * n
    o["run_mem"][0] = 64.0 * 4096.0 - o["mem"][0]
    cpus, equals, expect = [4.0, 4.0], [[], []], []
    used = 1
    hot, cold = (EQ_V, EQ_W) if take else (EQ_W, EQ_V)
    attr0 = o["attr"][:, 0]
    attr0[0] = cold

    def add(c, eq=None):
        cpus.append(c), equals.append([eq] if eq else [])
        return len(cpus) - 1
    for _ in range(4):
        if reopen:
            attr0[order[used]] = cold
            used += 1
            if dies_at_once:
                add(8.0)
            else:
                add(2.0), add(2.0), add(4.0)
        x = order[used]
        used += 1
        attr0[x] = hot
        add(2.0)
        q = add(2.0, (0, EQ_V))
        if take:
            add(4.0)
            expect.append((q, x, x))
        else:
            y = order[used]
            used += 1
            add(6.0), add(6.0)
            expect.append((q, x, y))
    add(8.0), add(1.0)
    return dict(jobs=_jobs(cpus, np.full(len(cpus), 256.0), equals=equals), offers=A.Offers(**o), groups=None, expect=expect, take=take)


def case_nobody_in_run():
    rng = np.random.default_rng(55)
    k = 150
    cpus = rng.integers(1, 5, k).astype(np.float64)
    mem = 512.0 * rng.integers(1, 4, k)
    cpus[7], cpus[-1] = 8.0, 1.0
    equals = [[] for _ in range(k)]
    nobody = [0, 9, 10, 30, 63, 64, 100, 127, 128, 149]
    for q in nobody:
        equals[q] = [(0, 3)] if q % 2 == 0 else [(0, 1), (7, 250)]  # no offer has 3 under key 0; none has 250 under key 7
    for q in (20, 40, 90):
        equals[q] = [(0, 1 + q % 2)]  # (EQUALS jobs that are placed, among them)
    n = 140
    o = _offers(n, attr0=1 + np.arange(n) % 2, seed=5)
    return dict(jobs=_jobs(cpus, mem, equals=equals), offers=A.Offers(**o), groups=None, nobody=np.array(nobody))


N_EPOCH_OPEN = 60  # more than CF_EPOCH_AT of the shipped build (58) and of the emulated one (8)


def case_epoch_in_run():
    k = 100
    cpus = np.full(k, 5.0)  # an offer of 8 takes one of them and stays alive (3 cpus: the smallest job asks for 1): every job opens a lane
    mem = np.full(k, 1024.0)
    cpus[N_EPOCH_OPEN:64] = 1.0  # plain steps behind the epoch's end, in the same batch: onto what the openers left
    cpus[64:80] = 5.0
    cpus[80:] = 2.0
    return dict(jobs=_jobs(cpus, mem), offers=A.Offers(**_offers(200, seed=6)), groups=None)


def case_tie_in_run():
    rng = np.random.default_rng(57)
    k = 100
    cpus = rng.integers(1, 5, k).astype(np.float64)
    mem = 512.0 * rng.integers(1, 4, k)
    cpus[3], cpus[-1] = 8.0, 1.0
    n = 140
    o = _offers(n, seed=7)  # free mem 10240 .. 10240 + 16 * 139 = 12464
    pair = []
    for q, (a, b), m in ((30, (41, 77), 16384.0), (70, (12, 90), 20480.0)):
        o["mem"][[a, b]] = m  # the only two offers that hold m: the job that asks for it finds them equal
        o["run_mem"][[a, b]] = 64.0 * 4096.0 - m
        cpus[q], mem[q] = 2.0, m
        pair.append((q, a))
    return dict(jobs=_jobs(cpus, mem), offers=A.Offers(**o), groups=None, pair=pair)


CASES = {
    "long_run": case_long_run,
    "reentry_phases": case_reentry_phases,
    "equals_fresh_lane_take": lambda: _lane_case(False, True),
    "equals_fresh_lane_leave": lambda: _lane_case(False, False),
    "equals_reopened_lane_take": lambda: _lane_case(True, True),
    "equals_reopened_lane_leave": lambda: _lane_case(True, False),
    "equals_reopened_at_once_take": lambda: _lane_case(True, True, dies_at_once=True),
    "equals_reopened_at_once_leave": lambda: _lane_case(True, False, dies_at_once=True),
    "nobody_in_run": case_nobody_in_run,
    "epoch_in_run": case_epoch_in_run,
    "tie_in_run": case_tie_in_run,
}

_oracle = {}


def oracle_of(name, c, p3):
    """the oracle's answer of a case, computed once and shared (read-only) by the emulated and the GPU tests of a session"""
    if name not in _oracle:
        o = pyoracle.match(p3, c["jobs"], c["offers"], c["groups"], ())
        o[0].flags.writeable = False
        o[1].flags.writeable = False
        _oracle[name] = o
    return _oracle[name]


def check_case(make_engine, name):
    """the case under match_algo 3 and match_algo 2 against the oracle, bit for bit; then what makes it the case it is meant to be"""
    c = CASES[name]()
    jobs, offers, groups = c["jobs"], c["offers"], c["groups"]
    p3 = A.default_params(good_enough_fitness=1.0, match_algo=3)
    p2 = A.default_params(good_enough_fitness=1.0, match_algo=2)
    with make_engine(p3) as e:
        j3, f3, h3 = e.match(jobs, offers, groups, ())
        j3, f3, st3 = j3.copy(), f3.copy(), e.match_stats()
    with make_engine(p2) as e:
        j2, f2, h2 = e.match(jobs, offers, groups, ())
        j2, f2 = j2.copy(), f2.copy()
    o = oracle_of(name, c, p3)
    k = len(j3)
    print(name, "K", k, "M", len(offers.cpus), {x: st3.get(x) for x in ("placement_form", "classfit_refused", "cf_walked", "cf_matched", "cf_epochs", "cf_exact_turns", "cf_batches")})
    assert st3["placement_form"] == 3 and st3["classfit_refused"] == 0, (name, st3["placement_form"], hex(st3["classfit_refused"]))
    bad = np.nonzero((j3 != o[0]) | (j3 != j2))[0]
    assert len(bad) == 0, (name, "job_to_offer", bad[:8], j3[bad[:8]], o[0][bad[:8]], j2[bad[:8]])
    badf = np.nonzero((f3 != o[1]) | (f3 != f2))[0]
    assert len(badf) == 0, (name, "fail_code", badf[:8], f3[badf[:8]], o[1][badf[:8]], f2[badf[:8]])
    assert h3 == o[2] == h2, (name, "head_matched", h3, o[2], h2)
    placed = j3 >= 0
    if name == "long_run":
        assert k == 193 and placed.all() and st3["cf_walked"] == k and st3["cf_batches"] == 4 and st3["cf_exact_turns"] == 0, st3
        first = np.array([q == 0 or j3[q] not in j3[:q] for q in range(64)])  # the first job on an offer comes from its class, the next ones win on its lane
        assert 10 <= first.sum() <= 40 and (~first).sum() >= 20, (first.sum(), "overlay wins and class wins are mixed in batch 0")
        assert np.unique(np.nonzero(np.diff(first.astype(int)))[0] // 12).size >= 5, "both kinds of step on every pass over the board's rows"
    elif name == "reentry_phases":
        sp = c["special"]
        walked = np.concatenate([np.arange(64 * r, 64 * r + PH_WALK) for r in range(N_PH)])
        assert k == (N_PH - 1) * 64 + PH_WALK and st3["cf_batches"] == N_PH and st3["cf_walked"] == len(walked), st3
        assert placed[walked].all() and not placed[np.setdiff1d(np.arange(k), walked)].any()
        assert list(sp - 64 * np.arange(N_PH)) == list(range(N_PH)), "in batch r the job that is not plain is the walked job of ordinal r"
        assert (offers.gpu_count[j3[sp[0::3]]] > 0).all(), "the gpu jobs sit on gpu hosts"
        assert (offers.gpu_count[j3[np.setdiff1d(walked, sp[0::3])]] == 0).all()
        for q in sp[1::3]:
            assert len(c["novel"][q]) == 2 and offers.host[j3[q]] not in c["novel"][q], (q, j3[q], c["novel"][q], "the constraint moves the job")
        for q in sp[2::3]:
            q2 = q + 1 if (q % 64) + 1 < PH_WALK else q - 1
            assert j3[q] != j3[q2], "the group's members do not share a host"
    elif name.startswith("equals_"):
        for q, x, to in c["expect"]:
            assert j3[q - 1] == x, (name, q, j3[q - 1], x, "the opener in front of the EQUALS job takes the offer the pattern means")
            assert j3[q] == to, (name, q, j3[q], to, "the lane's offer's byte decides")
        assert placed.all() and st3["cf_exact_turns"] == 0 and st3["cf_batches"] == 1, st3
    elif name == "nobody_in_run":
        nb = c["nobody"]
        assert not placed[nb].any() and placed[np.setdiff1d(np.arange(k), nb)].all(), (name, np.nonzero(~placed)[0])
        assert st3["cf_walked"] == k, (st3["cf_walked"], "the tables promise room: the jobs nobody takes are walked")
    elif name == "epoch_in_run":
        assert st3["cf_epochs"] >= 1 and placed.all(), st3
        assert np.unique(j3[:N_EPOCH_OPEN]).size == N_EPOCH_OPEN, "every opener takes an offer of its own: the overlay fills inside batch 0"
        assert np.isin(j3[N_EPOCH_OPEN:64], j3[:N_EPOCH_OPEN]).all(), "the small jobs behind the epoch's end go onto what the openers left"
    elif name == "tie_in_run":
        assert st3["cf_exact_turns"] >= len(c["pair"]), st3
        for q, a in c["pair"]:
            assert j3[q] == a, (q, j3[q], a, "equal fitness: the lower offer")
        assert placed.all()
    return st3
