"""Cases for the class-ordered walk (match_algo 3) at its batch boundaries, bit for bit against the oracle; shared by the emulated and the GPU
test files.  Not a test module.

A batch is 64 consecutive ranked jobs.  The cases are built for what happens BETWEEN batches: runs of batches no job of which is walked (the
bookkeeper settles them alone and hands the other waves the first batch with a walked job: base, ring slot, walk mask), a queue that ends in
such batches or inside one, room that goes away during the batch before, an epoch and an exact turn right behind a boundary, and constrained
jobs inside batches nobody walks.  Every case must be placed by the class-ordered form (placement_form 3, nothing refused): resources are
integers on the 8 cpus levels and dyadic, as synth.py's are.

Every function below is one test's body: it takes the test file's make_engine and the test's parameters (the lists below).
"""
import dataclasses

import numpy as np

from cook_amd import _abi as A
from cook_amd import synth
from oracle import pyoracle
from tests import parity_cases as P

# the tests' parameters (the emulated and the GPU file run the same)
LEADS, RUNS = [64, 128, 100], [1, 2, 3, 5]
QUEUE_ENDS = [(70, 150), (70, 122), (10, 30), (0, 64), (0, 40), (0, 200), (64, 1), (63, 66), (1, 0), (64, 0), (130, 0)]
ROOM_SHAPES = ["same", "mixed", "constrained"]
SHIFTS = list(range(0, 24, 3))
TIE_SEEDS = [1, 2, 3]
SHIPPED_SCALE = 24  # epoch_and_exact_turn_behind_a_boundary's scale where the overlay has its shipped 64 lanes

BIG_MEM = 1048576.0  # more than any offer below holds


def make_offers(n, seed=1, attr=False, gpu_every=0, free_frac=None):
    rng = np.random.default_rng(seed)
    tot_c = rng.choice([16.0, 32.0, 64.0, 96.0], size=n, p=[.2, .4, .3, .1])
    frac = rng.uniform(0.3, 1.0, n) if free_frac is None else np.full(n, free_frac)
    oc = np.floor(tot_c * frac)
    om = np.floor(tot_c * 4096.0 * frac)
    run_c, run_m = tot_c - oc, tot_c * 4096.0 - om
    run_n = np.rint(run_c / 3.0).astype(np.int32)
    kw = {}
    if attr:
        a = np.zeros((n, 8), dtype=np.uint32)
        for k, card in enumerate([2, 3, 4, 8, 16, 32, 64, 0]):
            a[:, k] = (np.arange(n) + 1) if card == 0 else rng.integers(1, card + 1, n)
        kw["attr"] = a
    if gpu_every:
        gm = np.zeros(n, dtype=np.uint32)
        gc = np.zeros(n)
        gm[::gpu_every] = 1
        gc[::gpu_every] = 4.0
        run_n[::gpu_every] = 0
        kw.update(gpu_model=gm, gpu_count=gc)
    return A.Offers(cpus=oc, mem=om, host=np.arange(n, dtype=np.uint32), k8s=np.ones(n, dtype=np.uint8), run_cpus=run_c, run_mem=run_m,
                    run_count=run_n, **kw)


def _small(rng, n):
    return rng.integers(1, 5, n).astype(np.float64), (rng.integers(1, 9, n) * 512).astype(np.float64)


def _big(rng, n):
    return rng.integers(1, 9, n).astype(np.float64), np.full(n, BIG_MEM)


def check(make_engine, jobs, offers, groups=None, tag="", explain=True):
    p = A.default_params(good_enough_fitness=1.0, match_algo=3)
    with make_engine(p) as e:
        j2o, fail, head = e.match(jobs, offers, groups, ())
        stt = e.match_stats()
    assert stt["placement_form"] == 3 and stt["classfit_refused"] == 0, (tag, stt)
    o = pyoracle.match(p, jobs, offers, groups, ())
    bad = np.nonzero((j2o != o[0]) | (fail != o[1]))[0]
    assert len(bad) == 0, (tag, bad[:8], j2o[bad[:8]], o[0][bad[:8]], fail[bad[:8]], o[1][bad[:8]])
    assert head == o[2], tag
    if explain and (j2o < 0).any():
        P.explain_parity(make_engine, jobs, offers, groups, p, tag=tag)
    return j2o, fail, stt


def run_of_batches_nobody_walks_in_the_middle(make_engine, lead, run):
    """small jobs, `run` whole batches of jobs larger than any offer, small jobs again: the walk goes on at the right base and ring slot
    (run lengths of both parities, from an even and an odd batch, and from inside a batch)"""
    rng = np.random.default_rng(100 * lead + run)
    tail = 150
    # (lead = 100: the run starts inside batch 1; enough large jobs that `run` WHOLE batches hold nothing else)
    n_big = 64 * run + (64 - lead % 64) % 64 + (32 if lead % 64 else 0)
    c0, m0 = _small(rng, lead)
    c1, m1 = _big(rng, n_big)
    c2, m2 = _small(rng, tail)
    jobs = A.Jobs(cpus=np.concatenate([c0, c1, c2]), mem=np.concatenate([m0, m1, m2]))
    j2o, fail, stt = check(make_engine, jobs, make_offers(90, seed=run), tag=f"middle {lead} {run}")
    assert (j2o[:lead] >= 0).all() and (j2o[lead:lead + n_big] < 0).all() and (fail[lead:lead + n_big] == 1).all()
    assert (j2o[lead + n_big:] >= 0).sum() > tail // 2, "the jobs behind the run are placed"
    assert stt["cf_walked"] <= lead + tail and stt["cf_batches"] == (jobs.n + 63) // 64


def queue_ends_in_batches_nobody_walks(make_engine, k_small, k_big):
    """K not a multiple of 64 with the last batches empty, K <= 64, a queue nobody walks at all"""
    rng = np.random.default_rng(1000 * k_small + k_big)
    c0, m0 = _small(rng, k_small)
    c1, m1 = _big(rng, k_big)
    jobs = A.Jobs(cpus=np.concatenate([c0, c1]), mem=np.concatenate([m0, m1]))
    j2o, fail, _ = check(make_engine, jobs, make_offers(60, seed=3), tag=f"tail {k_small} {k_big}")
    assert (j2o[:k_small] >= 0).all() and (j2o[k_small:] < 0).all() and (fail[k_small:] == 1).all()


def room_goes_away_during_the_batch_before(make_engine, shape):
    """the offers take exactly 100 small jobs: batch 1 uses up the room, the jobs behind it end unmatched with the oracle's failure codes
    (1: some offer lacks room; 2: an offer with room refuses on a constraint; never 8)"""
    n_off = 25
    oc, om = np.full(n_off, 8.0), np.full(n_off, 8192.0)
    attr = np.zeros((n_off, 8), dtype=np.uint32)
    attr[:, 0] = 1 + (np.arange(n_off) % 2)
    attr[:, 7] = np.arange(n_off) + 1
    offers = A.Offers(cpus=oc, mem=om, host=np.arange(n_off, dtype=np.uint32), k8s=np.ones(n_off, dtype=np.uint8), attr=attr,
                      run_cpus=np.full(n_off, 8.0), run_mem=np.full(n_off, 8192.0), run_count=np.full(n_off, 3, dtype=np.int32))
    n = 300
    cpus, mem = np.full(n, 2.0), np.full(n, 2048.0)
    equals = [[] for _ in range(n)]
    if shape != "same":
        cpus[1::3], mem[1::3] = 4.0, 4096.0
        cpus[5::7], mem[5::7] = 1.0, 512.0
    if shape == "constrained":
        for q in range(0, n, 5):
            equals[q] = [(0, 1 + (q // 5) % 3)]  # value 3: no offer has it
    jobs = A.Jobs.with_constraints(cpus, mem, equals=equals) if shape == "constrained" else A.Jobs(cpus=cpus, mem=mem)
    j2o, fail, stt = check(make_engine, jobs, offers, tag=f"room {shape}")
    unm = j2o < 0
    assert unm[128:].all() and unm.sum() > 100 and not (fail[unm] == 8).any()
    assert set(np.unique(fail[unm]).tolist()) <= {1, 2, 3}
    if shape == "same":
        assert (j2o[:100] >= 0).all() and unm[100:].all() and (fail[100:] == 1).all()


def epoch_and_exact_turn_behind_a_boundary(make_engine, shift, scale=1, epochs=True):
    """offers half free and jobs of few shapes: exact turns (the literal fitness decides) and epochs (the overlay goes back into the
    classes' arrays) all along the queue; the shift moves them across the batch boundaries, behind batches with removals.
    scale: that many times the offers and the jobs — an epoch ends at 8 live overlay lanes in the everyday emulated build and at 58 in the
    shipped shape, so the GPU file also runs a pool SHIPPED_SCALE times as large, with the same shifts and the same counters asked for.
    epochs=False: the pool is run where its size cannot fill the overlay (the small pool on the GPU: 58 live lanes never come together, it ends
    no epoch there); everything but the epoch count is asserted, which the scaled pool carries"""
    rng = np.random.default_rng(7)
    offers = make_offers(160 * scale, seed=2, free_frac=0.5)
    n = 284 * scale + shift
    cpus = rng.integers(1, 9, n).astype(np.float64)
    mem = (rng.integers(1, 9, n) * 2048).astype(np.float64)
    jobs = A.Jobs(cpus=cpus, mem=mem).take(np.arange(24 - shift, n))
    _, _, stt = check(make_engine, jobs, offers, tag=f"epochs {shift} x{scale}", explain=shift == 0 and scale == 1)
    assert stt["cf_exact_turns"] >= 3, stt
    if epochs:
        assert stt["cf_epochs"] >= 2, stt


def tie_heavy_pools_with_a_run_in_the_middle(make_engine, seed):
    """synth.py's tie-heavy pools (epochs, exact turns, constraints, groups) cut in two by a run of batches nobody walks"""
    pool = synth.make_pool(seed=0xBA7C0 + seed, n_pending=520, n_running=40, n_users=9, n_offers=140, constraints=True, tie_heavy=True)
    jobs = pool.pending_jobs
    cpus, mem = jobs.cpus.copy(), jobs.mem.copy()
    lo = 64 * seed + 7
    mem[lo:lo + 64 * seed + 70] = BIG_MEM
    jobs = dataclasses.replace(jobs, cpus=cpus, mem=mem)
    j2o, fail, stt = check(make_engine, jobs, pool.offers, pool.groups, tag=f"tie-heavy {seed}")
    assert (j2o[lo:lo + 64 * seed + 70] < 0).all() and (j2o[lo + 64 * seed + 70:] >= 0).any()


def constrained_jobs_in_batches_nobody_walks(make_engine):
    """unmatched jobs with attribute / novel-host / unique-group constraints, and gpu jobs no host can take, inside batches nobody walks"""
    rng = np.random.default_rng(11)
    lead, n_big, tail = 70, 64 * 3 + 58, 90
    n = lead + n_big + tail
    c0, m0 = _small(rng, lead)
    c1, m1 = _big(rng, n_big)
    c2, m2 = _small(rng, tail)
    cpus, mem = np.concatenate([c0, c1, c2]), np.concatenate([m0, m1, m2])
    n_off = 80
    equals = [[] for _ in range(n)]
    novel = [[] for _ in range(n)]
    grp = np.full(n, A.NONE_U32, dtype=np.uint32)
    gpus = np.zeros(n)
    gmodel = np.zeros(n, dtype=np.uint32)
    for q in range(lead + 2, lead + n_big, 4):
        equals[q] = [(int(rng.integers(0, 6)), int(rng.integers(1, 3)))]
    for q in range(lead + 3, lead + n_big, 9):
        novel[q] = [int(h) for h in rng.integers(0, n_off, 2)]
    for g, q in enumerate(range(lead + 5, lead + n_big - 8, 31)):
        grp[[q, q + 4, q + 8]] = g
    n_g = g + 1
    grp[[3, 9, lead + n_big + 4]] = n_g  # a group with members in front of and behind the run
    # gpu jobs of a small size in the run: the gpu hosts are taken by then (4 hosts, the lead's gpu jobs take them), so nobody walks them
    # although hosts without gpus have room
    for q in (5, 11, 17, 23):
        gpus[q], gmodel[q] = 1.0, 1
    for q in range(lead + 130, lead + 190, 6):
        cpus[q], mem[q], gpus[q], gmodel[q] = 1.0, 512.0, 1.0, 1
        equals[q], novel[q], grp[q] = [], [], A.NONE_U32
    groups = A.Groups(type=np.ones(n_g + 1, dtype=np.uint8), run_hosts=[[int(rng.integers(0, n_off))] if x % 2 else [] for x in range(n_g + 1)])
    jobs = A.Jobs.with_constraints(cpus, mem, equals=equals, novel=novel, group=grp, gpus=gpus, gpu_model=gmodel)
    offers = make_offers(n_off, seed=5, attr=True, gpu_every=20)
    j2o, fail, stt = check(make_engine, jobs, offers, groups, tag="constrained run")
    run = slice(lead, lead + n_big)
    assert (j2o[run] < 0).all() and (j2o[lead + n_big:] >= 0).any()
    assert stt["cf_walked"] <= lead + tail, "the run's batches are not walked"
    small_gpu = np.arange(lead + 130, lead + 190, 6)
    assert (fail[run] & 1).all() and (fail[small_gpu] & 2).all(), "large jobs lack room; the small gpu jobs are refused by hosts with room"
