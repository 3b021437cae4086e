"""Cases for the class-ordered walk's batch-end summary pass (classfit_walk.hpp, "batch end, phase 1"), shared by the emulated and the GPU
test files.  Not a test module.

At the end of a batch every class wave looks at the batch's placements (the decider's log) and recomputes the level summaries of the chunks that
lost a level maximum; the wave's rows of the level-maxima tables follow.  The pools below are small and built so that this pass has something to
get wrong: members of ONE chunk leaving together (the chunk's maximum and a member equal to it among them), placements spread over chunks, sets and
replica waves, gpu hosts occupied in place next to plain removals, an epoch inside a batch (only the log entries behind it count), a full log, and
jobs whose fate hangs on one chunk's summary: a stale summary would promise room that is gone (a wrong failure code, a job walked for nothing) or a
wrongly recomputed one would deny room that is there.

What carries the detection in every case is its PROBES: jobs that ask for TOP in a batch behind the one in which TOP's last holder left, that nobody
walks, and whose failure code (1, against 3 from a stale row) reads the level-maxima tables.  The pools have slack and no job between the removal and
the probes makes a class wave scan the holder's chunk for nothing — a wave that does recomputes the chunk on the spot, batch-end pass or none.
Seen against mutated copies of the pass (emulated build): with the pass disabled every case fails, each through its probes.  With no plain entry
flagged: same_chunk, spread_sets, epoch_in_batch, full_log (gpu_in_place's entries carry the gpu bit).  Summaries fetched from the wrong lane:
same_chunk, epoch_in_batch, full_log.  Only the first flagged chunk recomputed: same_chunk, gpu_in_place, epoch_in_batch.  Two mutations fail nothing:
the gpu bit ignored (redundant: an occupied host was free, so the maximum test flags it whenever a summary moves), and the log's last entry skipped
(emulated build: the wave that loses a member at the batch's last step answers that step again and recomputes the chunk; on the GPU a matter of timing).

Resources are integers on the 8 cpus levels (1..8) and dyadic, so every case is placed by the class-ordered form (placement_form 3).
"""
import numpy as np

from cook_amd import _abi as A
from oracle import pyoracle

MEMS = np.array([2048.0, 4096.0, 8192.0, 16384.0])  # few values: every chunk holds its level maxima several times over


def offers_of(tot_c, free_c, free_m, gpu_at=(), attr=False):
    """offers with the given totals (cpus; mem = 4096 per cpu) and free values; gpu_at: indices of gpu hosts (4 gpus of model 1, nothing running)"""
    tot_c, free_c, free_m = np.asarray(tot_c, dtype=np.float64), np.asarray(free_c, dtype=np.float64), np.asarray(free_m, dtype=np.float64)
    n = len(tot_c)
    tot_m = tot_c * 4096.0
    assert (free_c <= tot_c).all() and (free_m <= tot_m).all()
    run_n = np.maximum(1, np.rint((tot_c - free_c) / 3.0)).astype(np.int32)
    kw = {}
    if attr:
        a = np.zeros((n, 8), dtype=np.uint32)
        a[:, 0] = 1 + (np.arange(n) % 2)
        a[:, 7] = np.arange(n) + 1
        kw["attr"] = a
    if len(gpu_at):
        gm, gc = np.zeros(n, dtype=np.uint32), np.zeros(n)
        gm[list(gpu_at)], gc[list(gpu_at)] = 1, 4.0
        run_n[list(gpu_at)] = 0
        kw.update(gpu_model=gm, gpu_count=gc)
    return A.Offers(cpus=free_c, mem=free_m, host=np.arange(n, dtype=np.uint32), k8s=np.ones(n, dtype=np.uint8), run_cpus=tot_c - free_c,
                    run_mem=tot_m - free_m, run_count=run_n, **kw)


def _jobs(cpus, mem, equals=None, gpus=None):
    cpus, mem = np.asarray(cpus, dtype=np.float64), np.asarray(mem, dtype=np.float64)
    if equals is None and gpus is None:
        return A.Jobs(cpus=cpus, mem=mem)
    kw = {}
    if equals is not None:
        kw["equals"] = equals
    if gpus is not None:
        g = np.asarray(gpus, dtype=np.float64)
        kw.update(gpus=g, gpu_model=(g > 0).astype(np.uint32))
    return A.Jobs.with_constraints(cpus, mem, **kw)


TOP2 = 40960.0
TOP = 32768.0  # a free mem above every other host's: its holders leave in one batch, and the jobs behind them ask for it again


def _probes(cpus, mem, gpus, at, c, as_gpu):
    """jobs at `at` that ask for TOP when no host holds it any more.  Placements cannot show a stale summary (it is an upper bound, and a class wave
    that scans a chunk for nothing recomputes it on the spot): what shows it is the failure code of a job nobody walks, through the level-maxima
    tables.  A gpu job is walked by its kind's row only and a plain job by the rows of the hosts without gpus, but "some offer has room" (code 3
    instead of 1) reads EVERY wave's row: so gpu jobs probe the rows of the plain sets, plain jobs the row of the gpu set."""
    at = np.asarray(list(at))
    cpus[at], mem[at] = c, TOP
    gpus[at] = 4.0 if as_gpu else 0.0
    return at


def case_same_chunk():
    """one class of 150 members (three chunks in one class wave).  Free mem takes four values only, and the jobs ask for exactly these: a job of
    16384 can only take a member that IS its chunk's maximum, the next one takes its equal, and so on until none is left.  Then: one member of
    20480 that only a late job can use (a summary recomputed wrongly would deny it), late jobs of 16384 when every such member is gone (a stale
    summary would promise room: the constrained ones among them would get the code of a refusal instead of 1).  Two holders of TOP sit among the
    others and leave in batch 0; gpu jobs (no host has gpus: nobody walks them) ask for TOP in batch 1."""
    rng = np.random.default_rng(41)
    n = 150
    free_c = rng.integers(1, 9, n).astype(np.float64)
    free_m = MEMS[rng.integers(0, 4, n)]
    free_c[77], free_m[77] = 1.0, 20480.0
    free_c[[30, 120]], free_m[[30, 120]] = 8.0, TOP  # (the emptiest hosts: only the jobs that need them take them)
    offers = offers_of(np.full(n, 64.0), free_c, free_m, attr=True)
    k = 260
    cpus = rng.integers(2, 5, k).astype(np.float64)
    mem = MEMS[rng.integers(0, 4, k)]
    gpus = np.zeros(k)
    mem[:128] = MEMS[rng.integers(0, 3, 128)]  # (in batches 0 and 1 only the jobs below ask for 16384: members of 16384 are left behind them, so
    mem[:40:3] = 16384.0                      # nobody scans the last chunk for nothing)  several of one batch: the maxima and their equals
    cpus[[20, 50]], mem[[20, 50]] = 2.0, TOP  # the holders of TOP leave (no mem is left of them: no overlay lane)
    equals = [[] for _ in range(k)]
    cpus[200], mem[200] = 1.0, 20480.0  # only offer 77 holds it, and it has the cpus for no other job
    cpus[259], mem[259] = 8.0, 2048.0   # (the cpus levels span 1..8)
    mem[201:259:2] = 16384.0
    for q in range(203, 259, 4):
        equals[q] = [(0, 3)]  # no offer has the value: refused wherever there is room
    probes = _probes(cpus, mem, gpus, range(70, 100, 5), 2.0, True)
    return _jobs(cpus, mem, equals=equals, gpus=gpus), offers, probes


def case_spread_sets():
    """three classes of hosts without gpus (their sets share the class waves the gpu set leaves: the two largest have replica waves) and a gpu
    class; every class spans several chunks and the jobs of a batch take members all over them.  Three holders of TOP in the largest class (a set
    with replica waves) leave in batch 0; gpu jobs ask for TOP in batch 1, plain and constrained jobs in batch 2."""
    rng = np.random.default_rng(42)
    tot = np.repeat([32.0, 64.0, 96.0], [140, 200, 90])
    n = len(tot)
    free_c = rng.integers(1, 9, n).astype(np.float64)
    free_m = MEMS[rng.integers(0, 4, n)]
    gpu_at = np.arange(5, n, 37)
    free_c[gpu_at], free_m[gpu_at] = 8.0, 16384.0
    hold = np.array([150, 230, 300])  # (none of them a gpu host)
    free_c[hold], free_m[hold] = 2.0, TOP
    offers = offers_of(tot, free_c, free_m, gpu_at=gpu_at, attr=True)
    k = 300
    cpus = rng.integers(1, 9, k).astype(np.float64)
    mem = MEMS[rng.integers(0, 4, k)]
    gpus = np.zeros(k)
    cpus[[7, 31, 63]], mem[[7, 31, 63]] = 2.0, TOP
    equals = [[] for _ in range(k)]
    probes = np.concatenate([_probes(cpus, mem, gpus, range(66, 126, 6), 2.0, True), _probes(cpus, mem, gpus, range(130, 190, 6), 2.0, False)])
    for q in range(136, 190, 12):
        equals[q] = [(0, 3)]
    return _jobs(cpus, mem, equals=equals, gpus=gpus), offers, probes


def case_gpu_in_place():
    """gpu jobs (their host stays in its chunk, occupied, with new free values) in the same batches as plain jobs.  The gpu class has 110 members
    (two chunks); two of them hold TOP — the emptiest, so they sit in the second chunk — and are occupied in batch 0 by the gpu jobs 12 and 62,
    which ask for all of it.  Every other gpu job asks for 2048, which every free gpu host has: no job scans a chunk for nothing, so nothing but
    the batch-end pass recomputes the second chunk.  In batch 1 PLAIN jobs ask for TOP: nobody walks them (no host without gpus holds it), and
    their code hangs on the gpu set's row of all members, occupied ones with their new values included.  (A gpu job that asks for TOP behind
    them would be walked by the gpu kind's stale row, scan the chunk and recompute it: those come in batch 2.)"""
    rng = np.random.default_rng(43)
    n = 220
    tot = np.full(n, 64.0)
    free_c = rng.integers(2, 9, n).astype(np.float64)
    free_m = MEMS[rng.integers(0, 4, n)]
    gpu_at = np.arange(0, n, 2)
    free_c[gpu_at] = rng.integers(4, 9, len(gpu_at))
    free_c[[10, 140]], free_m[[10, 140]] = 8.0, TOP
    offers = offers_of(tot, free_c, free_m, gpu_at=gpu_at)
    k = 200
    cpus = rng.integers(1, 5, k).astype(np.float64)
    mem = MEMS[rng.integers(0, 4, k)]
    gpus = np.zeros(k)
    gpus[:128:2] = 4.0  # (a gpu job takes a host whose gpus it asks for, all of them)
    mem[:128:2] = 2048.0
    cpus[[12, 62]], mem[[12, 62]] = 2.0, TOP
    probes = np.concatenate([_probes(cpus, mem, gpus, range(65, 128, 6), 2.0, False), _probes(cpus, mem, gpus, range(130, 160, 6), 2.0, True)])
    return _jobs(cpus, mem, gpus=gpus), offers, probes


def case_epoch_in_batch():
    """jobs 0..57 each take an offer of their own and leave it alive (it cannot take a second job of this size): the overlay fills up and epochs
    end INSIDE batch 0 — in the shipped shape (58 live lanes) at job 57, in the emulated one (8) after every eighth job, the last at job 55.
    Behind the batch's last epoch nothing opens a lane any more: jobs 58..63 take whole offers, and job 60 takes the one holder of TOP.  So the log
    has entries in front of the epoch (CFX_LOG_APPLIED > 0) and the removal that matters behind it.  Batch 1 is gpu jobs that ask for TOP (nobody
    walks them) between jobs that take whole offers: no epoch there, which would recompute every summary.
    That the pass SKIPS the entries in front of the epoch cannot be made to fail: the epoch recomputed every summary from the new arrays, so
    looking at those entries again would flag chunks for nothing and recompute them to the same values."""
    n = 300
    rng = np.random.default_rng(44)
    tot = np.repeat([32.0, 64.0], [150, 150])
    free_c = np.full(n, 8.0)
    free_m = 10240.0 + 512.0 * rng.integers(0, 4, n)
    free_m[250] = TOP  # (the emptiest host: only the job that needs it takes it)
    offers = offers_of(tot, free_c, free_m)
    k = 150
    cpus = np.full(k, 2.0)
    mem = np.full(k, 8192.0)
    gpus = np.zeros(k)
    cpus[58:128] = 8.0  # whole offers: nothing of them is left, no overlay lane
    cpus[60], mem[60] = 2.0, TOP
    cpus[-1], mem[-1] = 1.0, 512.0  # the smallest request: what jobs 0..57 leave behind is still an offer
    probes = _probes(cpus, mem, gpus, range(66, 126, 10), 2.0, True)
    return _jobs(cpus, mem, gpus=gpus), offers, probes


def case_full_log():
    """batches of 64 walked and matched jobs, each taking a whole offer out of its class's arrays: 64 entries in the log, none from the overlay.
    The pool has slack (400 offers for 230 jobs): with a pool that the jobs use up, the chunks run empty, jobs scan them for nothing and the class
    waves recompute them on the spot, batch-end pass or none.  One host holds TOP and job 10 takes it; one of the other class holds TOP2 and job
    63 — the log's LAST entry — takes that (a class wave that sees its member leave may answer the decider's current step again and recompute
    the chunk on the way: whether entry 63 is left to the batch-end pass is a matter of timing, entry 10 always is).  gpu jobs ask for TOP in
    batch 2 (batch 1 is another full log), plain and constrained ones behind them."""
    rng = np.random.default_rng(45)
    n = 400
    tot = np.repeat([32.0, 64.0], [200, 200])
    free_c = np.full(n, 4.0)
    free_m = MEMS[rng.integers(0, 4, n)]
    free_m[330], free_m[40] = TOP, TOP2
    offers = offers_of(tot, free_c, free_m, attr=True)
    k = 230
    cpus = np.full(k, 4.0)
    mem = MEMS[rng.integers(0, 3, k)]
    gpus = np.zeros(k)
    mem[10], mem[63] = TOP, TOP2  # (a later job that asks for TOP or less than it above 16384 would make the wave scan the chunk and recompute it)
    cpus[-1], mem[-1] = 1.0, 2048.0
    cpus[-2] = 8.0
    equals = [[] for _ in range(k)]
    probes = np.concatenate([_probes(cpus, mem, gpus, range(130, 190, 6), 4.0, True), _probes(cpus, mem, gpus, range(194, 226, 4), 4.0, False)])
    for q in range(198, 226, 8):
        equals[q] = [(0, 3)]
    return _jobs(cpus, mem, equals=equals, gpus=gpus), offers, probes


CASES = {"same_chunk": case_same_chunk, "spread_sets": case_spread_sets, "gpu_in_place": case_gpu_in_place, "epoch_in_batch": case_epoch_in_batch,
         "full_log": case_full_log}


def run_case(make_engine, name):
    """the case under match_algo 3 (twice: the second engine is built afresh), match_algo 2 and the oracle; the assertions every case shares"""
    jobs, offers, probes = CASES[name]()
    p3 = A.default_params(good_enough_fitness=1.0, match_algo=3)
    p2 = A.default_params(good_enough_fitness=1.0, match_algo=2)
    runs = []
    for p in (p3, p3, p2):
        with make_engine(p) as e:
            j2o, fail, head = e.match(jobs, offers, None, ())
            runs.append((j2o.copy(), fail.copy(), head, e.match_stats()))
    (j3, f3, h3, st3), (j3b, f3b, _, st3b), (j2, f2, h2, _) = runs
    o = pyoracle.match(p3, jobs, offers, None, ())
    assert st3["placement_form"] == 3 and st3["classfit_refused"] == 0, (name, st3)
    bad = np.nonzero((j3 != o[0]) | (j3 != j2))[0]
    assert len(bad) == 0, (name, bad[:8], j3[bad[:8]], o[0][bad[:8]], j2[bad[:8]])
    badf = np.nonzero((f3 != f2) | (f3 != o[1]))[0]
    assert len(badf) == 0, (name, badf[:8], f3[badf[:8]], f2[badf[:8]], o[1][badf[:8]])
    assert h3 == o[2] == h2, name
    assert st3b["placement_form"] == 3 and np.array_equal(j3b, j3) and np.array_equal(f3b, f3), name
    assert st3["cf_walked"] == st3b["cf_walked"], (name, st3["cf_walked"], st3b["cf_walked"])
    assert (j3[probes] < 0).all() and (f3[probes] == 1).all(), (name, "no host holds TOP any more: nothing has room for these", probes, j3[probes], f3[probes])
    return jobs, offers, j3, f3, st3


def check_case(make_engine, name):
    """run_case and what makes the case the case it is meant to be (from the placements and the counters every build keeps)"""
    jobs, offers, j2o, fail, stt = run_case(make_engine, name)
    unm = j2o < 0
    if name == "same_chunk":
        assert j2o[200] == 77, "the one member of 20480 is found behind the removals from its chunk"
        assert stt["cf_retightened"] > 0 and (j2o[:40:3] >= 0).all()
        late = np.arange(201, 259, 2)
        assert unm[late].sum() >= 10 and (fail[late[unm[late]]] == 1).all(), "no member of 16384 is left: nothing promises room for these"
    elif name == "spread_sets":
        assert stt["cf_retightened"] > 0 and (~unm).sum() > 150 and set(j2o[[7, 31, 63]].tolist()) == {150, 230, 300}
    elif name == "gpu_in_place":
        g = np.nonzero(jobs.gpus > 0)[0]
        on = j2o[g][~unm[g]]
        assert j2o[12] in (10, 140) and j2o[62] in (10, 140) and j2o[12] != j2o[62], "the holders of TOP are occupied in batch 0"
        assert len(on) > 20 and np.unique(on).size == len(on) and (offers.gpu_count[on] > 0).all(), "a gpu host takes one gpu job, in place"
        assert (~unm[1:64:2]).sum() > 20, "plain jobs are placed in the same batches"
    elif name == "epoch_in_batch":
        assert stt["cf_epochs"] >= 1 and (~unm[:64]).all() and j2o[60] == 250, stt
        assert np.unique(j2o[:128][~unm[:128]]).size == (~unm[:128]).sum() >= 64 + 50, "every job takes an offer of its own: the epochs end inside batch 0"
    elif name == "full_log":
        assert (~unm[:128]).all() and np.unique(j2o[:128]).size == 128 and stt["cf_epochs"] == 0, stt
        assert j2o[10] == 330 and j2o[63] == 40, "the holder of TOP leaves in the middle of the log, the holder of TOP2 with its entry 63"
