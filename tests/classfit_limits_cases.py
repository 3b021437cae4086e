"""Cases for the class-ordered walk (match_algo 3, classfit*.hpp) AT THE LIMITS OF ITS TABLES, shared by the emulated and the GPU test files.
Not a test module.

The form sizes everything to hard capacities: 48 classes, 32 gpu kinds, 8192 offers with 13-bit ids in the sort key, 64 chunks per class and per
class wave, 4096 groups of at most 16 pending members, resources as u32 multiples of 2^-k (k <= 20, value * 2^k < 2^30), 2 Tc Tm < 2^45, eight
cpus levels, EQUALS on keys < 8 with byte values, four novel hosts, host ids up to 8 M + 65536, 60000 running cotasks + pending members, and an LDS sum that the host
(cf_lds_bytes_host) and the kernel (cf_walk_pool) compute on their own.  Every case below is a pair or a short sweep that straddles ONE of them:
  * at the limit: placement_form 3, classfit_refused 0; job_to_offer, fail_code and head_matched equal the oracle's bit for bit and match_algo 2's;
  * one beyond: the window rounds (placement_form 0) with EXACTLY the refusal word written beside the case, and the oracle's placements.
The words come from the rules the code states (the CF_X_* comments of classfit.hpp; 0x10000 where cf_setup's own checks answer before any
set-up launch), not from a run.  Two rules are narrower than they first read, and the cases say so:
  * levels: the eight levels are cmin + floor(i (cmax - cmin) / 7) in fixed point.  With whole cpus (k = 0) the requests {1, 2, 4} get the levels
    1 1 1 2 2 3 3 4 and are ON them (form 3); with a quarter cpu anywhere in the call (k = 2) the levels are 4 5 7 9 10 12 14 16 quarters, 2.0 is
    missing, and the call is refused.  Both are cases.
  * the sort key and the fixed-point width meet in one pool: Tm = 2^30 - 1 needs k = 0 for mem, and then Tc = 2^14 is the greatest total below
    2 Tc Tm = 2^45; the cpus width (2^-20) is a pool of its own with small totals.

An at-limit case makes the walk WORK at capacity, not only get through the set-up (build_pool): every offer has 8 cpus free and one of four
free-mem values (equal E inside a class: exact turns); N_OPEN "openers" each take an offer of their own and leave it alive but too small for
the next opener, so the overlay fills and epochs end (at 8 live lanes in the everyday emulated build, at 58 in the shipped shape: 140 openers
are two epochs there) and the merge goes back into arrays that are full; a few EMPTIEST members of the class at its limit — they sort last,
into the last chunk — hold a free mem (TOP) found nowhere else, and a few jobs ask for exactly TOP, in front of the first epoch and behind the
last: such a placement exists only if the walk reaches the last chunk of the full class; two more ask for TOP when no holder is left, others for
more than any host has: they end unmatched with the oracle's codes.  Asserted per at-limit call: cf_epochs >= 2, cf_exact_turns >= 1,
cf_batches = ceil(K / 64), the holders taken by exactly the jobs that ask for TOP.

Seen against mutated copies of the checks (a scratch copy built with the everyday emulator only: a relaxed limit overruns the tables it guards,
so never on the GPU) — the mutation, and what failed:
  * cf_prepare `nc >= CF_MAXCLS` -> `>`: classes (the 49-class call overruns the class tables: the emulated process dies with a segmentation fault).
  * cf_prepare `nk >= CF_MAXKIND` -> `>`: kinds (32 signatures + plain: form 3, word 0, where CF_X_SHAPE is expected).
  * cf_prepare `(s_cnt[c] + 63) / 64 > 64` -> `> 65` ALONE: nothing fails.  The check is redundant: the wave assignment below it
    (`load[x] + nch <= 64`) finds no wave for a class of 65 chunks and refuses with the same word.  With that one relaxed to `<= 65` as well: one_class
    (4097 members: form 3, word 0).
  * cf_prepare `load[wsel] > 64` -> `> 65` (the gpu waves' load): wave_load (2048 + 2049: form 3, word 0).
  * cf_pack_jobs `slot < CF_GMEM` -> `<=`: groups (17 members: form 3, word 0).
  * cf_setup `M > CF_SORT_N` -> `> CF_SORT_N + 1`: offers (8193 offers: cf_prepare's own check answers, CF_X_SHAPE where 0x10000 is expected).
  * cf_setup `G > CF_MAXG` -> `> CF_MAXG + 1`: groups (4097 groups: likewise CF_X_SHAPE where 0x10000 is expected).
  * cf_setup `max_host > 8 M + 65536` -> `+ 65537`: host_ids (form 3, word 0).
  * cf_scan `eq_val >= 256` -> `> 256`: equals (value 256: form 3, word 0).
  * cf_prepare `kc > 20` -> `> 21`: fixed_cpus (2^-21: form 3, word 0).
  * cf_prepare `2 Tc Tm < 2^45` -> `< 2^46`: sort_key (Tc = 2^14 + 1: form 3, word 0).
  * cf_lds_bytes_host `NP * 10` -> `NP * 8` (the host's sum short of the kernel's): the EQUALS sweep, at M = 8192, by cf_run's "tables do not fit" error.
  * cf_setup `S > 60000` -> `> 60001`: cotasks (S = 60001: form 3, word 0).
  * cf_scan `eq_key >= 8` -> `> 8`: equals (key 8: form 3, word 0).
  * cf_prepare `value * 2^k < 2^30` -> `<=` (both resources): sort_key (Tm = 2^30 gets past it and is refused by the sort-key check instead:
    CF_X_SHAPE where CF_X_NUMBERS is expected).
  * cf_prepare `G > CF_MAXG` ALONE cannot fail anything: cf_setup asks the same question first and answers 0x10000 (the mutation of cf_setup's
    check above shows cf_prepare's behind it).  Both relaxed to `> CF_MAXG + 1`: groups (4097 groups: form 3, word 0).
Not mutated, and why:
  * the levels: there is no comparison to relax by one.  A request is on the levels if it EQUALS one of eight computed values (cf_pack_jobs);
    the pair's two sides differ in the values' spacing, not in a count, and a changed spacing is another rule, not a relaxed one.
  * the novel-host count: `MV_NC` = 4 is the number of fast constraint slots of the window rounds' own job records (match_v2.hpp), which cf_scan
    only reads: a fifth host has no slot to sit in, in either form.
The limit of 2^20 jobs (a board entry's tag) has no case: a call of that size does not fit a test.
"""
import dataclasses

import numpy as np

from cook_amd import _abi as A
from cook_amd import synth
from oracle import pyoracle
from tests import parity_cases as P

X_NUMBERS, X_JOB_SLOW, X_GROUP, X_OFFER, X_SHAPE, X_LEVELS = P.CF_X_NUMBERS, P.CF_X_JOB_SLOW, P.CF_X_GROUP, P.CF_X_OFFER, P.CF_X_SHAPE, P.CF_X_LEVELS
X_HOST = P.CF_REFUSED_HOST  # cf_setup's own checks (classfit_host.hpp)
WALK_ERROR = "the pool's tables do not fit"  # cf_run's error when the kernel's LDS sum exceeds what the host's let through

TOP = 32768.0        # a free mem only the holders have
BIG_MEM = 1048576.0  # more than any offer holds
N_OPEN = 140         # openers: two epochs of the shipped overlay (58 live lanes), seventeen of the everyday emulated one (8)
P3 = dict(good_enough_fitness=1.0, match_algo=3)
P2 = dict(good_enough_fitness=1.0, match_algo=2)


@dataclasses.dataclass
class Pool:
    """a call under construction: offer columns and per-job lists, finished by jobs() / offers()"""
    o: dict
    j: dict
    holders: np.ndarray
    askers: np.ndarray  # the jobs that ask for TOP: len(holders) of them find a holder, two more find none
    groups: object = None

    @property
    def M(self):
        return len(self.o["cpus"])

    @property
    def K(self):
        return len(self.j["cpus"])

    def offers(self):
        return A.Offers(k8s=np.ones(self.M, dtype=np.uint8), **self.o)

    def jobs(self):
        j = dict(self.j)
        kw = {}
        if any(len(x) for x in j["equals"]):
            kw["equals"] = j["equals"]
        if any(len(x) for x in j["novel"]):
            kw["novel"] = j["novel"]
        if (j["gpus"] > 0).any():
            kw.update(gpus=j["gpus"], gpu_model=j["gpu_model"])
        if (j["group"] != A.NONE_U32).any():
            kw["group"] = j["group"]
        return A.Jobs.with_constraints(j["cpus"], j["mem"], **kw)

    def add_jobs(self, cpus, mem, gpus=0.0, model=0, at=None):
        """n more jobs (behind the others, or in front of job `at`) -> their indices"""
        cpus = np.atleast_1d(np.asarray(cpus, dtype=np.float64))
        n = len(cpus)
        at = self.K if at is None else at
        ins = lambda a, v: np.insert(a, at, v)
        j = self.j
        j["cpus"], j["mem"] = ins(j["cpus"], cpus), ins(j["mem"], np.broadcast_to(np.asarray(mem, dtype=np.float64), n))
        j["gpus"], j["gpu_model"] = ins(j["gpus"], np.full(n, gpus)), ins(j["gpu_model"], np.full(n, model, dtype=np.uint32))
        j["group"] = ins(j["group"], np.full(n, A.NONE_U32, dtype=np.uint32))
        j["equals"][at:at] = [[] for _ in range(n)]
        j["novel"][at:at] = [[] for _ in range(n)]
        self.askers = np.where(self.askers >= at, self.askers + n, self.askers)
        return np.arange(at, at + n)


def sig(model, count):
    return (model, float(count))


def build_pool(classes, seed, hold_cls, n_hold=3, cs=1.0, roles=(1.0, 2.0, 8.0), fill=(), last_is_holder=False, n_open=N_OPEN):
    """classes: (Tc, Tm, gpu signature or None, members); their members are dealt over the offer ids at random.  hold_cls: the classes (of one
    kind) whose emptiest members hold TOP, n_hold each.  cs scales every cpus value; roles = the cpus of the smallest job, of an opener and of
    the jobs no host has the mem for; fill = cpus values of further small jobs (the levels cases)."""
    rng = np.random.default_rng(seed)
    ns = np.array([c[3] for c in classes])
    M = int(ns.sum())
    cls_of = np.repeat(np.arange(len(classes)), ns)[rng.permutation(M)]
    if last_is_holder:  # offer M - 1 belongs to the (first) class that holds TOP
        x = np.nonzero(cls_of == hold_cls[0])[0][0]
        cls_of[[x, M - 1]] = cls_of[[M - 1, x]]
    tot_c = np.array([c[0] for c in classes], dtype=np.float64)[cls_of]
    tot_m = np.array([c[1] for c in classes], dtype=np.float64)[cls_of]
    gm = np.array([c[2][0] if c[2] else 0 for c in classes], dtype=np.uint32)[cls_of]
    gc = np.array([c[2][1] if c[2] else 0.0 for c in classes])[cls_of]
    free_c = np.full(M, 8.0 * cs)
    free_m = 10240.0 + 512.0 * (np.arange(M) % 4)
    holders = []
    for c in hold_cls:
        mem = np.nonzero(cls_of == c)[0]
        pick = rng.choice(mem[:-1] if last_is_holder and c == hold_cls[0] else mem, n_hold - (1 if last_is_holder and c == hold_cls[0] else 0), replace=False)
        holders += list(pick) + ([M - 1] if last_is_holder and c == hold_cls[0] else [])
    holders = np.array(sorted(holders))
    free_m[holders] = TOP  # (free cpus as everybody's, more mem: the greatest E of the class, the last positions of its array)
    assert (free_c <= tot_c).all() and (free_m <= tot_m).all()
    run_n = np.maximum(1, np.rint((tot_c - free_c) / 3.0)).astype(np.int32)
    run_n[gm != 0] = 0  # gpu hosts with nothing running: a gpu job may take them
    o = dict(cpus=free_c, mem=free_m, host=np.arange(M, dtype=np.uint32), run_cpus=tot_c - free_c, run_mem=tot_m - free_m, run_count=run_n)
    if (gm != 0).any():
        o.update(gpu_model=gm, gpu_count=gc)
    hsig = classes[hold_cls[0]][2]
    c_tiny, c_open, c_big = (r * cs for r in roles)
    pool = Pool(o=o, j=dict(cpus=np.zeros(0), mem=np.zeros(0), gpus=np.zeros(0), gpu_model=np.zeros(0, dtype=np.uint32),
                            group=np.zeros(0, dtype=np.uint32), equals=[], novel=[]), holders=holders, askers=np.zeros(0, dtype=np.int64))
    ask = dict(gpus=hsig[1], model=hsig[0]) if hsig else {}
    n_early = (len(holders) + 1) // 2
    pool.add_jobs(np.full(10, c_open), 8192.0)
    a0 = pool.add_jobs(np.full(n_early, c_open), TOP, **ask)  # in front of the first epoch of either build
    pool.add_jobs(np.full(n_open - 10, c_open), 8192.0)
    pool.add_jobs(np.full(12, c_tiny), 512.0)                 # onto what the openers left
    a1 = pool.add_jobs(np.full(len(holders) - n_early + 2, c_open), TOP, **ask)  # behind the last epoch; two of them find no holder left
    pool.add_jobs(np.full(6, c_big), BIG_MEM)                 # nobody has the mem: nobody walks them
    if len(fill):
        pool.add_jobs(np.asarray(fill, dtype=np.float64) * cs, 512.0)
    pool.add_jobs([c_tiny], 512.0)
    pool.askers = np.concatenate([a0, a1])
    return pool


def plain(n_cls, members, tc0=16.0, step=2.0):
    return [(tc0 + step * i, (tc0 + step * i) * 4096.0, None, members) for i in range(n_cls)]


# ---- running a call --------------------------------------------------------------------------------------------------------------------------------
def _same(tag, got, want, what):
    for name, g, w in zip(("job_to_offer", "fail_code"), got[:2], want[:2]):
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, (tag, name, "differs from " + what, bad[:8], g[bad[:8]], w[bad[:8]])
    assert got[2] == want[2], (tag, "head_matched differs from " + what, got[2], want[2])


def call(e, jobs, offers, groups=None):
    j2o, fail, head = e.match(jobs, offers, groups, ())
    return (j2o.copy(), fail.copy(), head), e.match_stats()


def check_at(make_engine, tag, pool, capacity=True, engine=None):
    """an at-limit call: form 3, the oracle's and match_algo 2's results, the walk at capacity -> (results, statistics)"""
    jobs, offers, groups = pool.jobs(), pool.offers(), pool.groups
    p3 = A.default_params(**P3)
    if engine is None:
        with make_engine(p3) as e:
            got, stt = call(e, jobs, offers, groups)
    else:
        got, stt = call(engine, jobs, offers, groups)
    print(tag, "at the limit: K", pool.K, "M", pool.M, "form", stt["placement_form"], "refused", hex(stt["classfit_refused"]),
          {k: stt.get(k) for k in ("cf_walked", "cf_epochs", "cf_exact_turns", "cf_batches")})
    assert stt["placement_form"] == 3 and stt["classfit_refused"] == 0, (tag, stt["placement_form"], hex(stt["classfit_refused"]))
    want = pyoracle.match(p3, jobs, offers, groups, ())
    _same(tag, got, want, "the oracle")
    if engine is None:
        with make_engine(A.default_params(**P2)) as e2:
            got2, st2 = call(e2, jobs, offers, groups)
        assert st2["placement_form"] == 0, (tag, st2["placement_form"])
        _same(tag, got, got2, "match_algo 2")
    if capacity:
        j2o, fail = got[0], got[1]
        assert stt["cf_epochs"] >= 2 and stt["cf_exact_turns"] >= 1 and stt["cf_batches"] == (pool.K + 63) // 64, (tag, stt)
        on = j2o[pool.askers]
        assert sorted(on[on >= 0].tolist()) == pool.holders.tolist(), (tag, "the holders of TOP (last in their class) go to the jobs that ask for it", on, pool.holders)
        assert (on < 0).sum() == 2 and (j2o < 0).sum() >= 8 and (fail[j2o < 0] != 0).all(), (tag, on)
    return got, stt


def check_beyond(make_engine, tag, pool, word, engine=None):
    """a call one beyond a limit: the window rounds, exactly this refusal word, the oracle's results"""
    jobs, offers, groups = pool.jobs(), pool.offers(), pool.groups
    p3 = A.default_params(**P3)
    if engine is None:
        with make_engine(p3) as e:
            got, stt = call(e, jobs, offers, groups)
    else:
        got, stt = call(engine, jobs, offers, groups)
    print(tag, "beyond: K", pool.K, "M", pool.M, "form", stt["placement_form"], "refused", hex(stt["classfit_refused"]))
    assert stt["placement_form"] == 0 and stt["classfit_refused"] == word, (tag, stt["placement_form"], hex(stt["classfit_refused"]), "expected", hex(word))
    _same(tag, got, pyoracle.match(p3, jobs, offers, groups, ()), "the oracle")
    return got, stt


# ---- the pairs: name -> (at-limit pools, beyond-limit pools with their words) ----------------------------------------------------------------------
def pair_classes():
    """48 distinct (Tc, Tm) | 49: cf_prepare's `nc >= CF_MAXCLS`"""
    return [("48 classes", build_pool(plain(48, 20), 1, hold_cls=[47]))], [("49 classes", build_pool(plain(49, 20), 1, hold_cls=[48]), X_SHAPE)]


def _kinds(n_sig, seed=2):
    sigs = [sig(1 + i // 8, 1 + i % 8) for i in range(n_sig)]
    cl = plain(3, 100, tc0=32.0, step=32.0) + [(64.0, 262144.0, s, 6) for s in sigs]
    pool = build_pool(cl, seed, hold_cls=[2])
    for s in (sigs[0], sigs[n_sig // 2], sigs[-1], sigs[-1], sig(5, 1)):  # gpu jobs of the first, a middle and the LAST kind of the table, and of no kind
        pool.add_jobs([2.0], 2048.0, gpus=s[1], model=s[0], at=30)
    return pool


def pair_kinds():
    """31 (model, count) signatures beside hosts without gpus = 32 kinds | 32 signatures: cf_prepare's `nk >= CF_MAXKIND`"""
    return [("31 signatures + plain", _kinds(31))], [("32 signatures + plain", _kinds(32), X_SHAPE)]


def pair_one_class():
    """a class of 4096 members = 64 chunks, every lane of its wave | 4097: `(s_cnt[c] + 63) / 64 > 64`"""
    return ([("a class of 4096", build_pool([(64.0, 262144.0, None, 4096)], 3, hold_cls=[0]))],
            [("a class of 4097", build_pool([(64.0, 262144.0, None, 4097)], 3, hold_cls=[0]), X_SHAPE)])


def _wave_load(n2):
    cl = [(64.0, 262144.0, sig(1, 4), 2048), (96.0, 393216.0, sig(1, 4), n2), (32.0, 131072.0, None, 200)]
    return build_pool(cl, 4, hold_cls=[0, 1], n_hold=2)  # the holders are gpu hosts of both classes: gpu jobs ask for TOP


def pair_wave_load():
    """two gpu classes of ONE kind, 2048 members each: 64 chunks together on the gpu wave | 2048 + 2049: `load[wsel] > 64`"""
    return [("gpu classes of 2048 + 2048", _wave_load(2048))], [("gpu classes of 2048 + 2049", _wave_load(2049), X_SHAPE)]


def _offers_pool(M):
    ns = [2048, 2048, 2048, M - 3 * 2048]
    cl = [(32.0 + 32.0 * i, (32.0 + 32.0 * i) * 4096.0, None, n) for i, n in enumerate(ns)]
    return build_pool(cl, 5, hold_cls=[3], last_is_holder=True)


def pair_offers():
    """8192 offers, and offer 8191 (thirteen one bits in the sort key) is a holder of TOP | 8193: cf_setup's own check"""
    return [("8192 offers", _offers_pool(8192))], [("8193 offers", _offers_pool(8193), X_HOST)]


def _groups(G, members, seed=6):
    pool = build_pool(plain(2, 150, tc0=32.0, step=32.0), seed, hold_cls=[1])
    K0 = pool.K
    a = pool.add_jobs(np.full(members, 1.0), 512.0, at=K0 - 20)  # one group's members: small jobs that would share a host if they might
    pool.j["group"][a] = 7
    b = pool.add_jobs(np.full(3, 1.0), 512.0)
    pool.j["group"][b] = min(G, 4096) - 1  # the last group of a full table, with pending members and a running cotask
    run = [[] for _ in range(G)]
    run[7], run[min(G, 4096) - 1], run[1] = [int(pool.holders[0]), 5], [0, 1, 2], [3]
    pool.groups = A.Groups(type=np.ones(G, dtype=np.uint8), run_hosts=run)
    return pool


def pair_groups():
    """4096 unique groups, the last with pending members, and a group of 16 pending members | 4097 groups: cf_setup's own check; 17 members:
    cf_pack_jobs' `slot < CF_GMEM`"""
    return ([("4096 groups, 16 members", _groups(4096, 16))],
            [("4097 groups", _groups(4097, 16), X_HOST), ("17 members", _groups(4096, 17), X_GROUP)])


def _fixed_cpus(frac):
    pool = build_pool([(32.0, 131072.0, None, 150), (16.0, 65536.0, None, 150)], 7, hold_cls=[0])
    x = int(np.setdiff1d(np.arange(pool.M), pool.holders)[5])
    pool.o["cpus"][x] += frac  # (the totals stay: a class is its totals)
    pool.o["run_cpus"][x] -= frac
    return pool


def pair_fixed_cpus():
    """cpus as multiples of 2^-20 (Tc = 32 is 2^25 units, Tm = 2^17: 2 Tc Tm = 2^43) | a multiple of 2^-21: `kc > 20`"""
    return [("cpus in 2^-20", _fixed_cpus(2.0 ** -20))], [("cpus in 2^-21", _fixed_cpus(2.0 ** -21), X_NUMBERS)]


def _wide(tc, tm):
    return build_pool([(tc, tm, None, 150), (64.0, 262144.0, None, 150)], 8, hold_cls=[0])


def pair_sort_key():
    """mem up to 2^30 - 1 with whole MiB, and with it Tc = 2^14: 2 Tc Tm = 2^45 - 2^15, the greatest E the 58-bit sort key holds |
    mem 2^30: `value * 2^k < 2^30`; Tc = 2^14 + 1: `2 Tc Tm < 2^45`"""
    return ([("Tc 2^14, Tm 2^30 - 1", _wide(16384.0, 2.0 ** 30 - 1))],
            [("Tm 2^30", _wide(16384.0, 2.0 ** 30), X_NUMBERS), ("Tc 2^14 + 1", _wide(16385.0, 2.0 ** 30 - 1), X_SHAPE)])


def _levels(roles, fill=(), cs=1.0, quarter=False):
    pool = build_pool(plain(2, 150, tc0=32.0, step=32.0), 9, hold_cls=[1], roles=roles, fill=fill, cs=cs)
    if quarter:
        x = int(np.setdiff1d(np.arange(pool.M), pool.holders)[5])
        pool.o["cpus"][x] += 0.25
        pool.o["run_cpus"][x] -= 0.25
    return pool


def pair_levels():
    """eight evenly spaced cpus values (1..8; 0.5..4.0), two values, one value, and {1, 2, 4} with whole cpus (the levels 1 1 1 2 2 3 3 4) |
    a ninth value (1 + floor(8 i / 7) skips 8); {1, 2, 4} with a quarter cpu in the call (levels 4 5 7 9 10 12 14 16 quarters: 2.0 is missing)"""
    f8 = tuple(range(1, 9)) * 2
    return ([("1..8", _levels((1.0, 2.0, 8.0), f8)), ("0.5..4.0", _levels((1.0, 2.0, 8.0), f8, cs=0.5)), ("two values", _levels((2.0, 2.0, 8.0))),
             ("one value", _levels((2.0, 2.0, 2.0))), ("1 2 4, whole cpus", _levels((1.0, 2.0, 4.0)))],
            [("1..9", _levels((1.0, 2.0, 8.0), tuple(range(1, 10)) * 2), X_LEVELS), ("1 2 4, quarter cpus", _levels((1.0, 2.0, 4.0), quarter=True), X_LEVELS)])


def _equals(extra):
    pool = build_pool(plain(2, 150, tc0=32.0, step=32.0), 10, hold_cls=[1])
    M = pool.M
    a = np.zeros((M, 8), dtype=np.uint32)
    a[:, 0] = 1 + np.arange(M) % 2
    a[:, 6] = 1000 + np.arange(M)                         # >= 256, under a key no job names
    a[:, 7] = np.array([255, 254, 127])[np.arange(M) % 3]  # 254 / 127: one bit / the top bit away from 255
    pool.o["attr"] = a
    eq = pool.j["equals"]
    for q in range(12, pool.K - 30, 4):
        eq[q] = [[(7, 255)], [(7, 254), (0, 1)], [(7, 255), (0, 2)], [(7, 3)]][(q // 4) % 4]  # (7, 3): no host has it
    if extra:
        eq[40] = [extra]
    return pool


def pair_equals():
    """EQUALS on key 7 with value 255, and offer attributes >= 256 under a key no job names | a job's value 256, a job's key 8:
    cf_scan's `eq_key >= 8 || eq_val >= 256`; an offer value >= 256 under a key a job names: cf_prepare's attr_max check"""
    return ([("key 7, value 255", _equals(None))],
            [("value 256", _equals((7, 256)), X_JOB_SLOW), ("key 8", _equals((8, 1)), X_JOB_SLOW), ("a named key with values >= 256", _equals((6, 5)), X_OFFER)])


def _novel(n):
    """every seventh opener has run before on the host the oracle gives it otherwise (so the constraint moves it), on a host with no offer in
    the call below max_host and on one beyond max_host; the 4th / 5th entries are other hosts of the call"""
    pool = build_pool(plain(2, 150, tc0=32.0, step=32.0), 11, hold_cls=[1])
    pool.o["host"] = (2 * np.arange(pool.M)).astype(np.uint32)  # odd ids: hosts without an offer
    base = pyoracle.match(A.default_params(**P3), pool.jobs(), pool.offers(), None, ())[0]
    host = pool.o["host"]
    for q in range(14, pool.K - 30, 7):
        if base[q] >= 0:
            pool.j["novel"][q] = [int(host[base[q]]), 2 * (q % 100) + 1, 5000 + q] + [int(host[(3 * q + 17 * x) % pool.M]) for x in range(n - 3)]
    return pool


def pair_novel():
    """4 novel hosts per job, some without an offer in the call | 5: the job's constraints leave the fast slots"""
    return [("4 novel hosts", _novel(4))], [("5 novel hosts", _novel(5), X_JOB_SLOW)]


def _host_ids(over):
    pool = build_pool(plain(2, 150, tc0=32.0, step=32.0), 12, hold_cls=[1])
    top = 8 * pool.M + 65536 + over
    pool.o["host"][pool.holders[-1]] = top  # the host -> offer table's last entry is one that gets placed on
    pool.j["novel"][20] = [top, 3]
    return pool


def pair_host_ids():
    """the greatest host id 8 M + 65536 | one more: cf_setup's own check"""
    return [("max_host 8 M + 65536", _host_ids(0))], [("max_host 8 M + 65537", _host_ids(1), X_HOST)]


def _cotasks(S):
    """ONE unique group whose running cotasks + pending members are S: 10 pending members, S - 10 running cotasks, five of them on hosts of the
    call and the others on hosts without an offer (beyond max_host).  M = 300 and G = 1: the LDS sum stays far below its limit (2 S bytes of
    about 140 KiB), so what decides is the 16-bit offset limit alone"""
    pool = build_pool(plain(2, 150, tc0=32.0, step=32.0), 17, hold_cls=[1])
    a = pool.add_jobs(np.full(10, 1.0), 512.0, at=pool.K - 20)
    pool.j["group"][a] = 0
    run = [3, 40, 77, 150, 299] + list(range(100000, 100000 + S - 10 - 5))
    pool.groups = A.Groups(type=np.ones(1, dtype=np.uint8), run_hosts=[run])
    return pool


def pair_cotasks():
    """60000 running cotasks + pending members (the group table's offsets are 16 bits) | 60001: cf_setup's `S > 60000`, behind the set-up launches:
    CF_X_SHAPE"""
    return [("S = 60000", _cotasks(60000))], [("S = 60001", _cotasks(60001), X_SHAPE)]


PAIRS = {"classes": pair_classes, "kinds": pair_kinds, "one_class": pair_one_class, "wave_load": pair_wave_load, "offers": pair_offers,
         "groups": pair_groups, "fixed_cpus": pair_fixed_cpus, "sort_key": pair_sort_key, "levels": pair_levels, "equals": pair_equals,
         "novel": pair_novel, "host_ids": pair_host_ids, "cotasks": pair_cotasks}


def run_pair(make_engine, name, at=True, beyond=True):
    ats, beyonds = PAIRS[name]()
    for tag, pool in ats if at else ():
        check_at(make_engine, f"{name}: {tag}", pool)
    for tag, pool, word in beyonds if beyond else ():
        check_beyond(make_engine, f"{name}: {tag}", pool, word)


# ---- the smallest calls ------------------------------------------------------------------------------------------------------------------------------
def smallest(which):
    if which == "1x1":
        pool = build_pool([(32.0, 131072.0, None, 1)], 13, hold_cls=[0], n_hold=1)
        pool.j = {k: v[:1] for k, v in pool.j.items()}
    elif which == "1x8192":  # one job that asks for TOP: its offer is one of three among 8192
        pool = _offers_pool(8192)
        q = int(pool.askers[0])
        pool.j = {k: v[q:q + 1] for k, v in pool.j.items()}
    else:  # "65x1": two batches on one offer, the second of one job; eight jobs find room
        pool = build_pool([(32.0, 131072.0, None, 1)], 13, hold_cls=[0], n_hold=1)
        pool.j = {k: v[:0] for k, v in pool.j.items()}
        pool.add_jobs(np.full(65, 1.0), 512.0)
    pool.askers = np.zeros(0, dtype=np.int64)
    return pool


SMALLEST = ["1x1", "1x8192", "65x1"]


def run_smallest(make_engine, which):
    pool = smallest(which)
    got, stt = check_at(make_engine, f"smallest {which}", pool, capacity=False)
    assert stt["cf_batches"] == (pool.K + 63) // 64
    if which == "1x8192":
        assert got[0][0] in pool.holders
    elif which == "65x1":
        assert (got[0] >= 0).sum() == 8
    else:
        assert got[0][0] == 0


# ---- stale state: the engine's cf_* buffers only grow, and cf_init clears by the current call's sizes ------------------------------------------
STALE = ["classes", "one_class", "offers"]


def run_stale(make_engine, name):
    """on ONE engine: the at-limit call, a small call, the call beyond the limit, the at-limit call again"""
    ats, beyonds = PAIRS[name]()
    (tag, at), (btag, beyond, word) = ats[0], beyonds[0]
    small = build_pool(plain(2, 30), 14, hold_cls=[1], n_open=46)  # K = 70, M = 60
    assert small.K == 70 and small.M == 60
    with make_engine(A.default_params(**P3)) as e:
        _, st1 = check_at(make_engine, f"stale {name}: {tag}", at, engine=e)
        check_at(make_engine, f"stale {name}: small", small, capacity=False, engine=e)
        check_beyond(make_engine, f"stale {name}: {btag}", beyond, word, engine=e)
        _, st2 = check_at(make_engine, f"stale {name}: {tag} again", at, engine=e)
    assert st1["cf_walked"] == st2["cf_walked"], (name, st1["cf_walked"], st2["cf_walked"])


# ---- the LDS sum: a sweep, not a pair (sizeof(CfFixed) differs between builds: the turning point is not asserted) ---------------------------------
def _sweep(make_engine, tag, xs, make):
    """make(x) -> pool, for growing x: every call equals the oracle, is form 3 or refused with CF_X_SHAPE alone, stays refused once refused, both
    sides occur, and the walk never finds its tables larger than the host's sum let through"""
    forms = []
    p3 = A.default_params(**P3)
    for x in xs:
        pool = make(x)
        jobs, offers, groups = pool.jobs(), pool.offers(), pool.groups
        with make_engine(p3) as e:
            try:
                got, stt = call(e, jobs, offers, groups)
            except Exception as err:  # (any other error fails the test too: re-raised)
                assert WALK_ERROR not in str(err), (tag, x, "the host's LDS sum and the kernel's disagree", str(err))
                raise
        print(tag, x, "K", pool.K, "M", pool.M, "form", stt["placement_form"], "refused", hex(stt["classfit_refused"]))
        assert (stt["placement_form"], stt["classfit_refused"]) in ((3, 0), (0, X_SHAPE)), (tag, x, stt["placement_form"], hex(stt["classfit_refused"]))
        _same(f"{tag} {x}", got, pyoracle.match(p3, jobs, offers, groups, ()), "the oracle")
        forms.append(stt["placement_form"])
    assert forms == sorted(forms, reverse=True), (tag, "once refused, every larger input is refused", list(zip(xs, forms)))
    assert forms[0] == 3 and forms[-1] == 0, (tag, "both sides occur", list(zip(xs, forms)))


def _equals_at(M):
    ns = [2048, 2048, 2048, M - 3 * 2048]
    pool = build_pool([(32.0 + 32.0 * i, (32.0 + 32.0 * i) * 4096.0, None, n) for i, n in enumerate(ns)], 15, hold_cls=[3], n_open=60, last_is_holder=True)
    a = np.zeros((M, 2), dtype=np.uint32)
    a[:, 0] = 1 + np.arange(M) % 3
    a[:, 1] = 1 + np.arange(M) % 250
    pool.o["attr"] = a
    for q in range(12, pool.K, 5):
        pool.j["equals"][q] = [(0, 1 + q % 3)] if q % 2 else [(1, 1 + q % 250)]
    return pool


EQUALS_SWEEP = list(range(8000, 8193, 64))


def run_sweep_equals(make_engine, xs=EQUALS_SWEEP):
    """EQUALS jobs bring the offers' attribute bytes into LDS, 8 bytes an offer: the tables of 8192 offers no longer fit"""
    _sweep(make_engine, "LDS sum, EQUALS over M", xs, _equals_at)


GROUPS_SWEEP = [20000, 40000, 43000, 44000, 44400, 44500, 44600, 44800, 46000, 59000, 60000, 60001, 62000]


def _groups_at(S):
    """M = 4096, G = 4096 unique groups EVERY one of which has a pending member (the kernel's sum counts the groups with pending members, the
    host's all of them: so they are the same sum); S = running cotasks + pending members"""
    pool = build_pool([(64.0, 262144.0, None, 2048), (96.0, 393216.0, None, 2048)], 16, hold_cls=[1], n_open=60)
    G = 4096
    g = pool.add_jobs(np.full(G, 1.0), 512.0, at=pool.K - 8)
    pool.j["group"][g] = np.arange(G, dtype=np.uint32)
    n_run = S - G
    rng = np.random.default_rng(S)
    per = np.full(G, n_run // G)
    per[: n_run % G] += 1
    hosts = rng.integers(0, pool.M, n_run)
    off = np.concatenate([[0], np.cumsum(per)])
    pool.groups = A.Groups(type=np.ones(G, dtype=np.uint8), run_hosts=[hosts[off[x]:off[x + 1]].tolist() for x in range(G)])
    return pool


def run_sweep_groups(make_engine, xs=GROUPS_SWEEP):
    """unique groups with running cotasks: 2 bytes of LDS per cotask and pending member.  (At M = G = 4096 the LDS sum refuses from about
    S = 44500 on, so the points past 60000 are refused by it either way: `S > 60000` itself is the cotasks pair's.)"""
    _sweep(make_engine, "LDS sum, cotasks + members", xs, _groups_at)


# ---- more pools than one cf_walk launch holds (cf_run packs CF_PACK = 8 pools a launch), at mixed states -------------------------------------------
CF_PACK = 8  # classfit.hpp


def many_pools():
    """-> (pools, what each must report: (placement_form, classfit_refused), None where the pool has no pending job).  cf_run is handed only the
    pools whose set-up succeeded: of the twelve below the one beyond a limit and the one without a pending job are not among them, so TEN walk —
    a full pack of eight and a second launch of two, padded with copies of its first pool; the pools at a limit and with K = 1 sit in the first
    pack, small ones in the second"""
    mk = lambda i, n_pending, n_offers, **kw: synth.make_pool(seed=0x9B00 + i, n_pending=n_pending, n_running=60, n_users=12, n_offers=n_offers, **kw)
    at, beyond = pair_classes()
    pools = [dataclasses.replace(mk(0, 400, 960), offers=at[0][1].offers()),       # at a limit: 48 classes
             dataclasses.replace(mk(1, 300, 980), offers=beyond[0][1].offers()),   # one class beyond: refused
             mk(2, 0, 40),                                                         # no pending job
             mk(3, 1, 40),                                                         # K = 1
             mk(4, 150, 50), mk(5, 260, 90, constraints=True), mk(6, 70, 33), mk(7, 330, 120, constraints=True), mk(8, 200, 64),
             mk(9, 120, 45), mk(10, 90, 70, constraints=True), mk(11, 65, 20)]
    expect = [(3, 0), (0, X_SHAPE), None] + [(3, 0)] * 9
    return pools, expect


def run_many_pools(make_engine):
    """twelve pools through cook_cycle_run_rank_multi + cook_cycle_match_multi, two cycles on the resident inputs: every pool equals the oracle in
    both, the eligible ones are placed by the class-ordered form — more of them than one cf_walk launch holds —, the one beyond a limit is refused
    with its word"""
    pools, expect = many_pools()
    _, stats = P.multi_pool_parity(make_engine, pools, A.default_params(**P3), k=10 ** 9, cycles=2, with_stats=True)
    for cyc, per in enumerate(stats):
        said = [(st["placement_form"], st["classfit_refused"]) for st in per]
        print("many pools, cycle", cyc, said)
        for pi, (got, want) in enumerate(zip(said, expect)):
            assert want is None or got == want, (cyc, pi, got, want)
        assert sum(1 for pi, got in enumerate(said) if got[0] == 3 and expect[pi] is not None) > CF_PACK, (cyc, said)
