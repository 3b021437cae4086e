"""Rounding traps for every fp64 sum that claims to equal the reference's left-to-right sum, shared by the emulator
(test_sum_order_emu.py) and GPU (test_sum_order_gpu.py) suites.

A parallel sum equals the sequential one only if every prefix of the left-to-right order is exact (cook_amd/csrc/common.hpp).
The inputs here are built so that it is not: a "big" value B and half-ulp values h = ulp(B)/2 placed so that two halves meet
in the same partial sum of a kernel's layout.  Left to right, B + h rounds back to B (ties to even: every B here has an even
last significand bit) and so does the next + h: the sum is B.  A tree that adds h + h = 2h first and then B + 2h = B + ulp(B)
does not round at all, so a TwoSum check of its own additions sees nothing.  Integer-valued inputs (every order exact) and
0.1-step inputs (some tree addition rounds, the fallback runs) never reach that case; these do.

Every comparison is of bit patterns (int64 views), so -0.0 against +0.0 or B against B + ulp(B) is a failure.  The generator
stays here: synth.make_pool's defaults feed bench.py."""
from __future__ import annotations

import numpy as np

from cook_amd import _abi as A
from cook_amd import synth
from cook_amd.engine import rank_pool_usage_multi, user_stats_multi
from oracle import pyoracle
from tests import autoscale_cases as AS
from tests import user_stats_oracle as O

# big values: powers of two, 3 * 2^k, a value with a fraction, magnitudes of real mem columns (MiB, 2^16 .. 2^30)
BIGS_CPUS = [1.0, 3.0 * 2.0 ** 4, 1000.5, 0.75]
BIGS_MEM = [65536.0, 3.0 * 2.0 ** 20, 2.0 ** 30, 1000.5 * 2.0 ** 10]

# the launch shapes the placements are derived from (rank_kernels.hpp, scan.hpp, considerable_kernels.hpp)
POOL_THREADS, POOL_BLOCKS = 256, 64    # pool_usage_partial: thread t of block b folds i = b*256 + t, + 64*256, ...
POOL_STRIDE = POOL_THREADS * POOL_BLOCKS
SS_IPT, SS_TILE = 4, 1024              # seg_scan: 4 items per thread, 1024 items per block
CONS_THREADS = 1024                    # cons_pool_usage: thread t folds users t, t + 1024, ...


def half(b):
    """h = ulp(b) / 2: b + h rounds to b (b's last significand bit is even), h + h = ulp(b) is exact, and so is b + ulp(b)"""
    h = float(np.spacing(b)) / 2.0
    assert b + h == b and b + 2 * h != b and (b + h) + h == b
    return h


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def assert_bits(got, want, what):
    g, w = bits(got), bits(want)
    bad = np.flatnonzero(g.ravel() != w.ravel())
    assert len(bad) == 0, f"{what}: bit patterns differ at {bad[:6].tolist()}: got {np.ravel(got)[bad[:3]].tolist()} " \
                          f"want {np.ravel(want)[bad[:3]].tolist()}"


def trap_column(n, big, at_big, at_half, rest=0.0):
    x = np.full(n, rest, dtype=np.float64)
    x[at_half] = half(big)
    x[at_big] = big
    return x


def tasks_of(cpus, mem, user, pending, gpus=None):
    """per-user order = input order: priorities fall with the index (tools.clj:614-641 sorts by -priority first)"""
    n = len(cpus)
    pending = np.asarray(pending, dtype=np.uint8)
    return A.Tasks(cpus=np.asarray(cpus, np.float64), mem=np.asarray(mem, np.float64), user=np.asarray(user, np.uint32),
                   priority=(1_000_000 - np.arange(n)).astype(np.int32), start_ms=np.where(pending == 1, 0, 1_000).astype(np.int64),
                   task_id=(10_000 + np.arange(n)).astype(np.int64), job_id=(100 + np.arange(n)).astype(np.int64), pending=pending,
                   gpus=None if gpus is None else np.asarray(gpus, np.float64))


def users_of(n, div=1.0, **quota):
    return A.Users(div_cpus=np.full(n, div), div_mem=np.full(n, div), **{k: np.full(n, float(v)) for k, v in quota.items()})


# ---- pool usage (pool_usage_partial / pool_usage_reduce) ---------------------------------------------------------------------
def pool_usage_placements():
    """(name, n, index of B, indices of the halves), all tasks running"""
    return [
        # the issue's vector: lanes 1 and 3 meet at the butterfly's d = 2 (2h exact), lane 0 (B) meets them at d = 1 (B + 2h
        # exact); left to right B + h rounds at index 1
        ("xor-d2", 4, 0, [1, 3]),
        # lanes 5 and 37 meet at d = 32, the butterfly's first step, long before lane 0
        ("xor-d32", 64, 0, [5, 37]),
        # wave 1 of block 0: lanes 64 and 96 meet at d = 32, then ws[0] (B) + ws[1] (2h) in the block's fold
        ("cross-wave", 256, 0, [64, 96]),
        # block 1: threads 256 and 288 meet at d = 32, then part[0] (B) + part[1] (2h) in pool_usage_reduce
        ("cross-block", 600, 0, [256, 288]),
        # one thread's strided slice: items 1 and 1 + 64*256 are folded by the same thread (2h) before any other partial sum
        ("one-thread-stride", POOL_STRIDE + 100, 0, [1, 1 + POOL_STRIDE]),
        # a control: the halves come BEFORE B, so left to right h + h = 2h and 2h + B are exact too; every order gives B + ulp(B)
        ("halves-first", 64, 40, [1, 3]),
    ]


def pool_usage_tasks(n, at_big, at_half, big_c, big_m, pending_every=0):
    cpus = trap_column(n, big_c, at_big, at_half)
    mem = trap_column(n, big_m, at_big, at_half)
    gpus = trap_column(n, 4.0, at_big, at_half)
    pend = np.zeros(n, np.uint8)
    if pending_every:  # pending tasks carry values the sum must skip
        idx = np.setdiff1d(np.arange(n)[::pending_every], np.r_[at_big, at_half])
        pend[idx] = 1
        cpus[idx], mem[idx], gpus[idx] = 7.0, 3.0, 1.0
    return tasks_of(cpus, mem, np.arange(n) % 7, pend, gpus)


def random_pool_usage_tasks(seed, n):
    """seeded placements: one B per column, 2-6 halves, zeros, some pending tasks, occasional -0.0 and negatives"""
    rng = np.random.default_rng(seed)
    cols = []
    for big in (BIGS_CPUS[seed % len(BIGS_CPUS)], BIGS_MEM[seed % len(BIGS_MEM)], 8.0):
        pos = rng.choice(n, size=1 + int(rng.integers(2, 7)), replace=False)
        x = trap_column(n, big, pos[0], pos[1:])
        if seed % 3 == 0:
            x[rng.choice(n, size=3, replace=False)] = -0.0
        if seed % 4 == 1:  # a cancelling pair: -B somewhere behind B
            x[rng.integers(0, n)] = -big
        cols.append(x)
    pend = (rng.random(n) < 0.2).astype(np.uint8)
    return tasks_of(cols[0], cols[1], rng.integers(0, 50, n), pend, cols[2])


def _usage_bits(u):
    return np.array(u.as_tuple() if hasattr(u, "as_tuple") else u, dtype=np.float64)


def check_pool_usage(make_engine, tasks, what):
    want = _usage_bits(pyoracle.pool_usage(tasks))
    with make_engine(A.default_params()) as e:
        e.rank_stage(tasks, users_of(int(tasks.user.max()) + 1))
        assert_bits(_usage_bits(e.rank_pool_usage()), want, what)
    return want


def check_pool_usage_cases(make_engine):
    for name, n, b, hs in pool_usage_placements():
        for bc, bm in zip(BIGS_CPUS, BIGS_MEM):
            for pe in (0, 5):
                check_pool_usage(make_engine, pool_usage_tasks(n, b, hs, bc, bm, pe), f"{name} B={bc}/{bm} pending_every={pe}")
    # all zeros, -0.0 among them (left to right from +0.0: +0.0), and a sum that cancels to zero
    z = np.array([-0.0, 0.0, -0.0, -0.0])
    check_pool_usage(make_engine, tasks_of(z, z, [0] * 4, [0] * 4, z), "signed zeros")
    c = np.array([3.0, half(3.0), -3.0, half(3.0)])
    check_pool_usage(make_engine, tasks_of(c, c, [0] * 4, [0] * 4), "cancellation")


def check_pool_usage_random(make_engine, seeds, n):
    for s in seeds:
        check_pool_usage(make_engine, random_pool_usage_tasks(s, n), f"random seed {s} n {n}")


def check_pool_usage_multi(make_engine):
    """cook_rank_pool_usage_multi: several pools' sums in one call, each a trap of its own layout"""
    pools = [pool_usage_tasks(n, b, hs, BIGS_CPUS[i % 4], BIGS_MEM[i % 4]) for i, (_, n, b, hs) in enumerate(pool_usage_placements())]
    engines = [make_engine(A.default_params()) for _ in pools]
    try:
        for e, t in zip(engines, pools):
            e.rank_stage(t, users_of(7))
        got = rank_pool_usage_multi(engines)
        for i, (g, t) in enumerate(zip(got, pools)):
            assert_bits(_usage_bits(g), _usage_bits(pyoracle.pool_usage(t)), f"multi pool {i}")
    finally:
        for e in engines:
            e.close()


def quota_flip_pool(n_running=4, at_half=(1, 3)):
    """the issue's case: user 0's running cpus [1, h, 0, h] (left to right 1.0, a tree 1 + 2^-52) and a pending 0.5-cpu job of user 1
    under pool_quota(cpus=1.5) with the pool usage computed: left to right 1.0 + 0.5 <= 1.5 keeps the job, 1.5 + 2^-52 would not"""
    cpus = trap_column(n_running, 1.0, 0, list(at_half))
    cpus = np.r_[cpus, 0.5]
    mem = np.r_[np.full(n_running, 10.0), 10.0]
    user = np.r_[np.zeros(n_running, int), 1]
    pend = np.r_[np.zeros(n_running, int), 1]
    return tasks_of(cpus, mem, user, pend)


def check_rank_pool_quota(make_engine):
    p = A.default_params()
    for n_running, hs in ((4, (1, 3)), (POOL_STRIDE + 10, (1, 1 + POOL_STRIDE))):
        t = quota_flip_pool(n_running, hs)
        q = A.pool_quota(pool_quota=A.quota(cpus=1.5))
        want, want_dru = pyoracle.rank(p, t, users_of(2), quota=q)
        assert len(want) == 1  # the oracle keeps the job
        with make_engine(p) as e:
            got, dru = e.rank(t, users_of(2), quota=q)
        assert np.array_equal(got, want), (n_running, got, want)
        assert_bits(dru, want_dru, "dru")


def check_cycle_pool_quota(make_engine):
    """the same sum inside a cycle (cook_cycle_run_rank seeds the pool-quota filter with rank_pool_usage)"""
    p = A.default_params(good_enough_fitness=1.0)
    base = synth.make_pool(seed=5, n_pending=1, n_running=0, n_users=2, n_offers=4)
    t = quota_flip_pool()
    base.pending_jobs.cpus[:] = 0.5
    base.pending_jobs.mem[:] = 10.0
    q = A.pool_quota(pool_quota=A.quota(cpus=1.5))
    want, _ = pyoracle.rank(p, t, users_of(2), quota=q)
    with make_engine(p) as e:
        e.cycle_stage(t, users_of(2), base.pending_jobs, base.offers, base.groups)
        e.rank_set_quota(q)
        e.cycle_run(10)
        got, _, _ = e.cycle_fetch()
    assert np.array_equal(got, want), (got, want)


# ---- per-user running usage (seg_scan over the per-user order, user_usage_extract) ------------------------------------------
def user_usage_layouts():
    """(name, per-user lists of (position in the user's segment, value kind)) — kinds: "B", "h", "p" (a pending task), "z" (-0.0)"""
    return [
        # the issue's vector: 80 tasks, B at 0, halves at 4 and 5 — one thread's 4 items (SS_IPT): 4 + 5 = 2h inside the thread,
        # the segment's last prefix B + 2h is exact, the prefix at 4 (B + h) is not
        ("ipt", [(80, {0: "B", 4: "h", 5: "h"})]),
        # a segment longer than a tile: the halves in block 1 meet before the block carry B is added
        ("tile", [(3000, {0: "B", SS_TILE + 6: "h", SS_TILE + 7: "h"})]),
        # the halves in the same wave's shuffle steps (threads 2 and 3 of block 0)
        ("wave", [(64, {0: "B", 2 * SS_IPT: "h", 3 * SS_IPT: "h"})]),
        # pending tasks between them: masked to zero in the scan, skipped by the fold
        ("pending", [(40, {0: "B", 1: "p", 4: "h", 6: "p", 7: "h"})]),
        # users spread over several blocks, each with its trap; an untouched user between them
        ("users", [(700, {0: "B", 8: "h", 9: "h"}), (50, {}), (1500, {3: "B", SS_TILE + 4: "h", SS_TILE + 5: "h"}),
                   (9, {0: "B", 4: "h", 5: "h"})]),
        # -0.0: the fold starts at the first RUNNING task and keeps its -0.0; the scan adds the pending head's +0.0
        ("negzero", [(6, {0: "p", 1: "z", 2: "z", 3: "p", 4: "z", 5: "z"}), (3, {0: "z", 1: "z", 2: "z"})]),
    ]


def user_usage_tasks(layout, big_c, big_m):
    cpus, mem, gpus, user, pend = [], [], [], [], []
    for u, (length, marks) in enumerate(layout):
        for k in range(length):
            kind = marks.get(k)
            pend.append(1 if kind == "p" else 0)
            user.append(u)
            v = {"B": (big_c, big_m, 2.0), "h": (half(big_c), half(big_m), half(2.0)), "z": (-0.0, -0.0, -0.0),
                 "p": (5.0, 5.0, 5.0)}.get(kind, (0.0, 0.0, 0.0))
            cpus.append(v[0]), mem.append(v[1]), gpus.append(v[2])
    return tasks_of(cpus, mem, user, pend, gpus)


def random_user_usage_tasks(seed, n_users, n):
    rng = np.random.default_rng(seed)
    user = np.sort(rng.integers(0, n_users, n))  # (input order = per-user order: priorities fall with the index)
    big_c, big_m = BIGS_CPUS[seed % 4], BIGS_MEM[seed % 4]
    cpus, mem = np.zeros(n), np.zeros(n)
    for u in range(n_users):
        idx = np.flatnonzero(user == u)
        if len(idx) < 3:
            continue
        pos = rng.choice(idx, size=min(len(idx), 1 + int(rng.integers(2, 5))), replace=False)
        cpus[pos[0]], mem[pos[0]] = big_c, big_m
        cpus[pos[1:]], mem[pos[1:]] = half(big_c), half(big_m)
    pend = (rng.random(n) < 0.25).astype(np.uint8)
    return tasks_of(cpus, mem, user, pend)


def check_user_usage(make_engine, tasks, n_users, what, device=False):
    want = pyoracle.user_usage(tasks, n_users)
    with make_engine(A.default_params()) as e:
        e.rank_stage(tasks, users_of(n_users))
        e.rank_run()
        got = e.rank_user_usage(n_users)
        assert_bits(got, want, what)
        if device:
            import torch
            buf = torch.full((n_users, 3), 7.0, dtype=torch.float64, device="cuda")
            e.rank_user_usage(n_users, device_ptr=buf.data_ptr())
            torch.cuda.synchronize()
            assert_bits(buf.cpu().numpy(), want, what + " (device_ptr)")


def check_user_usage_cases(make_engine, device=False):
    for name, layout in user_usage_layouts():
        for bc, bm in zip(BIGS_CPUS, BIGS_MEM):
            check_user_usage(make_engine, user_usage_tasks(layout, bc, bm), len(layout), f"{name} B={bc}/{bm}", device)


def check_user_usage_random(make_engine, seeds, n_users, n, device=False):
    for s in seeds:
        check_user_usage(make_engine, random_user_usage_tasks(s, n_users, n), n_users, f"random seed {s}", device)


# ---- cook_rank: DRU prefixes, over-quota counting, pool and group queue-quota prefixes ------------------------------------------
def rank_trap_pool(seed, n_users, per_user, big_c, big_m):
    """every user: B running first, halves on running tasks of the same thread / tile, then pending tasks of h or 0 whose DRU is
    the prefix B (+ h ...) — left to right B, a tree B + ulp"""
    rng = np.random.default_rng(seed)
    cpus, mem, user, pend = [], [], [], []
    for u in range(n_users):
        L = per_user if u % 3 else per_user * 3
        hs = set(rng.choice(np.arange(1, L), size=min(L - 1, 4), replace=False).tolist()) | {SS_IPT, SS_IPT + 1}
        for k in range(L):
            kind = "B" if k == 0 else "h" if k in hs else "0"
            cpus.append(big_c if kind == "B" else half(big_c) if kind == "h" else 0.0)
            mem.append(big_m if kind == "B" else half(big_m) if kind == "h" else 0.0)
            user.append(u)
            pend.append(1 if k > SS_IPT + 1 and rng.random() < 0.6 else 0)
    return tasks_of(cpus, mem, user, pend)


def check_rank_traps(make_engine, seeds=(1, 2, 3), n_users=5, per_user=40):
    for s in seeds:
        bc, bm = BIGS_CPUS[s % 4], BIGS_MEM[s % 4]
        t = rank_trap_pool(s, n_users, per_user, bc, bm)
        # divisors 1: DRU = max(cpus, mem) prefix; user quota exactly B: a prefix of B + ulp would count as over quota
        for params, users in ((A.default_params(), users_of(n_users)),
                              (A.default_params(max_over_quota_jobs=2), users_of(n_users, quota_cpus=bc)),
                              (A.default_params(max_over_quota_jobs=0), users_of(n_users, quota_mem=bm))):
            want, want_dru = pyoracle.rank(params, t, users)
            with make_engine(params) as e:
                got, dru = e.rank(t, users)
            assert np.array_equal(got, want), (s, len(got), len(want))
            assert_bits(dru, want_dru, f"rank dru seed {s}")


def check_rank_queue_quota(make_engine):
    """pool and group queue-quota prefixes (queue_quota_flag): usage B given, pending jobs of h each, quota exactly B.  Left to right
    every prefix is B: all kept; a tree that forms B + 2h from element 0's B + h and a later pair would drop jobs"""
    n = 3000
    cpus = np.full(n, half(1000.5))
    mem = np.full(n, half(2.0 ** 30))
    t = tasks_of(cpus, mem, np.arange(n) % 11, np.ones(n))
    p = A.default_params()
    for q in (A.pool_quota(pool_quota=A.quota(cpus=1000.5, mem=2.0 ** 30), pool_usage=A.usage(count=1, cpus=1000.5, mem=2.0 ** 30)),
              A.pool_quota(group_quota=A.quota(cpus=1000.5), group_usage=A.usage(count=1, cpus=1000.5, mem=1.0))):
        want, _ = pyoracle.rank(p, t, users_of(11), quota=q)
        assert len(want) == n
        with make_engine(p) as e:
            got, _ = e.rank(t, users_of(11), quota=q)
        assert np.array_equal(got, want)


# ---- cook_considerable / cycle considerable / autoscale: the pool usage summed from the users' usage --------------------------------
def cons_state(n_users, usage_cpus, pool_cpus):
    big = np.full(n_users, A.DMAX)
    return A.UserState(quota_count=np.full(n_users, 2.0 ** 31 - 1), quota_cpus=big, quota_mem=big, quota_gpus=big,
                       usage_count=np.ones(n_users), usage_cpus=np.asarray(usage_cpus, np.float64), usage_mem=np.ones(n_users),
                       usage_gpus=np.zeros(n_users), pool_quota=A.quota(cpus=pool_cpus))


def cons_layouts():
    """(name, n_users, index of B, indices of the halves)"""
    return [
        # the issue's vector [1, h, 0, h]: lanes 1 and 3 meet at d = 2
        ("xor-d2", 4, 0, [1, 3]),
        # one thread's stride: users 1 and 1 + 1024 are folded by thread 1 (2h) before anything else
        ("thread-stride", CONS_THREADS + 10, 0, [1, 1 + CONS_THREADS]),
        # waves 1's lanes 64 and 96 meet at d = 32, then ws[0] + ws[1]
        ("cross-wave", 200, 0, [64, 96]),
    ]


def check_considerable(make_engine):
    for name, n, b, hs in cons_layouts():
        usage = trap_column(n, 1.0, b, hs)
        st = cons_state(n, usage, 1.5)
        queue = A.Queue(cpus=np.array([0.5, 0.25]), mem=np.array([1.0, 1.0]), user=np.array([2, 3]))
        want = pyoracle.considerable(queue, st, 10)
        assert list(want[0]) == [0]  # left to right 1.0 + 0.5 <= 1.5: kept; 1.5 + 0.25 is not
        with make_engine(A.default_params()) as e:
            got = e.considerable(queue, st, 10)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), (name, got, want)


def check_cycle_considerable_and_autoscale(make_engine):
    """cook_cycle_set_considerable and cook_cycle_autoscale run the same chain: a pool whose considerable jobs depend on the trap"""
    pool = synth.make_pool(seed=21, n_pending=40, n_running=0, n_users=4, n_offers=2)
    pool.pending_jobs.cpus[:] = 0.5
    pool.tasks.cpus[:] = 0.5
    st = cons_state(4, [1.0, half(1.0), 0.0, half(1.0)], 1.5)
    params = A.default_params(good_enough_fitness=1.0)
    AS.check_against_oracle(make_engine, params, pool, st, 10, None, [dict(max_jobs=5), dict(max_jobs=40, scale_factor=2.0)])


# ---- cook_user_stats / _multi ---------------------------------------------------------------------------------------------------------
def user_stats_trap_pools(n_pools, n_users, seed):
    """traps inside a pool's segment, across pools (a user's B in one pool, halves in others: the us_combine carry) and in the "all"
    rows (B for one user, halves for others); running and waiting columns both"""
    rng = np.random.default_rng(seed)
    out = []
    for p in range(n_pools):
        cpus, mem, user, pend = [], [], [], []
        for u in range(n_users):
            L = int(rng.integers(1, 12)) if u % 5 else SS_TILE + 20
            for k in range(L):
                first = k == 0 and (u + p) % 3 == 0
                h = k in (SS_IPT, SS_IPT + 1, SS_TILE + 2, SS_TILE + 3) or (k == 0 and not first)
                cpus.append(3.0 * 2.0 ** 4 if first else half(3.0 * 2.0 ** 4) if h else 0.0)
                mem.append(2.0 ** 30 if first else half(2.0 ** 30) if h else 0.0)
                user.append(u)
                pend.append(int(rng.random() < 0.5))
        out.append(tasks_of(cpus, mem, user, pend))
    return out


def check_user_stats(make_engine, n_users=9, seed=5):
    pools = user_stats_trap_pools(3, n_users, seed)
    lim = A.UserLimits(share_cpus=np.full(n_users, A.DMAX), share_mem=np.full(n_users, A.DMAX))
    engines = [make_engine(A.default_params()) for _ in pools]
    try:
        for e, t in zip(engines, pools):
            e.rank_stage(t, users_of(n_users))
            e.rank_run()
        for e, t in zip(engines, pools):
            O.assert_same(e.user_stats(lim), O.user_stats([(t, None)], n_users, lim))
        O.assert_same(user_stats_multi(engines, lim), O.user_stats([(t, None) for t in pools], n_users, lim))
    finally:
        for e in engines:
            e.close()

