"""The rank's shared device primitives at their tile and launch-path edges, shared by the emulator (test_sort_scan_edges_emu.py) and GPU
(test_sort_scan_edges_gpu.py) suites: the LSD radix sort and its drivers (cook_amd/csrc/sort.hpp, rank_host.hpp radix_pass /
radix_sort_masked), the segmented scan (scan.hpp, seg_scan), the single-workgroup excl_scan_u32_single and the LDS tile sort of tie groups
(tile_sort.hpp).  Everything goes through the public calls.  Every size is derived from the constants the headers state (read with a
regular expression, the side of a COOK_SHAPE(gpu, emu) the loaded library runs), so a case is "threshold - 1, threshold, threshold + 1"
whatever the constants become, and every case asserts, through set_profiling / kernel_timings, which launch path ran.  The expected
values never come from the engine: a few lines of numpy (the position probe, the per-user cumulative sums) or the oracle."""
from __future__ import annotations

import os
import re
import time
from types import SimpleNamespace

import numpy as np

from cook_amd import _abi as A
from cook_amd import synth
from oracle import pyoracle
from tests import parity_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE = 64
ID_BASE = 17_592_186_044_416
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
SPARSE_BITS = (0, 1, 9, 23, 24, 40, 55, 61)  # digits start inside bytes, and whole bytes in between never vary


# ---- the constants of the headers --------------------------------------------------------------------------------------------------------
def _header(name: str) -> str:
    with open(os.path.join(ROOT, "cook_amd", "csrc", name)) as f:
        return f.read()


def _const(text: str, name: str, ship: bool) -> int:
    m = re.search(rf"\b{name} = (?:COOK_SHAPE\((\d+), (\d+)\)|(\d+));", text)
    assert m, f"{name}: not stated as a number or a COOK_SHAPE pair any more"
    return int(m.group(3)) if m.group(3) is not None else int(m.group(1 if ship else 2))


_SHAPES = {}


def shapes(make_engine) -> SimpleNamespace:
    """the sizes at which the loaded library takes another path"""
    with make_engine(A.default_params()) as e:
        version = e.version
    if version in _SHAPES:
        return _SHAPES[version]
    ship = "shipped launch shapes" in version or "hip gfx950" in version
    sort, scan, tile = _header("sort.hpp"), _header("scan.hpp"), _header("tile_sort.hpp")
    c = {n: _const(sort, n, ship) for n in ("RS_THREADS", "RS_IPL_SMALL", "RS_IPL_LARGE", "RS_FUSED_BLOCKS", "RS_FUSED_BLOCKS_LARGE",
                                             "SCAN1_THREADS", "SCAN1_IPT", "SCAN1_NS")}
    c.update({n: _const(scan, n, ship) for n in ("SS_THREADS", "SS_IPT")})
    c.update({n: _const(tile, n, ship) for n in ("TS_NOMINAL", "TS_CAP")})
    assert "TS_MAX_GROUP = TS_CAP - TS_NOMINAL + 1;" in tile
    s = SimpleNamespace(
        version=version, ship=ship, **c,
        rs_chunk=WAVE * c["RS_IPL_SMALL"],                      # what one wave of a small tile walks
        rs_small=c["RS_THREADS"] * c["RS_IPL_SMALL"],           # the small tile
        rs_large=c["RS_THREADS"] * c["RS_IPL_LARGE"],           # the large tile
        scan_step=c["SCAN1_THREADS"] * c["SCAN1_IPT"],          # excl_scan_u32_single: one step
        ss_tile=c["SS_THREADS"] * c["SS_IPT"],                  # seg_scan: one tile
        ts_max_group=c["TS_CAP"] - c["TS_NOMINAL"] + 1)
    s.rs_fused_small = c["RS_FUSED_BLOCKS"] * s.rs_small        # up to here: small tiles, two launches
    s.rs_fused_large = c["RS_FUSED_BLOCKS_LARGE"] * s.rs_large  # up to here: large tiles, two launches; above: three (radix_scan)
    s.scan_super = s.scan_step * c["SCAN1_NS"]                  # excl_scan_u32_single: one super-step
    s.ss_fused = c["SS_THREADS"] * s.ss_tile                    # up to here seg_scan_propagate_fused, above seg_scan_blocksums
    assert s.rs_fused_small < s.rs_fused_large
    _SHAPES[version] = s
    return s


class Profiled:
    """an engine factory whose engines profile; .tags = kernel_timings() of the engine closed last: {tag: (ms, launches)}"""

    def __init__(self, make_engine):
        self.make_engine, self.tags = make_engine, {}

    def __call__(self, params):
        e = self.make_engine(params)
        e.set_profiling(True)
        close = e.close

        def closing():
            if getattr(e, "_h", None):
                self.tags = e.kernel_timings()
            close()
        e.close = closing
        return e

    def launches(self, tag) -> int:
        return int(self.tags.get(tag, (0.0, 0))[1])


# ---- 1. the per-user order: a position probe ---------------------------------------------------------------------------------------------
PROBE_EDGES = ("wave", "wave_chunk", "small_tile", "fused_small_tiles", "one_more_large_tile")
PROBE_SIZES = ("1", "2") + tuple(f"{b}{d}" for b in PROBE_EDGES for d in ("-1", "", "+1"))
PROBE_SWITCH = ("fused_large_tiles-1", "fused_large_tiles", "fused_large_tiles+1")  # two launches a pass up to there, three (radix_scan) above


def probe_size(sh, name: str) -> int:
    """the tile and path edges of radix_pass, by name.  One off-by-one no case here can tell: `<=` for `<` in radix_pass's FIRST threshold
    moves exactly n = RS_FUSED_BLOCKS small tiles from small fused tiles to large fused tiles.  Both are the two-launch pass under the same
    tags with the same launch counts and the same (stable) result; the grid and the tile are not part of any public observation.  The
    fused_small_tiles trio therefore pins that both shapes are RIGHT at that size, not which one runs."""
    if name.isdigit():
        return int(name)
    base, d = (name[:-2], int(name[-2:])) if name[-2] in "+-" else (name, 0)
    edge = dict(wave=WAVE,                                                      # one ballot step of the scatter
                wave_chunk=sh.rs_chunk,                                         # what one wave of a small tile walks
                small_tile=sh.rs_small,
                fused_small_tiles=sh.rs_fused_small,                            # the last size with small tiles
                one_more_large_tile=(sh.rs_fused_small // sh.rs_large + 1) * sh.rs_large,
                fused_large_tiles=sh.rs_fused_large)[base]
    return edge + d


def _spread(x, bits=SPARSE_BITS):
    """bit k of x -> bit bits[k]"""
    x = np.asarray(x, dtype=np.int64)
    out = np.zeros_like(x)
    for k, b in enumerate(bits):
        out |= ((x >> k) & 1) << b
    return out


def probe_tasks(n: int, kind: str = "mixed", seed: int = 1) -> A.Tasks:
    """ONE user's tasks of cpus = mem = 1: the DRU of a task under divisors of 1 is its 1-based position in the per-user order"""
    rng = np.random.default_rng(seed + 7919 * n)
    pending = (rng.random(n) < 0.5).astype(np.uint8)
    prio = rng.integers(0, 4, n).astype(np.int64)
    start = 1_600_000_000_000 + rng.integers(0, max(2, n // 4), n)  # several tasks per start time: the task id decides among them
    task = ID_BASE + 2_000_000_000 + rng.permutation(n)
    job = ID_BASE + rng.permutation(n)
    if kind == "mixed":
        pass
    elif kind == "sparse_bits":  # ids that differ only in SPARSE_BITS; (priority, id) pairs are unique, with id 0 among them
        assert n <= 2048
        cp, cr = rng.permutation(16 * 256), rng.permutation(4 * 16 * 256)
        cp[np.nonzero(cp == 0)[0][0]], cp[0] = cp[0], 0
        cr[np.nonzero(cr == 0)[0][0]], cr[0] = cr[0], 0
        pending[:2], pending[2:4] = 1, 0
        ip, ir = np.nonzero(pending)[0], np.nonzero(pending == 0)[0]
        prio[ip], job[ip] = cp[:len(ip)] >> 8, ID_BASE + _spread(cp[:len(ip)] & 255)
        prio[ir], task[ir], start[ir] = (cr[:len(ir)] >> 8) & 15, ID_BASE + _spread(cr[:len(ir)] & 255), 1_600_000_000_000 + (cr[:len(ir)] >> 12)
    elif kind == "start_dense":  # all of int64: every bit of key - min varies, the last digit ends exactly at bit 63
        pending[:] = 0
        start = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
        start[:2] = I64_MIN, I64_MAX
    elif kind == "start_high":  # negative to large positive in steps of 2^60: the only digit starts at bit 60 and runs past bit 63
        pending[:] = 0
        k = rng.integers(0, 16, n).astype(np.uint64)
        k[:2] = 0, 15
        start = ((k << np.uint64(60)) ^ np.uint64(1 << 63)).view(np.int64)  # I64_MIN + k * 2^60
    elif kind == "prio_extremes":
        prio = rng.choice([-(2 ** 30 - 1), 0, 2 ** 30 - 1], size=n)
        prio[:3] = -(2 ** 30 - 1), 0, 2 ** 30 - 1
    elif kind == "all_pending":  # word 2 is constant: no pass
        pending[:] = 1
    elif kind == "all_running_one_prio":
        pending[:] = 0
        prio[:] = 50
    elif kind == "one_byte":  # exactly one byte of every word varies: priority, start and job byte 1, task byte 3
        assert n <= 2 ** 15
        c = rng.permutation(2 ** 16)[:n]
        pending[:2], pending[2:4] = 1, 0
        prio = -(c >> 8)
        job = np.where(pending == 1, ID_BASE + ((c & 255) << 8), job)
        task = ID_BASE + ((c & 255) << 24)
        start = 1_600_000_000_000 + (rng.integers(0, 256, n) << 8)
    else:
        raise KeyError(kind)
    one = np.ones(n)
    return A.Tasks(cpus=one, mem=one.copy(), user=np.zeros(n, np.uint32), priority=prio.astype(np.int32), start_ms=start.astype(np.int64),
                   task_id=task.astype(np.int64), job_id=job.astype(np.int64), pending=pending)


PROBE_KINDS = ("sparse_bits", "start_dense", "start_high", "prio_extremes", "all_pending", "all_running_one_prio", "one_byte")


def probe_reference(t: A.Tasks):
    """the per-user order (tools.clj:614-641) of one user: -> (ranked, dru)"""
    pend = t.pending.astype(np.int64)
    k1, k2 = np.where(pend == 1, t.job_id, t.start_ms), np.where(pend == 1, 0, t.task_id)
    order = np.lexsort((k2, k1, pend, -t.priority.astype(np.int64)))
    dru = np.empty(t.n)
    dru[order] = np.arange(1, t.n + 1)
    return order[pend[order] == 1].astype(np.uint32), dru


def _u64(v):
    return np.asarray(v, dtype=np.int64).view(np.uint64)


def _varying(words) -> int:
    """the bits on which the words do not all agree"""
    w = np.asarray(words, dtype=np.uint64)
    return int(np.bitwise_or.reduce(w)) & ~int(np.bitwise_and.reduce(w)) & (2 ** 64 - 1)


def digit_shifts(mask: int) -> list:
    """radix_sort_masked's rule, restated: a digit of 8 bits starts at the lowest varying bit not sorted yet"""
    out = []
    while mask:
        s = (mask & -mask).bit_length() - 1
        out.append(s)
        mask &= ~((1 << (s + 8)) - 1)
    return out


def probe_word_masks(t: A.Tasks) -> list:
    """the varying bits of the three key words (rank_kernels.hpp rank_build_keys) and of the DRU keys 1..n, in the order they are sorted"""
    p = t.pending == 1
    sign = np.uint64(1 << 63)
    jk, sk, tk = _u64(t.job_id) ^ sign, _u64(t.start_ms) ^ sign, _u64(t.task_id) ^ sign
    zero = np.uint64(0)
    m_job = jk[p].min() if p.any() else zero
    m_start, m_task = (sk[~p].min(), tk[~p].min()) if (~p).any() else (zero, zero)
    npri = ((0x40000000 - t.priority.astype(np.int64)) & 0x7FFFFFFF).astype(np.uint64)
    w0 = (t.user.astype(np.uint64) << np.uint64(32)) | (npri << np.uint64(1)) | p.astype(np.uint64)
    w1 = np.where(p, jk - m_job, sk - m_start)
    w2 = np.where(p, zero, tk - m_task)
    dkey = np.arange(1, t.n + 1, dtype=np.float64).view(np.uint64) | sign
    return [_varying(w2), _varying(w1), _varying(w0), _varying(dkey)]


def run_probe(make_engine, t: A.Tasks, sh, expect_masks=None):
    """engine == numpy, bit for bit; the number of radix passes is what the varying bits ask for; radix_scan ran iff the size asks for the
    three-launch pass.  -> seconds in the engine call"""
    n = t.n
    want_ranked, want_dru = probe_reference(t)
    masks = probe_word_masks(t)
    if expect_masks is not None:  # (on the inputs alone: the case is what it was built to be)
        for name, m in expect_masks.items():
            assert masks[("w2", "w1", "w0").index(name)] == m, (name, hex(masks[("w2", "w1", "w0").index(name)]), hex(m))
    shifts = [digit_shifts(m) for m in masks]
    passes = sum(len(s) for s in shifts)
    users = A.Users(div_cpus=np.ones(1), div_mem=np.ones(1))
    prof = Profiled(make_engine)
    t0 = time.perf_counter()
    with prof(A.default_params(max_over_quota_jobs=2 ** 30)) as e:
        ranked, dru = e.rank(t, users)
    dt = time.perf_counter() - t0
    three = n > sh.rs_fused_large
    print(f"probe n={n}: digits at {shifts[:3]} + DRU {shifts[3]}; radix_hist {prof.launches('radix_hist')} radix_scan "
          f"{prof.launches('radix_scan')} iota {prof.launches('iota')}; {'three' if three else 'two'} launches a pass; {dt:.3f} s")
    assert np.array_equal(dru, want_dru), f"n={n}: DRU (= position in the per-user order) differs first at task {np.nonzero(dru != want_dru)[0][:5]}"
    assert np.array_equal(ranked, want_ranked), f"n={n}: ranked differs first at {np.nonzero(ranked != want_ranked)[0][:5]}"
    assert prof.launches("radix_hist") == passes and prof.launches("radix_scatter") == passes, (prof.launches("radix_hist"), passes)
    assert prof.launches("radix_scan") == (passes if three else 0), (n, sh.rs_fused_large, prof.launches("radix_scan"))
    assert prof.launches("iota") == sum(1 for s in (shifts[:3], shifts[3:]) if not any(s)), prof.launches("iota")
    return dt


def run_probe_size(make_engine, name: str):
    sh = shapes(make_engine)
    n = probe_size(sh, name)
    print(f"probe {name}: n = {n} ({sh.version})")
    return run_probe(make_engine, probe_tasks(n), sh)


def sparse_mask() -> int:
    return sum(1 << b for b in SPARSE_BITS)


def run_probe_kind(make_engine, kind: str, n: int = 2000):
    sh = shapes(make_engine)
    expect = None
    if kind == "sparse_bits":
        expect = {"w1": sparse_mask(), "w2": sparse_mask()}
        assert digit_shifts(sparse_mask()) == [0, 9, 23, 40, 55]
    elif kind == "start_dense":
        expect = {"w1": 2 ** 64 - 1}
        assert digit_shifts(2 ** 64 - 1)[-1] + 8 == 64
    elif kind == "start_high":
        expect = {"w1": 15 << 60}
    elif kind == "all_pending":
        expect = {"w2": 0}
    elif kind == "one_byte":
        expect = {"w2": 255 << 24, "w1": 255 << 8}
    t = probe_tasks(n, kind, seed=3)
    if kind == "prio_extremes":
        assert (_varying(((0x40000000 - t.priority.astype(np.int64)) & 0x7FFFFFFF).astype(np.uint64)) >> 30) & 1
    run_probe(make_engine, t, sh, expect)


SEVERAL_USERS_SIZES = ("small_tile-1", "small_tile+1", "fused_small_tiles+1")
FLAVOURS = ("ordinary", "tie_heavy", "fractional")


def run_several_users(make_engine, size: str, flavour: str):
    """the user word and the DRU-key sort at the same edges: synth pools against the oracle"""
    n = probe_size(shapes(make_engine), size)
    kw = dict(ordinary={}, tie_heavy=dict(tie_heavy=True), fractional=dict(fractional=True))[flavour]
    n_running = n // 3
    pool = synth.make_pool(seed=300 + n % 97, n_pending=n - n_running, n_running=n_running, n_users=max(2, min(40, n // 50)), n_offers=4, **kw)
    assert pool.tasks.n == n
    P.rank_parity(make_engine, pool, A.default_params(max_over_quota_jobs=10))


# ---- 2. the segmented scan ---------------------------------------------------------------------------------------------------------------
def scan_user_sizes(sh, n_total=None) -> list:
    """user sizes whose heads fall on a tile's first item (users 1 and 3) and on a tile's last item (user 2), user 2 covering three whole
    tiles behind its head; the last user takes what is left of n_total"""
    T = sh.ss_tile
    sizes = [T, T - 1, 1 + 3 * T, 7]
    sizes.append(T // 2 + 3 if n_total is None else n_total - sum(sizes))
    assert sizes[-1] > 0
    return sizes


def scan_pool(sizes, seed: int, fractional: bool = False):
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    n, U = int(sizes.sum()), len(sizes)
    user = np.repeat(np.arange(U), sizes).astype(np.uint32)
    where = rng.permutation(n)  # the table's order is not the users'
    cpus = np.full(n, 0.1) if fractional else rng.integers(1, 5, n).astype(np.float64)
    mem = rng.integers(1, 9, n) * 512.0
    pending = (rng.random(n) < 0.5).astype(np.uint8)
    t = A.Tasks(cpus=cpus, mem=mem, user=user[where], priority=rng.integers(0, 3, n).astype(np.int32),
                start_ms=(1_600_000_000_000 + rng.integers(0, 86_400_000, n)).astype(np.int64),
                task_id=(ID_BASE + 2_000_000_000 + rng.permutation(n)).astype(np.int64), job_id=(ID_BASE + rng.permutation(n)).astype(np.int64),
                pending=pending)
    users = A.Users(div_cpus=rng.choice([64.0, 96.0, 256.0], U), div_mem=rng.choice([262144.0, 393216.0], U))
    return t, users


def scan_reference(t: A.Tasks, users: A.Users):
    """-> (dru per task, [U, 3] running usage): np.cumsum over every user's tasks in the per-user order, which on a 1-D array is the
    left-to-right sum the reference computes (dru.clj:43-66)"""
    pend = t.pending.astype(np.int64)
    k1, k2 = np.where(pend == 1, t.job_id, t.start_ms), np.where(pend == 1, 0, t.task_id)
    order = np.lexsort((k2, k1, pend, -t.priority.astype(np.int64), t.user))
    dru, usage = np.empty(t.n), np.zeros((users.n, 3))
    bounds = np.searchsorted(t.user[order], np.arange(users.n + 1))
    for u in range(users.n):
        seg = order[bounds[u]:bounds[u + 1]]
        a, b = np.cumsum(t.mem[seg]) / users.div_mem[u], np.cumsum(t.cpus[seg]) / users.div_cpus[u]
        dru[seg] = np.where(a > b, a, b)
        run = seg[pend[seg] == 0]
        if len(run):
            usage[u, 0], usage[u, 1] = np.cumsum(t.cpus[run])[-1], np.cumsum(t.mem[run])[-1]
    return dru, usage, order


def run_scan_case(make_engine, sizes, sh, fractional=False, seed=11, oracle=True):
    T = sh.ss_tile
    sizes = np.asarray(sizes, dtype=np.int64)
    n = int(sizes.sum())
    nb = -(-n // T)
    heads = np.cumsum(sizes) - sizes
    # on the inputs alone: a head on a tile's first item behind tile 0, one on a tile's last item, a tile without any head
    assert ((heads % T == 0) & (heads > 0)).any() and (heads % T == T - 1).any(), heads
    assert set(range(nb)) - set((heads // T).tolist()), "every tile has a head"
    t, users = scan_pool(sizes, seed, fractional)
    want_dru, want_usage, order = scan_reference(t, users)
    assert np.array_equal((np.cumsum(sizes) - sizes), np.searchsorted(t.user[order], np.arange(users.n)))
    params = A.default_params(max_over_quota_jobs=2 ** 30)
    prof = Profiled(make_engine)
    t0 = time.perf_counter()
    with prof(params) as e:
        ranked, dru = e.rank(t, users)
        usage = e.rank_user_usage(users.n)
    dt = time.perf_counter() - t0
    two = nb > sh.SS_THREADS
    print(f"seg_scan n={n}: {nb} tiles, seg_scan_blocksums {prof.launches('seg_scan_blocksums')} launches, seg_scan_propagate "
          f"{prof.launches('seg_scan_propagate')}; {'blocksums + propagate' if two else 'fused propagate'}; {dt:.3f} s")
    assert np.array_equal(dru, want_dru), f"DRU differs first at per-user positions {np.nonzero(dru[order] != want_dru[order])[0][:5]} of {n}"
    assert np.array_equal(usage, want_usage), (usage, want_usage)
    assert (prof.launches("seg_scan_blocksums") > 0) == two, (nb, sh.SS_THREADS, prof.launches("seg_scan_blocksums"))
    assert prof.launches("seg_scan_propagate") > 0
    # the queue: every pending task once, DRUs ascending
    assert np.array_equal(np.sort(ranked), np.nonzero(t.pending)[0])
    assert (np.diff(dru[ranked]) >= 0).all()
    if oracle:
        o_ranked, o_dru = pyoracle.rank(params, t, users)
        assert np.array_equal(ranked, o_ranked) and np.array_equal(dru, o_dru)
    return dt


def run_scan_heads(make_engine, fractional=False):
    """a few tiles: heads on a tile's first and last item, a user over three whole tiles; also against the oracle"""
    sh = shapes(make_engine)
    return run_scan_case(make_engine, scan_user_sizes(sh), sh, fractional)


SCAN_SWITCH = ("fused", "blocksums")


def run_scan_switch(make_engine, which: str, fractional=False):
    """SS_THREADS tiles (every block folds the aggregates in front of it itself) / SS_THREADS + 1 tiles (seg_scan_blocksums, whose second
    round of SS_THREADS aggregates starts with the carry of the first): the same heads, and one user from tile 5 to the end"""
    sh = shapes(make_engine)
    n = sh.ss_fused + (1 if which == "blocksums" else 0)
    sizes = scan_user_sizes(sh, n)
    assert sizes[-1] > sh.ss_fused - 6 * sh.ss_tile  # the last user's segment crosses the switch
    return run_scan_case(make_engine, sizes, sh, fractional, oracle=False)


# ---- 3. excl_scan_u32_single through the rebalancer's host table -------------------------------------------------------------------------
HBASE_CASES = ("step-1", "step", "step+1", "super-1", "super", "super+1", "two_supers+1", "scalar_tail")


def hbase_host_counts(sh) -> dict:
    s, S = sh.scan_step, sh.scan_super
    return {"step-1": s - 1, "step": s, "step+1": s + 1, "super-1": S - 1, "super": S, "super+1": S + 1, "two_supers+1": 2 * S + 1,
            "scalar_tail": S + s + 5}


def rebal_lds_cap() -> int:
    """RB_CAP (rebalance_kernels.hpp): a host's candidate lists stay in LDS up to this many items, above it they lie in global memory at hbase"""
    return int(re.search(r"\bRB_CAP = (\d+);", _header("rebalance_kernels.hpp")).group(1))


def hbase_case(H: int, sh, seed: int):
    """H hosts of which a dozen hold tasks.  What the rebalancer reads of the scan: for a host of more than 64 items (big_list,
    rebalance_kernels.hpp rebal_big_init / rebal_host_big) hbase[h] is where its candidates lie in srt_slot, in priority order, and above
    RB_CAP items also where its lists lie in the global scratch; rebal_apply reads the winning host's preempted tasks back from there.  So
    the hosts that matter are BIG: the first and the last (both above RB_CAP), the middle one, the last but one, the hosts on both sides of every step and super-step edge,
    and the hosts on both sides of the scan's last step.  A base that is wrong for one of them puts its region on another big host's,
    and the preempted task list of a decision differs from the oracle's.  A few small hosts lie in between.  No spare resources: every
    decision preempts tasks of an occupied host.  Few pending jobs: every one of them costs a pass over all H hosts."""
    rng = np.random.default_rng(seed + H)
    s, S = sh.scan_step, sh.scan_super
    last = (H - 1) // s * s
    big = {0, H // 2, H - 2, H - 1}  # (H - 2: a second big host among the entries of the scan's last thread)
    for edge in (s, S, 2 * S, last):
        big |= {h for h in (edge - 1, edge) if 0 <= h < H}
    sizes = np.zeros(H, dtype=np.int64)
    for h in rng.integers(0, H, 6):
        sizes[int(h)] = int(rng.integers(2, 6))
    for h in sorted(big):
        sizes[h] = WAVE + int(rng.integers(2, 16))
    sizes[0] = sizes[H - 1] = rebal_lds_cap() + 2
    b = P.make_rebalance_case(seed=seed, n_running=None, n_pending=4, n_users=8, n_hosts=None, spare_frac=0.0, max_preemption=10 ** 6,
                              host_sizes=sizes, host_rng=rng)
    return b, sizes


def run_hbase_case(make_engine, name: str):
    """rebalance_parity at a host table of that length, with big hosts (whose bases the device reads, hbase_case) on both sides of every
    edge of the scan.  The seed is the first whose decisions, by the oracle, preempt on the last big host in front of the scan's last
    step and on the last host but one: a host behind one of them whose base lost a step's total, or took the tail's first entry for its
    own, writes its candidates over that host's."""
    sh = shapes(make_engine)
    assert tuple(hbase_host_counts(sh)) == HBASE_CASES
    H = hbase_host_counts(sh)[name]
    last = (H - 1) // sh.scan_step * sh.scan_step  # the scan's last step takes the hosts [last, H)
    tried = 0
    for seed in range(5, 261):
        tried += 1
        b, sizes = hbase_case(H, sh, seed)
        bigs = np.nonzero(sizes > WAVE)[0]
        need = {H - 2} | ({int(bigs[bigs < last].max())} if last else set())
        want = pyoracle.rebalance(b["params"], b["running"], b["pending"], b["pending_job_id"], b["pending_priority"], b["users"], b["spare"],
                                  b["rparams"], host_attrs=b["host_attrs"], groups=b["groups"])
        hosts = sorted({d["host"] for d in want["decisions"] if d["tasks"]})
        if need <= set(hosts) and all(sizes[h] > WAVE for h in hosts):
            break
    # on the inputs alone: hbase is read (hosts of more than 64 items, some above RB_CAP) in the scan's last step and in front of it, and
    # the decisions take tasks from such hosts
    assert (sizes[last:] > WAVE).any() and sizes[H - 1] > rebal_lds_cap() and sizes[0] > rebal_lds_cap(), (H, last)
    assert last == 0 or (sizes[:last] > WAVE).any()
    assert len(bigs) >= 3 and bigs[-1] == H - 1
    if name in ("scalar_tail", "step-1"):
        assert H % sh.SCAN1_IPT != 0  # the last thread's entries go through the scalar tail
    assert 100 <= b["running"].n < 1000, b["running"].n
    print(f"rebal_hbase_scan H={H}: {-(-H // sh.scan_step)} steps, {-(-H // sh.scan_super)} super-steps, tail of {H % sh.SCAN1_IPT}; seed {seed} "
          f"({tried} tried on the oracle), {b['running'].n} running tasks, big hosts {bigs.tolist()}, {len(want['decisions'])} decisions that "
          f"preempt on hosts {hosts}")
    assert need <= set(hosts) and all(sizes[h] > WAVE for h in hosts), (hosts, need)
    prof = Profiled(make_engine)
    t0 = time.perf_counter()
    P.rebalance_parity(prof, b, want=want)
    print(f"rebal_hbase_scan: {prof.launches('rebal_hbase_scan')} launches; {time.perf_counter() - t0:.3f} s in the engine's two runs")
    assert prof.launches("rebal_hbase_scan") >= 1, prof.tags.keys()


# ---- 4. the tie tiles at their capacity --------------------------------------------------------------------------------------------------
def tie_pool(G: int, singles: int):
    """G users with the same single first task (one tie group of G items) behind `singles` single items: the tasks of one extra user under
    a divisor that keeps all of its DRUs distinct and below the group's"""
    assert singles < 2 ** 20
    U = G + (1 if singles else 0)
    n = G + singles
    user = np.concatenate([np.arange(G), np.full(singles, G)]).astype(np.uint32)
    rng = np.random.default_rng(G * 31 + singles)
    where = rng.permutation(n)
    one = np.ones(n)
    t = A.Tasks(cpus=one, mem=one.copy(), user=user[where], priority=np.full(n, 50, np.int32), start_ms=np.zeros(n, np.int64),
                task_id=(ID_BASE + 2_000_000_000 + rng.permutation(n)).astype(np.int64), job_id=(ID_BASE + rng.permutation(n)).astype(np.int64),
                pending=np.ones(n, np.uint8))
    div = np.ones(U)
    if singles:
        div[G] = 2.0 ** 20
    return SimpleNamespace(tasks=t, users=A.Users(div_cpus=div, div_mem=div.copy()))


def singles_pool(n_users: int, per_user: int):
    """every DRU distinct: user u's divisors are the u-th prime above per_user (k / p = k' / p' needs p | k' p: k' < p is too small)"""
    primes, c = [], per_user + 1
    while len(primes) < n_users:
        if all(c % q for q in range(2, int(c ** 0.5) + 1)):
            primes.append(c)
        c += 1
    n = n_users * per_user
    rng = np.random.default_rng(n)
    one = np.ones(n)
    t = A.Tasks(cpus=one, mem=one.copy(), user=(rng.permutation(n) % n_users).astype(np.uint32), priority=np.full(n, 50, np.int32),
                start_ms=np.zeros(n, np.int64), task_id=(ID_BASE + 2_000_000_000 + rng.permutation(n)).astype(np.int64),
                job_id=(ID_BASE + rng.permutation(n)).astype(np.int64), pending=np.ones(n, np.uint8))
    d = np.array(primes, dtype=np.float64)
    return SimpleNamespace(tasks=t, users=A.Users(div_cpus=d, div_mem=d.copy()))


def tie_cases(sh) -> dict:
    """name -> (group size, single items in front, does the group's tile overflow)"""
    return {
        "cap-1": (sh.TS_CAP - 1, 0, False),
        "cap": (sh.TS_CAP, 0, False),
        "cap+1": (sh.TS_CAP + 1, 0, True),
        "max_group_on_last_position": (sh.ts_max_group, sh.TS_NOMINAL - 1, False),  # the tile is exactly TS_CAP items
        "max_group+1_on_last_position": (sh.ts_max_group + 1, sh.TS_NOMINAL - 1, True),
        "cap_on_first_position_of_tile_1": (sh.TS_CAP, sh.TS_NOMINAL, False),        # tile 0 ends where tile 1's stretch starts
        "cap+1_on_first_position_of_tile_1": (sh.TS_CAP + 1, sh.TS_NOMINAL, True),
    }


TIE_CASES = ("cap-1", "cap", "cap+1", "max_group_on_last_position", "max_group+1_on_last_position", "cap_on_first_position_of_tile_1",
             "cap+1_on_first_position_of_tile_1")


def _both_forms(make_engine, monkeypatch, pool, params):
    """rank_parity with the tie rule in LDS tiles and as radix passes: -> (launches of tie_sort_tiles, of tie_build) of the first form"""
    prof = Profiled(make_engine)
    monkeypatch.delenv("COOK_RANK_RADIX", raising=False)
    a = P.rank_parity(prof, pool, params)
    tiles, build = prof.launches("tie_sort_tiles"), prof.launches("tie_build")
    monkeypatch.setenv("COOK_RANK_RADIX", "1")
    b = P.rank_parity(prof, pool, params)
    monkeypatch.delenv("COOK_RANK_RADIX")
    assert prof.launches("tie_sort_tiles") == 0, "COOK_RANK_RADIX: the tiles ran all the same"
    assert np.array_equal(a, b)
    return tiles, build, prof.launches("tie_build")


def run_tie_case(make_engine, monkeypatch, name: str):
    sh = shapes(make_engine)
    assert tuple(tie_cases(sh)) == TIE_CASES
    G, singles, overflow = tie_cases(sh)[name]
    assert (singles % sh.TS_NOMINAL + G > sh.TS_CAP) == overflow  # the tile of the group: from its stretch's first position to the group's end
    pool = tie_pool(G, singles)
    tiles, build, build_radix = _both_forms(make_engine, monkeypatch, pool, A.default_params(max_over_quota_jobs=2 ** 30))
    print(f"tie tiles {name}: a group of {G} at position {singles} (TS_NOMINAL {sh.TS_NOMINAL}, TS_CAP {sh.TS_CAP}): tie_sort_tiles {tiles} "
          f"launches, tie_build {build} ({'overflow: radix passes' if overflow else 'fits'}); as radix passes tie_build {build_radix}")
    assert tiles > 0 and build_radix > 0
    assert (build > 0) == overflow, (name, build)


def run_all_singles(make_engine, monkeypatch, n_users=7, tiles=5):
    """every group a single item: every tile returns early, and neither form has anything to sort"""
    sh = shapes(make_engine)
    per_user = -(-tiles * sh.TS_NOMINAL // n_users) + 1
    pool = singles_pool(n_users, per_user)
    tiles_l, build, build_radix = _both_forms(make_engine, monkeypatch, pool, A.default_params(max_over_quota_jobs=2 ** 30))
    print(f"tie tiles, all singles: {pool.tasks.n} items, tie_sort_tiles {tiles_l} launches, tie_build {build} / {build_radix}")
    assert tiles_l > 0 and build == 0 and build_radix == 0
