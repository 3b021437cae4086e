"""The window rounds (match_eval2, match_merge2, match_resolve2: cook_amd/csrc/match_v2_*.hpp) at the guard bands of their approximate
fitness and at the edges of their tables and tiles, shared by the emulator (test_match_edges_emu.py) and GPU (test_match_edges_gpu.py)
suites.  Not a test module.  Everything goes through the public calls (Engine.match, the cycle calls, cook_cycle_match_multi, match_stats).
Every size is derived from the constants the headers state (read with a regular expression, the side of a COOK_SHAPE(gpu, emu) pair that
the loaded library runs), the band exponents are stated once below and the headers' text is asserted to still hold each literal.  Expected
placements, fail codes and head_matched never come from the engine: pyoracle.match at cook_params.fitness 0; under the one-resource packers
(fitness 1, 2), which oracle/ does not know, tests/fitness_oracle.py — the restatement of the same loop that test_fitness_emu.py holds to
pyoracle.match — and at fitness 0 every case asserts that the two agree.

PART 1, near-ties.  Two offers whose exact fitness for one job differs by a relative gap g, 2^-(k+1) < g < 2^-k: lease D against
D (1 + 2^-k) of the resource the packer looks at (cpus under fitness 0 and 1, mem under 2; written x below, the other resource y), the y terms
identical, running resources where a touched offer has a numerator an untouched one lacks.  check_pair asserts, on the inputs alone (fractions
for the real values, Python floats for the oracle's formula): the two fp64 values differ (tie control: are equal), their order is the real
values' order, g lies on the stated side of EVERY band, the oracle gives the job to the offer the case names.  Each pair runs with the worse
offer at the lower and at the higher index, and with either role as the worse one.  Situations:
  N1  two untouched offers in one eval wave's batch (top-MV_L insertion); N1w in two waves of one block (the tile's epilogue)
  N2  in two chunks (the merge's maximum across lanes, its index rule on equal keys)
  N3  in chunk c and c + 64, the two chunks of ONE merge lane (plain layout, and virtual chunks under COOK_EVAL_SPLIT=4)
  N4  nine feasible offers in one batch, fitness rising with the index by g a step: one job gets the ninth; nine jobs, one offer each
  N5  touched against the first untouched list entry;  N6  two touched offers
  N7  good-enough: the threshold at F, nextafter(F, 0) and F (1 +- 2^-k) of the deciding offer's fitness F, untouched and touched
The spreaders (fitness 3..5) go to the serial sweep; one runs as a control of the oracle comparison.  match_algo 3 runs N1, N2, N5, N6 at
fitness 0 / good-enough 1.0 as C1, C2, C5, C6: pairs whose gap comes from cancellation (GAPS_ABS below), around CF_BAND (an ABSOLUTE band: the
case asserts the absolute gap's side) and CF_BAND32, far inside the form's limits: placement_form == 3, refusal word 0.  The plain N1 / N1w / N2
pairs run under it too: from k = 24 on the form REFUSES them — placement_form 0 and exactly CF_X_NUMBERS asserted — and places the wider ones.

PART 2, table and tile edges.  Parity with the oracle plus the path taken, from match_stats() and the per-round log (COOK_ROUND_LOG).  An
assertion is EXACT where a header states the rule it follows from (first_window and resolve_finish for the window sequence; the merge's
truncation rule; alloc_lane for the touched set), otherwise NON-ZERO; each says which.

ROUNDED RECIPROCALS.  With totals that are powers of two times (1 + 2^-k) the approximation fl(n * fl(1 / d)) mostly EQUALS fl(n / d), and a walk
that trusted it would pass all of the above.  T5 and N7's `inexact` form therefore use a total whose reciprocal is rounded (10: 7 * fl(0.1) >
fl(0.7)), chosen by inexact_reciprocal so that the touched offer's approximate fitness — the walk's formula, restated in touched_approx — lies
strictly above (below) the fp64 fitness of an offer it ties with exactly, or of the good-enough threshold it equals.

ONE-TOKEN CHANGES to the kernels, each tried once on a scratch copy built with the everyday emulator, and what failed (none is committed):
  * match_v2_eval.hpp, the pruning threshold `E.thr = ... (1.0 - 0x1p-40)` -> `0x1p-60` (thr = the list's worst entry itself): NOT caught.  To be
    pruned wrongly an offer needs an approximation BELOW the worst kept fitness and an exact value above it.  N4 puts the ninth offer 1 ulp
    above a full list; no (n, d) of the family has such a rounding (searched: 4 M random pairs of totals 1 and 2 ulps apart, none), so what the
    2^-40 margin absorbs is an error bound (2^-51) that these inputs never reach.
  * match_v2_resolve.hpp `eps_lo(fw) > u_fit` -> `fw > u_fit`: T5 (test_exact_ties_on_a_rounded_reciprocal, the three packers under match_algo 0:
    the touched offer at the higher index wins a tie it must lose).  N5 alone does not catch it: its approximations are exact.
  * `kf >= mx * (1.0f - 0x1p-20f)` -> `0x1p-26f` (in fp32 that factor is 1: only equal images count as near): NOT caught.  Rounding to fp32 is
    monotone, so images that differ order the approximations correctly; a wrong decision needs two touched offers whose approximations straddle
    an fp32 rounding boundary AND are ordered against their exact values, within 2^-51 of each other.  N6's pairs at 2^-24 .. 2^-19 differ by more.
  * match_v2_eval.hpp `fit > E.ge` -> `>=` (the gem bit): N7 untouched (test_good_enough_thresholds[*-0-False], threshold F) and N7 multi.
  * match_v2_resolve.hpp, general path `pe_fit > good_enough` -> `>=`: N7 touched (test_good_enough_thresholds[*-0-True]) and N7 multi.
  * match_v2_resolve.hpp, fast path `eps_lo(fa) > good_enough` -> `fa > good_enough`: N7 inexact (test_good_enough_at_a_rounded_reciprocal[*-0-above]).
  * match_v2_merge.hpp `n == MV_L` -> `n > MV_L` in `hide`: the nine-in-a-batch cases (test_nine_offers_rising, test_list_in_one_batch[1-*]) and 26 more.
  * match_v2_merge.hpp `!(R.fit[q] > tf[MV_L - 1])` -> `>=`: NOT caught, and cannot be: the entry that now gets through meets
    topl_insert_ascending, whose own comparison is strict and leaves the list as it is.  That comparison, `fit > tf[q]` -> `>=` (match_v2_eval.hpp):
    N3 in both layouts, N4, tie controls of test_near_ties, the list cases and the window pools (46 tests).
  * match_v2_resolve.hpp `tg > wave_read_lane(cur.g_off, ng - 1)` -> `<`: all four good-enough list cases (the path assertions of both sides, and with
    LG + 1 offers and T behind the placement itself: T instead of the unlisted offer in front of it).
  * MV_T off by one, as `nT < (unsigned)MV_T - 1u` in alloc_lane and as `MV_T = COOK_WAVE - 1`: the touched-set pair — the emulated process dies
    there with a segmentation fault (alloc_lane's "all 64 lanes own an offer" no longer holds), in both forms.
"""
from __future__ import annotations

import csv
import os
import re
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

from cook_amd import _abi as A
from cook_amd.engine import CookError
from oracle import pyoracle
from tests import fitness_oracle as FO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE = 64
ID_BASE = 17_592_186_044_416

# ---- the band exponents, stated once, and the text that states them in the code -------------------------------------------------------------
PRUNE, EPS, GE_NEAR, F32 = 40, 38, 30, 20   # relative bands of the window rounds: 2^-40 pruning / ge_lo, 2^-38 eps_lo / eps_hi, 2^-30 ge_near_f, 2^-20 fp32 image
CF_X_NUMBERS = 1  # classfit.hpp: "a resource is ... not a multiple of 2^-20"
CF, CF32 = 37, 21                           # the class-ordered walk: CF_BAND 2^-37 (absolute), CF_BAND32 2^-21
REL_BANDS = (PRUNE, EPS, GE_NEAR, F32, CF32)
BAND_TEXT = {
    "match_v2_eval.hpp": ("E.ge_lo = in.good_enough * (1.0 - 0x1p-40);", "E.thr = E.tf[MV_L - 1] * (1.0 - 0x1p-40);"),
    "match_v2_resolve.hpp": ("ldexp(good_enough < 0.0 ? -good_enough : good_enough, -30)", "return x - ldexp(x, -38);", "return x + ldexp(x, -38);",
                             "kf >= mx * (1.0f - 0x1p-20f)"),
    "classfit.hpp": ("CF_BAND = 1.0 / 137438953472.0;", "CF_X_NUMBERS = 1u,", "if (kc > 20u || km > 20u) bad |= CF_X_NUMBERS;"),
    "classfit_walk.hpp": ("CF_BAND32 = 1.0f / 2097152.0f;",),
}
# the gaps, by k (2^-(k+1) < g < 2^-k): 1 ulp of the fitness, 2^-45, both sides of 2^-40, of 2^-38, of 2^-30, 2^-24 (fp32's own
# resolution), both sides of 2^-21 and 2^-20
GAPS = (52, 45, 41, 39, 37, 31, 29, 24, 22, 21, 20, 19)
# The class-ordered form takes resources as multiples of 2^-20 only and requests on eight cpus levels (classfit.hpp), so D (1 + 2^-k) with k > 20 is
# refused (CF_X_NUMBERS) before it can be a near-tie.  Its pairs get their gap by CANCELLATION instead: offer P has totals (D, E (1 + 2^-e)),
# offer Q (D (1 + 2^-e), E), both the same numerators with cf - mf = 2^-j: the fitness values differ by 2^-j 2^-e / (2 (1 + 2^-e)), an ABSOLUTE gap
# in (2^-(n+1), 2^-n), n = e + j + 1.  (e, j) below: 2^-43 (the totals need e - 3 fraction bits each, and the form's sort key asks 2 Tc Tm < 2^45 of
# them in fixed point: (21, 21) is the finest pair it takes), both sides of CF_BAND = 2^-37, both sides of CF_BAND32 = 2^-21
GAPS_ABS = ((21, 21), (20, 18), (20, 17), (20, 16), (20, 15), (20, 14), (18, 3), (17, 3), (16, 3), (15, 3))
A_GAP = 18  # N7's lower-index offer sits this far below the deciding one


def _header(name: str) -> str:
    with open(os.path.join(ROOT, "cook_amd", "csrc", name)) as f:
        return f.read()


def check_band_literals():
    """a changed band makes this fail instead of silently testing the wrong gap"""
    for name, texts in BAND_TEXT.items():
        h = _header(name)
        for t in texts:
            assert t in h, f"{name} no longer contains `{t}`: restate the band exponents of tests/match_edges_cases.py"
    assert 2 ** CF == 137438953472 and 2 ** CF32 == 2097152


def _const(text: str, name: str, ship: bool) -> int:
    """`NAME = n;`, `NAME = COOK_SHAPE(gpu, emu);`, or `NAME = COOK_NAME;` behind `#define COOK_NAME n | COOK_SHAPE(gpu, emu)`"""
    m = re.search(rf"\b{name} = (?:COOK_SHAPE\((\d+), (\d+)\)|(\d+)u?);", text)
    if not m:
        assert re.search(rf"\b{name} = COOK_{name};", text), f"{name}: not stated as a number, a COOK_SHAPE pair or its COOK_ define any more"
        m = re.search(rf"#define COOK_{name} (?:COOK_SHAPE\((\d+), (\d+)\)|(\d+)(?!\d))", text)
        assert m, f"COOK_{name}: no #define with a number or a COOK_SHAPE pair"
    return int(m.group(3)) if m.group(3) is not None else int(m.group(1 if ship else 2))


_SHAPES = {}


def shapes(make_engine) -> SimpleNamespace:
    with make_engine(A.default_params()) as e:
        version = e.version
    if version in _SHAPES:
        return _SHAPES[version]
    ship = "shipped launch shapes" in version or "hip gfx950" in version
    sh, ev, rs = _header("match_v2_shapes.hpp"), _header("match_v2_eval.hpp"), _header("match_v2_resolve.hpp")
    c = {n: _const(sh, n, ship) for n in ("MV_L", "MV_OCW", "MV_EW", "MV_WSEG", "MV_WEVAL", "MV_WLONG", "MV_NC", "MV_NA", "MV_FH")}
    c["LM"] = int(re.search(r"#define COOK_MV_LM (\d+)", sh).group(1))
    c["LM_GE"] = int(re.search(r"#define COOK_MV_LM_GE (\d+)", sh).group(1))
    assert "static constexpr int LM = GE ? COOK_MV_LM_GE : COOK_MV_LM;" in sh and "static constexpr int LG = GE ? 64 : 0;" in sh
    assert "constexpr int MV_OCB = MV_OCW * MV_EW;" in sh and "constexpr int MV_T = COOK_WAVE;" in sh and "constexpr int MV_JG = MV_WEVAL / 64;" in sh
    c["MV_SPLIT_MAX"] = _const(ev, "MV_SPLIT_MAX", ship)
    c["MV_WSEG_MIN"] = _const(rs, "MV_WSEG_MIN", ship)
    c["MV_RETIRE_CAP"] = _const(rs, "MV_RETIRE_CAP", ship)
    assert "constexpr unsigned MV_RLDS_BYTES = 160u * 1024u - 2048u;" in rs
    s = SimpleNamespace(version=version, ship=ship, LG=64, MV_T=WAVE, MV_RLDS_BYTES=160 * 1024 - 2048, **c)
    s.MV_OCB = s.MV_OCW * s.MV_EW
    s.MV_JG = s.MV_WEVAL // 64
    _SHAPES[version] = s
    return s


def eval_split(sh, wcur: int, split_max: int) -> int:
    """match_v2_eval.hpp eval_split, restated"""
    active = (wcur + WAVE - 1) // WAVE
    r = 1
    while r * 2 <= split_max and r * 2 * active <= sh.MV_JG and sh.MV_OCW // (r * 2) >= 8:
        r *= 2
    return r


# ---- the two fitness values of a pair: the oracle's formula in fp64, and the real values --------------------------------------------------------
def fit64(f: int, rc, ac, c, oc, rm, am, m, om) -> float:
    """cook_oracle.cpp:471 operation for operation (Python floats are IEEE doubles)"""
    cf, mf = (rc + ac + c) / (oc + rc), (rm + am + m) / (om + rm)
    return {0: (cf + mf) / 2.0, 1: cf, 2: mf}[f]


def fit_real(f: int, rc, ac, c, oc, rm, am, m, om) -> Fraction:
    F = Fraction
    cf, mf = (F(rc) + F(ac) + F(c)) / (F(oc) + F(rc)), (F(rm) + F(am) + F(m)) / (F(om) + F(rm))
    return {0: (cf + mf) / 2, 1: cf, 2: mf}[f]


def oracle_match(params, jobs, offers, groups=None):
    """pyoracle.match at fitness 0 (and the parametrised restatement agrees); the restatement under the one-resource packers"""
    if int(params.fitness) == 0:
        want = pyoracle.match(params, jobs, offers, groups, ())
        if FO.supports(jobs, offers, groups):
            other = FO.match(params, jobs, offers, groups)
            assert np.array_equal(want[0], other[0]) and np.array_equal(want[1], other[1]) and want[2] == other[2], "fitness_oracle != pyoracle at fitness 0"
        return want
    return FO.match(params, jobs, offers, groups)


def _assigned_before(jobs, j2o, job: int, v: int):
    """what the oracle's state holds on offer v when `job` is looked at: the same additions in the same order"""
    ac = am = 0.0
    for q in range(job):
        if j2o[q] == v:
            ac, am = ac + float(jobs.cpus[q]), am + float(jobs.mem[q])
    return ac, am


def pair_values(case, fitness: int, j2o):
    jobs, o = case.jobs, case.offers
    out = []
    for v in case.pair:
        ac, am = _assigned_before(jobs, j2o, case.job, v)
        args = (float(o.run_cpus[v]), ac, float(jobs.cpus[case.job]), float(o.cpus[v]), float(o.run_mem[v]), am, float(jobs.mem[case.job]), float(o.mem[v]))
        out.append((fit64(fitness, *args), fit_real(fitness, *args)))
    return out


def check_pair(case, fitness: int, k, want, ge: float = 1.0):
    """the conditions of a near-tie case, from the inputs and the oracle alone; -> the side of every band ('inside' / 'outside')"""
    (fp, rp), (fq, rq) = pair_values(case, fitness, want[0])
    p, q = case.pair
    assert 0.0 < fp < ge and 0.0 < fq < ge, (case.name, fp, fq, ge)  # (N1..N6: nothing clears good-enough)
    if k is None:
        assert fp == fq and rp == rq, (case.name, "tie control", fp, fq)
        assert want[0][case.job] == case.expect == min(p, q), (case.name, "tie: the lowest index", want[0][case.job], p, q)
        return {}
    assert fp != fq, (case.name, k, "the fp64 values are equal")
    assert (fp > fq) == (rp > rq), (case.name, k, "fp64 orders the pair against the real values")
    sides = {}
    if isinstance(k, tuple):  # (e, j): an absolute gap by cancellation, for the class-ordered walk's absolute bands
        n = k[0] + k[1] + 1
        g = abs(rp - rq)
        assert Fraction(1, 2 ** (n + 1)) < g < Fraction(1, 2 ** n), (case.name, k, float(g))
        for b in (CF, CF32):
            inside = g < Fraction(1, 2 ** b)
            assert inside == (n >= b), (case.name, k, b)
            sides[b] = "inside" if inside else "outside"
    else:
        g = abs(rp - rq) / max(rp, rq)
        assert Fraction(1, 2 ** (k + 1)) < g < Fraction(1, 2 ** k), (case.name, k, float(g))
        for b in REL_BANDS:
            inside = g < Fraction(1, 2 ** b)
            assert inside == (k >= b), (case.name, k, b)
            sides[b] = "inside" if inside else "outside"
    better = p if rp > rq else q
    assert case.expect == better and want[0][case.job] == better, (case.name, k, "the oracle places on", want[0][case.job], "the better offer is", better)
    return sides


# ---- pools in x / y units -------------------------------------------------------------------------------------------------------------------------
def _tot(D: float, k):
    """D (1 + 2^-k), exactly"""
    if k is None:
        return D
    t = D + D * 2.0 ** -k
    assert Fraction(t) == Fraction(D) * (1 + Fraction(1, 2 ** k)), (D, k)
    return t


def _free(total: float, run: float):
    f = total - run
    assert Fraction(f) + Fraction(run) == Fraction(total) and f + run == total, (total, run)
    return f


def _pool(name, fitness, M, placed, jobs, pair, job, expect, tiny=True, groups=None, filler_y=4096.0):
    """placed: {offer index: (x free, x running, y free, y running)}; every other offer is filler that no job but the tiny one fits (half of
    them alive thanks to it, half dead); jobs: [(x, y)], and a tiny job behind them"""
    xf, xr, yf, yr = np.empty(M), np.zeros(M), np.full(M, filler_y), np.zeros(M)
    xf[0::2], xf[1::2] = 0.5, 0.125
    for v, (a, b, c, d) in placed.items():
        xf[v], xr[v], yf[v], yr[v] = a, b, c, d
    jx = np.array([j[0] for j in jobs] + ([0.25] if tiny else []))
    jy = np.array([j[1] for j in jobs] + ([256.0] if tiny else []))
    assert jx[:len(jobs)].min() > 0.5
    if fitness == 2:  # memoryBinPacker looks at mem: x is mem, y (in units of 512) cpus
        off = A.Offers(cpus=yf / 512.0, mem=xf, run_cpus=yr / 512.0, run_mem=xr, k8s=np.ones(M, np.uint8))
        jb = A.Jobs(cpus=jy / 512.0, mem=jx)
    else:
        off = A.Offers(cpus=xf, mem=yf, run_cpus=xr, run_mem=yr, k8s=np.ones(M, np.uint8))
        jb = A.Jobs(cpus=jx, mem=jy)
    return SimpleNamespace(name=name, jobs=jb, offers=off, groups=groups, pair=pair, job=job, expect=expect)


def _roles(k, flip, swap, i0, i1):
    """-> (index of role A, index of role B, A's total factor k, B's): role B is the worse one unless flip; A sits at i0 unless swap"""
    ia, ib = (i1, i0) if swap else (i0, i1)
    ka, kb = (k, None) if flip else (None, k)
    return ia, ib, ka, kb


def _expect(ia, ib, k, flip):
    return min(ia, ib) if k is None else (ib if flip else ia)


def two_untouched(sh, fitness, k, flip, swap, where):
    """N1 / N1w / N2 / N3: one job of x 4, y 1024 on offers of x 8 | 8 (1 + 2^-k), y 4096: cf = 1/2, mf = 1/4"""
    B = sh.MV_OCB
    i0, i1, M = {"N1": (3, sh.MV_OCW - 2, 2 * sh.MV_OCW + 5),            # one wave's batch
                 "N1w": (sh.MV_OCW - 1, sh.MV_OCW, 2 * sh.MV_OCW + 5),   # the last offer of wave 0, the first of wave 1
                 "N2": (B - 1, B, B + sh.MV_OCW + 1),                    # the last offer of chunk 0, the first of chunk 1
                 "N3": (5, 64 * B + 7, 64 * B + B),                      # chunk 0 and chunk 64: lane 0's first and second chunk
                 "N3s": (0, 16 * B, 16 * B + 1)}[where]                  # COOK_EVAL_SPLIT=4: virtual chunks 0 and 64, 65 chunk lists in all
    ia, ib, ka, kb = _roles(k, flip, swap, i0, i1)
    placed = {ia: (_tot(8.0, ka), 0.0, 4096.0, 0.0), ib: (_tot(8.0, kb), 0.0, 4096.0, 0.0)}
    return _pool(f"{where} k={k} flip={flip} swap={swap}", fitness, M, placed, [(4.0, 1024.0)], (ia, ib), 0, _expect(ia, ib, k, flip))


def nine_rising(sh, fitness, k, n_jobs):
    """N4: nine offers at indices 1, 4, ... 25 of one batch, x free 8 (1 + (8 - i) 2^-k): the fitness rises with the index by g a step.  One job
    of x 5: the ninth offer, evaluated against a full list; nine such jobs: one offer each, best first; the ninth job's offer is the one entry
    beyond MV_L"""
    assert sh.MV_L == 8 and sh.MV_OCW >= 27
    idx = [1 + 3 * i for i in range(9)]
    placed = {}
    for i, v in enumerate(idx):
        t = 8.0 if k is None else 8.0 + (8 - i) * 8.0 * 2.0 ** -k
        assert k is None or Fraction(t) == 8 * (1 + (8 - i) * Fraction(1, 2 ** k))
        placed[v] = (t, 0.0, 4096.0, 0.0)
    c = _pool(f"N4 k={k} jobs={n_jobs}", fitness, sh.MV_OCW + 3, placed, [(5.0, 1024.0)] * n_jobs, (idx[0] if k is None else idx[7], idx[8]), 0,
              idx[0] if k is None else idx[8])
    c.idx = idx
    return c


def touched_untouched(sh, fitness, k, flip, swap, D=8.0, c0=5.0, c1=2.0):
    """N5: job 0 (x 5) fits offer A alone (x free 8 | 8 (1 + 2^-k)); B runs x 5 on the same total.  Job 1 (x 2): (5 + 2) / total on both, A touched,
    B the first untouched entry of its list; y: (1024 + 512) / 4096 on both"""
    assert c0 > D - c0 and c0 + c1 <= D
    ia, ib, ka, kb = _roles(k, flip, swap, 6, 2 * sh.MV_OCW + 1)
    placed = {ia: (_tot(D, ka), 0.0, 4096.0, 0.0), ib: (_free(_tot(D, kb), c0), c0, 3072.0, 1024.0)}
    return _pool(f"N5 k={k} flip={flip} swap={swap} D={D}", fitness, 2 * sh.MV_OCW + 9, placed, [(c0, 1024.0), (c1, 512.0)], (ia, ib), 1, _expect(ia, ib, k, flip))


def touched_approx(fitness: int, D, c0, c1) -> float:
    """what the walk computes for the TOUCHED offer of N5 / N7 (match_v2_resolve.hpp: a1 = (t_basec + c) * t_invc, fitness_terms, (a1 + a2) * 0.5;
    match_v2_pack.hpp: inv_dc = 1.0 / (oc + rc)), restated for these pools: x (0 + c0 + c1) * fl(1 / D), y (0 + 1024 + 512) * fl(1 / 4096)"""
    a1, a2 = ((0.0 + c0) + c1) * (1.0 / D), ((0.0 + 1024.0) + 512.0) * (1.0 / 4096.0)
    if fitness != 0:  # a one-resource packer: the x term alone (x is cpus under 1, mem under 2)
        a2 = a1
    return (a1 + a2) * 0.5


def inexact_reciprocal(fitness: int, above: bool):
    """-> (D, c0, c1): a total whose reciprocal is rounded, such that the touched offer's APPROXIMATE fitness lies above (below) its fp64 fitness.
    Two offers of this total tie exactly, and a walk that trusted the approximation would prefer (pass over) the touched one"""
    for D in (10.0, 5.0, 20.0, 6.0, 12.0, 14.0, 7.0):
        for c0 in np.arange(np.floor(D / 2) + 1.0, D, 0.5):
            for c1 in np.arange(1.0, D - c0 + 0.25, 0.5):
                x = fit64(1 if fitness else 0, 0.0, c0, c1, D, 0.0, 1024.0, 512.0, 4096.0)
                ap = touched_approx(fitness, D, float(c0), float(c1))
                if (ap > x) if above else (ap < x):
                    return D, float(c0), float(c1)
    raise AssertionError("no total with a rounded reciprocal in the family")


def two_touched(sh, fitness, k, flip, swap):
    """N6: job 0 (x 9) fits A1 alone, job 1 (y 3584) fits A2 alone; job 2 (x 5, y 512): x (9 + 5) / 16 on A1, (8 + 1 + 5) / 16 on A2 (which runs x 8),
    y (4608 + 1024 + 512) / 8192 on A1 and (2048 + 3584 + 512) / 8192 on A2"""
    ia, ib, ka, kb = _roles(k, flip, swap, 9, sh.MV_OCW + 4)
    placed = {ia: (_tot(16.0, ka), 0.0, 3584.0, 4608.0), ib: (_free(_tot(16.0, kb), 8.0), 8.0, 6144.0, 2048.0)}
    return _pool(f"N6 k={k} flip={flip} swap={swap}", fitness, 2 * sh.MV_OCW + 9, placed, [(9.0, 1024.0), (1.0, 3584.0), (5.0, 512.0)], (ia, ib), 2,
                 _expect(ia, ib, k, flip))


def _cancel(k, flip, swap, i0, i1, D, E):
    """-> (index of A, of B, A's totals (x, y), B's, 8 d): the better role P = (D, E (1 + 2^-e)) is A's unless flip"""
    ia, ib = (i1, i0) if swap else (i0, i1)
    if k is None:
        return ia, ib, (D, E), (D, E), 2.0 ** -15
    e, j = k
    P, Q = (D, _tot(E, e)), (_tot(D, e), E)
    return (ia, ib) + ((Q, P) if flip else (P, Q)) + (E * 2.0 ** -j,)


def cancel_untouched(sh, k, flip, swap, where):
    """C1 / C2: N1 / N2 in the class-ordered form's numbers.  One job of x 4, y 2 on two offers that run y 2 - 8 d: cf = 1 / 2, mf = 1 / 2 - d"""
    i0, i1, M = {"C1": (3, sh.MV_OCW - 2, 2 * sh.MV_OCW + 5), "C2": (sh.MV_OCB - 1, sh.MV_OCB, sh.MV_OCB + sh.MV_OCW + 1)}[where]
    ia, ib, (ax, ay), (bx, by), d8 = _cancel(k, flip, swap, i0, i1, 8.0, 8.0)
    r = 2.0 - d8
    placed = {ia: (ax, 0.0, _free(ay, r), r), ib: (bx, 0.0, _free(by, r), r)}
    return _pool(f"{where} (e, j)={k} flip={flip} swap={swap}", 0, M, placed, [(4.0, 2.0)], (ia, ib), 0, _expect(ia, ib, k, flip), tiny=False, filler_y=8.0)


def cancel_touched_untouched(sh, k, flip, swap):
    """C5: N5 likewise.  Job 0 (x 5, y 2) fits A alone; job 1 (x 2, y 1): x 7 / 8 on both, y (4 - 8 d + 2 + 1) / 8 on A, (6 - 8 d + 1) / 8 on B"""
    ia, ib, (ax, ay), (bx, by), d8 = _cancel(k, flip, swap, 6, 2 * sh.MV_OCW + 1, 8.0, 8.0)
    placed = {ia: (ax, 0.0, _free(ay, 4.0 - d8), 4.0 - d8), ib: (_free(bx, 5.0), 5.0, _free(by, 6.0 - d8), 6.0 - d8)}
    return _pool(f"C5 (e, j)={k} flip={flip} swap={swap}", 0, 2 * sh.MV_OCW + 9, placed, [(5.0, 2.0), (2.0, 1.0)], (ia, ib), 1, _expect(ia, ib, k, flip),
                 tiny=False, filler_y=8.0)


def cancel_two_touched(sh, k, flip, swap):
    """C6: N6 likewise, the requests 10, 3, 4 on the levels 3 .. 10.  Job 0 (x 10) fits A1 alone (A2 runs x 7 of 16), job 1 (x 3, y 3) A2 alone
    (A1 has y 1.5 left); job 2 (x 4, y 0.5): x 14 / 16 on both, y (6 - 8 d + 0.5 + 0.5) / 8 on A1, (3.5 - 8 d + 3 + 0.5) / 8 on A2"""
    ia, ib, (ax, ay), (bx, by), d8 = _cancel(k, flip, swap, 9, sh.MV_OCW + 4, 16.0, 8.0)
    placed = {ia: (ax, 0.0, _free(ay, 6.0 - d8), 6.0 - d8), ib: (_free(bx, 7.0), 7.0, _free(by, 3.5 - d8), 3.5 - d8)}
    return _pool(f"C6 (e, j)={k} flip={flip} swap={swap}", 0, 2 * sh.MV_OCW + 9, placed, [(10.0, 0.5), (3.0, 3.0), (4.0, 0.5)], (ia, ib), 2,
                 _expect(ia, ib, k, flip), tiny=False, filler_y=8.0)


CANCEL = {"C1": lambda sh, k, fl, sw: cancel_untouched(sh, k, fl, sw, "C1"), "C2": lambda sh, k, fl, sw: cancel_untouched(sh, k, fl, sw, "C2"),
          "C5": cancel_touched_untouched, "C6": cancel_two_touched}
def touched_untouched_inexact(sh, fitness, k, flip, swap):
    """T5: N5's exact tie on a total whose reciprocal is rounded; flip: the touched offer's approximation lies below, else above"""
    assert k is None
    return touched_untouched(sh, fitness, None, False, swap, *inexact_reciprocal(fitness, not flip))


SITUATIONS = {"T5": touched_untouched_inexact, "N1": lambda sh, f, k, fl, sw: two_untouched(sh, f, k, fl, sw, "N1"), "N1w": lambda sh, f, k, fl, sw: two_untouched(sh, f, k, fl, sw, "N1w"),
              "N2": lambda sh, f, k, fl, sw: two_untouched(sh, f, k, fl, sw, "N2"), "N3": lambda sh, f, k, fl, sw: two_untouched(sh, f, k, fl, sw, "N3"),
              "N3s": lambda sh, f, k, fl, sw: two_untouched(sh, f, k, fl, sw, "N3s"), "N5": touched_untouched, "N6": two_touched}
GE_SHAPES = (1.0, 0.96875)  # the two list shapes: best fit, and good-enough lists with a threshold above every fitness of these pools


def _same(tag, got, want):
    for name, g, w in zip(("job_to_offer", "fail_code"), got[:2], want[:2]):
        bad = np.nonzero(np.asarray(g) != np.asarray(w))[0]
        assert len(bad) == 0, (tag, name, "differs from the oracle at", bad[:8], np.asarray(g)[bad[:8]], np.asarray(w)[bad[:8]])
    assert got[2] == want[2], (tag, "head_matched", got[2], want[2])


def _form(fitness, algo):
    return 1 if (algo == 1 or fitness >= 3) else (3 if algo == 3 else 0)


def run_near_ties(make_engine, situation, fitness, algo, gaps=None, ges=GE_SHAPES):
    """every gap and the tie control, both index orders, either role as the worse one: the conditions, then the engine against the oracle"""
    sh = shapes(make_engine)
    check_band_literals()
    cancel = situation in CANCEL
    # match_algo 3 on the plain pairs: lease 8 (1 + 2^-k) needs k - 3 fraction bits, and the class-ordered form takes at most 20 (cf_prepare's
    # `kc > 20`: CF_X_NUMBERS, before anything else is looked at) — from k = 24 on the window rounds place the call and the word says why; the
    # wider gaps are placed by the form itself.  Only N1 / N2: their requests (one job and the tiny one) are on the cpus levels
    assert cancel or algo != 3 or situation in ("N1", "N1w", "N2"), "N5 / N6 under match_algo 3 are C5 / C6"
    gaps = gaps if gaps is not None else (GAPS_ABS if cancel else GAPS)
    seen = {}
    n = 0
    for ge in ((1.0,) if algo == 3 else ges):
        params = A.default_params(fitness=fitness, good_enough_fitness=ge, match_algo=algo)
        with make_engine(params) as e:
            for k in (None,) + tuple(gaps):
                for flip in (False, True):
                    for swap in (False, True):
                        if k is None and flip and situation != "T5":
                            continue
                        case = CANCEL[situation](sh, k, flip, swap) if cancel else SITUATIONS[situation](sh, fitness, k, flip, swap)
                        want = oracle_match(params, case.jobs, case.offers)
                        sides = check_pair(case, fitness, k, want, ge)
                        for b, s in sides.items():
                            seen.setdefault(b, set()).add(s)
                        got = e.match(case.jobs, case.offers)
                        st = e.match_stats()
                        _same((case.name, "fitness", fitness, "algo", algo, "good-enough", ge, sides), got, want)
                        if algo == 3 and not cancel and k is not None and k - 3 > 20:
                            assert (st["placement_form"], st["classfit_refused"]) == (0, CF_X_NUMBERS), (case.name, st["placement_form"], hex(st["classfit_refused"]))
                        else:
                            assert st["placement_form"] == _form(fitness, algo), (case.name, st["placement_form"], hex(st["classfit_refused"]))
                            assert algo != 3 or st["classfit_refused"] == 0, (case.name, hex(st["classfit_refused"]))
                        n += 1
    if len(gaps) > 2:
        for b in ((CF, CF32) if cancel else (PRUNE, EPS, GE_NEAR, F32)):
            assert seen.get(b) == {"inside", "outside"}, (b, seen.get(b), "the gap list no longer has both sides of the band")
    return n


def run_nine_rising(make_engine, monkeypatch, fitness, algo, split=1, gaps=GAPS):
    """N4.  With COOK_EVAL_SPLIT=1 a wave's batch is one lane's list (a small window's idle rows otherwise cut it in four): the ninth offer meets a
    full list, and with nine jobs the ninth needs the entry beyond MV_L, so a truncated list runs out (NON-ZERO: trunc_lists, stop_list).
    split 4: parity alone"""
    sh = shapes(make_engine)
    check_band_literals()
    monkeypatch.setenv("COOK_EVAL_SPLIT", str(split))
    for ge in GE_SHAPES:
        params = A.default_params(fitness=fitness, good_enough_fitness=ge, match_algo=algo)
        with make_engine(params) as e:
            for k in (None,) + tuple(gaps):
                for n_jobs in (1, 9):
                    case = nine_rising(sh, fitness, k, n_jobs)
                    want = oracle_match(params, case.jobs, case.offers)
                    check_pair(case, fitness, k, want, ge)
                    if n_jobs == 9:  # on the oracle alone: one offer each, best first (the tie control: lowest index first)
                        assert list(want[0][:9]) == (case.idx if k is None else case.idx[::-1]), (case.name, want[0])
                    got = e.match(case.jobs, case.offers)
                    st = e.match_stats()
                    _same((case.name, fitness, algo, ge), got, want)
                    if n_jobs == 9 and algo != 1 and split == 1:
                        assert st["placement_form"] == 0 and st["trunc_lists"] > 0 and st["stop_list"] > 0, (case.name, st["trunc_lists"], st["stop_list"])
    monkeypatch.delenv("COOK_EVAL_SPLIT")


def run_spreader_control(make_engine):
    """control of the oracle comparison: cpuMemSpreader goes to the serial sweep whatever match_algo says, and takes the EMPTIER offer of a pair"""
    sh = shapes(make_engine)
    case = two_untouched(sh, 0, 39, False, False, "N1")
    params = A.default_params(fitness=3, good_enough_fitness=1.0, match_algo=0)
    want = FO.match(params, case.jobs, case.offers)
    assert want[0][0] == max(case.pair, key=lambda v: case.offers.cpus[v]) != case.expect
    with make_engine(params) as e:
        got = e.match(case.jobs, case.offers)
        assert e.match_stats()["placement_form"] == 1
    _same("spreader", got, want)


# ---- N7: good-enough ---------------------------------------------------------------------------------------------------------------------------------
def good_enough_case(sh, fitness, touched: bool, D=8.0, c0=5.0, c1=2.0):
    """offers a < b < c: b decides (x (5 + 2) / 8, y (1024 + 512) / 4096: fitness F, exact), a the same total times (1 + 2^-18) — just below F —,
    c far above (x (13 + 2) / 16).  touched: b's x 5, y 1024 come from job 0, which fits b alone; else b runs them"""
    a, b, c = 4, sh.MV_OCW + 2, 2 * sh.MV_OCW + 3
    assert c1 + 1.0 < c0 and c0 > D - c0 and (c0 + c1) / D < (2 * D - 1.0) / (2 * D)
    placed = {a: (_free(_tot(D, A_GAP), c0), c0, 3072.0, 1024.0),
              b: (D, 0.0, 4096.0, 0.0) if touched else (D - c0, c0, 3072.0, 1024.0),
              c: (c1 + 1.0, 2 * D - c1 - 1.0, 3072.0, 1024.0)}
    jobs = ([(c0, 1024.0)] if touched else []) + [(c1, 512.0)]
    case = _pool(f"N7 touched={touched} D={D}", fitness, 2 * sh.MV_OCW + 9, placed, jobs, (a, b), len(jobs) - 1, None)
    case.abc = (a, b, c)
    return case


def thresholds(F: float, gaps=GAPS):
    """-> [(name, good-enough, is F above it)]: F itself is NOT above (the reference is strict, cook_oracle.cpp:479)"""
    out = [("F", F, False), ("nextafter(F, 0)", float(np.nextafter(F, 0.0)), True), ("nextafter(F, 1)", float(np.nextafter(F, 1.0)), False)]
    for k in gaps:
        out.append((f"F (1 + 2^-{k})", F + F * 2.0 ** -k, False))
        out.append((f"F (1 - 2^-{k})", F - F * 2.0 ** -k, True))
    return out


def run_good_enough(make_engine, fitness, algo, touched, inexact=None):
    """inexact 'above' / 'below': the deciding offer's total has a rounded reciprocal and its approximate fitness lies on that side of F; the threshold
    is then F itself (fp64; the reference compares fp64 values) and its two neighbours, not the real value's"""
    sh = shapes(make_engine)
    check_band_literals()
    dims = inexact_reciprocal(fitness, inexact == "above") if inexact else (8.0, 5.0, 2.0)
    case = good_enough_case(sh, fitness, touched, *dims)
    a, b, c = case.abc
    base = oracle_match(A.default_params(fitness=fitness, good_enough_fitness=1.0), case.jobs, case.offers)
    (fa, ra), (fb, rb) = pair_values(case, fitness, base[0])
    if inexact:
        ap = touched_approx(fitness, *dims)
        assert (ap > fb) if inexact == "above" else (ap < fb), (dims, ap, fb)
        rb = Fraction(fb)  # (the side of the threshold is the fp64 value's: the real value is not a double here)
    assert Fraction(fb) == rb, "the deciding offer's fitness is exact in fp64"
    assert fa < fb and ra < rb and Fraction(1, 2 ** (A_GAP + 1)) < (rb - ra) / rb < Fraction(1, 2 ** A_GAP)
    assert base[0][case.job] == c, "best fit is the third offer"
    F = fb
    winners = set()
    with make_engine(A.default_params(fitness=fitness, good_enough_fitness=1.0, match_algo=algo)) as e:
        for name, ge, above in (thresholds(F)[:3] if inexact else thresholds(F)):
            # on the inputs alone: the side of the threshold in fp64 is the side of the real values; the offer below stays below
            assert (F > ge) == above and (rb > Fraction(ge)) == above, (name, F, ge)
            assert not fa > ge and not ra > Fraction(ge), (name, fa, ge)
            params = A.default_params(fitness=fitness, good_enough_fitness=ge, match_algo=algo)
            want = oracle_match(params, case.jobs, case.offers)
            assert want[0][case.job] == (b if above else c), (name, want[0], "first offer above the threshold in array order")
            winners.add(int(want[0][case.job]))
            e.set_params(params)
            got = e.match(case.jobs, case.offers)
            st = e.match_stats()
            _same((case.name, name, "fitness", fitness, "algo", algo), got, want)
            assert st["placement_form"] == _form(fitness, algo), st["placement_form"]
    assert winners == {b, c}


# ---- cook_cycle_match_multi: two pools, served and lockstep -----------------------------------------------------------------------------------
def as_cycle_pool(jobs: A.Jobs, offers: A.Offers, groups=None):
    """one user whose pending jobs rank in the order given (the per-user order of pending tasks is the job id's)"""
    n = jobs.n
    t = A.Tasks(cpus=jobs.cpus.copy(), mem=jobs.mem.copy(), user=np.zeros(n, np.uint32), priority=np.full(n, 50, np.int32), start_ms=np.zeros(n, np.int64),
                task_id=(ID_BASE + 2_000_000_000 + np.arange(n)).astype(np.int64), job_id=(ID_BASE + np.arange(n)).astype(np.int64), pending=np.ones(n, np.uint8))
    return SimpleNamespace(tasks=t, users=A.Users(div_cpus=np.ones(1), div_mem=np.ones(1)), pending_jobs=jobs, offers=offers, groups=groups)


def run_multi(make_engine, cases, params):
    """the cases as the pools of ONE cook_cycle_match_multi behind one cook_cycle_run_rank_multi: every pool's placement equals the oracle's"""
    from cook_amd.engine import cycle_match_multi, cycle_run_rank_multi
    pools = [as_cycle_pool(c.jobs, c.offers, c.groups) for c in cases]
    engines = [make_engine(params) for _ in pools]
    try:
        for e, pool in zip(engines, pools):
            e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        cycle_run_rank_multi(engines, 10 ** 9)
        cycle_match_multi(engines)
        got = [e.cycle_fetch() for e in engines]
        forms = [e.match_stats()["placement_form"] for e in engines]
    finally:
        for e in engines:
            e.close()
    for c, (ranked, j2o, head), form in zip(cases, got, forms):
        assert np.array_equal(ranked, np.arange(c.jobs.n)), (c.name, "the queue is not the order given", ranked)
        want = pyoracle.match(params, c.jobs, c.offers, c.groups, ())
        assert np.array_equal(j2o, want[0]) and head == want[2], (c.name, j2o, want[0])
        assert form == 0, (c.name, form)


def run_multi_near_ties(make_engine, situation, gaps=(52, 41, 39, 37, 24, 21, 19)):
    """N5 / N6 as two pools of one chain — the pair one way round in one pool, the other way round in the other — at fitness 0"""
    sh = shapes(make_engine)
    params = A.default_params(fitness=0, good_enough_fitness=1.0, max_over_quota_jobs=2 ** 30)
    for k in (None,) + tuple(gaps):
        for flip in ((False,) if k is None else (False, True)):
            cases = [SITUATIONS[situation](sh, 0, k, flip, swap) for swap in (False, True)]
            for c in cases:
                check_pair(c, 0, k, pyoracle.match(params, c.jobs, c.offers, None, ()))
            run_multi(make_engine, cases, params)


def run_multi_good_enough(make_engine, gaps=(52, 41, 39, 31, 29)):
    """N7 as two pools of one chain: the deciding offer untouched in one, touched in the other, under the same threshold"""
    sh = shapes(make_engine)
    cases = [good_enough_case(sh, 0, False), good_enough_case(sh, 0, True)]
    base = pyoracle.match(A.default_params(good_enough_fitness=1.0), cases[0].jobs, cases[0].offers, None, ())
    F = pair_values(cases[0], 0, base[0])[1][0]
    for name, ge, above in thresholds(F, gaps):
        params = A.default_params(fitness=0, good_enough_fitness=ge, max_over_quota_jobs=2 ** 30)
        for c in cases:
            assert pyoracle.match(params, c.jobs, c.offers, None, ())[0][c.job] == (c.abc[1] if above else c.abc[2]), (c.name, name)
        run_multi(make_engine, cases, params)


# ================================================================================================================================================
# PART 2
# ================================================================================================================================================
STAT_KEYS = ("rounds", "segments", "stop_list", "stop_full", "stop_group", "stop_window", "trunc_lists", "touched", "visited")


def run_logged(make_engine, monkeypatch, tmp_path, params, jobs, offers, groups=None, env=()):
    """one match with the per-round log kept -> (results, statistics, the log's rows as dicts of ints)"""
    path = os.path.join(str(tmp_path), "rounds.csv")
    monkeypatch.setenv("COOK_ROUND_LOG", path)
    monkeypatch.setenv("COOK_WGROW_PCT", "200")  # (the growth factor otherwise follows the number of engines on the device)
    for name, val in env:
        monkeypatch.setenv(name, val)
    try:
        with make_engine(params) as e:
            got = e.match(jobs, offers, groups)
            st = e.match_stats()
    finally:
        for name in ("COOK_ROUND_LOG", "COOK_WGROW_PCT") + tuple(n for n, _ in env):
            monkeypatch.delenv(name, raising=False)
    with open(path) as f:
        rows = [{k: int(r[k]) for k in ("head", "wcur", "resolved", "n_list", "touched", "stop", "matched", "segments")} for r in csv.DictReader(f)]
    os.remove(path)
    return got, st, rows


def first_window(sh, K: int) -> int:
    """match_host.hpp first_window, restated"""
    return max(min(K, sh.MV_WEVAL), 1) if K <= 2 * sh.MV_WEVAL else min(sh.MV_WEVAL, 128)


def next_window(sh, K, row, wlong=True, pct=200) -> int:
    """match_v2_resolve.hpp resolve_finish, restated: the window behind the round that `row` of the log describes"""
    nwin = min(row["wcur"], K - row["head"])
    wn = row["wcur"] * 2 if row["stop"] == 0 else (row["resolved"] * pct + 99) // 100
    wn = max(wn, 64)
    cap = sh.MV_WEVAL
    if row["stop"] == 0 and nwin >= sh.MV_WEVAL and row["n_list"] * 8 <= nwin:
        cap = max(cap, sh.MV_WLONG if wlong else sh.MV_WEVAL)
    return min(wn, cap)


def check_log(sh, K, st, rows, wlong=True):
    """EXACT, from first_window and resolve_finish: the first window, every later one, the heads, the counts of match_stats()"""
    assert len(rows) == st["rounds"] >= 1, (len(rows), st["rounds"])
    assert rows[0]["head"] == 0 and rows[0]["wcur"] == first_window(sh, K), (rows[0], first_window(sh, K))
    for a, b in zip(rows, rows[1:]):
        assert b["head"] == a["head"] + a["resolved"], (a, b)
        assert b["wcur"] == next_window(sh, K, a, wlong), (a, b, next_window(sh, K, a, wlong))
    assert rows[-1]["head"] + rows[-1]["resolved"] == K, rows[-1]
    assert st["stop_window"] == sum(r["stop"] == 0 for r in rows) and st["stop_list"] == sum(r["stop"] == 1 for r in rows)
    assert st["stop_full"] == sum(r["stop"] in (2, 5) for r in rows) and st["stop_group"] == sum(r["stop"] == 3 for r in rows)
    assert st["segments"] == sum(r["segments"] for r in rows) and st["touched"] == sum(r["touched"] for r in rows)


# ---- offers: M at every batch, word and chunk edge -------------------------------------------------------------------------------------------
def offer_sizes(sh) -> dict:
    W, B = sh.MV_OCW, sh.MV_OCB
    return {"1": 1, "2": 2, "batch-1": W - 1, "batch": W, "batch+1": W + 1, "63": 63, "64": 64, "65": 65, "chunk-1": B - 1, "chunk": B, "chunk+1": B + 1,
            "two_chunks+1": 2 * B + 1, "64_chunks-1": 64 * B - 1, "64_chunks": 64 * B, "64_chunks+1": 64 * B + 1}


OFFER_SIZES = ("1", "2", "batch-1", "batch", "batch+1", "63", "64", "65", "chunk-1", "chunk", "chunk+1", "two_chunks+1", "64_chunks-1", "64_chunks",
               "64_chunks+1")


def offers_edge_case(sh, M: int):
    """target offers at index 0, M - 1 and on both sides of every boundary below M; job i fits target i alone (cpus rise with i, mem falls); one
    job that fits the targets on resources and nothing by its EQUALS pair (fail code 3: c1 counts the fillers over a partial last chunk and
    alive word, c2 the targets); fillers too small for anything"""
    bounds = [b for b in (sh.MV_OCW, 64, sh.MV_OCB, 2 * sh.MV_OCB, 64 * sh.MV_OCB) if b <= M]
    targets = sorted({0, M - 1} | {b - 1 for b in bounds} | {b for b in bounds if b < M})
    n = len(targets)
    cpus, mem = np.full(M, 0.25), np.full(M, 512.0)
    for i, v in enumerate(targets):
        cpus[v], mem[v] = 2.5 + i, (n - i) * 1024.0 + 256.0  # (half a cpu and 256 MB to spare: the constrained job fits every target on resources)
    attr = np.ones((M, 1), np.uint32)
    offers = A.Offers(cpus=cpus, mem=mem, attr=attr, k8s=np.ones(M, np.uint8))
    order = np.random.default_rng(M).permutation(n)
    jc, jm = [2.0 + i for i in order], [(n - i) * 1024.0 for i in order]
    eq = [[] for _ in order]
    jc.insert(1, 0.5), jm.insert(1, 256.0), eq.insert(1, [(0, 7)])
    jobs = A.Jobs.with_constraints(np.array(jc), np.array(jm), equals=eq)
    return jobs, offers, targets, order


def run_offers_edge(make_engine, size: str, ge: float):
    sh = shapes(make_engine)
    assert tuple(offer_sizes(sh)) == OFFER_SIZES
    M = offer_sizes(sh)[size]
    jobs, offers, targets, order = offers_edge_case(sh, M)
    params = A.default_params(good_enough_fitness=ge, match_algo=2)
    want = pyoracle.match(params, jobs, offers, None, ())
    # on the oracle alone: every target is taken by its own job, the constrained job by nothing, with both failure classes
    w = np.delete(want[0], 1)
    assert [int(x) for x in w] == [targets[i] for i in order] and want[0][1] == -1 and want[1][1] == (3 if M > len(targets) else 2), (want, targets)
    with make_engine(params) as e:
        got = e.match(jobs, offers)
        st = e.match_stats()
    _same(("offers", size, M, ge), got, want)
    assert st["guard_hits"] == 0, st["guard_hits"]  # (COOK_GUARD=1 runs: no write outside a device buffer)
    print("offers", size, M, {k: st[k] for k in STAT_KEYS})
    # EXACT (first_window: K <= 2 MV_WEVAL is one window; nothing ends it early: every job's offer is the head of its list): one round that the window ends;
    # touched_sum counts an offer per placed job
    assert st["placement_form"] == 0 and st["rounds"] == 1 and st["stop_window"] == 1 and st["touched"] == len(targets), st
    assert st["visited"] > 0  # NON-ZERO


# ---- jobs and windows ---------------------------------------------------------------------------------------------------------------------------
def job_sizes(sh) -> dict:
    W = sh.MV_WEVAL
    lo, hi = 64 * (sh.MV_JG // 4), 64 * (sh.MV_JG // 2)  # up to here eval_split gives 4 / 2
    d = {"1": 1, "63": 63, "64": 64, "65": 65}
    for name, v in (("split4", lo), ("split2", hi), ("weval", W)):
        d.update({f"{name}-1": v - 1, name: v, f"{name}+1": v + 1})
    d.update({"two_weval": 2 * W, "two_weval+1": 2 * W + 1})
    return d


JOB_SIZES = ("1", "63", "64", "65", "split4-1", "split4", "split4+1", "split2-1", "split2", "split2+1", "weval-1", "weval", "weval+1", "two_weval",
             "two_weval+1")
SPLIT_SIZES = tuple(s for s in JOB_SIZES if s.startswith("split"))


def window_pool(K: int, M: int = 150, seed: int = 5):
    """an ordinary over-subscribed pool: about two thirds of the jobs find room"""
    rng = np.random.default_rng(seed + K)
    jobs = A.Jobs(cpus=rng.integers(1, 4, K).astype(float), mem=rng.integers(1, 5, K) * 1024.0)
    per = max(4.0, np.ceil(0.66 * jobs.cpus.sum() / M))
    offers = A.Offers(cpus=per + rng.integers(0, 3, M), mem=(per + rng.integers(0, 3, M)) * 1536.0, run_cpus=rng.integers(0, 5, M).astype(float),
                      run_mem=rng.integers(0, 5, M) * 1024.0, k8s=np.ones(M, np.uint8))
    return jobs, offers


def run_window_size(make_engine, monkeypatch, tmp_path, size: str, split=None, ge=1.0):
    """K at a window edge: parity, and the log follows first_window / resolve_finish (EXACT: check_log) — the first wcur among them"""
    sh = shapes(make_engine)
    assert tuple(job_sizes(sh)) == JOB_SIZES
    K = job_sizes(sh)[size]
    jobs, offers = window_pool(K)
    params = A.default_params(good_enough_fitness=ge, match_algo=2)
    want = pyoracle.match(params, jobs, offers, None, ())
    got, st, rows = run_logged(make_engine, monkeypatch, tmp_path, params, jobs, offers, env=(("COOK_EVAL_SPLIT", str(split)),) if split else ())
    _same(("window", size, K, split), got, want)
    check_log(sh, K, st, rows)
    if split:  # on the rule alone: the sizes are the last with a cut in four / in two, and the first without
        lo, hi = 64 * (sh.MV_JG // 4), 64 * (sh.MV_JG // 2)
        assert eval_split(sh, lo, 4) == 4 and eval_split(sh, lo + 1, 4) == 2 and eval_split(sh, hi, 4) == 2 and eval_split(sh, hi + 1, 4) == 1
    print("window", size, K, split, [(r["head"], r["wcur"], r["resolved"], r["stop"]) for r in rows][:12], {k: st[k] for k in STAT_KEYS})
    assert rows[0]["wcur"] == (128 if K > 2 * sh.MV_WEVAL else min(K, sh.MV_WEVAL)), rows[0]
    return st


def full_cluster_windows(sh, K, wlong=True):
    """the windows of a call nothing of which can be placed or has to be walked: every round ends with its window (stop 0, n_list 0)"""
    out, head, w = [], 0, first_window(sh, K)
    while head < K:
        n = min(w, K - head)
        out.append((head, w))
        w = next_window(sh, K, dict(head=head, wcur=w, resolved=n, n_list=0, stop=0), wlong)
        head += n
    return out


def long_window_end(sh) -> int:
    """the end of the first window of MV_WLONG jobs of such a call"""
    seq = full_cluster_windows(sh, 64 * sh.MV_WLONG)
    head, w = next((h, w) for h, w in seq if w == sh.MV_WLONG)
    return head + w


LONG_K = ("end-1", "end", "end+1")


def run_full_cluster(make_engine, monkeypatch, tmp_path, which: str, wlong=True):
    """eight offers, all too small for any job: the windows double from the first to MV_WEVAL and, nothing being walked, on to MV_WLONG (or stay at
    MV_WEVAL under COOK_WLONG=0).  EXACT: the (head, wcur) sequence of the log is the one first_window and resolve_finish give"""
    sh = shapes(make_engine)
    K = long_window_end(sh) + {"end-1": -1, "end": 0, "end+1": 1}[which]
    rng = np.random.default_rng(3)
    jobs = A.Jobs(cpus=rng.integers(2, 5, K).astype(float), mem=rng.integers(2, 5, K) * 1024.0)
    offers = A.Offers(cpus=np.full(8, 1.0), mem=np.full(8, 1024.0), k8s=np.ones(8, np.uint8))
    params = A.default_params(good_enough_fitness=1.0, match_algo=2)
    want = pyoracle.match(params, jobs, offers, None, ())
    assert (want[0] == -1).all() and (want[1] == 1).all()
    got, st, rows = run_logged(make_engine, monkeypatch, tmp_path, params, jobs, offers, env=() if wlong else (("COOK_WLONG", "0"),))
    _same(("full cluster", which, K, wlong), got, want)
    assert st["guard_hits"] == 0, st["guard_hits"]  # (COOK_GUARD=1 runs: no write outside a device buffer)
    check_log(sh, K, st, rows, wlong)
    seq = full_cluster_windows(sh, K, wlong)
    print("full cluster", which, K, wlong, seq, {k: st[k] for k in STAT_KEYS})
    assert [(r["head"], r["wcur"]) for r in rows] == seq and all(r["stop"] == 0 and r["n_list"] == 0 for r in rows), rows
    assert max(w for _, w in seq) == (sh.MV_WLONG if wlong else sh.MV_WEVAL)
    assert st["stop_window"] == len(seq) and st["visited"] == 0 and st["touched"] == 0


# ---- lists ------------------------------------------------------------------------------------------------------------------------------------------
def one_job_each(M, feasible, W, tail=0):
    """offers `feasible` each hold exactly one of W identical jobs (cpus 4 of 6), every other offer none: equal fitness sends job i to the i-th"""
    cpus = np.full(M, 0.5)
    cpus[list(feasible)] = 6.0
    return A.Jobs(cpus=np.full(W, 4.0), mem=np.full(W, 1024.0)), A.Offers(cpus=cpus, mem=np.full(M, 4096.0), k8s=np.ones(M, np.uint8))


def run_list_in_chunk(make_engine, monkeypatch, n_feasible: int, ge: float):
    """MV_L | MV_L + 1 feasible offers in one wave's batch and as many jobs, under COOK_EVAL_SPLIT=1 (the batch is one list).  MV_L: every job's
    offer is in its list (EXACT: no list runs out, one round); MV_L + 1: the last job needs the entry beyond MV_L (NON-ZERO: trunc_lists, stop_list)"""
    sh = shapes(make_engine)
    assert n_feasible in (sh.MV_L, sh.MV_L + 1)
    feas = [2 + 3 * i for i in range(n_feasible)]
    assert feas[-1] < sh.MV_OCW
    monkeypatch.setenv("COOK_EVAL_SPLIT", "1")
    jobs, offers = one_job_each(sh.MV_OCB, feas, n_feasible)
    params = A.default_params(good_enough_fitness=ge, match_algo=2)
    want = pyoracle.match(params, jobs, offers, None, ())
    assert list(want[0]) == feas
    with make_engine(params) as e:
        got = e.match(jobs, offers)
        st = e.match_stats()
    monkeypatch.delenv("COOK_EVAL_SPLIT")
    _same(("list in chunk", n_feasible, ge), got, want)
    assert st["guard_hits"] == 0, st["guard_hits"]  # (COOK_GUARD=1 runs: no write outside a device buffer)
    print("list in chunk", n_feasible, ge, {k: st[k] for k in STAT_KEYS})
    if n_feasible == sh.MV_L:
        assert st["stop_list"] == 0 and st["rounds"] == 1, st
    else:
        assert st["trunc_lists"] > 0 and st["stop_list"] > 0, st


def run_list_over_chunks(make_engine, extra: int, ge: float):
    """one feasible offer per chunk over LM | LM + 1 chunks (LM of the list shape that good-enough selects), as many jobs.  LM: the merged list is
    complete (EXACT: trunc_lists 0, stop_list 0); LM + 1: it holds LM entries and some lane holds more (NON-ZERO: trunc_lists, stop_list)"""
    sh = shapes(make_engine)
    LM = sh.LM if ge >= 1.0 else sh.LM_GE
    n = LM + extra
    feas = [ch * sh.MV_OCB + (7 * ch) % sh.MV_OCB for ch in range(n)]
    jobs, offers = one_job_each(n * sh.MV_OCB, feas, n)
    params = A.default_params(good_enough_fitness=ge, match_algo=2)
    want = pyoracle.match(params, jobs, offers, None, ())
    assert list(want[0]) == feas
    with make_engine(params) as e:
        got = e.match(jobs, offers)
        st = e.match_stats()
    _same(("list over chunks", n, ge), got, want)
    assert st["guard_hits"] == 0, st["guard_hits"]  # (COOK_GUARD=1 runs: no write outside a device buffer)
    print("list over chunks", n, ge, {k: st[k] for k in STAT_KEYS})
    if extra == 0:
        assert st["trunc_lists"] == 0 and st["stop_list"] == 0, st
    else:
        assert st["trunc_lists"] > 0 and st["stop_list"] > 0, st


def run_good_enough_list(make_engine, extra: int, touched_low: bool):
    """The two sides of `tg > g_off[ng - 1]` (match_v2_resolve.hpp, good-enough fast path) with gtrunc set.  n = LG | LG + 1 small offers above the
    threshold, each holding one small job; the first LG of them are every small job's good-enough list (gtrunc: the merge sets it from LG on).
    A big offer T is below the threshold for a small job while untouched — so it is on no list — and above it once the big job, which fits T alone,
    sits on it.  Jobs: LG small ones (they take the listed offers, in array order), the big one (T), two more small ones.  Those two find EVERY
    listed offer taken and T touched, feasible and above the threshold:
      touched_low  T at index 1, in front of the list's last entry: every offer in front of T is a filler or listed and taken, so the fast path
                   gives the job to T.  EXACT (that rule): no list runs out, stop_list 0, one round.
      else         T behind every small offer: unlisted offers above the threshold may lie between the list's last entry and T (with LG + 1 one
                   does, and the oracle places on it), so the job leaves the fast path and the truncated list is exhausted.  NON-ZERO: stop_list,
                   and more than one round.
    The LG small offers are full to the smallest job behind their own (their lanes are given away, so T finds a lane)."""
    sh = shapes(make_engine)
    n = sh.LG + extra
    M = n + 12
    small = [3 + i for i in range(n)]
    T = 1 if touched_low else M - 2
    cpus, mem = np.full(M, 0.5), np.full(M, 65536.0)
    cpus[small] = 6.0
    cpus[T] = 30.0
    jc = [4.0] * sh.LG + [22.0] + [4.0] * 2
    jobs = A.Jobs(cpus=np.array(jc), mem=np.full(len(jc), 1024.0))
    offers = A.Offers(cpus=cpus, mem=mem, k8s=np.ones(M, np.uint8))
    ge = 0.3
    params = A.default_params(good_enough_fitness=ge, match_algo=2)
    # on the inputs alone: a small job on a small offer is above the threshold, on T below it until the big job is there, above it from then on
    assert fit64(0, 0.0, 0.0, 4.0, 6.0, 0.0, 0.0, 1024.0, 65536.0) > ge > fit64(0, 0.0, 0.0, 4.0, 30.0, 0.0, 0.0, 1024.0, 65536.0)
    assert fit64(0, 0.0, 22.0, 4.0, 30.0, 0.0, 1024.0, 1024.0, 65536.0) > ge
    want = pyoracle.match(params, jobs, offers, None, ())
    big = sh.LG
    # on the oracle alone: the listed offers in array order, the big job on T, the last two on T — or, T behind and LG + 1, the first on the unlisted offer
    assert list(want[0][:big]) == small[:sh.LG] and want[0][big] == T, want[0]
    assert list(want[0][big + 1:]) == ([small[sh.LG], T] if (extra and not touched_low) else [T, T]), want[0]
    with make_engine(params) as e:
        got = e.match(jobs, offers)
        st = e.match_stats()
    _same(("good-enough list", n, touched_low), got, want)
    assert st["guard_hits"] == 0, st["guard_hits"]  # (COOK_GUARD=1 runs: no write outside a device buffer)
    print("good-enough list", n, touched_low, list(want[0][-3:]), {k: st[k] for k in STAT_KEYS})
    assert st["placement_form"] == 0
    if touched_low:
        assert st["stop_list"] == 0 and st["rounds"] == 1 and st["stop_window"] == 1, st
    else:
        assert st["stop_list"] > 0 and st["rounds"] > 1, st


# ---- the touched set ---------------------------------------------------------------------------------------------------------------------------------
def touched_set_case(W: int, full: bool, ports: bool):
    """W jobs that each open an offer of their own: job i (mem falls with i) fits the offers 0 .. i and offer i best.  full: the offers are then
    full to the smallest job (dead: their lanes may be given away); else a tiny last job keeps them alive.  ports: every job asks for a port"""
    M = W + 7
    mem = np.array([(M - i) * 1024.0 + (0.0 if full else 512.0) for i in range(M)])
    offers = A.Offers(cpus=np.full(M, 4.0), mem=mem, k8s=np.ones(M, np.uint8), **(dict(ports=np.full(M, 4, np.int32)) if ports else {}))
    jc = [2.5] * W + ([] if full else [0.5])
    jm = [(M - i) * 1024.0 for i in range(W)] + ([] if full else [256.0])
    jobs = A.Jobs(cpus=np.array(jc), mem=np.array(jm), **(dict(ports=np.ones(len(jc), np.int32)) if ports else {}))
    return jobs, offers


def run_touched_set(make_engine, which: str):
    """EXACT (alloc_lane: the next free lane of MV_T, else the lane of a dead offer unless has_x or MV_RETIRE_CAP, else the round ends):
       T     MV_T offers opened in one window, all alive: stop_full 0, one round
       T+1   one more: stop_full 1, two rounds
       full  MV_T + 8 offers, each dead behind its job: lanes are given away, stop_full 0, one round that touches them all
       ports the same with a ports request on every job (has_x switches the give-away off): stop_full 1"""
    sh = shapes(make_engine)
    W, full, ports = {"T": (sh.MV_T, False, False), "T+1": (sh.MV_T + 1, False, False), "full": (sh.MV_T + 8, True, False), "ports": (sh.MV_T + 8, True, True)}[which]
    assert W - sh.MV_T <= sh.MV_RETIRE_CAP
    jobs, offers = touched_set_case(W, full, ports)
    params = A.default_params(good_enough_fitness=1.0, match_algo=2)
    want = pyoracle.match(params, jobs, offers, None, ())
    assert list(want[0][:W]) == list(range(W)) and (want[0] >= 0).all(), want[0]
    with make_engine(params) as e:
        got = e.match(jobs, offers)
        st = e.match_stats()
    _same(("touched set", which), got, want)
    assert st["guard_hits"] == 0, st["guard_hits"]  # (COOK_GUARD=1 runs: no write outside a device buffer)
    print("touched set", which, {k: st[k] for k in STAT_KEYS})
    exp_full, exp_rounds = {"T": (0, 1), "T+1": (1, 2), "full": (0, 1), "ports": (1, 2)}[which]
    assert st["placement_form"] == 0 and st["stop_full"] == exp_full and st["rounds"] == exp_rounds and st["stop_list"] == 0, st
    # ... and `touched` sums, per round, the offers that round placed on: a round ends in front of the job that needs a lane beyond MV_T
    per_round, seen = [], set()
    for v in want[0].tolist():
        if v not in seen and len(seen) == sh.MV_T and which != "full":
            per_round.append(len(seen))
            seen = set()
        seen.add(v)
    per_round.append(len(seen))
    assert len(per_round) == exp_rounds and st["touched"] == sum(per_round), (st["touched"], per_round)


# ---- constraint slots ----------------------------------------------------------------------------------------------------------------------------------
CONSTRAINT_CASES = ("equals_nc", "equals_nc+1", "novel_nc", "novel_nc+1", "key_na-1", "key_na", "unique_fh", "unique_fh+1")


def constraint_case(sh, which: str):
    """a deterministic slow_constraint_case: one constrained job whose LAST pair / host / cotask bars the otherwise best offer (index 5); the
    second best (index 40) takes it.  -> (jobs, offers, groups, the constrained job, best, second)"""
    M, best, second = 70, 5, 40
    cpus = np.full(M, 16.0)
    run = np.zeros(M)
    run[best], run[second] = 10.0, 8.0  # fullest, second fullest
    n_keys = sh.MV_NA + 2
    attr = np.ones((M, n_keys), np.uint32)
    eq, novel, group, groups = [[]], [[]], np.array([A.NONE_U32], np.uint32), None
    if which.startswith("equals"):
        n = sh.MV_NC + (1 if which.endswith("+1") else 0)
        attr[best, n - 1] = 2
        eq = [[(q, 1) for q in range(n)]]
    elif which.startswith("novel"):
        n = sh.MV_NC + (1 if which.endswith("+1") else 0)
        novel = [[60 + q for q in range(n - 1)] + [best]]  # (host = offer index)
    elif which.startswith("key"):
        key = sh.MV_NA - (1 if which.endswith("-1") else 0)
        attr[best, key] = 2
        eq = [[(key, 1)]]
    else:  # a unique group: cotasks on n hosts, half of them running, half placed by the jobs in front; the last placed one sits on `best`
        n = sh.MV_FH + (1 if which.endswith("+1") else 0)
        groups = A.Groups(type=np.array([1], np.uint8), run_hosts=[[60 + q for q in range(n // 2)]])
    jobs_c, jobs_m = [2.0], [1024.0]
    if groups is not None:
        # the members in front: each pinned to one host by its size (cpus rise, mem falls), the last of them to `best`
        n_front = n - n // 2
        hosts = [20 + q for q in range(n_front - 1)] + [best]
        mem = np.full(M, 8192.0)
        for i, h in enumerate(hosts):
            cpus[h], mem[h] = 20.0 + i, 8192.0 + (n_front - i) * 1024.0
        cpus[best] += 2.0  # room for the job under test behind the member it holds
        mem[best] += 512.0
        run[best] = 30.0
        jobs_c = [20.0 + i for i in range(n_front)] + [2.0]
        jobs_m = [8192.0 + (n_front - i) * 1024.0 for i in range(n_front)] + [512.0]
        group = np.zeros(n_front + 1, np.uint32)
        eq, novel = [[] for _ in jobs_c], [[] for _ in jobs_c]
        offers = A.Offers(cpus=cpus, mem=mem, run_cpus=run, attr=attr, k8s=np.ones(M, np.uint8))
    else:
        offers = A.Offers(cpus=cpus, mem=np.full(M, 8192.0), run_cpus=run, attr=attr, k8s=np.ones(M, np.uint8))
    jobs = A.Jobs.with_constraints(np.array(jobs_c), np.array(jobs_m), equals=eq, novel=novel, group=group)
    return jobs, offers, groups, len(jobs_c) - 1, best, second


def run_constraint_slots(make_engine, which: str, ge=1.0):
    """parity; on the oracle alone: without its constraints the job takes `best`, with them `second` (so the last slot decides).  The path (fast
    slots or the general check) is not part of any public observation: both sides of MV_NC / MV_NA / MV_FH must simply be RIGHT"""
    sh = shapes(make_engine)
    jobs, offers, groups, job, best, second = constraint_case(sh, which)
    params = A.default_params(good_enough_fitness=ge, match_algo=2)
    want = pyoracle.match(params, jobs, offers, groups, ())
    free = pyoracle.match(params, A.Jobs(cpus=jobs.cpus, mem=jobs.mem), offers, None, ())
    assert free[0][job] == best and want[0][job] == second, (which, free[0], want[0])
    if groups is not None:
        assert want[0][job - 1] == best, (which, "the last member in front sits on the best offer", want[0])
    with make_engine(params) as e:
        got = e.match(jobs, offers, groups)
        st = e.match_stats()
    _same(("constraint slots", which), got, want)
    assert st["placement_form"] == 0


# ---- groups: the round that ends on the second member ----------------------------------------------------------------------------------------
def run_group_barrier(make_engine, gtype: int):
    """two members of a balanced (2) / attribute-equals (3) group in one window: the second one ends the round (NON-ZERO: stop_group)"""
    M, K = 40, 24
    rng = np.random.default_rng(gtype)
    attr = np.stack([1 + np.arange(M) % 3, 1 + np.arange(M) % 4], axis=1).astype(np.uint32)
    offers = A.Offers(cpus=rng.integers(6, 12, M).astype(float), mem=rng.integers(6, 12, M) * 1024.0, attr=attr, k8s=np.ones(M, np.uint8))
    group = np.full(K, A.NONE_U32, np.uint32)
    group[[3, 9, 10, 20]] = 0
    jobs = A.Jobs(cpus=rng.integers(1, 4, K).astype(float), mem=rng.integers(1, 4, K) * 1024.0, group=group)
    groups = A.Groups(type=np.array([gtype], np.uint8), attr_key=np.array([1], np.uint32), minimum=np.array([2], np.int32))
    params = A.default_params(good_enough_fitness=1.0, match_algo=2)
    want = pyoracle.match(params, jobs, offers, groups, ())
    assert (want[0][[3, 9, 10, 20]] >= 0).all()
    with make_engine(params) as e:
        got = e.match(jobs, offers, groups)
        st = e.match_stats()
    _same(("group barrier", gtype), got, want)
    print("group barrier", gtype, {k: st[k] for k in STAT_KEYS})
    assert st["placement_form"] == 0 and st["stop_group"] > 0 and st["rounds"] > st["stop_group"], st


# ---- the owner table (GPU file only) ---------------------------------------------------------------------------------------------------------------
def owner_table_offers(M: int):
    cpus, mem = np.full(M, 0.5), np.full(M, 512.0)
    for v in (0, M // 2, M - 1):
        cpus[v], mem[v] = 128.0, 1048576.0  # (the 200 jobs ask for about 400 cpus: they fill all three, the last ones find no room)
    return A.Offers(cpus=cpus, mem=mem, k8s=np.ones(M, np.uint8))


def run_refusal_keeps_the_last_match(make_engine, M_big=200_000):
    """a pool beyond the owner table is refused when it is STAGED, with the other checks on the inputs: the match before it is still fetched.
    (Found by run_owner_table: the refusal used to come from the run, behind the reset of the placement state, and the fetch then failed with
    "before a match has run".)"""
    params = A.default_params(good_enough_fitness=1.0, match_algo=2)
    jobs, offers = window_pool(40, M=30)
    want = pyoracle.match(params, jobs, offers, None, ())
    with make_engine(params) as e:
        _same("the match before", e.match(jobs, offers), want)
        try:
            e.match(jobs, A.Offers(cpus=np.full(M_big, 4.0), mem=np.full(M_big, 4096.0)))
        except CookError as ex:
            assert "too many offers" in str(ex), ex
        else:
            raise AssertionError(f"{M_big} offers were accepted")
        _same("the match before, fetched behind the refused call", e.match_fetch(), want)
        _same("the same match again", e.match(jobs, offers), want)


def run_owner_table(make_engine):
    """the largest pool the walk's offer-owner table holds, by bisection on the engine's own refusal: between 140 000 offers and MV_RLDS_BYTES
    (one LDS byte an offer).  There a segment is MV_WSEG_MIN jobs: 200 jobs that only the offers at 0, M / 2 and M - 1 can take — parity, and
    EXACT (resolve_wseg) segments >= walked jobs / MV_WSEG_MIN.  One offer more is refused before anything of the last match changes"""
    sh = shapes(make_engine)
    params = A.default_params(good_enough_fitness=1.0, match_algo=2)
    rng = np.random.default_rng(9)
    jobs = A.Jobs(cpus=rng.integers(1, 4, 200).astype(float), mem=rng.integers(1, 4, 200) * 1024.0)
    one = A.Jobs(cpus=np.array([1.0]), mem=np.array([1024.0]))
    with make_engine(params) as e:
        def accepted(M):
            try:
                e.match(one, owner_table_offers(M))
                return True
            except CookError as ex:
                assert "too many offers" in str(ex), ex
                return False
        lo, hi = 140_000, sh.MV_RLDS_BYTES  # accepted / refused
        assert accepted(lo) and not accepted(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if accepted(mid) else (lo, mid)
        M = lo
        offers = owner_table_offers(M)
        want = pyoracle.match(params, jobs, offers, None, ())
        assert set(want[0].tolist()) == {0, M // 2, M - 1, -1}
        got = e.match(jobs, offers)
        st = e.match_stats()
        _same(("owner table", M), got, want)
        print("owner table: the largest pool is", M, "offers;", {k: st[k] for k in STAT_KEYS})
        assert st["placement_form"] == 0 and st["segments"] * sh.MV_WSEG_MIN >= st["visited"] > 0, st
        try:
            e.match(jobs, owner_table_offers(M + 1))
        except CookError as ex:
            assert "too many offers" in str(ex), ex
        else:
            raise AssertionError(f"{M + 1} offers were accepted")
        _same(("owner table: the match before the refused call", M), e.match_fetch(), want)
    assert 140_000 <= M < sh.MV_RLDS_BYTES, M
    return M

