"""The window rounds at their fitness guard bands and table edges (tests/match_edges_cases.py), on the SIMT emulator with the emulated
suite's small launch shapes (MV_WSEG 96, MV_WEVAL 256, MV_WLONG 1 024): every near-tie situation at every gap under the three packers and
match_algo 0 / 1, the class-ordered form's pairs, the multi-pool calls in both modes, and every table and tile edge of part 2 at the sizes the
emulated constants give.  Two things run in the GPU file only: the owner table (150 000 offers a probe) and the buffers' guard bands
(COOK_GUARD is the shipped library's); N3's plain layout (8 320 offers a call) runs here at fitness 0 with three gaps, in full there."""
import pytest

from cook_amd.engine import Engine
from tests import match_edges_cases as X


@pytest.fixture(scope="module")
def make_engine():
    from tests.simt_emu import build_emu
    so = build_emu.build()
    return lambda params: Engine(params, lib_path=so)


def test_the_constants_are_the_emulated_ones(make_engine):
    sh = X.shapes(make_engine)
    assert not sh.ship and sh.MV_WEVAL < 960 and sh.MV_WLONG < 10240, sh
    X.check_band_literals()


# ---- part 1: near-ties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [0, 1])
@pytest.mark.parametrize("fitness", [0, 1, 2])
@pytest.mark.parametrize("situation", ["N1", "N1w", "N2", "N5", "N6"])
def test_near_ties(make_engine, situation, fitness, algo):
    X.run_near_ties(make_engine, situation, fitness, algo)


@pytest.mark.parametrize("algo", [0, 1])
@pytest.mark.parametrize("fitness", [0, 1, 2])
def test_near_ties_in_the_two_chunks_of_a_merge_lane_split(make_engine, monkeypatch, fitness, algo):
    """N3 under COOK_EVAL_SPLIT=4 at the smallest M with more than 64 virtual chunks"""
    monkeypatch.setenv("COOK_EVAL_SPLIT", "4")
    sh = X.shapes(make_engine)
    assert X.eval_split(sh, 2, 4) == 4 and -(-(16 * sh.MV_OCB + 1) // sh.MV_OCB) * 4 == 68
    X.run_near_ties(make_engine, "N3s", fitness, algo, ges=(1.0,))


def test_near_ties_in_the_two_chunks_of_a_merge_lane(make_engine, monkeypatch):
    monkeypatch.setenv("COOK_EVAL_SPLIT", "1")
    X.run_near_ties(make_engine, "N3", 0, 0, gaps=(52, 39, 19), ges=(1.0,))


@pytest.mark.parametrize("split", [1, 4])
@pytest.mark.parametrize("algo", [0, 1])
@pytest.mark.parametrize("fitness", [0, 1, 2])
def test_nine_offers_rising(make_engine, monkeypatch, fitness, algo, split):
    X.run_nine_rising(make_engine, monkeypatch, fitness, algo, split)


@pytest.mark.parametrize("touched", [False, True])
@pytest.mark.parametrize("algo", [0, 1])
@pytest.mark.parametrize("fitness", [0, 1, 2])
def test_good_enough_thresholds(make_engine, fitness, algo, touched):
    X.run_good_enough(make_engine, fitness, algo, touched)


@pytest.mark.parametrize("algo", [0, 1])
@pytest.mark.parametrize("fitness", [0, 1, 2])
def test_exact_ties_on_a_rounded_reciprocal(make_engine, fitness, algo):
    """T5: the touched offer's approximate fitness lies above (below) the exact value it ties with: the lowest index wins all the same"""
    X.run_near_ties(make_engine, "T5", fitness, algo, gaps=())


@pytest.mark.parametrize("inexact", ["above", "below"])
@pytest.mark.parametrize("algo", [0, 1])
@pytest.mark.parametrize("fitness", [0, 1, 2])
def test_good_enough_at_a_rounded_reciprocal(make_engine, fitness, algo, inexact):
    """N7, touched: the threshold is the fp64 fitness F while the walk's approximation of it lies above (below) F"""
    X.run_good_enough(make_engine, fitness, algo, True, inexact)


@pytest.mark.parametrize("algo", [0, 1, 3])
@pytest.mark.parametrize("situation", ["C1", "C2", "C5", "C6"])
def test_near_ties_by_cancellation(make_engine, situation, algo):
    """the pairs the class-ordered form takes (match_algo 3: placement_form 3), around CF_BAND and CF_BAND32; the same pairs through the rounds"""
    X.run_near_ties(make_engine, situation, 0, algo)


@pytest.mark.parametrize("situation", ["N1", "N1w", "N2"])
def test_near_ties_class_ordered_refusal(make_engine, situation):
    """match_algo 3 on the plain pairs: refused with CF_X_NUMBERS from k = 24 on (the window rounds place them), placed by the form below"""
    X.run_near_ties(make_engine, situation, 0, 3)


def test_a_spreader_is_the_sweeps(make_engine):
    X.run_spreader_control(make_engine)


@pytest.mark.parametrize("situation", ["N5", "N6"])
def test_near_ties_multi(make_engine, multi_mode, situation):
    X.run_multi_near_ties(make_engine, situation)


def test_good_enough_thresholds_multi(make_engine, multi_mode):
    X.run_multi_good_enough(make_engine)


# ---- part 2: table and tile edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ge", [1.0, 0.5])
@pytest.mark.parametrize("size", X.OFFER_SIZES)
def test_offers_at_batch_word_and_chunk_edges(make_engine, size, ge):
    X.run_offers_edge(make_engine, size, ge)


@pytest.mark.parametrize("size", X.JOB_SIZES)
def test_jobs_at_window_edges(make_engine, monkeypatch, tmp_path, size):
    X.run_window_size(make_engine, monkeypatch, tmp_path, size)


@pytest.mark.parametrize("split", [4, 2, 1])
@pytest.mark.parametrize("size", X.SPLIT_SIZES)
def test_jobs_at_eval_split_thresholds(make_engine, monkeypatch, tmp_path, size, split):
    X.run_window_size(make_engine, monkeypatch, tmp_path, size, split)


@pytest.mark.parametrize("wlong", [True, False])
@pytest.mark.parametrize("which", X.LONG_K)
def test_full_cluster_windows(make_engine, monkeypatch, tmp_path, which, wlong):
    X.run_full_cluster(make_engine, monkeypatch, tmp_path, which, wlong)


@pytest.mark.parametrize("ge", [1.0, 0.99])
@pytest.mark.parametrize("extra", [0, 1])
def test_list_in_one_batch(make_engine, monkeypatch, extra, ge):
    X.run_list_in_chunk(make_engine, monkeypatch, X.shapes(make_engine).MV_L + extra, ge)


@pytest.mark.parametrize("ge", [1.0, 0.99])
@pytest.mark.parametrize("extra", [0, 1])
def test_list_over_chunks(make_engine, extra, ge):
    X.run_list_over_chunks(make_engine, extra, ge)


@pytest.mark.parametrize("touched_low", [True, False])
@pytest.mark.parametrize("extra", [0, 1])
def test_good_enough_list(make_engine, extra, touched_low):
    X.run_good_enough_list(make_engine, extra, touched_low)


@pytest.mark.parametrize("which", ["T", "T+1", "full", "ports"])
def test_touched_set(make_engine, which):
    X.run_touched_set(make_engine, which)


@pytest.mark.parametrize("ge", [1.0, 0.99])
@pytest.mark.parametrize("which", X.CONSTRAINT_CASES)
def test_constraint_slots(make_engine, which, ge):
    X.run_constraint_slots(make_engine, which, ge)


@pytest.mark.parametrize("gtype", [2, 3])
def test_second_group_member_ends_the_round(make_engine, gtype):
    X.run_group_barrier(make_engine, gtype)


def test_refused_pool_keeps_the_last_match(make_engine):
    X.run_refusal_keeps_the_last_match(make_engine)
