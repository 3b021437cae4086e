"""The class-ordered walk (match_algo 3) at its batch boundaries on the GPU — sixteen waves polling an LDS board, with the hand-placed gfx950
code of classfit_asm.hpp that the emulated build replaces — bit for bit against the oracle: the cases of tests/classfit_batches_cases.py, as
test_classfit_batches_emu.py runs them.  No CPU fallback: without the library or the GPU these tests FAIL."""
import pytest

from cook_amd.engine import Engine
from tests import classfit_batches_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd import build
    so = build.build()
    return lambda params: Engine(params, lib_path=so)


@pytest.mark.parametrize("lead", C.LEADS)
@pytest.mark.parametrize("run", C.RUNS)
def test_run_of_batches_nobody_walks_in_the_middle(make_engine, lead, run):
    C.run_of_batches_nobody_walks_in_the_middle(make_engine, lead, run)


@pytest.mark.parametrize("k_small,k_big", C.QUEUE_ENDS)
def test_queue_ends_in_batches_nobody_walks(make_engine, k_small, k_big):
    C.queue_ends_in_batches_nobody_walks(make_engine, k_small, k_big)


@pytest.mark.parametrize("shape", C.ROOM_SHAPES)
def test_room_goes_away_during_the_batch_before(make_engine, shape):
    C.room_goes_away_during_the_batch_before(make_engine, shape)


@pytest.mark.parametrize("shift", C.SHIFTS)
def test_epoch_and_exact_turn_behind_a_boundary(make_engine, shift):
    """(the pool of the emulated file ends no epoch in a 64-lane overlay: its exact turns and its placements here, the epochs in the test below)"""
    C.epoch_and_exact_turn_behind_a_boundary(make_engine, shift, epochs=False)


@pytest.mark.parametrize("shift", C.SHIFTS)
def test_epoch_and_exact_turn_behind_a_boundary_at_the_shipped_overlay(make_engine, shift):
    """the same pool 24 times as large (3840 offers, 6800 jobs): epochs end at 58 live overlay lanes here, not at the everyday emulated build's 8,
    and the small pool ends none.  (In the shipped shape on the emulator, shift 0: one epoch at 8 times, two at 16 times, five at 24 times.)"""
    C.epoch_and_exact_turn_behind_a_boundary(make_engine, shift, scale=C.SHIPPED_SCALE)


@pytest.mark.parametrize("seed", C.TIE_SEEDS)
def test_tie_heavy_pools_with_a_run_in_the_middle(make_engine, seed):
    C.tie_heavy_pools_with_a_run_in_the_middle(make_engine, seed)


def test_constrained_jobs_in_batches_nobody_walks(make_engine):
    C.constrained_jobs_in_batches_nobody_walks(make_engine)
