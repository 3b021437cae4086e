"""The rebalancer over the pool's resident cycle state (cook_cycle_rebalance_stage, cook_cycle_rebalance_fetch) on a machine WITHOUT a
GPU: the cook_amd/csrc sources compiled against the SIMT emulator (tests/simt_emu), against the oracle of
tests/resident_rebalance_oracle.py (cases in tests/resident_rebalance_cases.py)."""
import pytest

from cook_amd.engine import Engine
from tests import resident_rebalance_cases as X


@pytest.fixture(scope="module")
def make_engine():
    from tests.simt_emu import build_emu
    so = build_emu.build()
    return lambda params: Engine(params, lib_path=so)


def test_resident_rebalance_base(make_engine):
    X.check_base(make_engine)


@pytest.mark.parametrize("R", X.boundary_sizes())
def test_resident_rebalance_running_rows(make_engine, R):
    X.check_running_rows(make_engine, R)


def test_resident_rebalance_row_ends(make_engine):
    X.check_row_ends(make_engine)


def test_resident_rebalance_max_preemption(make_engine):
    X.check_max_preemption(make_engine)


def test_resident_rebalance_masks(make_engine):
    X.check_masks(make_engine)


def test_resident_rebalance_fullest_host(make_engine):
    X.check_fullest_host(make_engine)


def test_resident_rebalance_rescoring_paths(make_engine):
    X.check_rescoring_paths(make_engine)


def test_resident_rebalance_update(make_engine):
    X.check_update(make_engine)


def test_resident_rebalance_update_without_host(make_engine):
    X.check_update_without_host(make_engine)


def test_resident_rebalance_skip_matched(make_engine):
    X.check_skip_matched(make_engine)


def test_resident_rebalance_sources(make_engine):
    X.check_sources(make_engine)


def test_resident_rebalance_golden(make_engine):
    X.check_golden(make_engine)


def test_resident_rebalance_refusals(make_engine):
    X.check_refusals(make_engine)


def test_resident_rebalance_untouched(make_engine):
    X.check_untouched(make_engine)


def test_resident_rebalance_loop(make_engine):
    X.check_loop(make_engine)
