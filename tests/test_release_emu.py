"""The release (cook_cycle_run_queue_release*) on a machine WITHOUT a GPU: the cook_amd/csrc sources compiled against the SIMT emulator
(tests/simt_emu), every cycle against the oracle of tests/release_oracle.py (cases in tests/release_cases.py)."""
import pytest

from cook_amd.engine import Engine
from tests import release_cases as X


@pytest.fixture(scope="module")
def make_engine():
    from tests.simt_emu import build_emu
    so = build_emu.build()
    return lambda params: Engine(params, lib_path=so)


def test_release_base(make_engine):
    X.check_base(make_engine)


def test_release_non_dyadic(make_engine):
    X.check_base(make_engine, fractional=True)


@pytest.mark.parametrize("null_cols", [False, True])
def test_release_every_column(make_engine, null_cols):
    X.check_columns(make_engine, null_cols=null_cols)


def test_release_groups(make_engine):
    X.check_groups(make_engine)


def test_release_segment_lengths(make_engine):
    X.check_segment_lengths(make_engine)


def test_release_many_segments(make_engine):
    X.check_many_segments(make_engine)


def test_release_long_group_list(make_engine):
    X.check_long_group_list(make_engine)


def test_release_hosts_without_a_row(make_engine):
    X.check_no_rows(make_engine)


def test_release_sparse_host_ids(make_engine):
    X.check_no_rows(make_engine, hosts=(5, 4000000, 9000000))


def test_release_no_advance(make_engine):
    X.check_no_advance(make_engine)


def test_release_without_and_behind_a_carry(make_engine):
    X.check_explain(make_engine)


def test_release_clamp(make_engine):
    X.check_clamp(make_engine)


def test_release_multi(make_engine, multi_mode):
    X.check_multi(make_engine)


def test_release_class_ordered_walk(make_engine):
    X.check_classfit(make_engine)


def test_release_refusals_and_persistence(make_engine):
    X.check_refusals(make_engine)
