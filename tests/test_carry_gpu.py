"""The carry (cook_cycle_run_queue_carry*) on the MI355X (cook_amd/libcookmatch.so, gfx950): the cases of tests/carry_cases.py, every
cycle against the oracle of tests/carry_oracle.py."""
import os
import subprocess
import sys

import pytest

from cook_amd.engine import Engine
from tests import carry_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd import build
    so = build.build()
    return lambda params: Engine(params, lib_path=so)


def test_carry_base(make_engine):
    K.check_base(make_engine)


def test_carry_non_dyadic(make_engine):
    K.check_base(make_engine, fractional=True)


def test_carry_segment_lengths(make_engine):
    K.check_segment_lengths(make_engine)


@pytest.mark.parametrize("null_cols", [False, True])
def test_carry_every_column(make_engine, null_cols):
    K.check_columns(make_engine, null_cols=null_cols)


def test_carry_skipped_offers_and_remove_all(make_engine):
    K.check_skipped(make_engine)


def test_carry_tokens(make_engine):
    K.check_tokens(make_engine)


def test_carry_split_equivalence(make_engine):
    K.check_split(make_engine)


def test_carry_class_ordered_walk(make_engine):
    K.check_classfit(make_engine)


def test_carry_multi(make_engine, multi_mode):
    K.check_multi(make_engine)


def test_carry_built_offers_in_place(make_engine):
    K.check_built_offers(make_engine)


def test_carry_refusals_and_persistence(make_engine):
    K.check_refusals(make_engine)


def test_carry_guarded_run():
    """every other test of this file once more in a process of its own with every device buffer between two guard bands (COOK_GUARD=1
    is read when the library is loaded): all pass, and no write outside a buffer is reported"""
    env = dict(os.environ, COOK_GUARD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "not guarded_run"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "COOK_GUARD: " not in r.stderr, r.stderr[-1500:]
