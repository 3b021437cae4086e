"""cook_match_launch_resources on the MI355X (cook_amd/libcookmatch.so, gfx950): the cases of tests/launch_cases.py, each against the
oracle of tests/launch_oracle.py, bit for bit."""
import os
import subprocess
import sys

import pytest

from cook_amd.engine import Engine
from tests import launch_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd import build
    so = build.build()
    return lambda params: Engine(params, lib_path=so)


def test_launch_golden(make_engine):
    K.check_golden(make_engine)


def test_launch_range_boundaries(make_engine):
    K.check_range_boundaries(make_engine)


def test_launch_single_port_ranges(make_engine):
    K.check_single_port_ranges(make_engine)


def test_launch_segment_lengths(make_engine):
    K.check_segment_lengths(make_engine)


def test_launch_one_offer_none_kept_k1(make_engine):
    K.check_one_offer_none_kept_k1(make_engine)


def test_launch_roles(make_engine):
    K.check_roles(make_engine)


def test_launch_offer_skipped(make_engine):
    K.check_offer_skipped(make_engine)


def test_launch_call_forms(make_engine):
    K.check_call_forms(make_engine)


@pytest.mark.parametrize("seed", K.SEEDS)
def test_launch_random(make_engine, seed):
    K.check_random(make_engine, seed)


def test_launch_refusals(make_engine):
    K.check_refusals(make_engine)


def test_launch_binding_finds_room(make_engine):
    K.check_binding_finds_room(make_engine)


def test_launch_no_jobs(make_engine):
    K.check_no_jobs(make_engine)


def test_launch_guarded_run():
    """every other test of this file once more in a process of its own with every device buffer between two guard bands (COOK_GUARD=1
    is read when the library is loaded): all pass, and no write outside a buffer is reported"""
    env = dict(os.environ, COOK_GUARD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "not guarded_run"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "COOK_GUARD: " not in r.stderr, r.stderr[-1500:]
