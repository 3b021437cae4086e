"""cook_sweep_running on the MI355X (cook_amd/libcookmatch.so, gfx950): the golden cases, a running set of 1 000 000 rows (5 % unknown,
1 % cancelled) with 100 000 groups of skewed size over 4 000 000 successful instances, one group of 1 000 000 of them (a segment over
many sort tiles), many ties in s, the error rows at that size, and one call on an engine with a staged C4 pool whose cycle stays as it
was — every call against the oracle of tests/sweep_oracle.py, bit for bit."""
import pytest

from cook_amd import workload
from cook_amd.engine import Engine
from tests import sweep_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd import build
    so = build.build()
    return lambda params: Engine(params, lib_path=so)


@pytest.fixture(scope="module")
def large():
    return S.random_table(11, 1_000_000, 100_000, 4_000_000, big_group=1_000_000)


def test_sweep_golden(make_engine):
    S.check_golden(make_engine)


def test_sweep_large(make_engine, large):
    want = S.check_random(make_engine, large, whats=(7, 2))
    assert want["info"]["stragglers"] > 0 and want["info"]["groups_ready"] > 1000


def test_sweep_ties(make_engine):
    S.check_random(make_engine, S.random_table(12, 300_000, 20_000, 1_500_000, big_group=400_000, ties=True), whats=(7, 2, 5))


def test_sweep_small_groups(make_engine):
    S.check_random(make_engine, S.random_table(13, 200_000, 150_000, 300_000), whats=(7,))


def test_sweep_errors(make_engine, large):
    S.check_errors(make_engine, large, 14)


def test_sweep_beside_a_staged_c4_pool(make_engine):
    pool = workload.make_pool(workload.ClusterSpec(), 0)
    S.check_cycle_undisturbed(make_engine, pool, S.random_table(15, 50_000, 5_000, 200_000), k=1000)
