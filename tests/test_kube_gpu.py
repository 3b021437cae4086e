"""cook_kube_distribute on the MI355X (cook_amd/libcookmatch.so, gfx950): the cases of tests/kube_cases.py, every choice, list, offset
and info field against tests/kube_oracle.py."""
import pytest

from cook_amd.engine import Engine
from tests import kube_cases as KC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd import build
    so = build.build()
    return lambda params: Engine(params, lib_path=so)


def test_kube_golden(make_engine):
    KC.check_golden(make_engine)


@pytest.mark.parametrize("n_clusters", KC.CLUSTER_COUNTS)
def test_kube_sizes(make_engine, n_clusters):
    KC.check_sizes(make_engine, n_clusters)


def test_kube_exhaustion_places(make_engine):
    KC.check_exhaustion_places(make_engine)


@pytest.mark.parametrize("seed,n_clusters", KC.RANDOM_CASES)
def test_kube_random(make_engine, seed, n_clusters):
    KC.check_random(make_engine, seed, n_clusters)


def test_kube_one_launch(make_engine):
    KC.check_one_launch(make_engine)


def test_kube_refusals(make_engine):
    KC.check_refusals(make_engine)


def test_kube_cycles(make_engine):
    KC.check_cycles(make_engine)


def test_kube_cycles_tokens(make_engine):
    KC.check_cycles(make_engine, tokens=True)


def test_kube_cycles_limiters(make_engine):
    KC.check_cycles(make_engine, limiters=True)


def test_kube_cycles_paused_between(make_engine):
    KC.check_cycles(make_engine, paused_between=True)


def test_kube_cycles_release(make_engine):
    KC.check_release(make_engine)


def test_kube_fenzo_cycle_after(make_engine):
    KC.check_fenzo_after_kube(make_engine)


def test_kube_distribute_beside_cycle(make_engine):
    KC.check_distribute_beside_cycle(make_engine)


def test_kube_offer_skipped_not_read(make_engine):
    KC.check_offer_skipped_ignored(make_engine)


def test_kube_state_answers(make_engine):
    KC.check_state_answers(make_engine)


def test_kube_cycle_refusals(make_engine):
    KC.check_cycle_refusals(make_engine)


def test_kube_multi(make_engine):
    got = KC.run_multi(make_engine)
    KC.check_multi_batched(got, emu=False)
    KC.check_multi_unbatched_child(got, emu=False)
