"""cook_kube_distribute on a machine WITHOUT a GPU: the cook_amd/csrc sources compiled against the SIMT emulator (tests/simt_emu) and the
cases of tests/kube_cases.py."""
import pytest

from cook_amd.engine import Engine
from tests import kube_cases as KC


@pytest.fixture(scope="module")
def make_engine():
    from tests.simt_emu import build_emu
    so = build_emu.build()
    return lambda params: Engine(params, lib_path=so)


def test_kube_golden_oracle():
    KC.check_golden_oracle()


def test_kube_random_seeds_meet_their_precondition():
    for seed, n in KC.RANDOM_CASES:
        K, cl_loc, cl_cap, loc, draw = KC.random_case(seed, n)
        for dr in (draw, None):
            assert KC.random_precondition(KC.O.distribute(K, cl_loc, cl_cap, loc, dr, seed)), (seed, n)


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
    KC.check_multi_batched(got, emu=True)
    KC.check_multi_unbatched_child(got, emu=True)


def test_kube_synchronisations(make_engine):
    KC.check_sync_count(make_engine)
