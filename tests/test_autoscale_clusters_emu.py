"""cook_cycle_set_job_hashes / cook_cycle_autoscale_clusters(_multi) on a machine WITHOUT a GPU: the cook_amd/csrc sources compiled against
the SIMT emulator (tests/simt_emu), the cases of tests/autoscale_cluster_cases.py, and the synchronisation count, which on the emulator
is that of the host code."""
import pytest

from cook_amd.engine import Engine
from tests import autoscale_cluster_cases as CC


@pytest.fixture(scope="module")
def make_engine():
    from tests.simt_emu import build_emu
    so = build_emu.build()
    return lambda params: Engine(params, lib_path=so)


def test_clusters_golden_oracle():
    CC.check_golden_oracle()


def test_clusters_golden(make_engine):
    CC.check_golden(make_engine)


def test_clusters_candidate_counts(make_engine):
    CC.check_counts(make_engine)


def test_clusters_simple_shapes(make_engine):
    CC.check_simple_shapes(make_engine)


@pytest.mark.parametrize("seed,n_clusters,max_room", CC.RANDOM_CASES)
def test_clusters_random(make_engine, seed, n_clusters, max_room):
    CC.check_random(make_engine, seed, n_clusters, max_room=max_room)


def test_clusters_hash_column(make_engine):
    CC.check_hash_column(make_engine)


def test_clusters_refusals(make_engine):
    CC.check_refusals(make_engine)


def test_clusters_leave_the_cycle_alone(make_engine):
    CC.check_cycle_undisturbed(make_engine)


def test_clusters_multi(make_engine):
    got = CC.run_multi(make_engine)
    CC.check_multi_unbatched_child(got, emu=True)


def test_clusters_multi_after_queue_cycle(make_engine):
    CC.run_multi(make_engine, queue_cycle=True)


def test_clusters_multi_one_refused(make_engine):
    CC.check_multi_one_refused(make_engine)


def test_clusters_synchronisations(make_engine):
    CC.check_sync_count(make_engine)
