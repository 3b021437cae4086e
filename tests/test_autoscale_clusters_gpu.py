"""cook_cycle_set_job_hashes / cook_cycle_autoscale_clusters(_multi) on the MI355X (cook_amd/libcookmatch.so, gfx950): the cases of
tests/autoscale_cluster_cases.py, every launch list, offset and info field against tests/distribute_oracle.py composed behind
tests/autoscale_cases.oracle."""
import pytest

from cook_amd.engine import Engine
from tests import autoscale_cluster_cases as CC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd import build
    so = build.build()
    return lambda params: Engine(params, lib_path=so)


def test_clusters_golden(make_engine):
    CC.check_golden(make_engine)


def test_clusters_candidate_counts(make_engine):
    CC.check_counts(make_engine)


def test_clusters_simple_shapes(make_engine):
    CC.check_simple_shapes(make_engine)


@pytest.mark.parametrize("seed,n_clusters,max_room", CC.RANDOM_CASES)
def test_clusters_random(make_engine, seed, n_clusters, max_room):
    CC.check_random(make_engine, seed, n_clusters, max_room=max_room)


def test_clusters_random_3000_pending(make_engine):
    CC.check_random(make_engine, 814, 3, n_pending=3000, n_running=1000, n_users=40, n_offers=60, k=1000)


def test_clusters_hash_column(make_engine):
    CC.check_hash_column(make_engine)


def test_clusters_refusals(make_engine):
    CC.check_refusals(make_engine)


def test_clusters_leave_the_cycle_alone(make_engine):
    CC.check_cycle_undisturbed(make_engine)


def test_clusters_multi(make_engine):
    got = CC.run_multi(make_engine)
    CC.check_multi_unbatched_child(got, emu=False)


def test_clusters_multi_after_queue_cycle(make_engine):
    CC.run_multi(make_engine, queue_cycle=True)


def test_clusters_multi_one_refused(make_engine):
    CC.check_multi_one_refused(make_engine)
