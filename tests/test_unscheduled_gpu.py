"""cook_unscheduled on the MI355X (cook_amd/libcookmatch.so, gfx950): the emulator suite's cases at GPU sizes, one C4 pool, the C5
table (1.5M tasks) and one user holding more than 100 000 rows, bit for bit against tests/unscheduled_oracle.py."""
import numpy as np
import pytest

from cook_amd import _abi as A
from cook_amd import synth, workload
from cook_amd.engine import Engine
from tests import unscheduled_cases as S
from tests import unscheduled_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd import build
    so = build.build()
    return lambda params: Engine(params, lib_path=so)


def test_unscheduled_golden(make_engine):
    S.check_golden(make_engine)


@pytest.mark.parametrize("kw", [
    dict(seed=61, n_pending=20000, n_running=30000, n_users=800),
    dict(seed=62, n_pending=9000, n_running=60000, n_users=9, fractional=True, must_fold=True),
    dict(seed=63, n_pending=40000, n_running=30000, n_users=3000, fractional=True, gpus=True, must_fold=True),
    dict(seed=64, n_pending=3000, n_running=0, n_users=20),
    dict(seed=65, n_pending=0, n_running=3000, n_users=20, fractional=True),
    dict(seed=66, n_pending=0, n_running=0, n_users=5),
    dict(seed=7, n_pending=125000, n_running=50000, n_users=10000, fractional=True, must_fold=True),   # one C4 pool, fractional
], ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_unscheduled_random(make_engine, kw):
    kw = dict(kw)
    must_fold = kw.pop("must_fold", False)
    S.check_random(make_engine, synth.make_pool(n_offers=8, **kw), seed=kw["seed"], must_fold=must_fold)


def test_unscheduled_c4_pool(make_engine):
    S.check_random(make_engine, workload.make_pool(workload.ClusterSpec(), 0), seed=40)


def test_unscheduled_c5_table(make_engine):
    pool = synth.make_pool(seed=0xC00C0005, n_pending=500_000, n_running=1_000_000, n_users=10_000, n_offers=50_000)
    got = S.check_random(make_engine, pool, seed=50)
    assert int(got["list_len"].sum()) == pool.tasks.n


def test_unscheduled_one_long_segment(make_engine):
    """one user with more rows than a workgroup covers (>= 100 000): the scan's cross-block carry of the listed counts and running
    sums, and that user's left-to-right fold"""
    pool = S.one_user_pool(67, n_running=70_000, n_pending=60_000)
    assert int((pool.tasks.user == 0).sum()) >= 100_000
    got = S.check_random(make_engine, pool, seed=67, must_fold=True)
    assert int(got["list_len"][0]) >= 100_000


def test_unscheduled_state_rule(make_engine):
    S.check_state_rule(make_engine)


def test_unscheduled_leaves_the_cycle_alone(make_engine):
    S.check_cycle_undisturbed(make_engine, synth.make_pool(seed=68, n_pending=20000, n_running=10000, n_users=300, n_offers=500), k=1000)


def test_unscheduled_device_output(make_engine):
    """total_is_device: the usage rows land in a device buffer, the rest comes back as usual"""
    import torch
    pool = synth.make_pool(seed=69, n_pending=5000, n_running=5000, n_users=200, n_offers=8, fractional=True)
    lim = S.random_limits(69, 200)
    buf = torch.zeros((pool.tasks.n, 4), dtype=torch.float64, device="cuda")
    with make_engine(A.default_params()) as e:
        e.rank_stage(pool.tasks, pool.users)
        e.rank_run()
        host = e.unscheduled(lim)
        dev = e.unscheduled(lim, total_device_ptr=buf.data_ptr())
    torch.cuda.synchronize()
    assert dev["total"] is None and np.array_equal(dev["reasons"], host["reasons"]) and np.array_equal(dev["queue_pos"], host["queue_pos"])
    assert np.array_equal(buf.cpu().numpy().view(np.uint64), host["total"].view(np.uint64))
    O.assert_same(host, O.unscheduled(pool.tasks, 200, lim))
