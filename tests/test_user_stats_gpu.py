"""cook_user_stats / cook_user_stats_multi on the MI355X (cook_amd/libcookmatch.so, gfx950): the emulator suite's cases at GPU sizes,
one C4 pool, the C5 table (1.5M tasks) and the eight pools of the timed configuration as one quota group, bit for bit against
tests/user_stats_oracle.py."""
import numpy as np
import pytest

from cook_amd import _abi as A
from cook_amd import synth, workload
from cook_amd.engine import Engine, user_stats_multi
from tests import user_stats_cases as S
from tests import user_stats_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd import build
    so = build.build()
    return lambda params: Engine(params, lib_path=so)


def test_user_stats_golden(make_engine):
    S.check_golden(make_engine)


def test_user_stats_merge_quirks_and_limits(make_engine):
    S.check_quirks(make_engine)


@pytest.mark.parametrize("kw", [
    dict(seed=61, n_pending=20000, n_running=30000, n_users=800),
    dict(seed=62, n_pending=9000, n_running=60000, n_users=9, fractional=True),
    dict(seed=63, n_pending=40000, n_running=30000, n_users=3000, fractional=True, no_shares=True),
    dict(seed=64, n_pending=3000, n_running=0, n_users=20),
    dict(seed=7, n_pending=125000, n_running=50000, n_users=10000, fractional=True),   # one C4 pool, fractional
], ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_user_stats_random(make_engine, kw):
    S.check_random(make_engine, synth.make_pool(n_offers=8, **kw), seed=kw["seed"])


def test_user_stats_c4_pool(make_engine):
    S.check_random(make_engine, workload.make_pool(workload.ClusterSpec(), 0), seed=40)


def test_user_stats_c5_table(make_engine):
    pool = synth.make_pool(seed=0xC00C0005, n_pending=500_000, n_running=1_000_000, n_users=10_000, n_offers=50_000)
    got = S.check_random(make_engine, pool, seed=50)
    assert got["counts"]["total"] > 9000


def test_user_stats_multi(make_engine):
    pools = [synth.make_pool(seed=70 + i, n_pending=npd, n_running=nr, n_users=nu, n_offers=8, fractional=(i != 1))
             for i, (npd, nr, nu) in enumerate([(5000, 9000, 300), (3000, 2000, 450), (0, 0, 10), (8000, 13000, 250)])]
    S.check_multi(make_engine, pools, n_users=640)


def test_user_stats_multi_timed_configuration(make_engine):
    """the eight pools of bench.py's timed configuration as one quota group (identity maps: the pools share the user ids)"""
    spec = workload.ClusterSpec()
    pools = [workload.make_pool(spec, p) for p in range(spec.pools)]
    lim = S.random_limits(80, spec.users)
    engines = [make_engine(A.default_params()) for _ in pools]
    try:
        for e, pl in zip(engines, pools):
            e.rank_stage(pl.tasks, pl.users)
            e.rank_run()
        got = user_stats_multi(engines, lim)
        O.assert_same(got, O.user_stats([(pl.tasks, None) for pl in pools], spec.users, lim))
        assert np.array_equal(got["all"][0][:1], [float(sum(int((pl.tasks.pending == 0).sum()) for pl in pools))])
    finally:
        for e in engines:
            e.close()


def test_user_stats_state_rule(make_engine):
    S.check_state_rule(make_engine)


def test_user_stats_leave_the_cycle_alone(make_engine):
    S.check_cycle_undisturbed(make_engine, synth.make_pool(seed=66, n_pending=20000, n_running=10000, n_users=300, n_offers=500), k=1000)


def test_user_stats_device_output(make_engine):
    """per_user_is_device: the rows land in a device buffer, the rest comes back as usual"""
    import torch
    pool = synth.make_pool(seed=67, n_pending=5000, n_running=5000, n_users=200, n_offers=8, fractional=True)
    lim = S.random_limits(67, 200)
    buf = torch.zeros((200, 4, 3), dtype=torch.float64, device="cuda")
    with make_engine(A.default_params()) as e:
        e.rank_stage(pool.tasks, pool.users)
        e.rank_run()
        host = e.user_stats(lim)
        dev = e.user_stats(lim, per_user_device_ptr=buf.data_ptr())
    torch.cuda.synchronize()
    assert dev["per_user"] is None and dev["counts"] == host["counts"]
    assert np.array_equal(buf.cpu().numpy().view(np.uint64), host["per_user"].view(np.uint64))
