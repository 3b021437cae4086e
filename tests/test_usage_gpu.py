"""cook_usage_breakdown / cook_usage_breakdown_multi on the MI355X (cook_amd/libcookmatch.so, gfx950): the emulator suite's cases at
GPU sizes, one C4 pool, C5's running set (1 000 000 running rows), one user holding more than 130 000 rows, one group of more than
100 000 rows and the eight pools of the timed configuration through the multi form, bit for bit against tests/usage_oracle.py."""
import numpy as np
import pytest

from cook_amd import _abi as A
from cook_amd import synth, workload
from cook_amd.engine import Engine, cycle_match_multi, cycle_run_rank_multi, usage_breakdown_multi
from tests import usage_cases as S
from tests import usage_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd import build
    so = build.build()
    return lambda params: Engine(params, lib_path=so)


def test_usage_golden(make_engine):
    S.check_golden(make_engine)


@pytest.mark.parametrize("kw", [
    dict(seed=71, n_pending=20000, n_running=30000, n_users=800, n_groups=5000),
    dict(seed=72, n_pending=9000, n_running=60000, n_users=9, n_groups=300, fractional=True, must_fold=True),
    dict(seed=73, n_pending=40000, n_running=30000, n_users=3000, n_groups=2000, fractional=True, gpus=True, must_fold=True),
    dict(seed=74, n_pending=3000, n_running=0, n_users=20, n_groups=5),
    dict(seed=75, n_pending=0, n_running=3000, n_users=20, n_groups=3000, fractional=True),
    dict(seed=76, n_pending=0, n_running=0, n_users=5, n_groups=3),
    dict(seed=7, n_pending=125000, n_running=50000, n_users=10000, n_groups=20000, fractional=True, must_fold=True),  # one C4 pool's shape, fractional
], ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_usage_random(make_engine, kw):
    kw = dict(kw)
    must_fold, n_groups = kw.pop("must_fold", False), kw.pop("n_groups")
    S.check_random(make_engine, synth.make_pool(n_offers=8, **kw), n_groups, seed=kw["seed"], must_fold=must_fold)


def test_usage_c4_pool(make_engine):
    S.check_random(make_engine, workload.make_pool(workload.ClusterSpec(), 0), 30000, seed=40)


def test_usage_c5_running_set(make_engine):
    pool = synth.make_pool(seed=0xC00C0005, n_pending=500_000, n_running=1_000_000, n_users=10_000, n_offers=50_000)
    got = S.check_random(make_engine, pool, 200_000, seed=50)
    assert len(got["rows"]) == 1_000_000


def test_usage_every_row_its_own_group(make_engine):
    S.check_every_row_its_own_group(make_engine, synth.make_pool(seed=78, n_pending=30000, n_running=90000, n_users=300, n_offers=8, fractional=True))


def test_usage_one_group_for_all(make_engine):
    S.check_one_group_for_all(make_engine, synth.make_pool(seed=79, n_pending=30000, n_running=90000, n_users=300, n_offers=8, fractional=True))


def test_usage_long_segment_and_bucket(make_engine):
    """one user with >= 130 000 running rows, >= 100 000 of them in one group: the cross-block carries of both scans, and the
    left-to-right folds of that bucket and that user"""
    pool = S.one_user_pool(80, n_running=140_000, n_pending=20_000)
    got, g = S.check_long_segment_and_bucket(make_engine, pool, seed=80)
    assert int(got["total"][0, 3]) >= 130_000 and got["bucket_usage"][:, 3].max() >= 100_000


@pytest.mark.parametrize("n_engines,with_map", [(2, False), (3, True), (8, False), (5, True)])
def test_usage_multi(make_engine, n_engines, with_map):
    S.check_multi(make_engine, n_engines, seed=81 + n_engines, n_users=400, n_groups=3000, with_map=with_map, n_running=20000, n_pending=9000)


def _timed_pools(n=8):
    spec = workload.ClusterSpec()
    return [workload.make_pool(spec, i) for i in range(n)]


def test_usage_eight_timed_pools_multi(make_engine):
    """all eight pools of the timed configuration through the multi form, and the timed cycle's outputs unchanged by a call in between"""
    pools = _timed_pools()
    p = A.default_params()
    engines = [make_engine(p) for _ in pools]
    try:
        for e, pl in zip(engines, pools):
            e.cycle_stage(pl.tasks, pl.users, pl.pending_jobs, pl.offers, pl.groups)
        n_users = max(pl.users.n for pl in pools)
        groups = [S.random_groups(90 + i, pl.tasks, 50_000) for i, pl in enumerate(pools)]

        def cycle():
            cycle_run_rank_multi(engines, 10 ** 9)
            cycle_match_multi(engines)
            return [(r.copy(), j.copy(), h) for r, j, h in (e.cycle_fetch() for e in engines)]

        first = cycle()
        cycle_run_rank_multi(engines, 10 ** 9)
        got = usage_breakdown_multi(engines, n_users, groups, 50_000)   # between the rank part and the placement of a cycle
        cycle_match_multi(engines)
        second = [(r.copy(), j.copy(), h) for r, j, h in (e.cycle_fetch() for e in engines)]
        for a, b in zip(first, second):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
        O.assert_same(got, O.usage([(pl.tasks, g) for pl, g in zip(pools, groups)], n_users, None, None, True), "eight pools")
        assert len(got["rows"]) == sum(int((pl.tasks.pending == 0).sum()) for pl in pools)
    finally:
        for e in engines:
            e.close()


def test_usage_rounding_traps(make_engine):
    S.check_traps(make_engine)


def test_usage_negative_zero(make_engine):
    S.check_negative_zero(make_engine)


def test_usage_state_rule(make_engine):
    S.check_state_rule(make_engine)


def test_usage_leaves_the_cycle_alone(make_engine):
    S.check_cycle_undisturbed(make_engine, synth.make_pool(seed=88, n_pending=20000, n_running=10000, n_users=300, n_offers=500), k=1000, n_groups=2000)


def test_usage_device_outputs(make_engine):
    """bucket_usage_is_device / total_is_device: the usage arrays land in device buffers, the rest comes back as usual"""
    import torch
    pool = synth.make_pool(seed=89, n_pending=5000, n_running=5000, n_users=200, n_offers=8, fractional=True)
    grp = S.random_groups(89, pool.tasks, 400)
    bu = torch.zeros((pool.tasks.n, 4), dtype=torch.float64, device="cuda")
    tu = torch.zeros((200, 4), dtype=torch.float64, device="cuda")
    with make_engine(A.default_params()) as e:
        e.rank_stage(pool.tasks, pool.users)
        e.rank_run()
        host = e.usage_breakdown(grp, 400)
        dev = e.usage_breakdown(grp, 400, usage_device_ptr=bu.data_ptr(), total_device_ptr=tu.data_ptr())
    torch.cuda.synchronize()
    assert dev["bucket_usage"] is None and dev["total"] is None
    for k in ("bucket_off", "bucket_group", "row_off", "rows"):
        assert np.array_equal(dev[k], host[k])
    B = len(host["bucket_group"])
    assert np.array_equal(bu.cpu().numpy()[:B].view(np.uint64), host["bucket_usage"].view(np.uint64))
    assert np.array_equal(tu.cpu().numpy().view(np.uint64), host["total"].view(np.uint64))
    O.assert_same(host, O.usage([(pool.tasks, grp)], 200))
