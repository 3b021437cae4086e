"""The queue cycles (cook_cycle_run_queue*) on the MI355X (cook_amd/libcookmatch.so, gfx950): the emulator suite's cases at GPU sizes —
the shapes of test_autoscale_gpu.py, one C4 pool at K = 1000 for six queue cycles, the eight timed pools through the multi form under
both placement modes, all three placement forms on a pool with groups — every cycle against the oracle of tests/queue_cases.py."""
import os
import subprocess
import sys

import pytest

from cook_amd import _abi as A
from cook_amd import synth, workload
from cook_amd.engine import Engine
from tests import queue_cases as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd import build
    so = build.build()
    return lambda params: Engine(params, lib_path=so)


def test_queue_golden(make_engine):
    S.check_golden(make_engine)


def test_queue_edges(make_engine):
    S.check_edges(make_engine)


@pytest.mark.parametrize("kw", [
    dict(seed=81, n_pending=20000, n_running=10000, n_users=300, n_offers=800, q_offers=150, k=4000, host_path=True),
    dict(seed=82, n_pending=9000, n_running=30000, n_users=9, n_offers=300, q_offers=200, k=9000, fractional=True, skip_frac=0.3),  # K = all
    dict(seed=84, n_pending=6000, n_running=0, n_users=50, n_offers=8, q_offers=8, k=1000, states=False, remove_modes=[0, 0, 1, 0, 1, 0, 0]),
], ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_queue_random(make_engine, kw):
    kw = dict(kw)
    seed, k, n_offers = kw.pop("seed"), kw.pop("k"), kw.pop("q_offers")
    cyc = {x: kw.pop(x) for x in ("states", "skip_frac", "remove_modes") if x in kw}
    host_path = kw.pop("host_path", False)
    pool = synth.make_pool(seed=seed, **kw)
    cycles = S.make_cycles(pool, seed, k, 7, n_offers, fractional=kw.get("fractional", False), **cyc)
    S.check_cycles(make_engine, A.default_params(good_enough_fitness=1.0), pool, cycles, host_path=host_path)


@pytest.mark.parametrize("algo", [1, 2, 3])
def test_queue_random_groups(make_engine, algo):
    """every placement form on a pool with groups, each at a shape where it is eligible (asserted from the placement statistics):
    the serial sweep and the window rounds with unique, balanced and attribute-equals groups, fractional resources, constraints and
    gpus; class-ordered best fit takes unique groups and resources on its grid only (cookmatch.h, statistics word [38])"""
    cf = algo == 3
    seed = 84 if cf else 83  # (seeds chosen on the oracle alone: the fold must change a placement)
    kw = dict(n_pending=6000, n_running=3000, n_users=200, n_offers=300, gpus=True, constraints=True, fractional=not cf)
    pool = synth.make_pool(seed=seed, **kw)
    if not cf:
        pool = S.mix_group_types(pool, seed)
    cycles = S.make_cycles(pool, seed, 1200, 6, 200, fractional=not cf, offer_kw=dict(gpus=True, constraints=True))
    S.check_cycles(make_engine, A.default_params(good_enough_fitness=1.0, match_algo=algo), pool, cycles, group_case=True,
                   table_variant=(algo != 1), expect_form={1: 1, 2: 0, 3: 3}[algo])


def test_queue_c4_pool_k1000(make_engine):
    pool = workload.make_pool(workload.ClusterSpec(), 0)
    cycles = S.make_cycles(pool, 40, 1000, 7, 150, offer_kw=dict(gpus=True, constraints=True))
    got, _ = S.check_cycles(make_engine, A.default_params(), pool, cycles)
    assert len(got) == 7 and len(got[-1].Q) < len(got[0].Q)


def test_queue_timed_pools(make_engine, multi_mode):
    spec = workload.ClusterSpec()
    pools = [workload.make_pool(spec, p) for p in range(spec.pools)]
    cycles_of = [S.make_cycles(pl, 60 + i, 1000, 5, 120, offer_kw=dict(gpus=True, constraints=True)) for i, pl in enumerate(pools)]
    S.check_multi(make_engine, pools, A.default_params(), cycles_of)


def test_queue_state_rule(make_engine):
    S.check_state_rule(make_engine, synth.make_pool(seed=106, n_pending=3000, n_running=2000, n_users=120, n_offers=160, constraints=True), k=400)


def test_queue_guarded_run():
    """every other test of this file once more in a process of its own with every device buffer between two guard bands (COOK_GUARD=1
    is read when the library is loaded): all pass, and no write outside a buffer is reported"""
    env = dict(os.environ, COOK_GUARD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "not guarded_run"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=2400)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "COOK_GUARD: " not in r.stderr, r.stderr[-1500:]
