"""The queue cycles (cook_cycle_run_queue*) on a machine WITHOUT a GPU: the cook_amd/csrc sources compiled against the SIMT emulator
(tests/simt_emu), against tests/golden/queue_cycles.json, the hand-derived edges and the oracle of tests/queue_cases.py (hundreds of rows)."""
import ctypes as C
import os
import subprocess

import pytest

from cook_amd import _abi as A
from cook_amd import synth
from cook_amd.engine import Engine
from tests import queue_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def make_engine():
    from tests.simt_emu import build_emu
    so = build_emu.build()
    return lambda params: Engine(params, lib_path=so)


def test_queue_golden(make_engine):
    S.check_golden(make_engine)


def test_queue_edges(make_engine):
    S.check_edges(make_engine)


@pytest.mark.parametrize("kw", [
    dict(seed=101, n_pending=600, n_running=300, n_users=30, n_offers=12, q_offers=6, k=120, host_path=True),
    dict(seed=102, n_pending=500, n_running=200, n_users=9, n_offers=10, q_offers=10, k=500, fractional=True, skip_frac=0.3),          # K = all
    dict(seed=103, n_pending=400, n_running=100, n_users=20, n_offers=10, q_offers=4, k=80, states=False, remove_modes=[0, 0, 1, 0, 1, 0]),
], ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_queue_random(make_engine, kw):
    kw = dict(kw)
    seed, k, n_offers = kw.pop("seed"), kw.pop("k"), kw.pop("q_offers")
    cyc = {x: kw.pop(x) for x in ("states", "skip_frac", "remove_modes") if x in kw}
    host_path = kw.pop("host_path", False)
    pool = synth.make_pool(seed=seed, **kw)
    cycles = S.make_cycles(pool, seed, k, 6, n_offers, fractional=kw.get("fractional", False), **cyc)
    S.check_cycles(make_engine, A.default_params(good_enough_fitness=1.0), pool, cycles, host_path=host_path)


@pytest.mark.parametrize("algo", [1, 2, 3])
def test_queue_random_groups(make_engine, algo):
    """every placement form on a pool with groups, each at a shape where it is eligible (asserted from the placement statistics):
    the serial sweep and the window rounds with unique, balanced and attribute-equals groups, fractional resources, constraints and
    gpus; class-ordered best fit takes unique groups and resources on its grid only (cookmatch.h, statistics word [38])"""
    cf = algo == 3
    seed = 105 if cf else 104  # (seeds chosen on the oracle alone: the fold must change a placement)
    kw = dict(n_pending=500, n_running=200, n_users=25, n_offers=24, gpus=True, constraints=True, fractional=not cf)
    pool = synth.make_pool(seed=seed, **kw)
    if not cf:
        pool = S.mix_group_types(pool, seed)
    cycles = S.make_cycles(pool, seed, 150, 6, 24, fractional=not cf, offer_kw=dict(gpus=True, constraints=True))
    S.check_cycles(make_engine, A.default_params(good_enough_fitness=1.0, match_algo=algo), pool, cycles, group_case=True,
                   table_variant=(algo != 1), expect_form={1: 1, 2: 0, 3: 3}[algo])


def test_queue_multi(make_engine, multi_mode):
    shapes = [(500, 300, 20, 12), (300, 100, 12, 10), (0, 20, 4, 8), (400, 50, 15, 10)]
    pools = [synth.make_pool(seed=110 + i, n_pending=npd, n_running=nr, n_users=nu, n_offers=no, fractional=(i == 1))
             for i, (npd, nr, nu, no) in enumerate(shapes)]
    cycles_of = [S.make_cycles(pl, 110 + i, 100, 6, no) for i, (pl, no) in enumerate(zip(pools, [5, 4, 8, 4]))]  # offers well below K
    S.check_multi(make_engine, pools, A.default_params(good_enough_fitness=1.0, match_algo=2), cycles_of)


def test_queue_state_rule(make_engine):
    S.check_state_rule(make_engine, synth.make_pool(seed=106, n_pending=300, n_running=200, n_users=12, n_offers=16, constraints=True))


class _Recorder:
    """an engine's library, noting the cook_cycle_run_queue* functions as they are called"""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("cook_cycle_run_queue"):
            return fn

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call


def test_queue_wrappers_reach_their_own_exports(make_engine):
    """every queue-cycle wrapper of cook_amd.engine calls the C entry of its own name (the wrappers are the only coverage the eleven
    exports have): one job leaves the queue per cycle, the deferred forms are placed by cycle_match_multi"""
    from cook_amd import engine as E
    single = ["cycle_run_queue", "cycle_run_queue_rank", "cycle_run_queue_carry", "cycle_run_queue_release", "cycle_run_queue_hosts",
              "cycle_run_queue_reserve"]
    multi = ["cycle_run_queue_multi", "cycle_run_queue_carry_multi", "cycle_run_queue_release_multi", "cycle_run_queue_hosts_multi",
             "cycle_run_queue_reserve_multi"]
    pool = S._tiny_pool(len(single) + len(multi) + 1, 2.0, offers=S._offers([2.0, 2.0]))
    with make_engine(A.default_params(good_enough_fitness=1.0)) as e:
        e._lib = rec = _Recorder(e._lib)
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        e.cycle_run(1)
        for i, name in enumerate(single + multi):
            step = dict(offers=S._offers([2.0, 2.0]))
            carry = [] if name in ("cycle_run_queue", "cycle_run_queue_rank", "cycle_run_queue_multi") else [A.QueueCarry()]  # (zero flags)
            if name in single:
                getattr(e, name)(1, *carry, **step)
            else:
                getattr(E, name)([e], 1, [step], *[carry] * len(carry))
            if name.endswith(("_rank", "_multi")):
                E.cycle_match_multi([e])
            assert rec.names == ["cook_" + name], (name, rec.names)
            del rec.names[:]
            Q, j2o, _ = e.cycle_fetch()
            assert len(Q) == len(single) + len(multi) - i and j2o.tolist() == [0], (name, len(Q), j2o)


def test_queue_struct_sizes(tmp_path):
    text, want = S.struct_size_sources()
    src = tmp_path / "sz.c"
    src.write_text(text)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want
