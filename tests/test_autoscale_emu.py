"""cook_cycle_autoscale on a machine WITHOUT a GPU: the cook_amd/csrc sources compiled against the SIMT emulator (tests/simt_emu),
against tests/golden/autoscale.json and the oracle of tests/autoscale_cases.py (small sizes)."""
import ctypes as C
import os
import subprocess

import pytest

from cook_amd import _abi as A
from cook_amd import synth
from cook_amd.engine import Engine
from tests import autoscale_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def make_engine():
    from tests.simt_emu import build_emu
    so = build_emu.build()
    return lambda params: Engine(params, lib_path=so)


def test_autoscale_golden(make_engine):
    S.check_golden(make_engine)


@pytest.mark.parametrize("kw", [
    dict(seed=81, n_pending=600, n_running=300, n_users=30, n_offers=40, k=200),
    dict(seed=82, n_pending=900, n_running=500, n_users=9, n_offers=120, k=900, fractional=True),   # K = all, fix-up paths
    dict(seed=83, n_pending=500, n_running=200, n_users=50, n_offers=60, k=300, fractional=True, gpus=True, constraints=True),
    dict(seed=84, n_pending=400, n_running=0, n_users=20, n_offers=8, k=50, tokens=False, pool_quota=False),
    dict(seed=85, n_pending=300, n_running=100, n_users=15, n_offers=500, k=300, enforce=False),   # most jobs match
], ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_autoscale_random(make_engine, kw):
    kw = dict(kw)
    seed, k = kw.pop("seed"), kw.pop("k")
    state = {x: kw.pop(x) for x in ("tokens", "pool_quota", "enforce") if x in kw}
    pool = synth.make_pool(seed=seed, **kw)
    S.check_random(make_engine, pool, seed, k, n_calls=4, fractional=kw.get("fractional", False), **state)


def test_autoscale_state_rule(make_engine):
    S.check_state_rule(make_engine, synth.make_pool(seed=86, n_pending=300, n_running=200, n_users=12, n_offers=16))


def test_autoscale_leaves_the_cycle_alone(make_engine):
    S.check_cycle_undisturbed(make_engine, synth.make_pool(seed=87, n_pending=600, n_running=400, n_users=30, n_offers=24))


def test_autoscale_struct_sizes(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "cookmatch.h"\nint main(){printf("%zu %zu\\n", sizeof(cook_autoscale_params), '
                   'sizeof(cook_autoscale_info));return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes == [C.sizeof(A.CookAutoscaleParams), C.sizeof(A.CookAutoscaleInfo)]


def test_autoscale_after_match_multi(make_engine, multi_mode):
    pools = [synth.make_pool(seed=88 + i, n_pending=npd, n_running=nr, n_users=nu, n_offers=no, fractional=(i == 1))
             for i, (npd, nr, nu, no) in enumerate([(500, 300, 20, 30), (300, 100, 12, 200), (0, 20, 4, 8)])]
    S.check_multi(make_engine, pools, A.default_params(good_enough_fitness=1.0, match_algo=2), 150)
