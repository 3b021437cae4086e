"""cook_sweep_running on a machine WITHOUT a GPU: the cook_amd/csrc sources compiled against the SIMT emulator (tests/simt_emu),
against tests/golden/sweep.json and the oracle of tests/sweep_oracle.py (small sizes)."""
import ctypes as C
import os
import subprocess

import pytest

from cook_amd import _abi as A
from cook_amd import synth
from cook_amd.engine import Engine
from tests import sweep_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def make_engine():
    from tests.simt_emu import build_emu
    so = build_emu.build()
    return lambda params: Engine(params, lib_path=so)


def test_sweep_golden_oracle():
    S.check_golden_oracle()


def test_sweep_golden(make_engine):
    S.check_golden(make_engine)


@pytest.mark.parametrize("kw", [
    dict(seed=1, n=3000, n_groups=60, n_succ=5000),
    dict(seed=2, n=2000, n_groups=300, n_succ=3000, ties=True),
    dict(seed=3, n=1500, n_groups=5, n_succ=9000, big_group=6000),   # one group over several sort tiles
    dict(seed=4, n=700, n_groups=1, n_succ=40),
    dict(seed=5, n=900, n_groups=0, n_succ=0),
], ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_sweep_random(make_engine, kw):
    kw = dict(kw)
    S.check_random(make_engine, S.random_table(kw.pop("seed"), **kw), whats=(7, 1, 2, 4, 3, 6))


def test_sweep_errors(make_engine):
    S.check_errors(make_engine, S.random_table(6, 2000, 40, 4000), 6)


def test_sweep_struct_sizes(tmp_path):
    src = tmp_path / "sz.c"
    names = ["cook_running_set", "cook_straggler_groups", "cook_sweep_params", "cook_sweep_info"]
    src.write_text('#include <stdio.h>\n#include "cookmatch.h"\nint main(){' + "".join(f'printf("%zu\\n", sizeof({n}));' for n in names) +
                   "return 0;}")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes == [C.sizeof(A.CookRunningSet), C.sizeof(A.CookStragglerGroups), C.sizeof(A.CookSweepParams), C.sizeof(A.CookSweepInfo)]


def test_sweep_leaves_the_cycle_alone(make_engine):
    pool = synth.make_pool(seed=91, n_pending=500, n_running=300, n_users=20, n_offers=30)
    S.check_cycle_undisturbed(make_engine, pool, S.random_table(7, 1500, 30, 2500))
