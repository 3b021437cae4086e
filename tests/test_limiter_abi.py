"""cook_limiters, cook_clock and cook_limiter_info (include/cookmatch.h) against their ctypes mirrors in cook_amd/_abi.py: sizes and the
offset of every field as a C compiler lays them out; the new entry points in the generated prototypes, in the header and in the
emulator build of the library; the ABI version; the JNI shim against the stub jni.h; and, on the emulator build, every refusal of the
limiters' contract leaving all state as it was, with the COOK_E_STATE orders.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from cook_amd import _abi as A
from cook_amd._protos import PROTOS
from cook_amd.engine import Engine
from tests import limiter_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cook_cycle_set_limiters", "cook_cycle_set_clock", "cook_cycle_limiters_spend", "cook_cycle_fetch_limiters", "cook_cycle_fetch_rate_limit",
       "cook_cycle_limiter_info")


@pytest.fixture(scope="module")
def make_engine():
    from tests.simt_emu import build_emu
    so = build_emu.build()
    return lambda params: Engine(params, lib_path=so)


def test_limiter_struct_layouts(tmp_path):
    text, want = X.struct_layout_sources()
    src = tmp_path / "layout.c"
    src.write_text(text)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want
    assert want[-1] == 4 and A.ABI_VERSION == 4  # everything is additive
    assert C.sizeof(A.CookLimiters) == 48 and C.sizeof(A.CookClock) == 16 and C.sizeof(A.LimiterInfo) == 24


def test_limiter_prototypes():
    header = open(os.path.join(ROOT, "include", "cookmatch.h")).read()
    for name in NEW:
        assert name in PROTOS and re.search(r"\bint %s\(" % name, header), name
    assert [len(PROTOS[n][1]) for n in NEW] == [2, 2, 4, 4, 3, 2]
    assert PROTOS["cook_cycle_limiters_spend"][1][2:] == [C.c_uint32, C.c_int64]
    subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "gen_protos.py"), "--check"])
    assert "cook_*" in open(os.path.join(ROOT, "cook_amd", "csrc", "exports.map")).read()  # (every cook_ symbol is exported)
    st, keep = A.Limiters([60.0, 6.0], [5, 7], [1, -2], [10, 20], user=[4, 2]).as_struct()
    assert st.n == 2 and [st.user[x] for x in range(2)] == [4, 2] and st.per_minute[1] == 6.0 and st.bucket[1] == 7 and st.tokens[1] == -2
    assert st.last_update_ms[0] == 10
    st, keep = A.Limiters([60.0], [5], [1], [10]).as_struct()
    assert st.n == 1 and not st.user


def test_limiter_symbols_exported_by_the_emulator_build():
    from tests.simt_emu import build_emu
    lib = C.CDLL(build_emu.build())
    for name in NEW:
        assert hasattr(lib, name), name
    lib.cook_abi_version.restype = C.c_int
    assert lib.cook_abi_version() == 4


def test_limiter_jni_shim_type_checks():
    """bindings/jni/cookmatch_jni.c, with the new entries, against the stub jni.h (as tests/test_abi.py does it)"""
    shim = os.path.join(ROOT, "bindings", "jni", "cookmatch_jni.c")
    text = open(shim).read()
    for name in NEW:
        assert name + "(" in text, name
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "tests", "jni_stub"), "-I", os.path.join(ROOT, "include"), shim])


def test_limiter_refusals_leave_state(make_engine):
    X.check_refusals(make_engine)


def test_limiter_null_arguments(make_engine):
    """NULL engine, NULL out, fetch with every array NULL, info without limiters"""
    with make_engine(X.P1()) as e:
        lib = e._lib
        assert lib.cook_cycle_set_limiters(None, None) == X.COOK_E_INVALID and lib.cook_cycle_set_clock(None, None) == X.COOK_E_INVALID
        assert lib.cook_cycle_limiter_info(e._h, None) == X.COOK_E_INVALID
        assert e.limiter_info() == dict(earned=0, spent_users=0, in_debt=0, spent=0)
        e.cycle_set_clock(5, 5)  # (host-only state: accepted before a stage, taken back by None)
        e.cycle_set_clock(None)
        assert lib.cook_cycle_fetch_rate_limit(e._h, None, None) == X.COOK_E_STATE
        pool = X.make_pool(7, 3, n_pending=40, n_offers=2)
        e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)
        e.cycle_set_limiters(X.random_limiters(7, 3))
        assert lib.cook_cycle_fetch_limiters(e._h, None, None, None) == 0
        until = np.zeros(3, np.int64)
        assert lib.cook_cycle_fetch_limiters(e._h, None, None, until.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(until, e.fetch_limiters(3)[2])
