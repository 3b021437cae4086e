"""cook_reservations and cook_reserve_info (include/cookmatch.h) against their ctypes mirrors in cook_amd/_abi.py: sizes and the offset
of every field as a C compiler lays them out; the five new entry points in the generated prototypes and in the header; the ABI
version; the JNI shim against the stub jni.h.  No GPU, no library needed."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

from cook_amd import _abi as A
from cook_amd._protos import PROTOS
from cook_amd.engine import reservations_of
from tests import reserve_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cook_cycle_set_reservations", "cook_cycle_run_queue_reserve", "cook_cycle_run_queue_reserve_multi", "cook_cycle_reserve_info",
       "cook_cycle_fetch_reservations")


def test_reserve_struct_layouts(tmp_path):
    text, want = X.struct_layout_sources()
    src = tmp_path / "layout.c"
    src.write_text(text)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want
    assert want[-1] == 4 and A.ABI_VERSION == 4  # everything is additive


def test_reserve_prototypes():
    header = open(os.path.join(ROOT, "include", "cookmatch.h")).read()
    for name in NEW:
        assert name in PROTOS and re.search(r"\bint %s\(" % name, header), name
    assert len(PROTOS["cook_cycle_run_queue_reserve"][1]) == 7 and len(PROTOS["cook_cycle_run_queue_reserve_multi"][1]) == 8
    assert len(PROTOS["cook_cycle_fetch_reservations"][1]) == 5 and len(PROTOS["cook_cycle_set_reservations"][1]) == 2
    subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "gen_protos.py"), "--check"])
    assert "cook_*" in open(os.path.join(ROOT, "cook_amd", "csrc", "exports.map")).read()  # (every cook_ symbol is exported)
    st, keep = A.Reservations([3, A.NONE_U32], [7, 9], release_matched=False).as_struct()
    assert (st.release_matched, st.replace, st.n) == (0, 1, 2) and [st.pending[x] for x in range(2)] == [3, A.NONE_U32] and st.host[1] == 9
    st, keep = A.Reservations().as_struct()
    assert (st.release_matched, st.replace, st.n) == (1, 1, 0) and not st.pending and not st.host
    assert C.sizeof(A.ReserveInfo) == 16


def test_reservations_of():
    """reserve-hosts!'s filter: more than one preempted task, the NONE_U32 entries counted"""
    d = [dict(pending_index=4, host=9, tasks=[1, 2]), dict(pending_index=5, host=8, tasks=[3]), dict(pending_index=6, host=7, tasks=[A.NONE_U32, 4]),
         dict(pending_index=7, host=6, task_n=3), dict(pending_index=8, host=5, task_n=1)]
    pend, host = reservations_of(d)
    assert pend.tolist() == [4, 6, 7] and host.tolist() == [9, 7, 6] and pend.dtype == np.uint32
    assert [len(x) for x in reservations_of([])] == [0, 0]


def test_reserve_symbols_exported_by_the_emulator_build():
    from tests.simt_emu import build_emu
    lib = C.CDLL(build_emu.build())
    for name in NEW:
        assert hasattr(lib, name), name
    lib.cook_abi_version.restype = C.c_int
    assert lib.cook_abi_version() == 4


def test_reserve_jni_shim_type_checks():
    """bindings/jni/cookmatch_jni.c, with the five new entries, against the stub jni.h (as tests/test_abi.py does it)"""
    shim = os.path.join(ROOT, "bindings", "jni", "cookmatch_jni.c")
    text = open(shim).read()
    for name in NEW:
        assert name + "(" in text, name
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "tests", "jni_stub"), "-I", os.path.join(ROOT, "include"), shim])
