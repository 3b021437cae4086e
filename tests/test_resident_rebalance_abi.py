"""cook_cycle_rebalance (include/cookmatch.h) against its ctypes mirror in cook_amd/_abi.py: size and the offset of every field as a C
compiler lays them out; the two new entry points in the generated prototypes, the header and the emulator build; the ABI version; the
JNI shim against the stub jni.h; reservations_of's pending_ord.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

from cook_amd import _abi as A
from cook_amd._protos import PROTOS
from cook_amd.engine import reservations_of
from tests import resident_rebalance_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cook_cycle_rebalance_stage", "cook_cycle_rebalance_fetch")


def test_resident_rebalance_struct_layout(tmp_path):
    text, want = X.struct_layout_sources()
    src = tmp_path / "layout.c"
    src.write_text(text)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want
    assert want[-1] == 4 and A.ABI_VERSION == 4  # everything is additive
    assert C.sizeof(A.CookCycleRebalance) == C.sizeof(A.CookRebalanceParams) + 3 * C.sizeof(C.c_void_p) + 8


def test_resident_rebalance_prototypes():
    header = open(os.path.join(ROOT, "include", "cookmatch.h")).read()
    for name in NEW:
        assert name in PROTOS and re.search(r"\bint %s\(" % name, header), name
    assert len(PROTOS["cook_cycle_rebalance_stage"][1]) == 2 and len(PROTOS["cook_cycle_rebalance_fetch"][1]) == 9
    subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "gen_protos.py"), "--check"])
    assert "cook_*" in open(os.path.join(ROOT, "cook_amd", "csrc", "exports.map")).read()  # (every cook_ symbol is exported)


def test_reservations_of_pending_ord():
    d = [dict(pending_index=0, host=9, tasks=[1, 2]), dict(pending_index=2, host=8, tasks=[3]), dict(pending_index=1, host=7, tasks=[A.NONE_U32, 4])]
    pend, host = reservations_of(d, pending_ord=np.array([40, 50, 60], np.uint32))
    assert pend.tolist() == [40, 50] and host.tolist() == [9, 7] and pend.dtype == np.uint32
    pend, host = reservations_of(d)  # the default is unchanged: indices into the pending list
    assert pend.tolist() == [0, 1] and host.tolist() == [9, 7]
    assert [len(x) for x in reservations_of([], pending_ord=np.zeros(0, np.uint32))] == [0, 0]


def test_resident_rebalance_symbols_exported_by_the_emulator_build():
    from tests.simt_emu import build_emu
    lib = C.CDLL(build_emu.build())
    for name in NEW:
        assert hasattr(lib, name), name
    lib.cook_abi_version.restype = C.c_int
    assert lib.cook_abi_version() == 4


def test_resident_rebalance_jni_shim_type_checks():
    """bindings/jni/cookmatch_jni.c, with the two new entries, against the stub jni.h (as tests/test_abi.py does it)"""
    shim = os.path.join(ROOT, "bindings", "jni", "cookmatch_jni.c")
    text = open(shim).read()
    for name in NEW:
        assert name + "(" in text, name
    assert "cycleRebalanceStage" in text and "cycleRebalanceFetch" in text
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "tests", "jni_stub"), "-I",
                           os.path.join(ROOT, "include"), shim])
