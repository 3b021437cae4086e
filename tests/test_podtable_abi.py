"""cook_pod_delta, cook_pod_delta_info and cook_pod_rows (include/cookmatch.h) against their ctypes mirrors in cook_amd/_abi.py: sizes and
the offset of every field as a C compiler lays them out; the new entry points in the generated prototypes, in the header and in the
emulator build of the library; the ABI version; the JNI shim against the stub jni.h; and, on the emulator build, every refusal of the
pod table's contract leaving all state as it was.  No GPU needed."""
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
from tests import podtable_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cook_offers_stage_pod_ids", "cook_offers_update", "cook_offers_update_info", "cook_offers_fetch_pods", "cook_cycle_set_built_offers",
       "cook_cycle_run_queue_pods", "cook_cycle_run_queue_pods_multi")


@pytest.fixture(scope="module")
def make_engine():
    from tests.simt_emu import build_emu
    so = build_emu.build()
    return lambda params: Engine(params, lib_path=so)


def test_podtable_struct_layouts(tmp_path):
    text, want = X.struct_layout_sources()
    src = tmp_path / "layout.c"
    src.write_text(text)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want
    assert want[-1] == 4 and A.ABI_VERSION == 4  # everything is additive
    assert C.sizeof(A.CookPodDelta) == 56 and C.sizeof(A.CookPodDeltaInfo) == 24 and C.sizeof(A.CookPodRows) == 80


def test_podtable_prototypes():
    header = open(os.path.join(ROOT, "include", "cookmatch.h")).read()
    for name in NEW:
        assert name in PROTOS and re.search(r"\bint %s\(" % name, header), name
    assert [len(PROTOS[n][1]) for n in NEW] == [4, 2, 2, 2, 2, 8, 9]
    assert PROTOS["cook_cycle_run_queue_pods"][1][6:] == [C.c_int, C.c_uint32]
    subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "gen_protos.py"), "--check"])
    assert "cook_*" in open(os.path.join(ROOT, "cook_amd", "csrc", "exports.map")).read()  # (every cook_ symbol is exported)
    add = A.Pods(node=[1, 2], cpus=[0.1, 0.3], mem=[1.0, 2.0])
    st, keep = A.PodDelta(remove=[7, 9, 11], add=add, add_id=[3, 4], node_rows=[5], node_values=A.Nodes(cpus=[2.0], mem=[3.0])).as_struct()
    assert st.n_remove == 3 and [st.remove_id[x] for x in range(3)] == [7, 9, 11] and st.add.contents.n == 2 and st.add_id[1] == 4
    assert st.n_node_rows == 1 and st.node_row[0] == 5 and st.node_values.contents.cpus[0] == 2.0 and not st.node_values.contents.host
    st, keep = A.PodDelta().as_struct()
    assert st.n_remove == 0 and not st.add and not st.node_values and st.n_node_rows == 0


def test_podtable_symbols_exported_by_the_emulator_build():
    from tests.simt_emu import build_emu
    lib = C.CDLL(build_emu.build())
    for name in NEW:
        assert hasattr(lib, name), name
    lib.cook_abi_version.restype = C.c_int
    assert lib.cook_abi_version() == 4


def test_podtable_jni_shim_type_checks():
    """bindings/jni/cookmatch_jni.c, with the new entries, against the stub jni.h (as tests/test_abi.py does it)"""
    shim = os.path.join(ROOT, "bindings", "jni", "cookmatch_jni.c")
    text = open(shim).read()
    for name in NEW:
        assert name + "(" in text, name
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "tests", "jni_stub"), "-I", os.path.join(ROOT, "include"), shim])


def test_podtable_refusals_leave_state(make_engine):
    X.check_refusals(make_engine)


def test_podtable_null_arguments(make_engine):
    """NULL engine, NULL delta, NULL out; info and fetch before anything is staged; a fetch whose cap is too small reports n"""
    with make_engine(X.P1()) as e:
        lib = e._lib
        assert lib.cook_offers_update(None, None) == X.COOK_E_INVALID and lib.cook_offers_stage_pod_ids(None, None, 0, 0) == X.COOK_E_INVALID
        assert lib.cook_offers_update_info(e._h, None) == X.COOK_E_INVALID and lib.cook_offers_fetch_pods(e._h, None) == X.COOK_E_INVALID
        assert lib.cook_cycle_set_built_offers(None, 0) == X.COOK_E_INVALID
        assert lib.cook_cycle_run_queue_pods_multi(None, 0, None, None, None, None, None, None, None) == X.COOK_E_INVALID
        assert e.offers_update_info() == dict(removed=0, remove_missing=0, added=0, node_rows=0, n_pods=0, n_offers=0)
        assert lib.cook_offers_fetch_pods(e._h, C.byref(A.CookPodRows())) == X.COOK_E_STATE
        nodes, pods = A.Nodes(cpus=[4.0], mem=[8.0], host=[3]), A.Pods(node=[0, 0], cpus=[0.1, 0.3], mem=[1.0, 1.0])
        e.offers_stage(nodes, pods, A.offer_params())
        assert lib.cook_offers_update(e._h, None) == X.COOK_E_INVALID
        probe = A.CookPodRows()
        assert lib.cook_offers_fetch_pods(e._h, C.byref(probe)) == X.COOK_E_INVALID and probe.n == 2
        rows = e.offers_fetch_pods()
        assert rows.column("cpus").tolist() == [0.1, 0.3] and (rows.column("id") == A.NONE_U32).all() and (rows.column("disk") == -1.0).all()
        e.offers_stage_pod_ids([5, 2], 6)
        assert e.offers_fetch_pods().column("id").tolist() == [5, 2]
        assert e.offers_update_info() == dict(removed=0, remove_missing=0, added=0, node_rows=0, n_pods=2, n_offers=0)
        e.offers_update(A.PodDelta(remove=[5, 0]))
        assert e.offers_update_info() == dict(removed=1, remove_missing=1, added=0, node_rows=0, n_pods=1, n_offers=0)
        assert np.array_equal(e.offers_fetch_pods().column("id"), [2])
