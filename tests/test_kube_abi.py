"""The C ABI of cook_kube_distribute, cook_cycle_run_kube(_multi) and cook_cycle_fetch_kube: struct sizes and offsets of the ctypes mirrors against include/cookmatch.h (compiled), the
generated prototype, the library's exports, the JNI shim, and the header's statement of the draw rule."""
import ctypes as C
import os
import subprocess

from cook_amd import _abi as A
from cook_amd._protos import PROTOS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cook_kube_distribute", "cook_cycle_run_kube", "cook_cycle_run_kube_multi", "cook_cycle_fetch_kube")
STRUCTS = {"cook_kube_clusters": A.CookKubeClusters, "cook_kube_cluster_info": A.CookKubeClusterInfo, "cook_kube_info": A.CookKubeInfo,
           "cook_kube_cycle": A.CookKubeCycle}


def test_struct_sizes_and_offsets(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cookmatch.h"', 'int main(){']
    want = []
    for cname, T in STRUCTS.items():
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        want.append(C.sizeof(T))
        for f, _ in T._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
            want.append(getattr(T, f).offset)
    lines += ['printf("%d %d %d %d\\n", COOK_KUBE_TILE, (int)COOK_KUBE_NO_CLUSTER, COOK_MAX_CLUSTERS, COOK_ABI_VERSION);', 'return 0;}']
    src = tmp_path / "sz.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:-4] == want
    assert got[-4:] == [A.KUBE_TILE, A.KUBE_NO_CLUSTER, A.MAX_CLUSTERS, 4]  # (additive: the ABI version stays)


def test_prototypes():
    assert PROTOS["cook_kube_distribute"] == (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 3 +
                                              [C.c_uint32] + [C.c_void_p] * 3)
    assert PROTOS["cook_cycle_run_kube"] == (C.c_int, [C.c_void_p] * 3 + [C.c_uint32] + [C.c_void_p] * 3)
    assert PROTOS["cook_cycle_run_kube_multi"] == (C.c_int, [C.c_void_p, C.c_uint32] + [C.c_void_p] * 7)
    assert PROTOS["cook_cycle_fetch_kube"] == (C.c_int, [C.c_void_p] * 3)
    r = subprocess.run(["python", os.path.join(ROOT, "scripts", "gen_protos.py"), "--check"])
    assert r.returncode == 0  # cook_amd/_protos.py is what scripts/gen_protos.py writes


def test_emulator_library_exports():
    from tests.simt_emu import build_emu
    lib = C.CDLL(build_emu.build())
    for name in NEW:
        assert getattr(lib, name)


def test_shipped_library_exports():
    """the gfx950 library's dynamic symbol table holds the new calls (built here: hipcc cross-compiles without a GPU)"""
    from cook_amd import build
    syms = subprocess.check_output(["nm", "-D", "--defined-only", build.build()], text=True)
    defined = {line.split()[-1] for line in syms.splitlines() if line.split()}
    for name in NEW:
        assert name in defined, name
    assert all(s.startswith("cook_") for s in defined if not s.startswith(("_", "__"))), "exports.map keeps everything else local"


def test_jni_shim_names_the_calls():
    txt = open(os.path.join(ROOT, "bindings", "jni", "cookmatch_jni.c")).read()
    for java, c in (("kubeDistribute", "cook_kube_distribute("), ("cycleRunKube", "cook_cycle_run_kube("),
                    ("cycleRunKubeMulti", "cook_cycle_run_kube_multi("), ("cycleFetchKube", "cook_cycle_fetch_kube(")):
        assert f"Java_cook_hip_Native_{java}(" in txt and c in txt
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "tests", "jni_stub"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "bindings", "jni", "cookmatch_jni.c")])


def test_header_states_the_draw_rule():
    """the splitmix64 constants are the contract: the header writes them out, and the Python mirror computes with the same ones"""
    txt = open(os.path.join(ROOT, "include", "cookmatch.h")).read()
    for const in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", ">> 11", "2^-53"):
        assert const in txt, const
    assert "rand-nth" in txt and "picks with rand-nth" not in txt  # the distributor is covered, not excused
    assert A.splitmix64(0) == 0xE220A8397B1DCDAF  # the generator's first output from state 0
    assert A.kube_seed_draw(0, 0) == float(0xE220A8397B1DCDAF >> 11) * 2.0 ** -53
