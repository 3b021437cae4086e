"""The C ABI of cook_cycle_set_job_hashes / cook_cycle_autoscale_clusters(_multi): struct sizes and offsets of the ctypes mirrors
against include/cookmatch.h (compiled), the generated prototypes, the library's exports, the JNI shim, and uuid_hash."""
import ctypes as C
import os
import subprocess
import uuid

from cook_amd import _abi as A
from cook_amd._protos import PROTOS
from tests import distribute_oracle as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cook_cycle_set_job_hashes", "cook_cycle_autoscale_clusters", "cook_cycle_autoscale_clusters_multi")
STRUCTS = {"cook_autoscale_clusters": A.CookAutoscaleClusters, "cook_autoscale_cluster_info": A.CookAutoscaleClusterInfo,
           "cook_autoscale_no_cluster": A.CookAutoscaleNoCluster}


def test_struct_sizes_and_offsets(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cookmatch.h"', 'int main(){']
    want = []
    for cname, T in STRUCTS.items():
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        want.append(C.sizeof(T))
        for f, _ in T._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
            want.append(getattr(T, f).offset)
    lines += ['printf("%d %d\\n", COOK_MAX_CLUSTERS, COOK_ABI_VERSION);', 'return 0;}']
    src = tmp_path / "sz.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:-2] == want
    assert got[-2] == A.MAX_CLUSTERS == 32 and got[-1] == 4  # (additive: the ABI version stays)


def test_prototypes():
    assert PROTOS["cook_cycle_set_job_hashes"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32])
    assert PROTOS["cook_cycle_autoscale_clusters"] == (C.c_int, [C.c_void_p] * 4 + [C.c_uint32] + [C.c_void_p] * 4)
    assert PROTOS["cook_cycle_autoscale_clusters_multi"] == (C.c_int, [C.c_void_p, C.c_uint32] + [C.c_void_p] * 9)
    r = subprocess.run(["python", os.path.join(ROOT, "scripts", "gen_protos.py"), "--check"])
    assert r.returncode == 0  # cook_amd/_protos.py is what scripts/gen_protos.py writes


def test_emulator_library_exports():
    from tests.simt_emu import build_emu
    lib = C.CDLL(build_emu.build())
    for name in NEW:
        assert getattr(lib, name)


def test_exports_map_covers_the_calls():
    txt = open(os.path.join(ROOT, "cook_amd", "csrc", "exports.map")).read()
    assert "cook_*" in txt
    src = open(os.path.join(ROOT, "cook_amd", "csrc", "engine.hip")).read()
    for name in NEW:
        assert f"int {name}(" in src


def test_jni_shim_names_the_calls():
    txt = open(os.path.join(ROOT, "bindings", "jni", "cookmatch_jni.c")).read()
    for java, c in (("cycleSetJobHashes", "cook_cycle_set_job_hashes("), ("cycleAutoscaleClusters", "cook_cycle_autoscale_clusters("),
                    ("cycleAutoscaleClustersMulti", "cook_cycle_autoscale_clusters_multi(")):
        assert f"Java_cook_hip_Native_{java}(" in txt and c in txt
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "tests", "jni_stub"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "bindings", "jni", "cookmatch_jni.c")])


def test_uuid_hash():
    # java.util.UUID.hashCode by hand: hilo = msb ^ lsb, (int)(hilo >> 32) ^ (int)hilo
    assert A.uuid_hash(uuid.UUID(int=0)) == 0
    assert A.uuid_hash(uuid.UUID(int=1)) == 1
    assert A.uuid_hash(uuid.UUID(int=1 << 63)) == -2 ** 31                 # lsb = 0x8000000000000000
    assert A.uuid_hash(uuid.UUID(int=(1 << 64) | 1)) == 0                  # msb = lsb = 1
    assert A.uuid_hash(uuid.UUID(int=0xFFFFFFFF)) == -1
    assert A.uuid_hash(uuid.UUID("123e4567-e89b-12d3-a456-426614174000")) == 0x123e4567 ^ 0xe89b12d3 ^ 0xa4564266 ^ 0x14174000 == 0x4ae455d2
    for k in range(50):
        u = uuid.UUID(int=(k * 0x9E3779B97F4A7C15F39CC0605CEDC835) % (1 << 128))
        assert A.uuid_hash(u) == D.java_uuid_hash(u) and -2 ** 31 <= A.uuid_hash(u) < 2 ** 31
