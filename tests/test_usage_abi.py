"""The layout of cook_usage_out against its ctypes mirror (compiled against the header), the two calls among the exports, and their
names in the JNI shim."""
import ctypes as C
import os
import re
import subprocess

from cook_amd import _abi as A
from cook_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["cap_rows", "n_buckets", "n_rows", "bucket_usage_is_device", "total_is_device", "reserved", "bucket_off", "bucket_group",
          "bucket_usage", "row_off", "rows", "total"]


def test_usage_out_layout_matches_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cookmatch.h"\nint main(){printf("%zu\\n", sizeof(cook_usage_out));' +
                   "".join(f'printf("%zu\\n", offsetof(cook_usage_out, {f}));' for f in FIELDS) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert [f for f, _ in A.CookUsageOut._fields_] == FIELDS
    assert got == [C.sizeof(A.CookUsageOut)] + [getattr(A.CookUsageOut, f).offset for f in FIELDS]


def test_usage_calls_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "cookmatch.h")).read()
    assert int(re.search(r"#define COOK_ABI_VERSION (\d+)", hdr).group(1)) == A.ABI_VERSION == 4  # nothing existing changed layout
    for fn in ("cook_usage_breakdown", "cook_usage_breakdown_multi"):
        assert re.search(r"^int %s\(" % fn, hdr, flags=re.M), fn
        assert fn in engine.EXPORTS and fn in engine.PROTOS
    assert callable(engine.Engine.usage_breakdown) and callable(engine.usage_breakdown_multi)


def test_jni_shim_binds_the_usage_calls():
    txt = open(os.path.join(ROOT, "bindings", "jni", "cookmatch_jni.c")).read()
    for fn, java in (("cook_usage_breakdown", "usageBreakdown"), ("cook_usage_breakdown_multi", "usageBreakdownMulti")):
        assert re.search(r"\b%s\(" % fn, txt), fn
        assert "Java_cook_hip_Native_%s(" % java in txt, java
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "tests", "jni_stub"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "bindings", "jni", "cookmatch_jni.c")])
