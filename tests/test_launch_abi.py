"""The layout of cook_launch_offers / cook_launch_out / cook_launch_info against their ctypes mirrors (compiled against the header),
COOK_ABI_VERSION still 4, the call among the exports of the header, the bindings and the built library."""
import os
import re
import subprocess
import sys

from cook_amd import _abi as A
from cook_amd import engine
from tests import launch_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = "cook_match_launch_resources"


def test_launch_structs_match_header(tmp_path):
    text, want = K.struct_size_sources()
    src = tmp_path / "sz.c"
    src.write_text(text)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want


def test_launch_call_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "cookmatch.h")).read()
    assert int(re.search(r"#define COOK_ABI_VERSION (\d+)", hdr).group(1)) == A.ABI_VERSION == 4  # nothing existing changed layout
    assert re.search(r"^int %s\(" % FN, hdr, flags=re.M)
    assert FN in engine.EXPORTS and FN in engine.PROTOS
    assert callable(engine.Engine.match_launch_resources)
    subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "gen_protos.py"), "--check"])


def test_launch_symbol_is_exported():
    """the emulated build exports what the header declares (load_library resolves every prototype), the version script lets it through"""
    from tests.simt_emu import build_emu
    lib = engine.load_library(build_emu.build())
    assert lib.cook_abi_version() == 4 and getattr(lib, FN) is not None
    assert "cook_*" in open(os.path.join(ROOT, "cook_amd", "csrc", "exports.map")).read()


def test_launch_symbol_is_exported_by_the_shipped_library():
    from cook_amd import build
    syms = subprocess.check_output(["nm", "-D", "--defined-only", build.build()], text=True)
    assert re.search(r"\bT %s$" % FN, syms, flags=re.M)


def test_jni_shim_binds_the_call():
    txt = open(os.path.join(ROOT, "bindings", "jni", "cookmatch_jni.c")).read()
    assert re.search(r"\b%s\(" % FN, txt) and "Java_cook_hip_Native_matchLaunchResources(" in txt
    body = txt[txt.index("Java_cook_hip_Native_matchLaunchResources("):]
    assert "cook_match_count(" in body[:body.index("\n}\n")], "k is compared with the engine's own count before the sizes are checked against it"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "tests", "jni_stub"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "bindings", "jni", "cookmatch_jni.c")])
