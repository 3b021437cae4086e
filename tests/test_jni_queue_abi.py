"""What the JNI shim (bindings/jni/cookmatch_jni.c) passes down to the queue-cycle entries of the C ABI: the shim compiled into
tests/jni_stub/queue_cycle_probe.c, which plays the JVM over fake buffers and the library over recording entries, against
tests/golden/jni_queue_cycle_probe.txt.  The fixture was recorded from the shim as it stood before its marshalling was folded into
one helper per struct; a change of the shim that is meant to change what crosses re-records it.  No GPU, no library, no JDK needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_jni_queue_cycle_exports_pass_down_what_they_did(tmp_path):
    exe = tmp_path / "queue_cycle_probe"
    # one section per function, unreferenced ones dropped: the shim's other exports need no cook_* symbol to exist
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-ffunction-sections", "-I", os.path.join(ROOT, "tests", "jni_stub"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "jni_stub", "queue_cycle_probe.c"),
                           "-Wl,--gc-sections", "-o", str(exe)])
    got = subprocess.run([str(exe)], stdout=subprocess.PIPE, check=True).stdout  # (exit 1: a short buffer reached an entry)
    with open(os.path.join(ROOT, "tests", "golden", "jni_queue_cycle_probe.txt"), "rb") as f:
        want = f.read()
    assert want.count(b"-> cook_cycle_") == 35 and want.count(b"a byte short: rc=-1 entries called=0") == 15
    assert got == want
