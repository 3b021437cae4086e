#!/usr/bin/env python3
"""Is the device code of the working tree the device code of a given commit?  (The check behind a host-only change: same kernels, so
same speed.)

Compiles cook_amd/csrc/engine.hip of REV (default HEAD) and of the working tree to gfx950 assembly with the flags of cook_amd/build.py plus
--cuda-device-only -S, cuts both by function symbol — the kernels and the device functions they call — and compares symbol by symbol: the
text from its label to .Lfunc_end, which for a kernel includes its .amdhsa_kernel descriptor (registers, LDS, scratch).  Dropped before the
comparison: .file / .loc / .ident lines and comments (whole lines, and the ones the compiler puts behind a label).  Renumbered: the function index in local labels (.LBB12_3, .Lfunc_end12, .LJTI12_0), which is
the function's position in the file and moves when a kernel is instantiated earlier or later in the translation unit.

Three builds: the shipped one, which must be identical, and the two study builds (-DCOOK_EVAL_TRACE; -DCOOK_WALK_PROF -DCF_PROF), which
must compile and keep their symbol sets (their bodies are compared too and reported).

  python scripts/device_code_diff.py [REV] [--work DIR]      # exit status 0: identical
--work DIR keeps the assembly files (REV's under DIR/parent, the tree's under DIR/head) and reuses the ones already there."""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# cook_amd/build.py's flags (the linker's apart), and assembly of the device side only
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-ffp-contract=off", "-fvisibility=hidden",
         "-fvisibility-inlines-hidden", "-Wall", "-Wno-unused-function", "--cuda-device-only", "-S"]
VARIANTS = [("shipped", []), ("eval_trace", ["-DCOOK_EVAL_TRACE"]), ("walk_prof", ["-DCOOK_WALK_PROF", "-DCF_PROF"])]
LOCAL = re.compile(r"\.(LBB|Lfunc_begin|Lfunc_end|LJTI|LCPI)\d+")


def compile_asm(src, out, defs):
    if os.path.exists(out) and os.path.getsize(out):
        return out
    r = subprocess.run([HIPCC] + FLAGS + defs + ["-o", out, src], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit(f"{src} {' '.join(defs)}: does not compile\n{r.stderr[-3000:]}")
    return out


def norm(line):
    s = line.strip()
    if not s.startswith((".asci", ".string")):
        s = s.split(";")[0].rstrip()
    if not s or s.startswith((".file", ".loc", ".ident")):
        return None
    return LOCAL.sub(lambda m: "." + m.group(1), s)


def functions(path):
    """symbol -> its lines, normalised"""
    lines = open(path).read().split("\n")
    funcs = set(m.group(1) for l in lines for m in [re.match(r"\s*\.type\s+(\S+),@function", l)] if m)
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"^([^\s:;.][^\s:;]*):", lines[i])
        if m and m.group(1) in funcs:
            j = i + 1
            while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
                j += 1
            out[m.group(1)] = [x for x in map(norm, lines[i + 1:j]) if x]
            i = j
        i += 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rev", nargs="?", default="HEAD")
    ap.add_argument("--work", default=None)
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp(prefix="device_code_diff.")
    parent = os.path.join(work, "parent")
    os.makedirs(os.path.join(work, "head"), exist_ok=True)
    if not os.path.isdir(os.path.join(parent, "cook_amd")):
        os.makedirs(parent, exist_ok=True)
        tar = subprocess.run(["git", "-C", ROOT, "archive", a.rev, "cook_amd/csrc", "include"], check=True, stdout=subprocess.PIPE).stdout
        subprocess.run(["tar", "-x", "-C", parent], input=tar, check=True)
    rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", a.rev], check=True, stdout=subprocess.PIPE, text=True).stdout.strip()
    jobs = {}
    with concurrent.futures.ThreadPoolExecutor(6) as ex:
        for name, defs in VARIANTS:
            jobs[name] = (ex.submit(compile_asm, os.path.join(parent, "cook_amd", "csrc", "engine.hip"), os.path.join(parent, name + ".s"), defs),
                          ex.submit(compile_asm, os.path.join(ROOT, "cook_amd", "csrc", "engine.hip"), os.path.join(work, "head", name + ".s"), defs))
    print(f"device code of the working tree against {rev}: hipcc {' '.join(FLAGS)}")
    bad = 0
    for name, defs in VARIANTS:
        p, h = functions(jobs[name][0].result()), functions(jobs[name][1].result())
        kernels = [s for s in p if any(x.startswith('.amdhsa_kernel ') for x in p[s])]
        missing, added = sorted(set(p) - set(h)), sorted(set(h) - set(p))
        differ = [s for s in sorted(set(p) & set(h)) if p[s] != h[s]]
        print(f"{name} ({' '.join(defs) or 'no definitions'}): {len(p)} function symbols at {rev}, {len(kernels)} of them kernels, "
              f"{sum(len(v) for v in p.values())} instruction and directive lines; the tree: {len(h)} symbols; "
              f"missing {len(missing)}, new {len(added)}, bodies that differ {len(differ)}")
        for s in missing:
            print(f"  missing: {s}")
        for s in added:
            print(f"  new: {s}")
        for s in differ:
            print(f"  differs: {s}")
        bad += len(missing) + len(added) + len(differ)
    print("verdict:", "IDENTICAL — the same symbols, every body the same, the kernels' descriptors included" if not bad else f"{bad} DIFFERENCES")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
