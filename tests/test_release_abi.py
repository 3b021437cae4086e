"""cook_finished and cook_release_info (include/cookmatch.h) against their ctypes mirrors in cook_amd/_abi.py: sizes and the offset of
every field as a C compiler lays them out, and the three new entry points in the generated prototypes.  No GPU, no library needed."""
import os
import subprocess
import sys

from cook_amd import _abi as A
from cook_amd._protos import PROTOS
from tests import release_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_release_struct_layouts(tmp_path):
    text, want = X.struct_layout_sources()
    src = tmp_path / "layout.c"
    src.write_text(text)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want


def test_release_prototypes():
    for name in ("cook_cycle_run_queue_release", "cook_cycle_run_queue_release_multi", "cook_cycle_release_info"):
        assert name in PROTOS
    subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "gen_protos.py"), "--check"])
    st, keep = A.Finished(host=[1, 2], cpus=[1.0, 2.0], mem=[3.0, 4.0], scalars=[[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], offers=1).as_struct()
    assert (st.n, st.n_scalars, st.offers, st.usage, st.groups) == (2, 3, 1, 0, 0)
    assert [st.scalars[x] for x in range(6)] == [1.0, 4.0, 2.0, 5.0, 3.0, 6.0]  # one contiguous column per name, as cook_jobs.scalars
