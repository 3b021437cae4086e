"""cook_host_churn, cook_churn_info and cook_offer_rows (include/cookmatch.h) against their ctypes mirrors in cook_amd/_abi.py: sizes and
the offset of every field as a C compiler lays them out, and the four new entry points in the generated prototypes.  No GPU, no
library needed."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from cook_amd import _abi as A
from cook_amd._protos import PROTOS
from tests import churn_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_churn_struct_layouts(tmp_path):
    text, want = X.struct_layout_sources()
    src = tmp_path / "layout.c"
    src.write_text(text)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want


def test_churn_prototypes():
    for name in ("cook_cycle_run_queue_hosts", "cook_cycle_run_queue_hosts_multi", "cook_cycle_churn_info", "cook_cycle_fetch_offers"):
        assert name in PROTOS
    assert len(PROTOS["cook_cycle_run_queue_hosts"][1]) == 6 and len(PROTOS["cook_cycle_run_queue_hosts_multi"][1]) == 7
    subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "gen_protos.py"), "--check"])
    join = A.Offers(cpus=[1.0, 2.0], mem=[3.0, 4.0], host=[8, 9])
    st, keep = A.HostChurn(leave=[5, 6, 7], join=join, before=[A.NONE_U32, 5]).as_struct()
    assert st.n_leave == 3 and [st.leave_host[x] for x in range(3)] == [5, 6, 7] and st.join.contents.n == 2
    assert [st.join_before[x] for x in range(2)] == [A.NONE_U32, 5]
    st, keep = A.HostChurn().as_struct()
    assert st.n_leave == 0 and not st.leave_host and not st.join and not st.join_before
    rows = A.OfferRows(4, n_attr_keys=2, skip=("mem",))
    assert rows.struct.cap == 4 and not rows.struct.mem and rows.struct.cpus and len(rows.arrays["attr"]) == 8
    assert len(rows.arrays["gpu_count"]) == 4 * A.MAX_RES_SLOTS and len(rows.arrays["scalars"]) == 4 * A.MAX_SCALARS
    assert C.sizeof(A.ChurnInfo) == 16 and rows.arrays["host_start_s"].dtype == np.int64
