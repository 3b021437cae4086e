"""cook_cycle_autoscale_multi / cook_match_metrics_multi / cook_batch_stats on a machine WITHOUT a GPU: the cook_amd/csrc sources compiled
against the SIMT emulator (tests/simt_emu), the cases of tests/followup_cases.py at small sizes, and the structure of the pool batches — how
many synchronisations, what is issued alone — which on the emulator is that of the host code."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from cook_amd import _abi as A
from cook_amd.engine import Engine
from tests import followup_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def make_engine():
    from tests.simt_emu import build_emu
    so = build_emu.build()
    return lambda params: Engine(params, lib_path=so)


def test_followups_ragged_pools(make_engine, multi_mode):
    F.check_ragged(make_engine)


def test_followups_nine_pools(make_engine):
    F.check_nine_pools(make_engine)


def test_followups_one_engine_fails(make_engine):
    F.check_one_engine_fails(make_engine)


def test_followups_whole_call_rejections(make_engine):
    F.check_rejections(make_engine)


def test_followups_leave_the_cycle_alone(make_engine):
    F.check_cycle_undisturbed(make_engine)


def test_followups_edge_shapes(make_engine):
    F.check_edges(make_engine)


def test_followups_struct_sizes(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cookmatch.h"\nint main(){printf("%zu %zu %zu %zu\\n", '
                   'sizeof(cook_metrics_req), offsetof(cook_metrics_req, n_users), offsetof(cook_metrics_req, n_gpu_models), '
                   'offsetof(cook_metrics_req, offer_gpus_by_model));return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    R = A.CookMetricsReq
    assert sizes == [C.sizeof(R), R.n_users.offset, R.n_gpu_models.offset, R.offer_gpus_by_model.offset]


# ---- the structure of the two pool batches, through cook_batch_stats ------------------------------------------------------------------
# n pools built from the SAME seed with the same calls: identical flows.  Every engine first runs the single calls (which also brings every
# buffer to its size: inside a batch a buffer that grows waits for what its flow has recorded), then the multi calls.
_STRUCTURE = r'''
import json, sys
sys.path.insert(0, %r)
import numpy as np
from cook_amd import _abi as A, synth
from cook_amd.engine import Engine, cycle_autoscale_multi, match_metrics_multi
from tests import autoscale_cases as S, followup_cases as F
from tests.simt_emu import build_emu
so = build_emu.build()
n = int(sys.argv[1])
pool = synth.make_pool(seed=500, n_pending=400, n_running=150, n_users=12, n_offers=20)
st = S.random_state(pool, 501, pool_quota=True)
rng = np.random.default_rng(502)
kw = dict(max_jobs=400, scale_factor=2.0, offer_skipped=(rng.random(pool.offers.n) < 0.3).astype(np.uint8))
with F.Pools(lambda p: Engine(p, lib_path=so), [pool] * n, A.default_params(good_enough_fitness=1.0, match_algo=2), [st] * n, 120) as P:
    kw["exclude_tasks"] = F.exclusions(P, 0, kw)
    single = [(e.cycle_autoscale(**kw), e.match_metrics(n_users=12, n_gpu_models=2)) for e in P.engines]
    zero = P.engines[0].batch_stats() if n == 1 else None
    auto = cycle_autoscale_multi(P.engines, [kw] * n)
    s_auto = P.engines[0].batch_stats()
    met = match_metrics_multi(P.engines, n_users=12, n_gpu_models=2)
    s_met = P.engines[0].batch_stats()
    F.S._same([a for a, _ in single], auto)
    F.S._same([m for _, m in single], met)
    info = auto[0][1]
    assert info["autoscalable"] > info["n_out"] > 0 and met[0]["considerable"] > 0 and met[0]["offers"] > 0  # (every step of both flows runs)
    out = dict(auto=s_auto, met=s_met, info=info, res=[a[0].tolist() for a in auto], considerable=met[0]["considerable"])
print(json.dumps(out))
''' % ROOT


def _structure(n, **env):
    envx = {k: v for k, v in os.environ.items() if k not in ("COOK_SYNC_TRACE", "COOK_BATCH_TRACE", "COOK_RANK_BATCH")}
    r = subprocess.run([sys.executable, "-c", _STRUCTURE, str(n)], env={**envx, **env}, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


def test_followups_batch_structure():
    # The synchronisations of the single calls, from the code.  cook_match_metrics: the read-back of the four varying-bits masks and the
    # read-back of the results = 2.  cook_cycle_autoscale for this input: the read-back of m (autoscale_host.hpp), cons_run_device's read-back
    # of the queue length, queue_filter_quota's read-back of the new length (the state has a pool quota and the queue is not empty), and the
    # one that brings |Out| and the task indices back (an exclude list) = 4.
    AUTO_SYNCS, METRICS_SYNCS = 4, 2
    got = {}
    for n in (2, 3):
        got[n], trace = _structure(n, COOK_BATCH_TRACE="1")
        a, m = got[n]["auto"], got[n]["met"]
        assert a["pools"] == n and m["pools"] == n
        assert a["syncs"] == AUTO_SYNCS and m["syncs"] == METRICS_SYNCS, (a, m)
        # identical flows: every launch is one launch for all n pools
        assert a["grouped_launches"] == a["launches"] >= 1 and m["grouped_launches"] == m["launches"] >= 1, (a, m)
        # what is issued alone is a copy or a fill: no kernel of either path
        alone = [ln.split()[1] for ln in trace.splitlines() if ln.startswith("batch: ") and ln.endswith(" alone")]
        assert alone and set(alone) <= {"copy", "fill"}, sorted(set(alone))
        kernels = {ln.split()[1] for ln in trace.splitlines() if ln.startswith("batch: ") and " x " in ln}
        assert {"metrics_gather_jobs", "metrics_totals", "metrics_pick", "metrics_job_counts", "metrics_keys", "metrics_offer_counts",
                "as_mark_matched", "as_compact_queue", "as_candidate_tasks", "as_compact_out"} <= kernels, sorted(kernels)
        assert a["singles"] > 0 and m["singles"] > 0
    # one pool's number of launches, whatever the number of pools
    assert got[2]["auto"]["launches"] == got[3]["auto"]["launches"] and got[2]["met"]["launches"] == got[3]["met"]["launches"]
    assert got[2]["res"][0] == got[3]["res"][0] and got[2]["info"] == got[3]["info"]
    # COOK_RANK_BATCH=0 in a fresh process: the engines one after another, no batch, the same results
    off, _ = _structure(3, COOK_RANK_BATCH="0")
    assert off["auto"] == off["met"] == dict(pools=0, launches=0, grouped_launches=0, singles=0, syncs=0)
    assert off["res"] == got[3]["res"] and off["info"] == got[3]["info"] and off["considerable"] == got[3]["considerable"]
