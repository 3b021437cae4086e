"""Writes tests/golden/sweep.json: the three task killers of the reference over small running sets.  The first cases transcribe the
reference's own tests (paths under scheduler/): test-get-lingering-tasks (all three asserts), test-kill-lingering-tasks,
test-find-stragglers (its four testing blocks, one case each and one with all four groups in one table), test-handle-stragglers and
test-cancelled-task-killer.  #inst values and (t/plus now (t/months 1)) / (t/years 1) are UTC milliseconds; a (t/ago ...) offset is
fixed against one `now`.  create-dummy-instance defaults to :instance.status/unknown and create-dummy-job to :max-runtime
Long/MAX_VALUE (src/cook/test/testutil.clj:237-266, 319-335).  The hand-derived cases follow, each with its derivation beside it.

Fields: now_ms, default_timeout_ms, max_timeout_ms, what (bit 0 lingering, 1 stragglers, 2 cancelled), cap (null: 3n); rows: start_ms
(null = absent), unknown, max_runtime_ms (null = absent), cancelled, group (null = none); groups (null or type, quantile, multiplier,
job_count, succ = [[start, end or null], ...] per group); expect: rc, and on rc 0 the three lists, threshold_s (null = NaN) and
groups_ready, on rc -1 bad_row (null = COOK_NONE_U32) and, where the error is cap, the list lengths.
`python tests/golden/make_sweep_golden.py` rewrites the file."""
import json
import os
from datetime import datetime, timezone

HERE = os.path.dirname(os.path.abspath(__file__))
T_SCHED = "test/cook/test/scheduler/scheduler.clj"
T_GROUP = "test/cook/test/group.clj"
LONG_MAX = 2 ** 63 - 1
H, M, S = 3_600_000, 60_000, 1000


def utc(*a):
    return int(datetime(*a, tzinfo=timezone.utc).timestamp() * 1000)


def row(start, unknown=0, max_runtime=None, cancelled=0, group=None):
    return dict(start_ms=start, unknown=unknown, max_runtime_ms=max_runtime, cancelled=cancelled, group=group)


def grp(typ, q=0.5, m=2.0, jobs=0, succ=()):
    return dict(type=typ, quantile=q, multiplier=m, job_count=jobs, succ=[list(x) for x in succ])


def case(name, ref, now, rows, *, groups=None, default=0, maximum=0, what=7, cap=None, expect):
    return dict(name=name, ref=ref, now_ms=now, default_timeout_ms=default, max_timeout_ms=maximum, what=what, cap=cap, rows=rows,
                groups=groups, expect=expect)


def ok(lingering=(), stragglers=(), cancelled=(), thr=(), ready=0):
    return dict(rc=0, lingering=list(lingering), stragglers=list(stragglers), cancelled=list(cancelled), threshold_s=list(thr),
                groups_ready=ready)


def err(bad_row=None, **counts):
    return dict(rc=-1, bad_row=bad_row, **counts)


CASES = []

# ---- test-get-lingering-tasks (T_SCHED:730-779): five unknown instances, now = #inst "2015-01-05T00:00:30" ----------------------------
NOW_L = utc(2015, 1, 5, 0, 0, 30)
LING_ROWS = [row(utc(2015, 1, 1), max_runtime=LONG_MAX),       # 1: min(MAX, 120 h) -> 2015-01-06
             row(utc(2015, 1, 4), max_runtime=60_000),         # 2: 2015-01-04T00:01
             row(utc(2015, 1, 5), max_runtime=30_000),         # 3: exactly now: time/after? is false
             row(utc(2015, 1, 5), max_runtime=10_000),         # 4: 2015-01-05T00:00:10
             row(utc(2015, 1, 1), max_runtime=64 * 24 * H)]    # 5: 64 days > Integer/MAX_VALUE ms; min(64 d, 120 h) -> 2015-01-06
CASES += [
    # (is (= #{task-id-2 task-id-4} (get-lingering-tasks test-db now 120 120)))
    case("get-lingering-tasks now", f"{T_SCHED}:730-777", NOW_L, LING_ROWS, default=120 * H, maximum=120 * H, what=1, expect=ok([1, 3])),
    # (is (not (contains? (get-lingering-tasks test-db next-month 1e4 1e4) task-id-5))): 5 ends 2015-03-06; 1 ends 2016-02-21
    case("get-lingering-tasks next month", f"{T_SCHED}:778", utc(2015, 2, 5, 0, 0, 30), LING_ROWS, default=10_000 * H,
         maximum=10_000 * H, what=1, expect=ok([1, 2, 3])),
    # (is (contains? (get-lingering-tasks test-db next-year 1e5 1e5) task-id-5)): 1 runs to 2026 (1e5 h)
    case("get-lingering-tasks next year", f"{T_SCHED}:779", utc(2016, 1, 5, 0, 0, 30), LING_ROWS, default=100_000 * H,
         maximum=100_000 * H, what=1, expect=ok([1, 2, 3, 4])),
]

# ---- test-kill-lingering-tasks (T_SCHED:781-856): :timeout-hours 4, instances started 5 h (unknown), 5 h and 3 h ago -----------------
NOW_K = utc(2026, 1, 1)
CASES.append(case("kill-lingering-tasks", f"{T_SCHED}:781-856", NOW_K,
                  [row(NOW_K - 5 * H, unknown=1, max_runtime=LONG_MAX), row(NOW_K - 5 * H, max_runtime=LONG_MAX),
                   row(NOW_K - 3 * H, max_runtime=LONG_MAX)], default=4 * H, maximum=4 * H, what=1, expect=ok([0, 1])))

# ---- test-find-stragglers (T_GROUP:12-120) and test-handle-stragglers (T_SCHED:1514-1543) ---------------------------------------------
NOW = utc(2026, 3, 1, 12)
ONE_H = (NOW - 3 * H, NOW - 2 * H)  # a success of 3600 s
QD = dict(q=0.5, m=2.0)
FS = [
    # "no straggler-handling": find-stragglers :none returns nil
    (grp(0, jobs=2, succ=[ONE_H]), [NOW - 30 * M], [], None, 0),
    # "no stragglers": idx = (int (* 1 0.5)) = 0, 1 success > 0, target 3600 s, threshold 7200; 90 min = 5400 s is not above
    (grp(1, jobs=2, succ=[ONE_H], **QD), [NOW - 90 * M], [], 7200.0, 1),
    # "stragglers found": 9 jobs, idx = (int (* 8 0.5)) = 4, 6 successes; 100 min = 6000 s no, 190 min = 11400 s and 121 min = 7260 s yes
    (grp(1, jobs=9, succ=[ONE_H] * 6, **QD), [NOW - 100 * M, NOW - 190 * M, NOW - 121 * M], [1, 2], 7200.0, 1),
    # "not enough jobs complete": 3 jobs (job-c has no instance), idx = (int (* 2 0.5)) = 1, one success (job-b's): not ready
    (grp(1, jobs=3, succ=[ONE_H], **QD), [NOW - 3 * H, NOW - 190 * M], [], None, 0),
]
FS_NAMES = ["no straggler-handling", "quantile deviation straggler-handling, no stragglers",
            "quantile deviation straggler-handling, stragglers found", "quantile deviation straggler-handling, not enough jobs complete"]
FS_LINES = ["12-25", "26-40", "41-95", "96-120"]
for (g, starts, strag, thr, ready), nm, ln in zip(FS, FS_NAMES, FS_LINES):
    CASES.append(case(f"find-stragglers: {nm}", f"{T_GROUP}:{ln}", NOW, [row(s, group=0) for s in starts], groups=[g], what=2,
                      expect=ok(stragglers=strag, thr=[thr], ready=ready)))
rows = [row(s, group=k) for k, f in enumerate(FS) for s in f[1]]
# (the third group's rows are rows 2, 3, 4 of this table; its stragglers, the second and third, are rows 3 and 4)
CASES.append(case("find-stragglers: the four groups in one table", f"{T_GROUP}:12-120", NOW, rows, groups=[f[0] for f in FS], what=2,
                  expect=ok(stragglers=[3, 4], thr=[f[3] for f in FS], ready=2)))
# handle-stragglers: a :none group (job-a success, job-b running 30 min) and a quantile-deviation one (job-c success, job-d running 190
# min): idx 0, threshold 7200, job-d's 11400 s is above -> only the straggler is killed
CASES.append(case("handle-stragglers", f"{T_SCHED}:1514-1543", NOW, [row(NOW - 30 * M, group=0), row(NOW - 190 * M, group=1)],
                  groups=[grp(0, jobs=2, succ=[ONE_H]), grp(1, jobs=2, succ=[ONE_H], **QD)], what=2,
                  expect=ok(stragglers=[1], thr=[None, 7200.0], ready=1)))

# ---- test-cancelled-task-killer (T_SCHED:1202-1219): a running cancelled instance, a running one; the cancelled success is not running --
CASES.append(case("cancelled-task-killer", f"{T_SCHED}:1202-1219", NOW, [row(NOW, cancelled=1), row(NOW)], what=4, expect=ok(cancelled=[0])))

# ---- hand-derived ------------------------------------------------------------------------------------------------------------------------
HD = "hand-derived"
NOW_E = 1_700_000_000_000
CASES += [
    # default 1000 ms, max 10^6 ms: on the boundary no, 1 ms past it yes; Long/MAX_VALUE capped at 10^6: 10^6 + 1 ms yes, 10^6 no; no start
    # time: never; max-runtime 0: now itself no, 1 ms yes; a start in the future: no
    case("lingering boundaries", HD, NOW_E,
         [row(NOW_E - 1000), row(NOW_E - 1001), row(NOW_E - 1_000_001, max_runtime=LONG_MAX), row(NOW_E - 1_000_000, max_runtime=LONG_MAX),
          row(None), row(NOW_E, max_runtime=0), row(NOW_E - 1, max_runtime=0), row(NOW_E + 5000), row(-(2 ** 62), max_runtime=LONG_MAX)],
         default=1000, maximum=1_000_000, what=1, expect=ok([1, 2, 6, 8])),
    # max_timeout below the default: min(default, max) even for a row without max-runtime
    case("lingering: the maximum caps the default", HD, NOW_E, [row(NOW_E - 600), row(NOW_E - 400)], default=10_000, maximum=500, what=1,
         expect=ok([0])),
    # an unknown row lingers and is cancelled but is never a straggler (group threshold 2 * 10 = 20 s); the running twin is all three
    case("unknown row", HD, NOW_E, [row(NOW_E - 100 * S, unknown=1, cancelled=1, group=0), row(NOW_E - 100 * S, cancelled=1, group=0),
                                    row(None, unknown=1, group=0)],
         groups=[grp(1, jobs=2, succ=[(NOW_E - 50 * S, NOW_E - 40 * S)], **QD)], default=60 * S, maximum=60 * S,
         expect=ok([0, 1], [1], [0, 1], [20.0], 1)),
    # s truncates: a success of 3600.999 s is 3600 (threshold 7200); running 7200.999 s is 7200 (not above), 7201 s is
    case("truncated seconds", HD, NOW_E, [row(NOW_E - 7_200_999, group=0), row(NOW_E - 7_201_000, group=0)],
         groups=[grp(1, jobs=2, succ=[(NOW_E - 10 * H, NOW_E - 10 * H + 3_600_999)], **QD)], what=2, expect=ok(stragglers=[1], thr=[7200.0], ready=1)),
    # 3 s * 2.5 = 7.5: 7 s no, 8 s yes
    case("non-dyadic multiplier", HD, NOW_E, [row(NOW_E - 7 * S, group=0), row(NOW_E - 8 * S, group=0)],
         groups=[grp(1, q=0.5, m=2.5, jobs=2, succ=[(NOW_E - 100 * S, NOW_E - 97 * S)])], what=2, expect=ok(stragglers=[1], thr=[7.5], ready=1)),
    # 4 jobs, q 0.5: idx = trunc(1.5) = 1, the second smallest of {30, 10, 20} s = 20 -> 40; 40 s no, 41 s yes
    case("idx truncation", HD, NOW_E, [row(NOW_E - 40 * S, group=0), row(NOW_E - 41 * S, group=0)],
         groups=[grp(1, jobs=4, succ=[(NOW_E - 90 * S, NOW_E - 60 * S), (NOW_E - 90 * S, NOW_E - 80 * S), (NOW_E - 90 * S, NOW_E - 70 * S)], **QD)],
         what=2, expect=ok(stragglers=[1], thr=[40.0], ready=1)),
    # jobs without instances count: 10 jobs need idx 4 < 4 successes: not ready; 9 jobs with 5: ready (target 5th smallest of 1..5 s = 5 -> 10)
    case("jobs without instances", HD, NOW_E, [row(NOW_E - 1000 * S, group=0), row(NOW_E - 11 * S, group=1), row(NOW_E - 10 * S, group=1)],
         groups=[grp(1, jobs=10, succ=[(NOW_E - 9 * S, NOW_E - 8 * S)] * 4, **QD),
                 grp(1, jobs=9, succ=[(NOW_E - 9 * S, NOW_E - (9 - k) * S) for k in range(5, 0, -1)], **QD)],
         what=2, expect=ok(stragglers=[1], thr=[None, 10.0], ready=1)),
    # a retried job with several successful instances: 2 jobs, 3 successes (s = 6, 4, 5), idx 0 -> 4 * 2 = 8; an instance without end-time
    # runs to now (a success of 100 s would be the 4th)
    case("retried jobs", HD, NOW_E, [row(NOW_E - 8 * S, group=0), row(NOW_E - 9 * S, group=0)],
         groups=[grp(1, jobs=2, succ=[(NOW_E - 60 * S, NOW_E - 54 * S), (NOW_E - 60 * S, NOW_E - 56 * S), (NOW_E - 60 * S, NOW_E - 55 * S),
                                      (NOW_E - 100 * S, None)], **QD)], what=2, expect=ok(stragglers=[1], thr=[8.0], ready=1)),
    # a group of 0 jobs: idx = trunc(-q) = 0, so one success makes it ready
    case("zero jobs", HD, NOW_E, [row(NOW_E - 21 * S, group=0)], groups=[grp(1, q=0.9, m=2.0, jobs=0, succ=[(NOW_E - 20 * S, NOW_E - 10 * S)])],
         what=2, expect=ok(stragglers=[0], thr=[20.0], ready=1)),
    # intervals the reference never evaluates do not fail: a not-ready group's bad success, a :none group's, an unknown row of a ready group
    case("unevaluated intervals", HD, NOW_E, [row(None, unknown=1, group=0), row(None, group=1), row(NOW_E + 1, group=2)],
         groups=[grp(1, jobs=2, succ=[(NOW_E - 5 * S, NOW_E - 4 * S)], **QD), grp(1, jobs=5, succ=[(NOW_E, NOW_E - 1)], **QD),
                 grp(0, jobs=1, succ=[(None, NOW_E)])], what=2, expect=ok(thr=[2.0, None, None], ready=1)),
    # every killer alone and together over one table
    *[case(f"what = {w}", HD, NOW_E, [row(NOW_E - 100 * S, cancelled=1, group=0), row(NOW_E - 5 * S), row(NOW_E - 30 * S, group=0, cancelled=1),
                                      row(NOW_E - 61 * S, unknown=1)],
           groups=[grp(1, jobs=2, succ=[(NOW_E - 20 * S, NOW_E - 10 * S)], **QD)], default=60 * S, maximum=60 * S, what=w,
           expect=ok([0, 3] if w & 1 else [], [0, 2] if w & 2 else [], [0, 2] if w & 4 else [], [20.0 if w & 2 else None],
                     1 if w & 2 else 0)) for w in (1, 2, 4, 7)],
    case("n = 0", HD, NOW_E, [], groups=[grp(1, jobs=2, succ=[(NOW_E - 20 * S, NOW_E - 10 * S)], **QD), grp(0)],
         expect=ok(thr=[20.0, None], ready=1)),
    case("n = 0, no groups", HD, NOW_E, [], what=5, expect=ok()),
    # ---- errors (COOK_E_INVALID) ----
    case("running row without start time in a ready group", HD, NOW_E, [row(NOW_E, group=0), row(None, group=0), row(None, group=0)],
         groups=[grp(1, jobs=2, succ=[(NOW_E - 2 * S, NOW_E - S)], **QD)], what=2, expect=err(1)),
    case("running row started after now in a ready group", HD, NOW_E, [row(NOW_E - S, group=0), row(NOW_E + 1, group=0)],
         groups=[grp(1, jobs=2, succ=[(NOW_E - 2 * S, NOW_E - S)], **QD)], what=2, expect=err(1)),
    case("running row above INT32_MAX s in a ready group", HD, NOW_E, [row(NOW_E - (2 ** 31) * S, group=0), row(NOW_E - (2 ** 31 - 1) * S, group=0)],
         groups=[grp(1, jobs=2, succ=[(NOW_E - 2 * S, NOW_E - S)], **QD)], what=2, expect=err(0)),
    case("successful instance ending before its start", HD, NOW_E, [row(NOW_E - S, group=1), row(NOW_E - S)],
         groups=[grp(1, jobs=2, succ=[(NOW_E - 2 * S, NOW_E - S)], **QD), grp(1, jobs=2, succ=[(NOW_E - 2 * S, NOW_E - S), (NOW_E - S, NOW_E - 2 * S)], **QD)],
         what=2, expect=err(2 + 2)),
    case("successful instance without start time", HD, NOW_E, [row(NOW_E - S, group=0)],
         groups=[grp(1, jobs=3, succ=[(NOW_E - 2 * S, NOW_E - S), (NOW_E - 3 * S, None), (None, NOW_E)], **QD)], what=2, expect=err(1 + 2)),
    case("successful instance above INT32_MAX s", HD, NOW_E, [],
         groups=[grp(1, jobs=2, succ=[(NOW_E - (2 ** 31) * S, NOW_E)], **QD)], what=2, expect=err(0)),
    case("a bad running row comes before a bad success", HD, NOW_E, [row(NOW_E - S, group=0), row(NOW_E + S, group=0)],
         groups=[grp(1, jobs=2, succ=[(NOW_E - 2 * S, NOW_E - S), (NOW_E, NOW_E - 1)], **QD)], what=2, expect=err(1)),
    case("job_count above INT32_MAX", HD, NOW_E, [], groups=[grp(1, jobs=2 ** 31, succ=[(NOW_E - 2 * S, NOW_E - S)], **QD)], what=2, expect=err()),
    *[case(f"quantile {q}", HD, NOW_E, [], groups=[grp(1, q=q, m=2.0, jobs=1)], what=2, expect=err()) for q in (0.0, 1.0, float("nan"))],
    *[case(f"multiplier {m}", HD, NOW_E, [], groups=[grp(1, q=0.5, m=m, jobs=1)], what=2, expect=err()) for m in (1.0, float("inf"), float("nan"))],
    case("straggler-handling type 2", HD, NOW_E, [], groups=[grp(2)], what=2, expect=err()),
    case("group index out of range", HD, NOW_E, [row(NOW_E), row(NOW_E, group=1)], groups=[grp(0)], what=2, expect=err(1)),
    case("the timeouts must not be negative", HD, NOW_E, [row(NOW_E)], default=-1, maximum=5, what=1, expect=err()),
    # the lists total 4 > cap 3: the lengths come back all the same
    case("cap too small", HD, NOW_E, [row(NOW_E - 100 * S, cancelled=1), row(NOW_E - 100 * S, cancelled=1)], default=S, maximum=S, what=5, cap=3,
         expect=err(None, lingering=2, stragglers=0, cancelled=2)),
]


def main():
    with open(os.path.join(HERE, "sweep.json"), "w") as f:
        json.dump({"cases": CASES}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
