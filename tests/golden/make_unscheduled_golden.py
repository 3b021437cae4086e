"""Writes tests/golden/unscheduled.json: the quota, share and queue-position reasons of cook.unscheduled/reasons over small task
tables.  The first cases transcribe the reference's own tests (scheduler/test/cook/test/unscheduled.clj):
test-how-job-would-exceed-resource-limits (:34-55, its three testing blocks), test-reasons (:72-168) and test-check-queue-position
(:170-199).  The hand-derived cases follow, each with its derivation beside it.  Data only.

Fields: users (names; ids = positions); tasks in CREATION order (row = position; the loader gives job ids, and running rows start
times and task ids, in that order, so "first" means what the reference's tests mean): user, state ("running" / "waiting"), cpus, mem,
gpus (optional), priority (optional, 50); no_gpus (the table has no gpus column); quota / share: {user: {key: limit}} (a key left out
is unset: DBL_MAX, count 2^31 - 1); window: null or the rows of the waiting jobs the host's "first 100 waiting jobs" query returns;
rows: null (all) or the list of rows asked for.  expect: rows = [{at (output index), bits (the exact set), queue_pos, total (null: not
checked; else [count, cpus, mem, gpus]), ahead (the task rows ahead: the first min(queue_pos, 10) of the user's list; null: not
checked)}], list_len {user: n}, ahead {user: the user's whole ahead row, null = COOK_NONE_U32}.
`python tests/golden/make_unscheduled_golden.py` rewrites the file."""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
T = "test/cook/test/unscheduled.clj"
HD = "hand-derived"


def run(user, cpus, mem, **kw):
    return dict(user=user, state="running", cpus=cpus, mem=mem, **kw)


def wait(user, cpus, mem, **kw):
    return dict(user=user, state="waiting", cpus=cpus, mem=mem, **kw)


def at(i, bits, queue_pos, total=None, ahead=None):
    return dict(at=i, bits=sorted(bits), queue_pos=queue_pos, total=total, ahead=ahead)


def case(name, ref, users, tasks, *, quota=None, share=None, window=None, rows=None, no_gpus=False, expect):
    return dict(name=name, ref=ref, users=users, tasks=tasks, quota=quota or {}, share=share or {}, window=window, rows=rows, no_gpus=no_gpus,
                expect=expect)


QP = "queue-position"
# test-how-job-would-exceed-resource-limits: quota {:mem 6000 :cpus 8 :count 5}, running {3000, 4} and {2000, 2} (:35-37); the function
# sees no queue, the queue position of the third row (2 running rows ahead) is the table's
LIMITS = {"u": {"mem": 6000, "cpus": 8, "count": 5}}
RUNNING = [run("u", 4, 3000), run("u", 2, 2000)]
# test-check-queue-position: 500 waiting jobs are created first, then 50 running ones (:172-186); the window is (take 100 waiting-jobs)
QP_TASKS = [wait("mforsythq", 1.0, 3.0) for _ in range(500)] + [run("mforsythq", 1.0, 3.0) for _ in range(50)]

CASES = [
    case("exceeding both mem and cpu", T + ":39-43", ["u"], RUNNING + [wait("u", 4, 4000)], quota=LIMITS, no_gpus=True,
         expect=dict(rows=[at(2, ["quota-mem", "quota-cpus", QP], 2, [3, 10, 9000, 0])])),
    case("exceeding just 1 resource", T + ":45-49", ["u"], RUNNING + [wait("u", 1, 2000)], quota=LIMITS, no_gpus=True,
         expect=dict(rows=[at(2, ["quota-mem", QP], 2, [3, 7, 7000, 0])])),
    case("exceeding cpus and count", T + ":51-55", ["u"], RUNNING + [wait("u", 4, 500)], quota={"u": {"mem": 6000, "cpus": 8, "count": 2}},
         no_gpus=True, expect=dict(rows=[at(2, ["quota-cpus", "quota-count", QP], 2, [3, 10, 5500, 0])])),
    # test-reasons: count quota 2 (:75), running {1.0, 3.0} and {1.0, 3.1}, waiting {1.0, 3.0} (:76-88); the uncommitted job (:82-84) is
    # no result of the queries; expected (:156-161) {:count {:limit 2 :usage 3}} and "You have 2 other jobs ahead" with both running jobs
    case("test-reasons", T + ":72-168", ["mforsythr"], [run("mforsythr", 1.0, 3.0), run("mforsythr", 1.0, 3.1), wait("mforsythr", 1.0, 3.0)],
         quota={"mforsythr": {"count": 2}},
         expect=dict(rows=[at(2, ["quota-count", QP], 2, [3, 1.0 + 1.0 + 1.0, 3.0 + 3.1 + 3.0, 0], [0, 1]), at(0, [], 0, [0, 0, 0, 0], []), at(1, [QP], 1, [0, 0, 0, 0], [0])],
                     list_len={"mforsythr": 3})),
    # :188-199 — the second running job: 1 ahead, [first running]; the first waiting job: 50 ahead, the first of them the first running
    # job; the last waiting job is outside the window: "at least 150", the first ahead the first running job
    case("test-check-queue-position", T + ":170-199", ["mforsythq"], QP_TASKS, window=list(range(100)),
         expect=dict(rows=[at(501, [QP], 1, None, [500]), at(0, [QP], 50, None, list(range(500, 510))),
                           at(499, [QP, "at-least"], 150, None, list(range(500, 510))), at(99, [QP], 149, None, list(range(500, 510))),
                           at(100, [QP, "at-least"], 150, None, list(range(500, 510)))],
                     list_len={"mforsythq": 150}, ahead={"mforsythq": list(range(500, 510))})),
    # ---- hand-derived ----
    # a user without running rows: its first waiting job has nobody ahead and usage = the job alone; "b" has no row at all
    case("no running rows", HD, ["a", "b"], [wait("a", 2, 100), wait("a", 3, 200)], quota={"a": {"cpus": 2.5, "mem": 1000}},
         expect=dict(rows=[at(0, [], 0, [1, 2, 100, 0], []), at(1, ["quota-cpus", QP], 1, [1, 3, 200, 0], [0])], list_len={"a": 2, "b": 0},
                     ahead={"a": [0, 1] + [None] * 8, "b": [None] * 10})),
    # total == limit exactly is not over it (strict >, unscheduled.clj:48): 4 + 2 + 2 = 8 cpus, 3 rows, 6000 mem; one more cpu is
    case("total equals the limit", HD, ["u"], RUNNING + [wait("u", 2, 1000), wait("u", 3, 1000)],
         quota={"u": {"cpus": 8, "count": 3, "mem": 6000}}, share={"u": {"cpus": 8, "mem": 6000}},
         expect=dict(rows=[at(2, [QP], 2, [3, 8, 6000, 0]), at(3, ["quota-cpus", "share-cpus", QP], 3, [3, 9, 6000, 0])])),
    # unset limits (DBL_MAX, count 2^31 - 1): nothing is exceeded
    case("unset limits", HD, ["u"], [run("u", 1e300, 1e300), wait("u", 1e300, 1e300)],
         expect=dict(rows=[at(1, [QP], 1, [2, 2e300, 2e300, 0], [0])])),
    # no gpus column: gpus usage 0.0 is not above a gpus quota of 0
    case("gpus column NULL", HD, ["u"], [run("u", 1, 1), wait("u", 1, 1)], quota={"u": {"gpus": 0}}, share={"u": {"gpus": 0}}, no_gpus=True,
         expect=dict(rows=[at(1, [QP], 1, [2, 2, 2, 0])])),
    # with the column: 1 + 1 gpus against quota 1 and share 1.5; the second user's job stays below its own limits
    case("gpus", HD, ["u", "v"], [run("u", 1, 1, gpus=1), wait("u", 1, 1, gpus=1), run("v", 1, 1, gpus=4), wait("v", 1, 1, gpus=0)],
         quota={"u": {"gpus": 1}, "v": {"gpus": 4}}, share={"u": {"gpus": 1.5}, "v": {"gpus": 4}},
         expect=dict(rows=[at(1, ["quota-gpus", "share-gpus", QP], 1, [2, 2, 2, 2]), at(3, [QP], 1, [2, 2, 2, 4], [2])])),
    # a waiting job of priority 90 stands in front of the running jobs of priority 50 (tools.clj:614-632: -priority comes first)
    case("a higher-priority pending row ahead of running rows", HD, ["u"], [run("u", 1, 1), run("u", 1, 1), wait("u", 1, 1, priority=90), wait("u", 1, 1)],
         expect=dict(rows=[at(2, [], 0, [3, 3, 3, 0], []), at(0, [QP], 1, None, [2]), at(1, [QP], 2, None, [2, 0]), at(3, [QP], 3, [3, 3, 3, 0], [2, 0, 1])],
                     list_len={"u": 4}, ahead={"u": [2, 0, 1, 3] + [None] * 6})),
    # the same with the priority-90 job outside the window: it is not in the list, it sees the whole list ahead
    case("a pending row outside the window", HD, ["u"], [run("u", 1, 1), run("u", 1, 1), wait("u", 1, 1, priority=90), wait("u", 1, 1)], window=[3],
         expect=dict(rows=[at(2, [QP, "at-least"], 3, [3, 3, 3, 0], [0, 1, 3]), at(0, [], 0, None, [])], list_len={"u": 3},
                     ahead={"u": [0, 1, 3] + [None] * 7})),
    # an empty window and no running rows: the list is empty; "at least 0" is no reason (no queue-position bit)
    case("an empty list", HD, ["u"], [wait("u", 1, 1)], window=[], expect=dict(rows=[at(0, ["at-least"], 0, [1, 1, 1, 0], [])], list_len={"u": 0})),
    case("an empty table", HD, ["a", "b"], [], expect=dict(rows=[], list_len={"a": 0, "b": 0}, ahead={"a": [None] * 10, "b": [None] * 10})),
    # rows: repeats, a running row, any order — answers by output index
    case("a list of rows", HD, ["u", "v"], RUNNING + [wait("u", 4, 4000), wait("v", 1, 1)], quota=LIMITS, rows=[2, 0, 2, 3, 1],
         expect=dict(rows=[at(0, ["quota-mem", "quota-cpus", QP], 2, [3, 10, 9000, 0], [0, 1]), at(1, [], 0, [0, 0, 0, 0], []),
                           at(2, ["quota-mem", "quota-cpus", QP], 2, [3, 10, 9000, 0], [0, 1]), at(3, [], 0, [1, 1, 1, 0], []),
                           at(4, [QP], 1, [0, 0, 0, 0], [0])], list_len={"u": 3, "v": 1})),
    case("an empty list of rows", HD, ["u"], RUNNING, rows=[], expect=dict(rows=[], list_len={"u": 2})),
]


def main():
    with open(os.path.join(HERE, "unscheduled.json"), "w") as f:
        json.dump({"cases": CASES}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
