"""Writes tests/golden/queue_cycles.json: the five cases of test-remove-matched-jobs-from-pending-jobs
(scheduler/test/cook/test/scheduler/scheduler.clj:1742-1800: empty / unknown / normal / gpu / both) as data — per pool the pending
jobs in queue order (the test's :job/uuid numbers as names), the matched job uuids handed to remove-matched-jobs-from-pending-jobs and
the atom's expected content afterwards.  tests/queue_cases.py::check_golden drives them through the engine (two pools, the matches
forced by offers that fit exactly the named jobs).  `python tests/golden/make_queue_golden.py` rewrites the file."""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = "scheduler/test/cook/test/scheduler/scheduler.clj"


def r(a, b):
    return [str(i) for i in range(a, b)]


PENDING = {"gpu": r(10, 15), "normal": r(1, 10)}


def case(name, lines, gpu, normal, exp_gpu, exp_normal):
    return dict(name=name, source=f"{SRC}:{lines}", pending=PENDING, matched=dict(gpu=gpu, normal=normal),
                expect=dict(gpu=exp_gpu, normal=exp_normal))


CASES = [
    case("empty", "1745-1753", [], [], r(10, 15), r(1, 10)),
    case("unknown", "1755-1764", r(30, 35), r(20, 25), r(10, 15), r(1, 10)),
    case("normal", "1766-1776", [], r(1, 5), r(10, 15), r(5, 10)),
    case("gpu", "1778-1788", r(10, 12), [], r(12, 15), r(1, 10)),
    case("both", "1790-1800", r(10, 12), r(5, 10), r(12, 15), r(1, 5)),
]

if __name__ == "__main__":
    path = os.path.join(HERE, "queue_cycles.json")
    with open(path, "w") as f:
        json.dump(CASES, f, indent=1)
        f.write("\n")
    print(path, len(CASES), "cases")
