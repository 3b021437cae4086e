"""Writes tests/golden/reservations.json: the reference's own tests of the rebalancer's host reservations as data.
"atom" cases move the atom {job-uuid->reserved-host, launched-job-uuids} alone: test-reserve-hosts (both cases),
test-reserve-hosts-integration and the three reservation cases of test-rebalance-host-reservation
(scheduler/test/cook/test/rebalancer.clj:1215-1366) — the latter as the decision lists the rebalancer returns there (host, job, number
of preempted tasks), which go through cook_amd.engine.reservations_of.  Per step: `decisions` (reserve-hosts! with them) or `launch`
(update-host-reservations! with those jobs), and the atom's expected map and launched set behind it.  A case's `launched_before` are
jobs the test puts into launched-job-uuids up front: a launch step in front does the same.  Hosts are numbered hostA = 1, hostB = 2.
"match" cases are the two reservation tests of handle-resource-offers! (scheduler/test/cook/test/scheduler/scheduler.clj:2108-2133):
the jobs of that fixture that ask for no gpus (:1860-1887; the offers have none), the one offer, the reservations, the jobs that
launch and the atom afterwards.  tests/reserve_cases.py drives all of them through the oracle and the engine.
`python tests/golden/make_reservations_golden.py` rewrites the file."""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
REB = "scheduler/test/cook/test/rebalancer.clj"
SCH = "scheduler/test/cook/test/scheduler/scheduler.clj"
A, B = 1, 2


def dec(job, host, tasks):
    return dict(job=job, host=host, tasks=tasks)


ATOM = [
    dict(name="only reserves hosts with multiple preemptions", source=f"{REB}:1321-1331", jobs=["jobA", "jobB"],
         steps=[dict(decisions=[dec("jobA", A, 2), dec("jobB", B, 1)], map={"jobA": A}, launched=[])]),
    dict(name="does not reserve hosts for jobs that have already launched", source=f"{REB}:1333-1340", jobs=["jobA"],
         steps=[dict(launch=["jobA"], map={}, launched=["jobA"]), dict(decisions=[dec("jobA", A, 2)], map={}, launched=[])]),
    dict(name="does not reserve another host after launching job", source=f"{REB}:1342-1366", jobs=["job"],
         steps=[dict(decisions=[dec("job", A, 2)], map={"job": A}, launched=[]), dict(launch=["job"], map={}, launched=["job"]),
                dict(decisions=[dec("job", B, 2)], map={}, launched=[])]),
    dict(name="reserves host for multiple preemptions", source=f"{REB}:1218-1252", jobs=["job4"],
         steps=[dict(decisions=[dec("job4", A, 2)], map={"job4": A}, launched=[])]),
    dict(name="does not reserve host for single preempted task", source=f"{REB}:1254-1282", jobs=["job2"],
         steps=[dict(decisions=[dec("job2", A, 1)], map={}, launched=[])]),
    dict(name="does not reserve host for job already launched", source=f"{REB}:1284-1317", jobs=["job4"],
         steps=[dict(launch=["job4"], map={}, launched=["job4"]), dict(decisions=[dec("job4", A, 2)], map={}, launched=[])]),
]

JOBS = ["job-1", "job-2", "job-3", "job-4"]
CPUS, MEM = [3, 13, 7, 11], [2048, 1024, 4096, 1024]
MATCH = [
    # the reservation is for a job that is not among the pool's pending jobs ((UUID/randomUUID)): nothing launches, the atom stays
    dict(name="will not launch jobs on reserved host", source=f"{SCH}:2108-2115", jobs=JOBS, job_cpus=CPUS, job_mem=MEM, host=A, host_cpus=10,
         host_mem=2048, reserve=[["(a job outside the pool)", A]], launched=[], map_after={"(a job outside the pool)": A}, released=0),
    # two jobs reserved on ONE host: both launch, afterwards the map is empty and launched holds both
    dict(name="only launches reserved jobs on reserved host", source=f"{SCH}:2117-2133", jobs=JOBS, job_cpus=CPUS, job_mem=MEM, host=A,
         host_cpus=100, host_mem=200000, reserve=[["job-1", A], ["job-2", A]], launched=["job-1", "job-2"], map_after={}, released=2),
]

if __name__ == "__main__":
    path = os.path.join(HERE, "reservations.json")
    with open(path, "w") as f:
        json.dump(dict(atom=ATOM, match=MATCH), f, indent=1)
        f.write("\n")
    print(path, len(ATOM), "+", len(MATCH), "cases")
