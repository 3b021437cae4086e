"""Writes tests/golden/user_stats.json: every set-stats-counters! step of the reference's test-set-stats-counters!
(scheduler/test/cook/test/monitor.clj:41-309) as one case — the jobs of the database at that point (user, cpus, mem, state,
pool), the shares and quotas the step's with-redefs put in place (absent: the defaults — share Double/MAX_VALUE, quota count
Integer/MAX_VALUE, the other quotas Double/MAX_VALUE, launch-rate quotas positive), the pools the step counts over (a quota-group
name such as "accum" counts the jobs of every member pool, :quota-grouping {"pool1" "accum" "pool2" "accum"}, monitor.clj:35-38),
and the counter values the reference asserts ([jobs cpus mem] per state and user, after set-counter!'s long cast; a user the
step does not assert is left out).  `python tests/golden/make_user_stats_golden.py` rewrites the file."""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LONG_MAX = 2 ** 63 - 1

JOB = {  # monitor.clj:52-54, 252-254, 273-275
    "job1": dict(user="alice", cpus=1.0, mem=128.0), "job2": dict(user="bob", cpus=2.0, mem=256.0),
    "job3": dict(user="sally", cpus=4.0, mem=float(LONG_MAX)),  # (double Long/MAX_VALUE) = 2^63
    "job4": dict(user="user", cpus=2.0, mem=3.0), "job5": dict(user="user", cpus=5.0, mem=8.0), "job6": dict(user="user", cpus=13.0, mem=21.0),
    "job7": dict(user="user", cpus=2.0, mem=30.0), "job8": dict(user="user", cpus=5.0, mem=80.0), "job9": dict(user="user", cpus=13.0, mem=210.0),
}
POOL = {"job7": "pool1", "job8": "pool1", "job9": "pool2"}
GROUP = {"pool1": ["pool1"], "pool2": ["pool2"], "accum": ["pool1", "pool2"]}
Z = [0, 0, 0]


def jobs(**state):
    return [dict(name=k, **JOB[k], state=v, pool=POOL.get(k, "pool1")) for k, v in state.items()]


def case(ref, pool, js, expect, counts=None, shares=None, quota=None):
    return dict(ref="scheduler/test/cook/test/monitor.clj:" + ref, pool=pool, member_pools=GROUP[pool], jobs=js, shares=shares, quota=quota,
                expect=expect, counts=counts or {})


def counts(total=None, starved=None, wuq=None, hungry=None, satisfied=None):
    c = {"total": total, "starved": starved, "waiting-under-quota": wuq, "hungry": hungry, "satisfied": satisfied}
    return {k: v for k, v in c.items() if v is not None}


def states(running=None, waiting=None, starved=None, wuq=None):
    e = {"running": running, "waiting": waiting, "starved": starved, "waiting-under-quota": wuq}
    return {k: v for k, v in e.items() if v is not None}


SHARE0 = {"cpus": 0, "mem": 0}  # monitor.clj:198 share/get-share (constantly {:cpus 0 :mem 0})
QUOTA_S8 = {"mem": 10, "cpus": 10, "gpus": 10, "count": 10, "launch-rate-saved": 1.0000097e7, "launch-rate-per-minute": 600013.0}  # :199
QUOTA_S10 = {"mem": 10, "cpus": 100, "gpus": 10, "count": 10, "launch-rate-saved": 10, "launch-rate-per-minute": 10}  # :258

AB_W = {"all": [2, 3, 384], "alice": [1, 1, 128], "bob": [1, 2, 256]}
BOB = {"all": [1, 2, 256], "alice": Z, "bob": [1, 2, 256]}
ZERO3 = {"all": Z, "alice": Z, "bob": Z}
CASES = [
    case("65-76", "pool1", [], states(running={"all": Z}, waiting={"all": Z}, starved={"all": Z}, wuq={"all": Z}), counts(0, 0, 0, 0, 0)),
    case("78-98", "pool1", jobs(job1="waiting", job2="waiting"),
         states(running={"all": Z}, waiting=AB_W, starved=AB_W, wuq=AB_W), counts(2, 2, 2, 0, 0)),
    case("100-111", "accum", jobs(job1="waiting", job2="waiting"), states(running={"all": Z}, waiting=AB_W, starved=AB_W, wuq=AB_W)),
    case("113-132", "pool1", jobs(job1="running", job2="waiting"),
         states(running={"all": [1, 1, 128], "alice": [1, 1, 128], "bob": Z}, waiting=BOB, starved=BOB, wuq=BOB), counts(2, 1, 1, 0, 1)),
    case("134-152", "pool1", jobs(job2="waiting"), states(running=ZERO3, waiting=BOB, starved=BOB, wuq=BOB), counts(1, 1, None, 0, 0)),
    case("154-173", "pool1", jobs(job2="running"),
         states(running={"all": [1, 2, 256], "alice": Z, "bob": [1, 2, 256]}, waiting=ZERO3, starved=ZERO3, wuq=ZERO3), counts(1, 0, None, 0, 1)),
    case("175-194", "pool1", [], states(running=ZERO3, waiting=ZERO3, starved=ZERO3, wuq=ZERO3), counts(0, 0, None, 0, 0)),
    case("196-223", "pool1", jobs(job3="waiting"),
         states(running={"all": Z, "alice": Z, "bob": Z, "sally": Z},
                waiting={"all": [1, 4, LONG_MAX], "alice": Z, "bob": Z, "sally": [1, 4, LONG_MAX]},
                starved={"all": Z, "alice": Z, "bob": Z, "sally": Z},
                wuq={"all": [1, 4, 10], "alice": Z, "bob": Z, "sally": [1, 4, 10]}), counts(1, 0, 1, 1, 0), shares=SHARE0, quota=QUOTA_S8),
    case("225-248", "pool1", jobs(job3="running"),  # (outside the with-redefs: default shares and quotas again)
         states(running={"all": [1, 4, LONG_MAX], "alice": Z, "bob": Z, "sally": [1, 4, LONG_MAX]},
                waiting={"all": Z, "alice": Z, "bob": Z, "sally": Z}, starved={"all": Z, "alice": Z, "bob": Z, "sally": Z},
                wuq={"all": Z, "alice": Z, "bob": Z, "sally": Z}), counts(1, 0, None, 0, 1)),
    case("257-260", "pool1", jobs(job4="waiting", job5="waiting", job6="waiting"), states(wuq={"user": [3, 20, 10]}), quota=QUOTA_S10),
    case("262-264", "pool1", jobs(job4="running", job5="waiting", job6="waiting"), states(wuq={"user": [2, 18, 7]}), quota=QUOTA_S10),
    case("266-268", "pool1", jobs(job4="running", job5="running", job6="waiting"), states(wuq={"user": Z}), quota=QUOTA_S10),
]
S13 = jobs(job7="waiting", job8="waiting", job9="waiting")
S14 = jobs(job7="running", job8="waiting", job9="running")
CASES += [
    case("276-287", "pool1", S13, states(waiting={"user": [2, 7, 110], "all": [2, 7, 110]})),
    case("276-287", "pool2", S13, states(waiting={"user": [1, 13, 210], "all": [1, 13, 210]})),
    case("276-287", "accum", S13, states(waiting={"user": [3, 20, 320], "all": [3, 20, 320]})),
    case("289-306", "pool1", S14, states(running={"user": [1, 2, 30], "all": [1, 2, 30]}, waiting={"user": [1, 5, 80], "all": [1, 5, 80]})),
    case("289-306", "pool2", S14, states(running={"user": [1, 13, 210], "all": [1, 13, 210]}, waiting={"user": Z, "all": Z})),
    case("289-306", "accum", S14, states(running={"user": [2, 15, 240], "all": [2, 15, 240]}, waiting={"user": [1, 5, 80], "all": [1, 5, 80]})),
]

if __name__ == "__main__":
    out = os.path.join(HERE, "user_stats.json")
    with open(out, "w") as f:
        json.dump(CASES, f, indent=1)
        f.write("\n")
    print(out, len(CASES), "cases")
