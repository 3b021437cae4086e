"""Writes tests/golden/usage.json: GET /usage with its job-group breakdown over small task tables.  The first cases transcribe the
reference's own tests: test-get-user-usage-no-usage and test-get-user-usage-with-some-usage (scheduler/test/cook/test/rest/api.clj:
2297-2417), test-total-resources-of-jobs (scheduler/test/cook/test/tools.clj:36-51) and the invariants of test_user_usage_grouped
(integration/tests/cook/test_basic.py:2221-2302).  The hand-derived cases follow, each with its derivation beside it.  Data only.

Fields: users (names; ids = positions); n_groups; pools: one task table per engine, tasks in CREATION order (row = position; the loader
gives ids and start times in that order): user, state ("running" / "waiting"), cpus, mem, gpus (optional), group (optional id),
priority (optional, 50); no_gpus (the table has no gpus column); no_groups (group_of_row is NULL); multi (the call without a pool over
all engines; rows are then [engine, row]); user_maps (null, or per engine null / the engine's own user names: the engine's table then
knows only those users, in that order); ask: null (all users) or the list of user ids asked for.
expect: total {user: [cpus, mem, gpus, jobs]}; buckets {user: [[group or null, [cpus, mem, gpus, jobs], rows]]} in the returned order
(the ungrouped bucket first); pools: per engine null or {total, buckets} of the call with that pool; error: "invalid".
`python tests/golden/make_usage_golden.py` rewrites the file."""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
API = "test/cook/test/rest/api.clj"
TOOLS = "test/cook/test/tools.clj"
ITEST = "integration/tests/cook/test_basic.py"
HD = "hand-derived"
Z = [0.0, 0.0, 0.0, 0]


def run(user, cpus, mem, gpus=None, **kw):
    return dict(user=user, state="running", cpus=cpus, mem=mem, **({"gpus": gpus} if gpus is not None else {}), **kw)


def wait(user, cpus, mem, **kw):
    return dict(user=user, state="waiting", cpus=cpus, mem=mem, **kw)


def pool(*tasks, no_gpus=False, no_groups=False, users=None):
    return dict(tasks=list(tasks), no_gpus=no_gpus, no_groups=no_groups, users=users)


def case(name, ref, users, pools, *, n_groups=0, multi=False, ask=None, expect):
    return dict(name=name, ref=ref, users=users, n_groups=n_groups, pools=pools, multi=multi, ask=ask, expect=expect)


J1 = run("alice", 12, 34, 56)       # api.clj:2331-2336
J2 = run("alice", 78, 910, 1112)    # :2367-2373, pool baz
J3 = run("alice", 13, 14, 15)       # :2395-2401, pool bar
NO = dict(total={"alice": Z}, buckets={"alice": []})
# tools.clj:39-42
TR = [run("u", 4.00, 0.5), run("u", 0.10, 10.0, 1.0), run("u", 1.00, 30.0, 2.0), run("u", 10.0, 5.0)]
# test_basic.py:2226-2228: two jobs of {cpus 0.11, mem 123} in one group
G2 = [run("u", 0.11, 123, group=0), run("u", 0.11, 123, group=0)]

CASES = [
    case("no usage, no pools", API + ":2297-2304", ["alice"], [pool()], expect=NO),
    # three pools, no job: zero in total and in every pool (:2306-2325)
    case("no usage, three pools", API + ":2306-2325", ["alice"], [pool(), pool(), pool()], multi=True,
         expect=dict(total={"alice": Z}, buckets={"alice": []}, pools=[NO, NO, NO])),
    case("one job, no pools", API + ":2331-2341", ["alice"], [pool(J1)],
         expect=dict(total={"alice": [12.0, 34.0, 56.0, 1]}, buckets={"alice": [[None, [12.0, 34.0, 56.0, 1], [0]]]})),
    # the job without a pool counts for the default pool "bar" (the host's rule, api.clj:2933-2937): engines foo, bar, baz (:2343-2364)
    case("a job without a pool shows up in the default pool", API + ":2343-2364", ["alice"], [pool(), pool(J1), pool()], multi=True,
         expect=dict(total={"alice": [12.0, 34.0, 56.0, 1]}, buckets={"alice": [[None, [12.0, 34.0, 56.0, 1], [[1, 0]]]]},
                     pools=[NO, dict(total={"alice": [12.0, 34.0, 56.0, 1]}, buckets={"alice": [[None, [12.0, 34.0, 56.0, 1], [0]]]}), NO])),
    # default pool foo holds the first job, baz the second: 90 / 944 / 1168 / 2 over the pools (:2366-2391)
    case("jobs of two pools", API + ":2366-2391", ["alice"], [pool(J1), pool(), pool(J2)], multi=True,
         expect=dict(total={"alice": [90.0, 944.0, 1168.0, 2]}, buckets={"alice": [[None, [90.0, 944.0, 1168.0, 2], [[0, 0], [2, 0]]]]},
                     pools=[dict(total={"alice": [12.0, 34.0, 56.0, 1]}, buckets={"alice": [[None, [12.0, 34.0, 56.0, 1], [0]]]}), NO,
                            dict(total={"alice": [78.0, 910.0, 1112.0, 1]}, buckets={"alice": [[None, [78.0, 910.0, 1112.0, 1], [0]]]})])),
    # a specific pool: foo nothing, bar the third job, baz (the default) the first two (:2393-2417); over all three (hand-derived, in
    # the engines' order) 13 + 12 + 78, 14 + 34 + 910, 15 + 56 + 1112
    case("asking for a specific pool", API + ":2393-2417", ["alice"], [pool(), pool(J3), pool(J1, J2)], multi=True,
         expect=dict(total={"alice": [103.0, 958.0, 1183.0, 3]},
                     buckets={"alice": [[None, [103.0, 958.0, 1183.0, 3], [[1, 0], [2, 0], [2, 1]]]]},
                     pools=[NO, dict(total={"alice": [13.0, 14.0, 15.0, 1]}, buckets={"alice": [[None, [13.0, 14.0, 15.0, 1], [0]]]}),
                            dict(total={"alice": [90.0, 944.0, 1168.0, 2]}, buckets={"alice": [[None, [90.0, 944.0, 1168.0, 2], [0, 1]]]})])),
    case("total-resources-of-jobs, take 1", TOOLS + ":44-45", ["u"], [pool(*TR[:1])],
         expect=dict(total={"u": [4.0, 0.5, 0.0, 1]}, buckets={"u": [[None, [4.0, 0.5, 0.0, 1], [0]]]})),
    case("total-resources-of-jobs, take 2", TOOLS + ":46-47", ["u"], [pool(*TR[:2])],
         expect=dict(total={"u": [4.1, 10.5, 1.0, 2]}, buckets={"u": [[None, [4.1, 10.5, 1.0, 2], [0, 1]]]})),
    case("total-resources-of-jobs, all", TOOLS + ":48-49", ["u"], [pool(*TR)],
         expect=dict(total={"u": [15.1, 45.5, 3.0, 4]}, buckets={"u": [[None, [15.1, 45.5, 3.0, 4], [0, 1, 2, 3]]]})),
    case("total-resources-of-jobs, nil", TOOLS + ":50-51", ["u"], [pool()], expect=dict(total={"u": Z}, buckets={"u": []})),
    # a group of n equal jobs: usage = n x the job, the listed jobs are exactly the group's (:2247-2253); with two ungrouped jobs
    # beside it grouped + ungrouped jobs = total jobs (:2271-2272); 0.11 + 0.11 + 1 + 2 left to right for the total
    case("a group of two equal jobs", ITEST + ":2221-2272", ["u"], [pool(*G2, run("u", 1, 10), run("u", 2, 20), no_gpus=True)], n_groups=1,
         expect=dict(total={"u": [0.11 + 0.11 + 1 + 2, 123.0 + 123 + 10 + 20, 0.0, 4]},
                     buckets={"u": [[None, [3.0, 30.0, 0.0, 2], [2, 3]], [0, [2 * 0.11, 2 * 123.0, 0.0, 2], [0, 1]]]})),
    # ---- hand-derived edges
    case("no users", HD, [], [pool()], expect=dict(total={}, buckets={})),
    case("no running rows", HD, ["a", "b"], [pool(wait("a", 1, 2), wait("b", 3, 4, group=0))], n_groups=1,
         expect=dict(total={"a": Z, "b": Z}, buckets={"a": [], "b": []})),
    # group_of_row NULL: the group fields of the tasks are not passed, every row is ungrouped
    case("group_of_row NULL", HD, ["a"], [pool(run("a", 1, 2, 1, group=0), run("a", 2, 4, 1, group=1), no_groups=True)], n_groups=2,
         expect=dict(total={"a": [3.0, 6.0, 2.0, 2]}, buckets={"a": [[None, [3.0, 6.0, 2.0, 2], [0, 1]]]})),
    # a: only grouped jobs (groups 2 and 0: ascending id, not creation order); b: only ungrouped ones; c: none
    case("only grouped / only ungrouped", HD, ["a", "b", "c"],
         [pool(run("a", 1, 10, 0, group=2), run("b", 2, 20, 0), run("a", 4, 40, 1, group=0), run("a", 8, 80, 0, group=2), run("b", 16, 160, 2))],
         n_groups=3,
         expect=dict(total={"a": [13.0, 130.0, 1.0, 3], "b": [18.0, 180.0, 2.0, 2], "c": Z},
                     buckets={"a": [[0, [4.0, 40.0, 1.0, 1], [2]], [2, [9.0, 90.0, 0.0, 2], [0, 3]]], "b": [[None, [18.0, 180.0, 2.0, 2], [1, 4]]],
                              "c": []})),
    # one group shared by two users: two buckets.  The priority-90 job of a sorts first in a's task order although created last.
    case("one group, two users", HD, ["a", "b"],
         [pool(run("a", 1, 1, group=0), run("b", 2, 2, group=0), run("a", 4, 4), run("a", 8, 8, group=0, priority=90))], n_groups=1,
         expect=dict(total={"a": [13.0, 13.0, 0.0, 3], "b": [2.0, 2.0, 0.0, 1]},
                     buckets={"a": [[None, [4.0, 4.0, 0.0, 1], [2]], [0, [9.0, 9.0, 0.0, 2], [3, 0]]], "b": [[0, [2.0, 2.0, 0.0, 1], [1]]]})),
    # one group in two pools: ONE bucket in the call without a pool, its rows engine by engine; the second engine's table knows the
    # users in another order (user_map)
    case("one group, two pools", HD, ["a", "b"],
         [pool(run("a", 1, 1, group=1), run("b", 2, 2)), pool(run("b", 4, 4, group=1), run("a", 8, 8, group=1), run("a", 16, 16), users=["b", "a"])],
         n_groups=2, multi=True,
         expect=dict(total={"a": [25.0, 25.0, 0.0, 3], "b": [6.0, 6.0, 0.0, 2]},
                     buckets={"a": [[None, [16.0, 16.0, 0.0, 1], [[1, 2]]], [1, [9.0, 9.0, 0.0, 2], [[0, 0], [1, 1]]]],
                              "b": [[None, [2.0, 2.0, 0.0, 1], [[0, 1]]], [1, [4.0, 4.0, 0.0, 1], [[1, 0]]]]},
                     pools=[dict(total={"a": [1.0, 1.0, 0.0, 1], "b": [2.0, 2.0, 0.0, 1]},
                                 buckets={"a": [[1, [1.0, 1.0, 0.0, 1], [0]]], "b": [[None, [2.0, 2.0, 0.0, 1], [1]]]}), None])),
    case("gpus column NULL", HD, ["a"], [pool(run("a", 1.5, 2.5, group=0), run("a", 2.5, 3.5, group=0), no_gpus=True)], n_groups=1,
         expect=dict(total={"a": [4.0, 6.0, 0.0, 2]}, buckets={"a": [[0, [4.0, 6.0, 0.0, 2], [0, 1]]]})),
    # a pending row's group id is ignored, even one that is no group
    case("a pending row carrying a group id", HD, ["a"], [pool(wait("a", 100, 100, group=0), run("a", 1, 2, 3, group=0), wait("a", 7, 7, group=99))],
         n_groups=1, expect=dict(total={"a": [1.0, 2.0, 3.0, 1]}, buckets={"a": [[0, [1.0, 2.0, 3.0, 1], [1]]]})),
    # a list of users: b twice, c (no rows), a — in list order, a repeated user counting again
    case("a list with repeats and a user without rows", HD, ["a", "b", "c"],
         [pool(run("a", 1, 10, group=0), run("b", 2, 20), run("b", 4, 40, group=0), run("a", 8, 80, group=0))], n_groups=1, ask=[1, 1, 2, 0],
         expect=dict(total={"a": [9.0, 90.0, 0.0, 2], "b": [6.0, 60.0, 0.0, 2], "c": Z},
                     buckets={"a": [[0, [9.0, 90.0, 0.0, 2], [0, 3]]], "b": [[None, [2.0, 20.0, 0.0, 1], [1]], [0, [4.0, 40.0, 0.0, 1], [2]]], "c": []})),
    case("an empty list of users", HD, ["a"], [pool(run("a", 1, 1))], ask=[], expect=dict(total={}, buckets={})),
    case("a bad group id", HD, ["a"], [pool(run("a", 1, 1, group=0), run("a", 1, 1, group=3))], n_groups=3, expect=dict(error="invalid")),
    case("a bad user id", HD, ["a", "b"], [pool(run("a", 1, 1))], ask=[0, 2], expect=dict(error="invalid")),
]

if __name__ == "__main__":
    out = os.path.join(HERE, "usage.json")
    with open(out, "w") as f:
        json.dump(dict(cases=CASES), f, indent=1)
        f.write("\n")
    print(out, len(CASES))
