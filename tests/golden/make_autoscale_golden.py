"""Writes tests/golden/autoscale.json: the pending-job candidates of handle-resource-offers-autoscaling-helper
(scheduler/src/cook/scheduler/scheduler.clj:1283-1335) after one match cycle of a pool.  The first case is the reference's own
"Autoscaler increases offers." (scheduler/test/cook/test/scheduler/scheduler.clj:2241-2256, with the test configuration
:max-jobs-for-autoscaling 1000, :autoscaling-scale-factor 1000.0 of src/cook/test/testutil.clj:120); the others are hand-derived,
each with its derivation beside it.  Every case is one user "u" whose jobs rank in list order (equal priority, no running tasks).

Fields: jobs / offers in the form of tests/golden/match.json (good_enough 0.8), num_considerable K, the staged user state in the form
of tests/golden/considerable.json (user_usage, user_quota — {} means no user filter —, tokens, enforce, pool_quota, pool_usage), ineligible
(job names the considerable path's eligible mask drops), max_jobs, scale_factor, skipped (offer indices whose matches the rate limit
dropped), exclude (job names in the recent-synthetic-pod cache); expected: matched (kept matches), out (names in order) and the info
fields.  `python tests/golden/make_autoscale_golden.py` rewrites the file."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import T_SCHED, _HRO8, _KO, _k8s, job  # noqa: E402

S_SCHED = "src/cook/scheduler/scheduler.clj"


def _jobs(prefix, n, cpus=1.0, mem=1024.0):
    return [job(f"{prefix}{i}", "u", cpus, mem) for i in range(1, n + 1)]


def case(name, ref, jobs, offers, k, matched, out, m, u, n, a, *, usage=None, quota=None, max_jobs=1000, scale=1.0, **kw):
    d = dict(name=name, ref=ref, good_enough=0.8, jobs=jobs, offers=offers, num_considerable=k, user_usage={"u": usage} if usage else {},
             user_quota={"u": quota} if quota else {}, max_jobs=max_jobs, scale_factor=scale, skipped=[], exclude=[], ineligible=[],
             expect_matched=matched, expect_out=out, expect_info=dict(matched=m, unmatched=u, scaled=n, autoscalable=a, n_out=len(out)))
    d.update(kw)
    return d


CASES = [
    # K = 6 of the eight jobs pass the user quota (cumulative count 9 <= 10, cpus 63 <= 70, mem 16384, gpus 6 <= 10) and are considered;
    # offers 1-3 take job-1..4; u = 2, fraction 2/6, min(333.3, 1) * 1000 = 1000 = N; Q' = job-5..8 all pass again
    case("Autoscaler increases offers.", f"{T_SCHED}:2241-2256", _HRO8, [_KO[1], _KO[2], _KO[3]], 6,
         [f"job-{i}" for i in range(1, 5)], [f"job-{i}" for i in range(5, 9)], 4, 2, 1000, 4,
         usage=dict(count=1, cpus=2, mem=1024, gpus=0), quota=dict(count=10, cpus=70, mem=32768, gpus=10), scale=1000.0),
    # cpus quota 10, four 4-cpu jobs: the considerable pass keeps a1, a2 (8; a3 makes 12); the 4-cpu offer takes a1.  Without a1 the
    # queue a2, a3, a4 reaches 4, 8, 12: a3 fits now (it would not if the matched a1 still counted), a4 does not.  fraction 1/2 -> N 500
    case("removing the matched jobs frees user quota", "hand: tools.clj:903-915 over Q'", _jobs("a", 4, cpus=4.0), [_k8s(4, 8192)], 2,
         ["a1"], ["a2", "a3"], 1, 1, 500, 2, quota=dict(count=100, cpus=10, mem=1e9, gpus=10)),
    # b2 is dropped by the considerable path's eligible mask (job-allowed-to-start? / launch plugin), and no offer fits: u = k = 2,
    # N = 1000; the autoscaling path has no such mask (:1307-1318), so b2 is a candidate
    case("an ineligible job is still a candidate", f"hand: {S_SCHED}:747-748 vs :1307-1318", _jobs("b", 3), [_k8s(0.5, 128)], 3,
         [], ["b1", "b2", "b3"], 0, 2, 1000, 3, ineligible=["b2"]),
    # max_jobs 2: u = 4 of k = 5, fraction 0.8 * 1 * 2 = 1.6 -> 1 < u: N = u = 4 of Q' = c2..c6
    case("N = u when the scaled share is smaller", f"hand: {S_SCHED}:1301-1306", _jobs("c", 6), [_k8s(1, 1024)], 5,
         ["c1"], ["c2", "c3", "c4", "c5"], 1, 4, 4, 4, max_jobs=2),
    # scale 1000: 0.5 * 1000 = 500 -> min(., 1) = 1 -> 1 * 3 = 3 = N (u = 1)
    case("min(fraction * scale, 1) caps N at max_jobs", f"hand: {S_SCHED}:1301-1306", _jobs("d", 6), [_k8s(1, 1024)], 2,
         ["d1"], ["d2", "d3", "d4"], 1, 1, 3, 3, max_jobs=3, scale=1000.0),
    # max_jobs 10, scale 1: two of four considered match (2 cpus), fraction 0.5 -> N 5 of the eight jobs of Q'
    case("the take cuts the list", f"hand: {S_SCHED}:1316", _jobs("e", 10), [_k8s(2, 2048)], 4,
         ["e1", "e2"], ["e3", "e4", "e5", "e6", "e7"], 2, 2, 5, 5, max_jobs=10),
    # N = 3 as in the min case: A = f2, f3, f4; f3 and f6 are in the cache: f3 leaves, f6 is no candidate; f5 does not move up
    case("exclusion after the take, no refill", f"hand: {S_SCHED}:1319", _jobs("f", 6), [_k8s(1, 1024)], 2,
         ["f1"], ["f2", "f4"], 1, 1, 3, 3, max_jobs=3, scale=1000.0, exclude=["f3", "f6"]),
    # g1 (2 cpus) only fits offer 1, g2 takes offer 0, g3 unmatched.  The rate limit dropped offer 1's cluster: g1 is unmatched, u = 2 of
    # k = 3, fraction (float)2 / 3 -> 666 = N, and Q' = g1, g3, g4
    case("a skipped offer's job is a candidate and counts in u", f"hand: {S_SCHED}:887-924", [job("g1", "u", 2.0, 2048.0)] + _jobs("g", 4)[1:],
         [_k8s(1, 1024), _k8s(2, 2048)], 3, ["g2"], ["g1", "g3", "g4"], 1, 2, 666, 3, skipped=[1]),
    # 2 tokens, enforcing: the considerable pass keeps h1, h2; the offer takes h1.  Fresh counters over Q' = h2..h5 pass h2, h3 again
    # (carried over from the considerable pass, no job would)
    case("the rate-limit counters start fresh", f"hand: tools.clj:935-955, {S_SCHED}:1313 (atom {{}})", _jobs("h", 5), [_k8s(1, 1024)], 5,
         ["h1"], ["h2", "h3"], 1, 1, 500, 2, tokens={"u": 2}, enforce=True),
    # pool quota count 4 seeded with the users' usage (count 1): the considerable pass keeps p1..p3 (2, 3, 4); the offer takes p1;
    # over Q' = p2..p5 the pool count reaches 2, 3, 4, 5: p2, p3, p4
    case("the pool quota over Q'", "hand: tools.clj:917-933, 966", _jobs("p", 5), [_k8s(1, 1024)], 5,
         ["p1"], ["p2", "p3", "p4"], 1, 2, 666, 3, usage=dict(count=1, cpus=1, mem=1024, gpus=0),
         quota=dict(count=100, cpus=100, mem=1e9, gpus=10), pool_quota=dict(count=4, cpus=100, mem=1e9)),
    # a user quota of count 0: nothing is considerable, k = 0 -> fraction 0, N = max(0, 0) = 0: no candidate although the queue is full
    case("k = 0 gives N = 0", f"hand: {S_SCHED}:1288-1290", _jobs("z", 3), [_k8s(4, 4096)], 5,
         [], [], 0, 0, 0, 0, quota=dict(count=0, cpus=100, mem=1e9, gpus=10)),
]


def main():
    path = os.path.join(HERE, "autoscale.json")
    with open(path, "w") as f:
        json.dump(CASES, f, indent=1)
        f.write("\n")
    print(path, len(CASES))


if __name__ == "__main__":
    main()
