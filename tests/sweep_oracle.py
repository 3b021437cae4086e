"""A plain-Python restatement of the three task killers of the reference, the oracle of cook_sweep_running.

Python ints carry the reference's Java longs (no overflow to guard against), and every long/double meeting is an explicit float(),
as in Clojure: (* int double) and (> long double) are double operations.  References are to scheduler/src/cook/.
"""
from __future__ import annotations

import math

INT32_MAX = 2 ** 31 - 1
START_ABSENT = -(2 ** 63)
NONE_U32 = 0xFFFFFFFF
LINGERING, STRAGGLERS, CANCELLED = 1, 2, 4


class SweepError(ValueError):
    """where the reference throws (Interval, Seconds.secondsIn, RT.intCast) or the arguments break the ABI's rules"""

    def __init__(self, msg, bad_row=NONE_U32):
        super().__init__(msg)
        self.bad_row = bad_row


def _list(x):
    """a column as a list of Python numbers (numpy arrays included), None as it stands"""
    return None if x is None else x.tolist() if hasattr(x, "tolist") else list(x)


def in_seconds(start, end):
    """t/in-seconds of (t/interval start end): Interval throws for end < start (a nil start: the ABI calls it absent and throws too),
    Seconds.secondsIn for more than Integer/MAX_VALUE seconds; else whole seconds, truncated.  None where the reference throws."""
    if start == START_ABSENT or end < start:
        return None
    s = (end - start) // 1000  # (end >= start: floor is truncation)
    return None if s > INT32_MAX else s


def lingering(now, start, max_runtime, default_timeout, max_timeout):
    """scheduler.clj:1888-1912 get-lingering-tasks for one running/unknown instance: the datalog query has no row without
    :instance/start-time; max-runtime is get-else the default; (time/after? now (time/plus start (millis->period (min rt max))))"""
    if start == START_ABSENT:
        return False
    rt = max_runtime if max_runtime is not None and max_runtime >= 0 else default_timeout  # (get-else $ ?j :job/max-runtime ?default)
    boundary = start + min(rt, max_timeout)  # Period of plain milliseconds
    return now > boundary  # time/after?: strict


def quantile_index(job_count, q):
    """group.clj:35 (int (* (dec (count jobs)) quantile)): a long times a double, truncated by RT.intCast"""
    if job_count > INT32_MAX:
        raise SweepError("job_count > INT32_MAX")
    return int(math.trunc(float(job_count - 1) * q))


def group_threshold(now, typ, q, mult, job_count, succ):
    """group.clj:17-44 find-stragglers for one group: -> (ready, threshold seconds or NaN).  succ: [(start, end or None)] of the
    :instance.status/success instances of the group's jobs."""
    if typ == 0:  # :none does nothing
        return False, math.nan
    if typ != 1:
        raise SweepError("straggler-handling type > 1")
    if not (0.0 < q < 1.0) or not (1.0 < mult < math.inf):  # api.clj:495-497 (NaN and inf fail both)
        raise SweepError("quantile / multiplier out of range")
    idx = quantile_index(job_count, q)
    if not len(succ) > idx:  # (when (> (count successful-tasks) quantile-job-idx) ...)
        return False, math.nan
    secs = []
    for j, (st, en) in enumerate(succ):  # sort-by (comp t/in-seconds util/task-run-time): every instance is evaluated
        s = in_seconds(st, now if en is None or en < 0 else en)  # tools.clj:670-676: no end-time -> now
        if s is None:
            raise SweepError("successful instance interval", bad_row=j)
        secs.append(s)
    target = sorted(secs)[idx]  # (nth sorted-success-tasks quantile-job-idx); ties do not matter: only s is used
    return True, float(target) * mult  # (* target-runtime-seconds multiplier)


def sweep(now, start, unknown=None, max_runtime=None, cancelled=None, group=None, groups=None, default_timeout=0, max_timeout=0,
          what=LINGERING | STRAGGLERS | CANCELLED):
    """-> dict(reason, lingering, stragglers, cancelled, threshold_s, info) as cook_sweep_running returns it (lists in row order: the
    reference's Datomic set order is unpinned), or raises SweepError (bad_row as the engine reports it: the lowest offending running
    row, else n + the lowest offending successful instance, else NONE).  groups: dict of type, quantile, multiplier, job_count,
    succ_off, succ_start_ms, succ_end_ms."""
    start, unknown, max_runtime, cancelled, group = (_list(x) for x in (start, unknown, max_runtime, cancelled, group))
    n = len(start)
    unk = [bool(x) for x in unknown] if unknown is not None else [False] * n
    reason = [0] * n
    if what & LINGERING:
        if default_timeout < 0 or max_timeout < 0:
            raise SweepError("negative timeout")
        for i in range(n):  # running and unknown rows alike (the ground of the query)
            rt = max_runtime[i] if max_runtime is not None else None
            if lingering(now, start[i], rt, default_timeout, max_timeout):
                reason[i] |= LINGERING
    G = len(groups["type"]) if (what & STRAGGLERS) and groups is not None else 0
    thr = [math.nan] * (len(groups["type"]) if groups is not None else 0)
    ready = 0
    if what & STRAGGLERS:
        if groups is None:
            raise SweepError("no groups")
        off = _list(groups["succ_off"]) if G else [0]
        gt, gq, gm, gj = (_list(groups[k]) for k in ("type", "quantile", "multiplier", "job_count"))
        ss, se = _list(groups["succ_start_ms"]), _list(groups["succ_end_ms"])
        if off[0] != 0 or any(off[g] > off[g + 1] for g in range(G)):
            raise SweepError("succ_off")
        errs, bad_succ = [], []
        evaluated = [False] * G  # ready groups of type 1, those whose successes threw included (their rows are looked at all the same)
        for g in range(G):
            succ = list(zip(ss[off[g]:off[g + 1]], se[off[g]:off[g + 1]]))
            try:
                ok, thr[g] = group_threshold(now, gt[g], float(gq[g]), float(gm[g]), gj[g], succ)
                ready += ok
                evaluated[g] = ok
            except SweepError as ex:
                if ex.bad_row != NONE_U32:
                    bad_succ.append(off[g] + ex.bad_row)
                    evaluated[g] = True
                else:
                    errs.append(ex)
                thr[g] = math.nan
        bad_rows = []
        for i in range(n):  # scheduler.clj:1955-1986 handle-stragglers over every group of a running job
            g = group[i] if group is not None else NONE_U32
            if g == NONE_U32:
                continue
            if g >= G:
                bad_rows.append(i)
                continue
            if not evaluated[g] or unk[i]:  # (not ready / no quantile-deviation; find-stragglers keeps status running only)
                continue
            s = in_seconds(start[i], now)
            if s is None:
                bad_rows.append(i)
            elif float(s) > thr[g]:  # (> (t/in-seconds (util/task-run-time %)) max-runtime-seconds)
                reason[i] |= STRAGGLERS
        bad = min(bad_rows) if bad_rows else (n + min(bad_succ) if bad_succ else NONE_U32)
        if errs or bad_rows or bad_succ:
            raise SweepError(str(errs[0]) if errs else "interval", bad_row=bad)
    if what & CANCELLED and cancelled is not None:  # scheduler.clj:1988-1996: :instance/cancelled true, running or unknown
        for i in range(n):
            if cancelled[i]:
                reason[i] |= CANCELLED
    lists = {k: [i for i in range(n) if reason[i] & bit] for k, bit in (("lingering", LINGERING), ("stragglers", STRAGGLERS),
                                                                          ("cancelled", CANCELLED))}
    info = dict(lingering=len(lists["lingering"]), stragglers=len(lists["stragglers"]), cancelled=len(lists["cancelled"]),
                groups_ready=ready, bad_row=NONE_U32)
    return dict(reason=reason, threshold_s=thr, info=info, **lists)
