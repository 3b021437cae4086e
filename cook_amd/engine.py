"""ctypes binding of libcookmatch.so (include/cookmatch.h).

The product path is the HIP library and nothing else: if the shared object is missing or no MI355X is visible,
construction raises — there is NO CPU fallback (the CPU oracle under oracle/ is test infrastructure and is never
imported from this package).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from . import _abi as A
from ._protos import PROTOS

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.environ.get("COOK_LIB") or os.path.join(_HERE, "libcookmatch.so")  # COOK_LIB: a tuning variant of the same library

EXPORTS = list(PROTOS)  # every function include/cookmatch.h declares (cook_amd/_protos.py is generated from the header)


class CookError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"cookmatch error {code}: {msg}")
        self.code = code


_LIBS = {}


def load_library(path: Optional[str] = None):
    path = os.path.abspath(path or DEFAULT_LIB)
    if path in _LIBS:
        return _LIBS[path]
    # PyTorch-ROCm wheels bundle their own libamdhip64/libhsa-runtime64 (same SONAME as /opt/rocm's).  Whichever HIP
    # runtime is loaded FIRST serves the whole process, and mixing the two fails at hsa_init.  Every caller of this
    # package (bench.py, smoke(), the tests) also uses torch for device plumbing, so load torch's runtime first.
    # Kernel arguments in device memory: the launch-latency setting of this ROCm build (a cycle is ~500 dependent launches per chain;
    # with it switched off the eight-pool cycle measured 63.5 ms against 58.9).  Already the default here; pinned for hosts where it is not.
    os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} not found: build the HIP extension first (python -m cook_amd.build). "
            "cook_amd has no CPU fallback.")
    lib = C.CDLL(path)
    for name, (restype, argtypes) in PROTOS.items():
        fn = getattr(lib, name)  # AttributeError if the ABI is incomplete
        fn.restype = restype
        fn.argtypes = argtypes   # pointers are c_void_p: ctypes checks the argument COUNT and pointer-vs-scalar for every call
    # the struct layouts of cook_amd._abi mirror include/cookmatch.h at COOK_ABI_VERSION: a library of another layout is refused before
    # the first call passes it a struct
    if lib.cook_abi_version() != A.ABI_VERSION:
        raise CookError(-1,
                        f"{path} has ABI version {lib.cook_abi_version()}, this binding was written for {A.ABI_VERSION}")
    _LIBS[path] = lib
    return lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Engine:
    """One engine per pool (one HIP stream); not re-entrant (cookmatch.h conventions)."""

    def __init__(self, params: Optional[A.CookParams] = None, device: int = 0, lib_path: Optional[str] = None):
        self._lib = load_library(lib_path)
        self.params = params or A.default_params()
        h = C.c_void_p()
        rc = self._lib.cook_engine_create(C.byref(self.params), int(device), C.byref(h))
        if rc != 0 or not h:
            why = self._lib.cook_last_error(None).decode()  # (the thread's last refused create; "null engine" when the params were not the reason)
            if why != "null engine":
                raise CookError(rc, f"cook_engine_create: {why}")
            raise CookError(rc, "cook_engine_create failed (no visible MI355X / HIP runtime error); "
                                "cook_amd has no CPU fallback")
        self._h = h
        self._keep = []

    def close(self):
        if getattr(self, "_h", None):
            self._lib.cook_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def version(self) -> str:
        return self._lib.cook_version().decode()

    def _chk(self, rc):
        if rc != 0:
            raise CookError(rc, self._lib.cook_last_error(self._h).decode())

    def set_params(self, params: A.CookParams):
        self.params = params
        self._chk(self._lib.cook_engine_set_params(self._h, C.byref(params)))

    # ---- rank --------------------------------------------------------------------------------------------
    def rank_stage(self, tasks: A.Tasks, users: A.Users):
        ts, us = tasks.as_struct(), users.as_struct()
        self._rank_n, self._rank_np = tasks.n, int(tasks.pending.sum()) if tasks.n else 0
        self._tasks_n = tasks.n  # the staged table's row count, exactly (unscheduled sizes its outputs by it)
        self._n_users = users.n
        self._chk(self._lib.cook_rank_stage(self._h, C.byref(ts), C.byref(us)))

    def rank_set_quota(self, quota: Optional[A.CookPoolQuota]):
        self._chk(self._lib.cook_rank_set_quota(self._h, C.byref(quota) if quota is not None else None))

    def rank_pool_usage(self) -> A.CookUsage:
        u = A.CookUsage()
        self._chk(self._lib.cook_rank_pool_usage(self._h, C.byref(u)))
        return u

    def rank_user_usage(self, n_users: int, device_ptr: Optional[int] = None):
        """[U, 3] = {cpus, mem, gpus} of every user's running tasks in this pool (cook_rank_user_usage).  With `device_ptr` (the
        address of a device buffer of U x 3 doubles, e.g. a torch tensor's data_ptr()) nothing comes back to the host."""
        if device_ptr is not None:
            self._chk(self._lib.cook_rank_user_usage(self._h, C.c_void_p(device_ptr), 1))
            return None
        out = np.zeros((max(1, n_users), 3), dtype=np.float64)
        self._chk(self._lib.cook_rank_user_usage(self._h, _p(out, C.c_double), 0))
        return out[:n_users]

    def user_stats(self, limits: Optional[A.UserLimits] = None, per_user_device_ptr: Optional[int] = None) -> dict:
        """set-stats-counters!'s numbers for this pool from the last rank run (cook_user_stats): a dict of per_user [U, 4, 3], state [U],
        all [4, 3] and the five counts (cook_amd._abi.user_stats_result).  limits None: the staged users' divisors as shares and their
        quotas.  per_user_device_ptr: the per-user rows go to that device buffer of U x 12 doubles instead (per_user is None then)."""
        n = limits.n if limits is not None else getattr(self, "_n_users", 0)
        lim = C.byref(limits.as_struct()) if limits is not None else None
        out = _StatsOut(n, per_user_device_ptr)
        _check_multi([self], self._lib.cook_user_stats(self._h, lim, *out.args()))
        return out.result()

    def unscheduled(self, limits: Optional[A.UnschedLimits] = None, in_window=None, rows=None, total_device_ptr: Optional[int] = None) -> dict:
        """Why the jobs of this pool wait, from the last rank run (cook_unscheduled): the quota, share and queue-position reasons of
        cook.unscheduled/reasons for every task row, or for the task rows `rows` (any order, repeats allowed).  limits None: the staged
        users' quotas and their divisors as shares.  in_window ([tasks.n] bytes): the pending rows the host's "first 100 waiting jobs"
        query returns, None = all.  -> dict(reasons [n] uint32 (A.UNSCHED_* bits), queue_pos [n] uint32, total [n, 4] float64
        ({count, cpus, mem, gpus}; None with total_device_ptr, the address of a device buffer of n x 4 doubles), ahead [U, 10] uint32
        task rows (A.NONE_U32 = none), list_len [U] uint32)."""
        N, U = getattr(self, "_tasks_n", 0), getattr(self, "_n_users", 0)
        lim = C.byref(limits.as_struct()) if limits is not None else None
        win = None
        if in_window is not None:
            win = np.ascontiguousarray(in_window, dtype=np.uint8)
            assert len(win) == N, "in_window has one byte per task row"
        rw = np.ascontiguousarray(rows, dtype=np.uint32) if rows is not None else None
        n = len(rw) if rw is not None else N
        reasons = np.zeros(max(1, n), dtype=np.uint32)
        qpos = np.zeros(max(1, n), dtype=np.uint32)
        total = np.zeros((max(1, n), 4), dtype=np.float64) if total_device_ptr is None else None
        ahead = np.zeros((max(1, U), A.UNSCHED_AHEAD), dtype=np.uint32)
        llen = np.zeros(max(1, U), dtype=np.uint32)
        # (an empty list of rows still is a list: numpy's pointer to an empty array is not NULL)
        self._chk(self._lib.cook_unscheduled(
            self._h, lim, win.ctypes.data_as(C.c_void_p) if win is not None else None,
            rw.ctypes.data_as(C.c_void_p) if rw is not None else None, n, reasons.ctypes.data_as(C.c_void_p),
            qpos.ctypes.data_as(C.c_void_p), C.c_void_p(int(total_device_ptr)) if total is None else total.ctypes.data_as(C.c_void_p),
            int(total is None), ahead.ctypes.data_as(C.c_void_p), llen.ctypes.data_as(C.c_void_p)))
        return dict(reasons=reasons[:n], queue_pos=qpos[:n], total=total[:n] if total is not None else None, ahead=ahead[:U], list_len=llen[:U])

    def usage_breakdown(self, group_of_row=None, n_groups: int = 0, users=None, usage_device_ptr: Optional[int] = None,
                        total_device_ptr: Optional[int] = None, cap_rows: Optional[int] = None) -> dict:
        """GET /usage of this pool with its job-group breakdown, from the last rank run (cook_usage_breakdown).  group_of_row
        ([tasks.n] uint32 by task row: interned group ids below n_groups, A.NONE_U32 = no group; None = every row ungrouped); users:
        a list of user ids (any order, repeats allowed) instead of all users.  -> dict(bucket_off [n_out + 1], bucket_group [B]
        (A.NONE_U32 = the ungrouped bucket, which comes first among a user's), bucket_usage [B, 4] float64 ({cpus, mem, gpus, jobs}),
        row_off [B + 1], rows [R] task rows, total [n_out, 4]).  usage_device_ptr / total_device_ptr: the address of a device buffer
        of cap_rows x 4 / n_out x 4 doubles; that entry of the dict is None then.  cap_rows: room for the rows (default: every task
        row, and what a list with repeats asks for)."""
        g = np.ascontiguousarray(group_of_row, dtype=np.uint32) if group_of_row is not None else None
        assert g is None or len(g) == getattr(self, "_tasks_n", len(g)), "group_of_row has one id per task row"
        return _usage_call([self], False, getattr(self, "_n_users", 0), None, [g], n_groups, users, usage_device_ptr, total_device_ptr,
                           cap_rows)

    def rank_run(self):
        self._chk(self._lib.cook_rank_run(self._h))

    def rank_fetch(self, want_dru: bool = True):
        out = np.zeros(max(1, self._rank_np), dtype=np.uint32)
        dru = np.zeros(max(1, self._rank_n), dtype=np.float64) if want_dru else None
        n = C.c_uint32(0)
        self._chk(self._lib.cook_rank_fetch(self._h, _p(out, C.c_uint32), C.byref(n),
                                            _p(dru, C.c_double) if want_dru else None))
        return out[: n.value].copy(), (dru[: self._rank_n].copy() if want_dru else None)

    def rank(self, tasks: A.Tasks, users: A.Users, quota: Optional[A.CookPoolQuota] = None, want_dru: bool = True):
        """sort-jobs-by-dru-helper + filter-based-on-quota + filter-offensive-jobs -> (ranked task idx, dru per task)."""
        self.rank_stage(tasks, users)
        self.rank_set_quota(quota)
        self.rank_run()
        return self.rank_fetch(want_dru)

    # ---- match -------------------------------------------------------------------------------------------
    def match_stage(self, jobs: A.Jobs, offers: A.Offers, groups: Optional[A.Groups] = None,
                    reserved_hosts: Sequence[int] = ()):
        js, os_ = jobs.as_struct(), offers.as_struct()
        gs = groups.as_struct() if groups is not None else None
        res = np.array(list(reserved_hosts) or [0], dtype=np.uint32)
        self._match_k = jobs.n
        self._chk(self._lib.cook_match_stage(self._h, C.byref(js), C.byref(os_), C.byref(gs) if gs is not None else None,
                                             _p(res, C.c_uint32), len(reserved_hosts)))

    def match_run(self):
        self._chk(self._lib.cook_match_run(self._h))

    def match_count(self) -> int:
        """jobs of the engine's last match = the length cook_match_fetch / cook_cycle_fetch write"""
        n = C.c_uint32(0)
        self._chk(self._lib.cook_match_count(self._h, C.byref(n)))
        return n.value

    def match_fetch(self, k: Optional[int] = None):
        n = self.match_count()  # the engine's own count sizes the buffers (a cycle takes at most num_considerable jobs)
        k = n if k is None else min(k, n)
        j2o = np.full(max(1, n), -1, dtype=np.int32)
        fail = np.zeros(max(1, n), dtype=np.uint32)
        head = C.c_uint8(0)
        self._chk(self._lib.cook_match_fetch(self._h, _p(j2o, C.c_int32), _p(fail, C.c_uint32), C.byref(head)))
        return j2o[:k].copy(), fail[:k].copy(), bool(head.value)

    def match(self, jobs: A.Jobs, offers: A.Offers, groups: Optional[A.Groups] = None, reserved_hosts: Sequence[int] = ()):
        """Body of match-offer-to-schedule: -> (job_to_offer, fail_code, head_matched)."""
        self.match_stage(jobs, offers, groups, reserved_hosts)
        self.match_run()
        return self.match_fetch()

    # ---- rank + match without a host round trip --------------------------------------------------------------
    def cycle_stage(self, tasks: A.Tasks, users: A.Users, pending_jobs: A.Jobs, offers: A.Offers,
                    groups: Optional[A.Groups] = None, reserved_hosts: Sequence[int] = ()):
        ts, us, js, os_ = tasks.as_struct(), users.as_struct(), pending_jobs.as_struct(), offers.as_struct()
        self._n_users = users.n
        gs = groups.as_struct() if groups is not None else None
        res = np.array(list(reserved_hosts) or [0], dtype=np.uint32)
        self._rank_n, self._rank_np = tasks.n, int(tasks.pending.sum()) if tasks.n else 0
        self._tasks_n = tasks.n  # the staged table's row count, exactly (unscheduled sizes its outputs by it)
        self._chk(self._lib.cook_cycle_stage(self._h, C.byref(ts), C.byref(us), C.byref(js), C.byref(os_),
                                             C.byref(gs) if gs is not None else None, _p(res, C.c_uint32),
                                             len(reserved_hosts)))

    def cycle_update(self, remove_task=(), add_tasks: Optional[A.Tasks] = None, add_pending: Optional[A.Jobs] = None,
                     offers: Optional[A.Offers] = None):
        """What changed since the last cycle (cook_cycle_update): task rows to remove (indices into the CURRENT arrays), task /
        pending-job rows to append, optionally fresh offers.  The resident columns are edited on the device."""
        rem = np.ascontiguousarray(np.asarray(list(remove_task) if not isinstance(remove_task, np.ndarray) else remove_task, dtype=np.uint32))
        ts = add_tasks.as_struct() if add_tasks is not None else None
        js = add_pending.as_struct() if add_pending is not None else None
        os_ = offers.as_struct() if offers is not None else None
        d = A.CookCycleDelta(len(rem), _p(rem, C.c_uint32) if len(rem) else None, C.pointer(ts) if ts is not None else None,
                             C.pointer(js) if js is not None else None, C.pointer(os_) if os_ is not None else None)
        self._chk(self._lib.cook_cycle_update(self._h, C.byref(d)))
        n_add = add_tasks.n if add_tasks is not None else 0
        p_add = int(add_tasks.pending.sum()) if n_add else 0
        # the mirror's sizes for the fetch buffers: upper bounds (removed rows only shrink them)
        self._rank_n = self._rank_n + n_add
        self._tasks_n = getattr(self, "_tasks_n", 0) + n_add - len(rem)  # (an accepted delta removes each listed row once)
        self._rank_np = self._rank_np + p_add

    def cycle_run(self, num_considerable: int):
        self._chk(self._lib.cook_cycle_run(self._h, int(num_considerable)))

    def cycle_run_rank(self, num_considerable: int):
        """The rank / considerable / take-K part of cycle_run; the placement then runs in cycle_match_multi()."""
        self._chk(self._lib.cook_cycle_run_rank(self._h, int(num_considerable)))

    def _queue_step(self, offer_skipped=None, remove_mode: int = 0, offers: Optional[A.Offers] = None, groups: Optional[A.Groups] = None):
        """-> (CookQueueStep, the objects its pointers refer to).  offer_skipped has one entry per offer of the LAST cycle: the library
        refuses another length (COOK_E_INVALID, nothing changed)."""
        sk = np.ascontiguousarray(offer_skipped if offer_skipped is not None else [0], dtype=np.uint8)
        os_ = offers.as_struct() if offers is not None else None
        gs = groups.as_struct() if groups is not None else None
        st = A.CookQueueStep(_p(sk, C.c_uint8) if offer_skipped is not None else None, int(remove_mode), len(sk) if offer_skipped is not None else 0,
                             C.pointer(os_) if os_ is not None else None, C.pointer(gs) if gs is not None else None)
        return st, (sk, os_, gs, offers, groups)

    def _queue_call(self, name: str, num_considerable: int, step: dict, *parts):
        """One queue cycle of this engine through the C entry `name`: the step's keywords, then the parts that entry takes, in ABI order
        (carry, finished, hosts, reservations; each None or an object whose as_struct() gives (struct, keep))."""
        st, keep = self._queue_step(**step)
        built = [p.as_struct() if p is not None else (None, None) for p in parts]
        self._chk(getattr(self._lib, name)(self._h, C.byref(st), *[C.byref(s) if s is not None else None for s, _ in built],
                                           int(num_considerable)))
        del keep, built

    def cycle_run_queue(self, num_considerable: int, offer_skipped=None, remove_mode: int = 0, offers: Optional[A.Offers] = None,
                        groups: Optional[A.Groups] = None, defer: bool = False):
        """A match cycle on the standing ranked queue, without a re-rank (cook_cycle_run_queue): the last cycle's kept matches
        (remove_mode 1: every considered job) leave the queue, their cotasks join their groups on the device (or `groups` replaces the
        table), `offers` replaces the staged offers, then considerable -> take K -> match.  defer: set the placement up only
        (cook_cycle_run_queue_rank); it runs in cycle_match_multi()."""
        self._queue_call("cook_cycle_run_queue_rank" if defer else "cook_cycle_run_queue", num_considerable,
                         dict(offer_skipped=offer_skipped, remove_mode=remove_mode, offers=offers, groups=groups))

    def cycle_run_queue_rank(self, num_considerable: int, **step):
        self.cycle_run_queue(num_considerable, defer=True, **step)

    def cycle_run_queue_carry(self, num_considerable: int, carry: Optional[A.QueueCarry] = None, **step):
        """cycle_run_queue with the carry (cook_cycle_run_queue_carry): before the last cycle's jobs leave the queue, its kept placements
        are subtracted from the staged offers (carry.offers; then no `offers` in the step) and added to the staged user state
        (carry.usage), on the device, in considered order.  carry None: exactly cycle_run_queue."""
        self._queue_call("cook_cycle_run_queue_carry", num_considerable, step, carry)

    def cycle_run_queue_release(self, num_considerable: int, carry: Optional[A.QueueCarry] = None, finished: Optional[A.Finished] = None, **step):
        """cycle_run_queue_carry with the release (cook_cycle_run_queue_release): behind the carry and the groups' fold the resources of
        the `finished` tasks go back to the staged offers (finished.offers), out of the staged user state (finished.usage) and out of the
        groups' running cotasks (finished.groups), on the device, in list order.  finished None: exactly cycle_run_queue_carry."""
        self._queue_call("cook_cycle_run_queue_release", num_considerable, step, carry, finished)

    def cycle_run_queue_hosts(self, num_considerable: int, carry: Optional[A.QueueCarry] = None, finished: Optional[A.Finished] = None,
                              hosts: Optional[A.HostChurn] = None, **step):
        """cycle_run_queue_release with the host churn (cook_cycle_run_queue_hosts): behind the carry, the groups' fold and the release
        the rows of the hosts in hosts.leave go out of the staged offers and the rows of hosts.join come in, each in front of its
        anchor, on the device; the surviving rows keep their order.  hosts None: exactly cycle_run_queue_release."""
        self._queue_call("cook_cycle_run_queue_hosts", num_considerable, step, carry, finished, hosts)

    def cycle_run_queue_reserve(self, num_considerable: int, carry: Optional[A.QueueCarry] = None, finished: Optional[A.Finished] = None,
                                hosts: Optional[A.HostChurn] = None, reservations: Optional[A.Reservations] = None, **step):
        """cycle_run_queue_hosts with the host reservations (cook_cycle_run_queue_reserve): behind the churn the last cycle's kept
        matches release their reservations (reservations.release_matched) and the list replaces the engine's map
        (reservations.replace), on the device.  reservations None: exactly cycle_run_queue_hosts."""
        self._queue_call("cook_cycle_run_queue_reserve", num_considerable, step, carry, finished, hosts, reservations)

    def cycle_set_reservations(self, reservations: Optional[A.Reservations] = None):
        """reserve-hosts! on its own (cook_cycle_set_reservations): the list replaces the engine's reservation map for the next cycle,
        rank cycle or queue cycle; None: no reservations.  Touches neither the standing queue nor the placement."""
        rs, rkeep = reservations.as_struct() if reservations is not None else (None, None)
        self._chk(self._lib.cook_cycle_set_reservations(self._h, C.byref(rs) if rs is not None else None))
        del rkeep

    def reserve_info(self) -> dict:
        """The counts of the last call that could change the reservation map (cook_cycle_reserve_info)."""
        out = A.CookReserveInfo()
        self._chk(self._lib.cook_cycle_reserve_info(self._h, C.byref(out)))
        return {k: int(getattr(out, k)) for k, _ in A.CookReserveInfo._fields_}

    def fetch_reservations(self):
        """-> (pending, host): the live reservations in list order (cook_cycle_fetch_reservations); pending NONE_U32: a job outside
        this pool."""
        n = C.c_uint32(0)
        rc = self._lib.cook_cycle_fetch_reservations(self._h, None, None, 0, C.byref(n))
        if rc != 0 and n.value == 0:
            self._chk(rc)
        cap = max(1, n.value)
        pend, host = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        self._chk(self._lib.cook_cycle_fetch_reservations(self._h, _p(pend, C.c_uint32), _p(host, C.c_uint32), cap, C.byref(n)))
        return pend[:n.value].copy(), host[:n.value].copy()

    def cycle_set_limiters(self, limiters: Optional[A.Limiters] = None):
        """The launch-rate limiters the engine keeps from here on (cook_cycle_set_limiters): every later cycle's considerable filter
        reads them instead of the staged tokens_left; a Limiters with a user list replaces only the listed users'; None drops them."""
        ls, keep = limiters.as_struct() if limiters is not None else (None, None)
        self._chk(self._lib.cook_cycle_set_limiters(self._h, C.byref(ls) if ls is not None else None))
        del keep

    def cycle_set_clock(self, now_ms: Optional[int] = None, spend_ms: Optional[int] = None):
        """The time of the NEXT cycle (cook_cycle_set_clock): now_ms the filters' clock reading, spend_ms when the last cycle's kept
        matches were launched (None: now_ms).  now_ms None: no clock — nobody earns."""
        if now_ms is None:
            self._chk(self._lib.cook_cycle_set_clock(self._h, None))
            return
        ck = A.CookClock(int(now_ms), int(now_ms if spend_ms is None else spend_ms))
        self._chk(self._lib.cook_cycle_set_clock(self._h, C.byref(ck)))

    def cycle_limiters_spend(self, spend_ms: int, offer_skipped=None):
        """The last cycle's kept placements spend their tokens now (cook_cycle_limiters_spend): for the cycle that no queue advance
        follows.  offer_skipped: per offer of the last cycle, as in a queue step."""
        sk = np.ascontiguousarray(offer_skipped, np.uint8) if offer_skipped is not None else None
        self._chk(self._lib.cook_cycle_limiters_spend(self._h, _p(sk, C.c_uint8) if sk is not None else None, len(sk) if sk is not None else 0,
                                                      int(spend_ms)))

    def fetch_limiters(self, n_users: int):
        """-> (tokens, last_update_ms, time_until_ms) of the engine's limiters, per user (cook_cycle_fetch_limiters)."""
        n = max(1, int(n_users))
        tok, last, until = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        self._chk(self._lib.cook_cycle_fetch_limiters(self._h, _p(tok, C.c_int64), _p(last, C.c_int64), _p(until, C.c_int64)))
        return tok[:n_users].copy(), last[:n_users].copy(), until[:n_users].copy()

    def fetch_rate_limit(self, n_users: int):
        """-> (rate_limited, passed): the rate-limit stage's per-user counts of the last cycle's considerable filter
        (cook_cycle_fetch_rate_limit)."""
        n = max(1, int(n_users))
        rl, ps = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        self._chk(self._lib.cook_cycle_fetch_rate_limit(self._h, _p(rl, C.c_uint32), _p(ps, C.c_uint32)))
        return rl[:n_users].copy(), ps[:n_users].copy()

    def limiter_info(self) -> dict:
        """The limiters' counts of the last cycle (cook_cycle_limiter_info)."""
        out = A.CookLimiterInfo()
        self._chk(self._lib.cook_cycle_limiter_info(self._h, C.byref(out)))
        return {k: int(getattr(out, k)) for k, _ in A.CookLimiterInfo._fields_ if k != "reserved"}

    def churn_info(self) -> dict:
        """The counts of the last queue cycle's host churn (cook_cycle_churn_info); all 0 (n_offers: the staged rows) when it had none."""
        out = A.CookChurnInfo()
        self._chk(self._lib.cook_cycle_churn_info(self._h, C.byref(out)))
        return {k: int(getattr(out, k)) for k, _ in A.CookChurnInfo._fields_}

    def fetch_offers(self, rows: Optional[A.OfferRows] = None) -> A.OfferRows:
        """The staged offer table as the next match will read it, behind any carry, release and churn (cook_cycle_fetch_offers).
        rows: the caller's columns (their cap too small: CookError); None: sized by the staged table.  -> the OfferRows; .offers() is
        the table as an Offers."""
        probe = A.CookOfferRows()  # cap 0, every column skipped: the call reports n and the widths (and refuses cap < n: no synchronisation)
        rc = self._lib.cook_cycle_fetch_offers(self._h, C.byref(probe))
        if rc != 0 and probe.n == 0:
            self._chk(rc)
        if rows is None:
            rows = A.OfferRows(probe.n, n_attr_keys=probe.n_attr_keys)
        elif rows.n_attr_keys < probe.n_attr_keys:
            raise ValueError(f"fetch_offers: the rows have room for {rows.n_attr_keys} attribute keys, the staged offers have {probe.n_attr_keys}")
        self._chk(self._lib.cook_cycle_fetch_offers(self._h, C.byref(rows.struct)))
        return rows

    def release_info(self) -> dict:
        """The counts of the last queue cycle's release (cook_cycle_release_info); all 0 when it had none."""
        out = A.CookReleaseInfo()
        self._chk(self._lib.cook_cycle_release_info(self._h, C.byref(out)))
        return {k: int(getattr(out, k)) for k, _ in A.CookReleaseInfo._fields_}

    def cycle_fetch(self, out=None):
        """-> (ranked task indices, job_to_offer by rank position, head matched).  `out` = (u32 buffer, i32 buffer) to fetch into
        (e.g. page-locked arrays of a PinnedArena, each with room for every pending task): views of them are returned."""
        if out is None:
            ranked = np.zeros(max(1, self._rank_np), dtype=np.uint32)
            j2o = np.full(max(1, self._rank_np), -1, dtype=np.int32)
        else:
            ranked, j2o = out
            assert len(ranked) >= self._rank_np and len(j2o) >= self._rank_np
        n, k = C.c_uint32(0), C.c_uint32(0)
        head = C.c_uint8(0)
        self._chk(self._lib.cook_cycle_fetch(self._h, _p(ranked, C.c_uint32), C.byref(n), _p(j2o, C.c_int32),
                                             C.byref(k), C.byref(head)))
        if out is None:
            return ranked[: n.value].copy(), j2o[: k.value].copy(), bool(head.value)
        return ranked[: n.value], j2o[: k.value], bool(head.value)

    # ---- considerable jobs -----------------------------------------------------------------------------------
    def considerable(self, queue: A.Queue, users: A.UserState, num_considerable: int):
        """pending-jobs->considerable-jobs (scheduler.clj:729-762) -> (queue positions, rate_limited per user, passed per user)."""
        out = np.zeros(max(1, min(int(num_considerable), queue.n)), dtype=np.uint32)
        rl = np.zeros(max(1, users.n), dtype=np.uint32)
        ps = np.zeros(max(1, users.n), dtype=np.uint32)
        n = C.c_uint32(0)
        qs, us = queue.as_struct(), users.as_struct()
        self._chk(self._lib.cook_considerable(self._h, C.byref(qs), C.byref(us), int(num_considerable), _p(out, C.c_uint32),
                                              C.byref(n), _p(rl, C.c_uint32), _p(ps, C.c_uint32)))
        return out[: n.value].copy(), rl[: users.n].copy(), ps[: users.n].copy()

    def cycle_set_considerable(self, users: Optional[A.UserState], eligible_by_pending=None):
        el = np.ascontiguousarray(eligible_by_pending, dtype=np.uint8) if eligible_by_pending is not None else None
        us = users.as_struct() if users is not None else None
        self._chk(self._lib.cook_cycle_set_considerable(self._h, C.byref(us) if us is not None else None,
                                                        _p(el, C.c_uint8) if el is not None else None))

    def cycle_fetch_considerable(self):
        out = np.zeros(max(1, self._rank_np), dtype=np.uint32)
        n = C.c_uint32(0)
        self._chk(self._lib.cook_cycle_fetch_considerable(self._h, _p(out, C.c_uint32), C.byref(n)))
        return out[: n.value].copy()

    def cycle_autoscale(self, max_jobs: int = 1000, scale_factor: float = 1.0, offer_skipped=None, exclude_tasks=None):
        """The jobs of the last cycle that get synthetic pods (handle-resource-offers-autoscaling-helper, scheduler.clj:1283-1335;
        cook_cycle_autoscale): -> (task indices of Out in queue order, info dict: considered, matched, unmatched, scaled (N),
        autoscalable (|A|), n_out, fraction_unmatched).  offer_skipped: per staged offer, 1 where the rate limit dropped its
        cluster's matches; exclude_tasks: task indices the host's recent-synthetic-pod cache names."""
        sk = np.ascontiguousarray(offer_skipped, dtype=np.uint8) if offer_skipped is not None else None
        ex = np.ascontiguousarray(exclude_tasks if exclude_tasks is not None else [], dtype=np.uint32)
        p = A.CookAutoscaleParams(int(max_jobs), len(ex), float(scale_factor), _p(sk, C.c_uint8) if sk is not None else None,
                                  _p(ex, C.c_uint32) if len(ex) else None)
        cap = max(int(max_jobs), getattr(self, "_rank_np", 0))  # >= max(max_jobs, K)
        out = np.zeros(max(1, cap), dtype=np.uint32)
        info = A.CookAutoscaleInfo()
        self._chk(self._lib.cook_cycle_autoscale(self._h, C.byref(p), _p(out, C.c_uint32), cap, C.byref(info)))
        return out[: info.n_out].copy(), info.as_dict()

    def cycle_set_job_hashes(self, hashes, first: int = 0):
        """Rows [first, first + len(hashes)) of the engine's (hash uuid) column by pending ordinal (cook_cycle_set_job_hashes; A.uuid_hash
        gives a java.util.UUID's value).  After a cycle_update: first = the kept pending count."""
        h = np.ascontiguousarray(hashes, dtype=np.int32)
        self._chk(self._lib.cook_cycle_set_job_hashes(self._h, _p(h, C.c_int32) if len(h) else None, int(first), len(h)))

    def cycle_autoscale_clusters(self, clusters: "A.AutoscaleClusters", max_jobs: int = 1000, scale_factor: float = 1.0, offer_skipped=None,
                                 exclude_tasks=None, cap: Optional[int] = None):
        """cycle_autoscale, then what trigger-autoscaling! does with its result (cook_cycle_autoscale_clusters): the jobs distributed to the
        pool's autoscaling compute clusters and cut per cluster.  -> (launch lists: one array of task indices per cluster, info dict as
        cycle_autoscale's, cluster info: one dict per cluster (assigned, outstanding_removed, max_launchable, launched), no_cluster dict
        (no_cluster, first_tasks))."""
        call = _ClusterCall(self, dict(clusters=clusters, max_jobs=max_jobs, scale_factor=scale_factor, offer_skipped=offer_skipped,
                                       exclude_tasks=exclude_tasks, cap=cap))
        self._chk(self._lib.cook_cycle_autoscale_clusters(self._h, C.byref(call.p), C.byref(call.cl), _p(call.out, C.c_uint32), call.cap,
                                                          _p(call.off, C.c_uint32), C.byref(call.info), call.cinfo, C.byref(call.none)))
        return call.result()

    def sweep_running(self, start_ms, now_ms: int, default_timeout_ms: int = 0, max_timeout_ms: int = 0, what: int = A.SWEEP_ALL,
                      unknown=None, max_runtime_ms=None, cancelled=None, group=None, groups: Optional[dict] = None, cap: Optional[int] = None):
        """The three task killers over the running set (cook_sweep_running): lingering (get-lingering-tasks), stragglers (find-stragglers
        :quantile-deviation) and cancelled (killable-cancelled-tasks).  Per running row: start_ms (A.START_ABSENT = none), unknown,
        max_runtime_ms (< 0 = none), cancelled, group (index into `groups` or A.NONE_U32).  groups: dict of the per-group columns type,
        quantile, multiplier, job_count and the successful instances as succ_off (CSR, n + 1), succ_start_ms, succ_end_ms (< 0 = none).
        -> dict(reason [n] uint8 bits, lingering / stragglers / cancelled: row indices ascending, threshold_s [groups] float64 (NaN: not
        ready or not type 1), info)."""
        keep = []

        def arr(x, dt):
            if x is None:
                return None
            a = np.ascontiguousarray(x, dtype=dt)
            keep.append(a)
            return a

        def ptr(a, t):
            return _p(a, t) if a is not None and len(a) else None

        st = arr(start_ms, np.int64)
        n = len(st)
        cols = [arr(unknown, np.uint8), arr(max_runtime_ms, np.int64), arr(cancelled, np.uint8), arr(group, np.uint32)]
        assert all(c is None or len(c) == n for c in cols), "every running-set column has n entries"
        ts = A.CookRunningSet(n, ptr(st, C.c_int64), ptr(cols[0], C.c_uint8), ptr(cols[1], C.c_int64), ptr(cols[2], C.c_uint8),
                              ptr(cols[3], C.c_uint32))
        gs, G = None, 0
        if groups is not None:
            ty = arr(groups["type"], np.uint8)
            G = len(ty)
            off = arr(groups.get("succ_off", np.zeros(G + 1)), np.uint32)
            gs = A.CookStragglerGroups(G, ptr(ty, C.c_uint8), ptr(arr(groups["quantile"], np.float64), C.c_double),
                                       ptr(arr(groups["multiplier"], np.float64), C.c_double), ptr(arr(groups["job_count"], np.uint32), C.c_uint32),
                                       ptr(off, C.c_uint32), ptr(arr(groups.get("succ_start_ms", []), np.int64), C.c_int64),
                                       ptr(arr(groups.get("succ_end_ms", []), np.int64), C.c_int64))
        p = A.CookSweepParams(int(now_ms), int(default_timeout_ms), int(max_timeout_ms), int(what), 0)
        cap = 3 * n if cap is None else int(cap)
        reason = np.zeros(max(1, n), dtype=np.uint8)
        idx = np.zeros(max(1, cap), dtype=np.uint32)
        thr = np.zeros(max(1, G), dtype=np.float64)
        info = A.CookSweepInfo()
        rc = self._lib.cook_sweep_running(self._h, C.byref(ts), C.byref(gs) if gs is not None else None, C.byref(p), _p(reason, C.c_uint8),
                                          _p(idx, C.c_uint32), cap, _p(thr, C.c_double), C.byref(info))
        self.last_sweep_info = info.as_dict()  # (filled in on COOK_E_INVALID too: the list lengths, bad_row)
        self._chk(rc)
        L, S = info.lingering, info.stragglers
        return dict(reason=reason[:n].copy(), lingering=idx[:L].copy(), stragglers=idx[L:L + S].copy(),
                    cancelled=idx[L + S:L + S + info.cancelled].copy(), threshold_s=thr[:G].copy(), info=info.as_dict())

    def kube_distribute(self, n_jobs: int, cluster_location, cluster_capacity, location=None, draw=None, seed: int = 0,
                        cap: Optional[int] = None):
        """The distributor of a Kubernetes-scheduler pool (cook_kube_distribute: scheduling-capacity-constrained-job-distributor,
        scheduler.clj:1110-1151) over jobs 0 .. n_jobs-1 in order.  cluster_location / cluster_capacity: per compute cluster, in the
        pool's order (location 0 = none; capacity = cc/max-launchable, int64).  location: per job, 0 = none (None: all 0); draw: per job
        a float64 in [0, 1) (None: generated from `seed`, A.kube_seed_draw).  -> dict(choice [n_jobs] uint8 (A.KUBE_NO_CLUSTER: none),
        lists: one array of job positions per cluster, off [n + 1], cluster_info: one dict per cluster (assigned, capacity), info)."""
        K = int(n_jobs)
        cl_loc = np.ascontiguousarray(cluster_location, dtype=np.uint32)
        cl_cap = np.ascontiguousarray(cluster_capacity, dtype=np.int64)
        n = len(cl_loc)
        assert len(cl_cap) == n, "one capacity per cluster"
        loc = np.ascontiguousarray(location, dtype=np.uint32) if location is not None else None
        dr = np.ascontiguousarray(draw, dtype=np.float64) if draw is not None else None
        assert all(c is None or len(c) >= K for c in (loc, dr)), "every job column has n_jobs entries"
        cl = A.CookKubeClusters(n, 0, _p(cl_loc, C.c_uint32) if n else None, _p(cl_cap, C.c_int64) if n else None)
        cap = K if cap is None else int(cap)
        choice = np.zeros(max(1, K), dtype=np.uint8)
        idx = np.zeros(max(1, cap), dtype=np.uint32)
        off = np.zeros(n + 1, dtype=np.uint32)
        cinfo = (A.CookKubeClusterInfo * max(1, n))()
        info = A.CookKubeInfo()
        rc = self._lib.cook_kube_distribute(self._h, K, _p(loc, C.c_uint32) if loc is not None and K else None,
                                            _p(dr, C.c_double) if dr is not None and K else None, C.c_uint64(int(seed) & (2 ** 64 - 1)), C.byref(cl),
                                            _p(choice, C.c_uint8), _p(idx, C.c_uint32), cap, _p(off, C.c_uint32), cinfo, C.byref(info))
        self.last_kube = dict(choice=choice[:K].copy(), off=off.copy(), cluster_info=[cinfo[c].as_dict() for c in range(n)],
                              info=info.as_dict())  # (filled in on "more than cap" too)
        self._chk(rc)
        return dict(self.last_kube, lists=[idx[off[c]:off[c + 1]].copy() for c in range(n)])

    def cycle_run_kube(self, cluster_location, cluster_capacity, max_jobs_considered: int = 500, min_capacity_threshold: int = 0,
                       rank_first: bool = False, draw=None, seed: int = 0, carry=None, finished=None, cap: Optional[int] = None, **step):
        """A Kubernetes-scheduler pool's cycle (cook_cycle_run_kube: handle-kubernetes-scheduler-pool, scheduler.clj:1747-1810): the gate
        over the clusters' capacities, then a fresh rank (rank_first) or a queue step with every considered job leaving the queue (carry,
        finished and the step's keywords as cycle_run_queue_release takes them), the considerable filters, and the distributor over the
        considered jobs.  -> dict(lists: one array of TASK indices per cluster, off, cluster_info, info); info["paused"] = 1: nothing ran."""
        call = _KubeCall(self, dict(cluster_location=cluster_location, cluster_capacity=cluster_capacity, max_jobs_considered=max_jobs_considered,
                                    min_capacity_threshold=min_capacity_threshold, rank_first=rank_first, draw=draw, seed=seed, carry=carry,
                                    finished=finished, cap=cap, **step))
        rc = self._lib.cook_cycle_run_kube(self._h, C.byref(call.c), _p(call.out, C.c_uint32), call.cap, _p(call.off, C.c_uint32), call.cinfo,
                                           C.byref(call.info))
        self.last_kube = call.result(lists=False)  # (filled in on "more than cap" too)
        self._chk(rc)
        return call.result()

    def cycle_fetch_kube(self) -> np.ndarray:
        """the cluster byte per considered position of the last Kubernetes cycle (A.KUBE_NO_CLUSTER: none)"""
        n = C.c_uint32(0)
        out = np.zeros(max(1, getattr(self, "_rank_np", 0)), dtype=np.uint8)
        self._chk(self._lib.cook_cycle_fetch_kube(self._h, _p(out, C.c_uint8), C.byref(n)))
        return out[: n.value].copy()

    # ---- rebalancer ------------------------------------------------------------------------------------------
    def rebalance_stage(self, running: A.Tasks, pending: A.Jobs, pending_job_id, pending_priority, users: A.Users,
                        spare: A.HostSpare, rparams: A.CookRebalanceParams, host_attrs: Optional[A.Offers] = None,
                        groups: Optional[A.Groups] = None, attrs_cached=None):
        rs, ps, us, ss = running.as_struct(), pending.as_struct(), users.as_struct(), spare.as_struct()
        hs = host_attrs.as_struct() if host_attrs is not None else None
        gs = groups.as_struct() if groups is not None else None
        jid = np.ascontiguousarray(pending_job_id, dtype=np.int64)
        pri = np.ascontiguousarray(pending_priority, dtype=np.int32)
        ck = np.ascontiguousarray(attrs_cached, dtype=np.uint8) if attrs_cached is not None else None
        self._rb_p, self._rb_r, self._rb_resident = pending.n, running.n, False
        self._chk(self._lib.cook_rebalance_stage(
            self._h, C.byref(rs), _p(ck, C.c_uint8) if ck is not None else None, C.byref(ps), _p(jid, C.c_int64),
            _p(pri, C.c_int32), C.byref(us), C.byref(ss), C.byref(hs) if hs is not None else None,
            C.byref(gs) if gs is not None else None, C.byref(rparams)))

    def rebalance_run(self):
        self._chk(self._lib.cook_rebalance_run(self._h))

    def rebalance_fetch(self):
        P, R = self._rb_p, self._rb_r
        if getattr(self, "_rb_resident", False):  # behind cycle_rebalance_stage _rb_p is a bound: the selected count is the engine's
            ns = C.c_uint32(0)
            self._chk(self._lib.cook_cycle_rebalance_fetch(self._h, None, None, None, None, None, None, None, C.byref(ns)))
            cap, P = P, ns.value
            assert P <= cap
        dec = (A.CookPreemption * max(1, P))()
        pre = np.zeros(max(1, R + P), dtype=np.uint32)
        pdru = np.zeros(max(1, P), dtype=np.float64)
        nd, npre = C.c_uint32(0), C.c_uint32(0)
        self._chk(self._lib.cook_rebalance_fetch(self._h, dec, C.byref(nd), _p(pre, C.c_uint32), C.byref(npre),
                                                 _p(pdru, C.c_double)))
        out = []
        for i in range(nd.value):
            d = dec[i]
            out.append(dict(pending_index=d.pending_index, host=d.host, dru=d.dru, cpus=d.cpus, mem=d.mem, gpus=d.gpus,
                            tasks=[int(x) for x in pre[d.task_off: d.task_off + d.task_n]]))
        return dict(decisions=out, pending_dru=pdru[:P].copy(), final=None)

    def rebalance(self, running, pending, pending_job_id, pending_priority, users, spare, rparams, host_attrs=None,
                  groups=None, attrs_cached=None):
        """init-state + the rebalance loop (rebalancer.clj:222-467) -> dict(decisions=[...], pending_dru=array)."""
        self.rebalance_stage(running, pending, pending_job_id, pending_priority, users, spare, rparams, host_attrs,
                             groups, attrs_cached)
        self.rebalance_run()
        return self.rebalance_fetch()

    def rebalance_timing(self) -> float:
        ms = C.c_double(0)
        self._lib.cook_rebalance_timing(self._h, C.byref(ms))
        return ms.value

    # ---- the rebalancer from the pool's resident cycle state ---------------------------------------------------
    def cycle_rebalance_stage(self, rparams: A.CookRebalanceParams, spare: Optional[A.HostSpare] = None,
                              host_attrs: Optional[A.Offers] = None, skip_matched: bool = False, offer_skipped=None):
        """cook_cycle_rebalance_stage: the rebalancer's stage built on the device from the resident task table (staged with hosts), the
        standing queue, the pending-job columns, the staged users, groups and offers.  spare / host_attrs None: from the staged offers.
        skip_matched: the jobs the last placement matched and kept do not count as pending (offer_skipped: per offer of that match).
        Then rebalance_run() and cycle_rebalance_fetch()."""
        ss = spare.as_struct() if spare is not None else None
        hs = host_attrs.as_struct() if host_attrs is not None else None
        sk = np.ascontiguousarray(offer_skipped, dtype=np.uint8) if offer_skipped is not None else None
        req = A.CookCycleRebalance(rparams, C.pointer(ss) if ss is not None else None,
                                   C.cast(C.pointer(hs), C.c_void_p) if hs is not None else None,
                                   _p(sk, C.c_uint8) if sk is not None else None, int(skip_matched), 0)
        self._rrb_p = max(0, min(int(rparams.max_preemption), getattr(self, "_rank_np", 0)))
        self._chk(self._lib.cook_cycle_rebalance_stage(self._h, C.byref(req)))
        self._rb_p, self._rb_r, self._rb_resident = self._rrb_p, getattr(self, "_rank_n", 0), True  # (rebalance_fetch behind a resident stage: the compacted spaces)

    def cycle_rebalance_fetch(self) -> dict:
        """cook_cycle_rebalance_fetch -> the dict of rebalance_fetch with `tasks` as rows of the resident task table (NONE_U32 = a job
        placed earlier in this call) and pending_index into the selected list, plus selected_task_idx (task rows, the space of
        cycle_fetch's ranked) and selected_pending_ord (pending ordinals, the key of Reservations) of that list."""
        P, R = self._rrb_p, getattr(self, "_rank_n", 0)
        dec = (A.CookPreemption * max(1, P))()
        pre = np.zeros(max(1, R + P), dtype=np.uint32)
        pdru = np.zeros(max(1, P), dtype=np.float64)
        st, so = np.zeros(max(1, P), dtype=np.uint32), np.zeros(max(1, P), dtype=np.uint32)
        nd, npre, ns = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._chk(self._lib.cook_cycle_rebalance_fetch(self._h, dec, C.byref(nd), _p(pre, C.c_uint32), C.byref(npre), _p(pdru, C.c_double),
                                                       _p(st, C.c_uint32), _p(so, C.c_uint32), C.byref(ns)))
        out = []
        for i in range(nd.value):
            d = dec[i]
            out.append(dict(pending_index=d.pending_index, host=d.host, dru=d.dru, cpus=d.cpus, mem=d.mem, gpus=d.gpus,
                            tasks=[int(x) for x in pre[d.task_off: d.task_off + d.task_n]]))
        n = ns.value
        return dict(decisions=out, pending_dru=pdru[:n].copy(), final=None, selected_task_idx=st[:n].copy(), selected_pending_ord=so[:n].copy())

    def cycle_rebalance(self, rparams: A.CookRebalanceParams, spare: Optional[A.HostSpare] = None, host_attrs: Optional[A.Offers] = None,
                        skip_matched: bool = False, offer_skipped=None) -> dict:
        """stage + run + fetch of the rebalancer over the resident cycle state (at a rank trigger: cycle_update -> cycle ->
        cycle_rebalance -> reservations_of(decisions, pending_ord=...) -> cycle_set_reservations)."""
        self.cycle_rebalance_stage(rparams, spare, host_attrs, skip_matched, offer_skipped)
        self.rebalance_run()
        return self.cycle_rebalance_fetch()

    # ---- consumers of the placement's by-products ----------------------------------------------------------------
    def match_explain(self, job_pos) -> np.ndarray:
        """fenzo-utils/summarize-placement-failure (fenzo_utils.clj:33-55) for the given job positions of the LAST match:
        -> uint32 [n, WHY_SLOTS] host counts (A.why_summary turns a row into the reference's map)."""
        pos = np.ascontiguousarray(job_pos, dtype=np.uint32)
        out = np.zeros((max(1, len(pos)), A.WHY_SLOTS), dtype=np.uint32)
        self._chk(self._lib.cook_match_explain(self._h, _p(pos, C.c_uint32) if len(pos) else None, len(pos),
                                               _p(out.reshape(-1), C.c_uint32)))
        return out[: len(pos)].copy()

    def match_launch_resources(self, offers: A.LaunchOffers, cap: Optional[int] = None, out: Optional[dict] = None) -> dict:
        """The assigned ports and the per-role takes of the placed tasks of the LAST match (cook_match_launch_resources: Fenzo's
        getAssignedPorts and mesos/task.clj's take-resources / take-ports).  -> dict(port_off [K + 1], port [P] int32 ascending per
        task, port_role [P], take [K, n_res, n_roles] float64 (0.0 = no message), short_mask [K], info = dict(kept, ports,
        offers_used, short_tasks, bad_row)).  cap: room for the ports; by default a guess from the job count, and a call the library
        refuses for lack of room alone is made again with the room its info asks for (a refused call has written nothing).  out: a
        dict of these arrays to write into instead of fresh ones (port / port_role of cap entries; cap is then required).  A refused
        call raises CookError with the library's code and message; its .info is the call's cook_launch_info."""
        try:
            K = self.match_count()
        except CookError:
            K = 0  # (no match to size the outputs by: the call itself refuses, with its own message and info)
        assert out is None or cap is not None, "out needs cap"
        total = launch_range_ports(offers)
        guess = cap is None
        if guess:
            cap = min(total, max(4096, 4 * K))
        cap = min(int(cap), 2 ** 32 - 1)
        while True:
            mine = out if out is not None else launch_outputs(K, len(offers.res_source), int(offers.n_roles), cap)
            ro, oo, keep = launch_call_args(offers, mine, cap)
            info = A.CookLaunchInfo()
            rc = self._lib.cook_match_launch_resources(self._h, C.byref(ro), C.byref(oo), C.byref(info))
            del keep
            d = dict(kept=info.kept, ports=info.ports, offers_used=info.offers_used, short_tasks=info.short_tasks, bad_row=info.bad_row)
            if guess and rc == -1 and info.bad_row == A.NONE_U32 and cap < info.ports <= total:  # only the room was short
                cap, guess = int(info.ports), False
                continue
            break
        try:
            self._chk(rc)
        except CookError as err:
            err.info = d
            raise
        P = int(mine["port_off"][K])
        return dict(port_off=mine["port_off"], port=mine["port"][:P], port_role=mine["port_role"][:P], take=mine["take"],
                    short_mask=mine["short_mask"], info=d)

    def match_metrics(self, n_users: int = 0, n_gpu_models: int = 0) -> dict:
        """handle-match-cycle-metrics' numbers (scheduler.clj:1210-1280) for the LAST match."""
        o = _MetricsOut(n_users, n_gpu_models)
        self._chk(self._lib.cook_match_metrics(self._h, C.byref(o.m), _p(o.uc, C.c_uint32) if n_users else None,
                                               _p(o.um, C.c_uint32) if n_users else None, n_users, _p(o.jg, C.c_int64), _p(o.og, C.c_int64),
                                               n_gpu_models))
        return o.result()

    # ---- offer construction from node state --------------------------------------------------------------------
    def offers_stage(self, nodes: A.Nodes, pods: A.Pods, oparams: A.CookOfferParams):
        ns, ps = nodes.as_struct(), pods.as_struct()
        self._of_n, self._of_attr, self._of_params = nodes.n, nodes.n_attr_keys, oparams
        self._chk(self._lib.cook_offers_stage(self._h, C.byref(ns), C.byref(ps), C.byref(oparams)))

    def offers_run(self):
        self._chk(self._lib.cook_offers_run(self._h))

    def offers_fetch(self) -> A.BuiltOffers:
        n, na, op = self._of_n, self._of_attr, self._of_params
        cap = max(1, n)
        gs, ds = max(1, int(op.gpu_slots)), max(1, int(op.disk_slots))
        tab = lambda k, dt: np.zeros(cap, dt) if k == 1 else np.zeros((cap, k), dt)  # noqa: E731
        cols = dict(node=np.zeros(cap, np.uint32), host=np.zeros(cap, np.uint32), cpus=np.zeros(cap), mem=np.zeros(cap),
                    gpu_model=tab(gs, np.uint32), gpu_count=tab(gs, np.float64), disk_type=tab(ds, np.uint32),
                    disk_space=tab(ds, np.float64), num_pods=np.zeros(cap, np.int32))
        attr = np.zeros((cap, na), np.uint32) if na else None
        o = A.CookNodeOffers(_p(cols["node"], C.c_uint32), _p(cols["host"], C.c_uint32), _p(cols["cpus"], C.c_double),
                             _p(cols["mem"], C.c_double), _p(cols["gpu_model"].reshape(-1), C.c_uint32),
                             _p(cols["gpu_count"].reshape(-1), C.c_double), _p(cols["disk_type"].reshape(-1), C.c_uint32),
                             _p(cols["disk_space"].reshape(-1), C.c_double), _p(cols["num_pods"], C.c_int32),
                             _p(attr.reshape(-1), C.c_uint32) if na else None)
        status = np.zeros(cap, np.uint8)
        tot = A.CookOfferTotals()
        gcap, gcons = np.zeros(op.n_gpu_models + 1, np.int64), np.zeros(op.n_gpu_models + 1, np.int64)
        dcap, dcons = np.zeros(op.n_disk_types + 1), np.zeros(op.n_disk_types + 1)
        r = C.c_uint32(0)
        self._chk(self._lib.cook_offers_fetch(self._h, C.byref(o), C.byref(r), _p(status, C.c_uint8), C.byref(tot),
                                              _p(gcap, C.c_int64), _p(gcons, C.c_int64), _p(dcap, C.c_double), _p(dcons, C.c_double)))
        k = r.value
        totals = {f: getattr(tot, f) for f, _ in A.CookOfferTotals._fields_}
        return A.BuiltOffers(attr=attr[:k].copy() if na else None, node_status=status[:n].copy(), totals=totals,
                             gpu_capacity_by_model=gcap, gpu_consumed_by_model=gcons, disk_capacity_by_type=dcap,
                             disk_consumed_by_type=dcons, **{c: v[:k].copy() for c, v in cols.items()})

    def offers_build(self, nodes: A.Nodes, pods: A.Pods, oparams: A.CookOfferParams) -> A.BuiltOffers:
        """generate-offers' numeric core (kubernetes/compute_cluster.clj:68-190): available = capacity - consumption per
        node, the schedulable filter, the offer rows in node order and the capacity / consumption gauges."""
        self.offers_stage(nodes, pods, oparams)
        self.offers_run()
        return self.offers_fetch()

    def match_stage_built_offers(self, jobs: A.Jobs, groups: Optional[A.Groups] = None, reserved_hosts: Sequence[int] = (),
                                 with_task_limits: bool = False):
        """cook_match_stage with the rows of the last offers_run as offers, in place on the device (no host round trip)."""
        js = jobs.as_struct()
        gs = groups.as_struct() if groups is not None else None
        res = np.array(list(reserved_hosts) or [0], dtype=np.uint32)
        self._match_k = jobs.n
        self._chk(self._lib.cook_match_stage_built_offers(self._h, C.byref(js), C.byref(gs) if gs is not None else None,
                                                          _p(res, C.c_uint32), len(reserved_hosts), int(bool(with_task_limits))))

    def cycle_stage_built_offers(self, tasks: A.Tasks, users: A.Users, pending_jobs: A.Jobs, groups: Optional[A.Groups] = None,
                                 reserved_hosts: Sequence[int] = (), with_task_limits: bool = False):
        """cook_cycle_stage with the rows of the last offers_run as offers, in place on the device."""
        ts, us, js = tasks.as_struct(), users.as_struct(), pending_jobs.as_struct()
        self._n_users = users.n
        gs = groups.as_struct() if groups is not None else None
        res = np.array(list(reserved_hosts) or [0], dtype=np.uint32)
        self._rank_n, self._rank_np = tasks.n, int(tasks.pending.sum()) if tasks.n else 0
        self._tasks_n = tasks.n  # the staged table's row count, exactly (unscheduled sizes its outputs by it)
        self._chk(self._lib.cook_cycle_stage_built_offers(self._h, C.byref(ts), C.byref(us), C.byref(js),
                                                          C.byref(gs) if gs is not None else None, _p(res, C.c_uint32),
                                                          len(reserved_hosts), int(bool(with_task_limits))))

    # ---- the resident pod table: a pool whose offers are rebuilt from its pods every cycle -----------------------------
    def offers_stage_pod_ids(self, pod_id, id_cap: int):
        """The staged pods' ids (cook_offers_stage_pod_ids): pod_id[i] names staged pod row i, dense slot numbers below id_cap."""
        ids = np.ascontiguousarray(pod_id, np.uint32)
        self._chk(self._lib.cook_offers_stage_pod_ids(self._h, _p(ids, C.c_uint32) if len(ids) else None, len(ids), int(id_cap)))

    def offers_update(self, delta: A.PodDelta):
        """A pod delta applied to the resident tables on the device (cook_offers_update): see A.PodDelta for the order rule."""
        st, keep = delta.as_struct()
        self._chk(self._lib.cook_offers_update(self._h, C.byref(st)))
        del keep

    def offers_update_info(self) -> dict:
        """The counts of the last pod delta (cook_offers_update_info)."""
        out = A.CookPodDeltaInfo()
        self._chk(self._lib.cook_offers_update_info(self._h, C.byref(out)))
        return {k: int(getattr(out, k)) for k, _ in A.CookPodDeltaInfo._fields_}

    def offers_fetch_pods(self, rows: Optional[A.PodRows] = None) -> A.PodRows:
        """The pod table as it stands, list order (cook_offers_fetch_pods).  rows None: sized by the table."""
        probe = A.CookPodRows()  # cap 0: the call reports n (and refuses cap < n without a synchronisation)
        rc = self._lib.cook_offers_fetch_pods(self._h, C.byref(probe))
        if rc != 0 and probe.n == 0:
            self._chk(rc)
        if rows is None:
            rows = A.PodRows(probe.n)
        self._chk(self._lib.cook_offers_fetch_pods(self._h, C.byref(rows.struct)))
        return rows

    def cycle_set_built_offers(self, with_task_limits: bool = False):
        """The rows of the last offers_run become the staged offers of the cycle in place (cook_cycle_set_built_offers); the next cycle
        is a rank cycle."""
        self._chk(self._lib.cook_cycle_set_built_offers(self._h, int(bool(with_task_limits))))

    def cycle_run_queue_pods(self, num_considerable: int, carry: Optional[A.QueueCarry] = None, finished: Optional[A.Finished] = None,
                             pods: Optional[A.PodDelta] = None, reservations: Optional[A.Reservations] = None,
                             with_task_limits: bool = False, **step):
        """A queue cycle of a pool whose offers are built from its pods (cook_cycle_run_queue_pods): cycle_run_queue_reserve without a
        host churn; behind the parts that read the old rows the pod delta is applied (None: none), the offers are rebuilt from the
        resident tables and become the staged offers, then considerable -> take K -> match."""
        st, keep = self._queue_step(**step)
        built = [p.as_struct() if p is not None else (None, None) for p in (carry, finished, pods, reservations)]
        self._chk(self._lib.cook_cycle_run_queue_pods(self._h, C.byref(st), *[C.byref(s) if s is not None else None for s, _ in built],
                                                      int(bool(with_task_limits)), int(num_considerable)))
        del keep, built

    def offers_timing(self) -> float:
        ms = C.c_double(0)
        self._lib.cook_offers_timing(self._h, C.byref(ms))
        return ms.value

    # ---- measurement -----------------------------------------------------------------------------------------
    def last_timing(self):
        r, m = C.c_double(0), C.c_double(0)
        self._lib.cook_last_timing(self._h, C.byref(r), C.byref(m))
        return r.value, m.value

    def match_stats(self):
        out = (C.c_uint32 * 64)()
        n = self._lib.cook_match_stats_ex(self._h, out, 64)
        keys = ("rounds", "matched", "stop_list", "stop_full", "stop_group", "stop_window", "segments", "resolved", "setup_us", "seq_us", "touched", "visited",
                "_12", "_13", "_14", "_15", "trunc_lists", "served_mode", "served_pools", "serve_iterations", "serve_empty_iterations",
                "serve_pool_windows", "serve_latch_wait_us", "served_fell_back", "serve_streams", "guard_hits", "update_us", "update_sync_us", "update_allocs", "update_slowest_phase", "update_slowest_phase_us", "queue_advance_us",
                "rank_batch_pools", "rank_batch_launches", "rank_batch_grouped_launches", "rank_batch_single_ops", "rank_batch_syncs",
                "placement_form", "classfit_refused", "spreader_serial_calls", "cf_walked", "cf_matched", "cf_overlay_wins", "cf_opened", "cf_opened_full", "cf_gpu_places", "cf_epochs",
                "cf_scans", "cf_exact_turns", "cf_retightened", "_50", "cf_batches", "cf_dead_lanes", "cf_ticks", "cf_ticks_prologue", "cf_ticks_epochs", "cf_ticks_books",
                "cf_spins", "cf_ticks_walk", "cf_ticks_phase1", "cf_rewinds", "cf_flips", "cf_hwid_decider", "cf_hwid_books")
        return {k: int(x) for k, x in zip(keys, out[:max(0, n)]) if not k.startswith("_")}

    def batch_stats(self) -> dict:
        """the last pool batch this engine led, whatever call made it (cook_batch_stats); all zeros before any"""
        out = (C.c_uint32 * 5)()
        self._chk(self._lib.cook_batch_stats(self._h, out))
        return dict(zip(("pools", "launches", "grouped_launches", "singles", "syncs"), (int(x) for x in out)))

    def set_profiling(self, on: bool):
        self._lib.cook_set_profiling(self._h, int(bool(on)))

    def kernel_timings(self):
        cap = 128
        names = (C.c_char_p * cap)()
        ms = (C.c_double * cap)()
        launches = (C.c_uint32 * cap)()
        n = self._lib.cook_kernel_timings(self._h, names, ms, launches, cap)
        return {names[i].decode(): (ms[i], launches[i]) for i in range(max(0, n))}


class _MetricsOut:
    """the output buffers of one engine's cook_match_metrics"""

    def __init__(self, n_users: int, n_gpu_models: int):
        self.n_users, self.n_gpu_models = int(n_users), int(n_gpu_models)
        self.m = A.CookCycleMetrics()
        self.uc = np.zeros(max(1, self.n_users), np.uint32)
        self.um = np.zeros(max(1, self.n_users), np.uint32)
        self.jg = np.zeros(self.n_gpu_models + 1, np.int64)
        self.og = np.zeros(self.n_gpu_models + 1, np.int64)

    def req(self) -> A.CookMetricsReq:
        return A.CookMetricsReq(C.pointer(self.m), _p(self.uc, C.c_uint32) if self.n_users else None,
                                _p(self.um, C.c_uint32) if self.n_users else None, self.n_users, self.n_gpu_models, _p(self.jg, C.c_int64),
                                _p(self.og, C.c_int64))

    def result(self) -> dict:
        m, n = self.m, self.n_users
        return dict(considerable=m.considerable, matched=m.matched, unmatched=m.unmatched, offers=m.offers,
                    offers_scheduled=m.offers_scheduled, head_matched=bool(m.head_matched), jobs=m.jobs.as_dict(),
                    offers_stats=m.offer_stats.as_dict(), user_considerable=self.uc[:n].copy(), user_matched=self.um[:n].copy(),
                    job_gpus_by_model=self.jg, offer_gpus_by_model=self.og)


class PinnedArena:
    """numpy arrays in page-locked host memory (cook_host_alloc): copies to and from the device run at link speed.  The
    arena owns the memory; arrays made by it must not outlive it."""

    def __init__(self, lib_path: Optional[str] = None):
        self._lib = load_library(lib_path)
        self._blocks = []

    def empty(self, shape, dtype) -> np.ndarray:
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) if np.ndim(shape) else int(shape)
        nbytes = max(1, n * dt.itemsize)
        p = self._lib.cook_host_alloc(nbytes)
        if not p:
            raise MemoryError("cook_host_alloc failed")
        self._blocks.append(p)
        buf = (C.c_char * nbytes).from_address(p)
        return np.frombuffer(buf, dtype=dt, count=n).reshape(shape)

    def copy(self, a: np.ndarray) -> np.ndarray:
        out = self.empty(a.shape, a.dtype)
        out[...] = a
        return out

    def pin(self, obj):
        """A copy of a dataclass of columns (A.Tasks, A.Jobs, A.Offers, ...) whose numpy arrays live in this arena."""
        import copy as _copy
        import dataclasses
        new = _copy.copy(obj)
        for f in dataclasses.fields(obj):
            v = getattr(obj, f.name)
            if isinstance(v, np.ndarray):
                object.__setattr__(new, f.name, self.copy(np.ascontiguousarray(v)))
        return new

    def close(self):
        for p in self._blocks:
            self._lib.cook_host_free(p)
        self._blocks = []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def rank_pool_usage_multi(engines: Sequence[Engine]):
    """rank_pool_usage of several engines of one device in ONE call (cook_rank_pool_usage_multi: the pools' sums as pool batches, one stream
    synchronisation) -> a list of (count, cpus, mem, gpus) tuples, engines' order."""
    if not engines:
        return []
    arr = (C.c_void_p * len(engines))(*[e._h for e in engines])
    out = (A.CookUsage * len(engines))()
    rc = engines[0]._lib.cook_rank_pool_usage_multi(arr, len(engines), out)
    if rc != 0:
        for e in engines:
            if e._lib.cook_last_error(e._h):
                e._chk(rc)
        engines[0]._chk(rc)
    return [u.as_tuple() for u in out]


class _StatsOut:
    """the output buffers of one cook_user_stats* call"""

    def __init__(self, n, device_ptr):
        self.n, self.device_ptr = n, device_ptr
        self.per_user = np.zeros((max(1, n), 4, 3), dtype=np.float64)
        self.state = np.zeros(max(1, n), dtype=np.uint8)
        self.totals = A.CookUserStatsTotals()

    def args(self):
        pu = C.c_void_p(int(self.device_ptr)) if self.device_ptr is not None else self.per_user.ctypes.data_as(C.c_void_p)
        return pu, int(self.device_ptr is not None), self.state.ctypes.data_as(C.c_void_p), C.byref(self.totals)

    def result(self) -> dict:
        return A.user_stats_result(self.per_user[:self.n] if self.device_ptr is None else None, self.state[:self.n], self.totals)


class _KubeCall:
    """the argument block and output buffers of one engine's cook_cycle_run_kube"""

    def __init__(self, e: "Engine", kw: dict):
        kw = dict(kw)
        self.cl_loc = np.ascontiguousarray(kw.pop("cluster_location"), dtype=np.uint32)
        self.cl_cap = np.ascontiguousarray(kw.pop("cluster_capacity"), dtype=np.int64)
        self.n = n = len(self.cl_loc)
        assert len(self.cl_cap) == n, "one capacity per cluster"
        self.cl = A.CookKubeClusters(n, 0, _p(self.cl_loc, C.c_uint32) if n else None, _p(self.cl_cap, C.c_int64) if n else None)
        mjc = int(kw.pop("max_jobs_considered", 500))
        draw = kw.pop("draw", None)
        self.draw = np.ascontiguousarray(draw, dtype=np.float64) if draw is not None else None
        carry, finished = kw.pop("carry", None), kw.pop("finished", None)
        cap = kw.pop("cap", None)
        thr, rank_first, seed = int(kw.pop("min_capacity_threshold", 0)), bool(kw.pop("rank_first", False)), int(kw.pop("seed", 0))
        n_draw = kw.pop("n_draw", None)
        self.step, self.keep = e._queue_step(**kw) if kw else (None, None)
        self.parts = [p.as_struct() if p is not None else (None, None) for p in (carry, finished)]
        ref = lambda s: C.cast(C.pointer(s), C.c_void_p) if s is not None else None  # noqa: E731
        self.c = A.CookKubeCycle(int(rank_first), mjc, thr, ref(self.step), ref(self.parts[0][0]), ref(self.parts[1][0]), ref(self.cl),
                                 _p(self.draw, C.c_double) if self.draw is not None and len(self.draw) else None,
                                 (len(self.draw) if self.draw is not None else 0) if n_draw is None else int(n_draw), 0, seed & (2 ** 64 - 1))
        self.cap = mjc if cap is None else int(cap)
        self.out = np.zeros(max(1, self.cap), dtype=np.uint32)
        self.off = np.zeros(n + 1, dtype=np.uint32)
        self.cinfo = (A.CookKubeClusterInfo * max(1, n))()
        self.info = A.CookKubeInfo()

    def result(self, lists: bool = True) -> dict:
        r = dict(off=self.off.copy(), cluster_info=[self.cinfo[c].as_dict() for c in range(self.n)], info=self.info.as_dict())
        if lists:
            r["lists"] = [self.out[self.off[c]:self.off[c + 1]].copy() for c in range(self.n)]
        return r


def cycle_run_kube_multi(engines: Sequence["Engine"], calls: Sequence[dict], raise_errors: bool = True):
    """cycle_run_kube of several engines (the Kubernetes-scheduler pools of one device) in ONE call (cook_cycle_run_kube_multi).  calls:
    per engine the keywords of Engine.cycle_run_kube.  -> one result per engine; raise_errors False: (results, codes), a refused engine's
    result as far as the library filled it."""
    n = len(engines)
    cs = [_KubeCall(e, kw) for e, kw in zip(engines, calls)]
    hs = (C.c_void_p * n)(*[e._h for e in engines])
    cyc = (C.c_void_p * n)(*[C.cast(C.pointer(c.c), C.c_void_p) for c in cs])
    outs = (C.c_void_p * n)(*[c.out.ctypes.data for c in cs])
    caps = (C.c_uint32 * n)(*[c.cap for c in cs])
    offs = (C.c_void_p * n)(*[c.off.ctypes.data for c in cs])
    cinfos = (C.c_void_p * n)(*[C.cast(c.cinfo, C.c_void_p) for c in cs])
    infos = (A.CookKubeInfo * n)()
    rcs = (C.c_int * n)()
    rc = engines[0]._lib.cook_cycle_run_kube_multi(hs, n, cyc, outs, caps, offs, cinfos, infos, rcs)
    for c, i in zip(cs, infos):
        c.info = i
    res = [c.result() for c in cs]
    if raise_errors:
        _check_multi(engines, rc)
        return res
    return res, [int(x) for x in rcs]


def launch_range_ports(offers: A.LaunchOffers) -> int:
    """the ports of all ranges of a role view: room that always suffices for Engine.match_launch_resources"""
    b, e = np.asarray(offers.range_begin, np.int64), np.asarray(offers.range_end, np.int64)
    return int(min(np.sum(np.maximum(e - b + 1, 0)), 2 ** 32 - 1))


def launch_outputs(K: int, n_res: int, n_roles: int, cap: int) -> dict:
    """fresh output arrays of cook_match_launch_resources for K considered jobs and cap ports"""
    return dict(port_off=np.zeros(K + 1, np.uint32), port=np.empty(max(1, cap), np.int32), port_role=np.empty(max(1, cap), np.uint8),
                take=np.zeros((K, n_res, n_roles)), short_mask=np.zeros(K, np.uint32))


def launch_call_args(offers: A.LaunchOffers, out: dict, cap: int):
    """-> (CookLaunchOffers, CookLaunchOut, the arrays their pointers refer to) for cook_match_launch_resources"""
    o = offers
    n, n_roles = int(o.n), int(o.n_roles)
    src = np.ascontiguousarray(o.res_source, dtype=np.uint32)
    n_res = len(src)
    roff = np.ascontiguousarray(o.range_off, dtype=np.uint32)
    rb, re_ = np.ascontiguousarray(o.range_begin, dtype=np.int32), np.ascontiguousarray(o.range_end, dtype=np.int32)
    rr = np.ascontiguousarray(o.range_role, dtype=np.uint8)
    avail = np.ascontiguousarray(o.avail, dtype=np.float64)
    assert len(roff) == n + 1 and len(rb) == len(re_) == len(rr) and avail.size == n_res * n_roles * n
    skipped = np.ascontiguousarray(o.offer_skipped, dtype=np.uint8) if o.offer_skipped is not None else None
    assert skipped is None or len(skipped) == n
    for key in ("port_off", "port", "port_role", "take", "short_mask"):
        assert out[key].flags["C_CONTIGUOUS"], key
    pn = lambda a, t: _p(a.reshape(-1), t) if a.size else None  # noqa: E731
    ro = A.CookLaunchOffers(n, n_roles, n_res, 0, _p(roff, C.c_uint32), pn(rb, C.c_int32), pn(re_, C.c_int32), pn(rr, C.c_uint8),
                            pn(src, C.c_uint32), pn(avail, C.c_double), _p(skipped, C.c_uint8) if skipped is not None else None)
    oo = A.CookLaunchOut(int(cap), 0, _p(out["port_off"], C.c_uint32), _p(out["port"], C.c_int32), _p(out["port_role"], C.c_uint8),
                         pn(out["take"], C.c_double), pn(out["short_mask"], C.c_uint32))
    return ro, oo, (roff, rb, re_, rr, src, avail, skipped, out)


def _check_multi(engines, rc):
    if rc != 0:
        for e in engines:  # the message is with the engine that failed
            if e._lib.cook_last_error(e._h):
                e._chk(rc)
        engines[0]._chk(rc)


def user_stats_multi(engines: Sequence[Engine], limits: A.UserLimits, user_maps: Optional[Sequence[Optional[np.ndarray]]] = None,
                     per_user_device_ptr: Optional[int] = None) -> dict:
    """user_stats of a quota group whose member pools are `engines` (one device; cook_user_stats_multi): user_maps[i] maps engine i's
    user ids one-to-one into the group's limits.n users (None: the identity); per-user sums run over the pools' segments in the
    engines' order."""
    n = limits.n
    lim = limits.as_struct()
    arr = (C.c_void_p * len(engines))(*[e._h for e in engines])
    maps = None
    if user_maps is not None:
        ms = [np.ascontiguousarray(m, dtype=np.uint32) if m is not None else None for m in user_maps]
        assert len(ms) == len(engines)
        maps = (C.c_void_p * len(engines))(*[m.ctypes.data if m is not None else None for m in ms])
    out = _StatsOut(n, per_user_device_ptr)
    _check_multi(engines, engines[0]._lib.cook_user_stats_multi(arr, len(engines), maps, n, C.byref(lim), *out.args()))
    return out.result()


def _usage_call(engines, multi, n_users, user_maps, groups, n_groups, users, usage_device_ptr, total_device_ptr, cap_rows):
    """one cook_usage_breakdown* call; a list of users whose rows need more room than cap_rows is asked again with the room it named"""
    lib = engines[0]._lib
    ul = np.ascontiguousarray(users, dtype=np.uint32) if users is not None else None
    n_out = len(ul) if ul is not None else n_users
    stride = 2 if multi else 1
    cap = int(cap_rows) if cap_rows is not None else sum(getattr(e, "_tasks_n", 0) for e in engines)
    arr = (C.c_void_p * len(engines))(*[e._h for e in engines])
    gs = (C.c_void_p * len(engines))(*[g.ctypes.data if g is not None else None for g in groups])
    maps = None
    if user_maps is not None:
        ms = [np.ascontiguousarray(m, dtype=np.uint32) if m is not None else None for m in user_maps]
        assert len(ms) == len(engines)
        maps = (C.c_void_p * len(engines))(*[m.ctypes.data if m is not None else None for m in ms])
    while True:
        boff = np.zeros(n_out + 1, dtype=np.uint32)
        bgroup = np.zeros(max(1, cap), dtype=np.uint32)
        busage = np.zeros((max(1, cap), 4), dtype=np.float64) if usage_device_ptr is None else None
        roff = np.zeros(cap + 1, dtype=np.uint32)
        rows = np.zeros((max(1, cap), stride), dtype=np.uint32)
        total = np.zeros((max(1, n_out), 4), dtype=np.float64) if total_device_ptr is None else None
        out = A.CookUsageOut(cap_rows=cap, bucket_usage_is_device=int(busage is None), total_is_device=int(total is None),
                             bucket_off=_p(boff, C.c_uint32), bucket_group=_p(bgroup, C.c_uint32),
                             bucket_usage=C.cast(C.c_void_p(int(usage_device_ptr)), A._f64p) if busage is None else _p(busage, C.c_double),
                             row_off=_p(roff, C.c_uint32), rows=_p(rows, C.c_uint32),
                             total=C.cast(C.c_void_p(int(total_device_ptr)), A._f64p) if total is None else _p(total, C.c_double))
        # (an empty list of users still is a list: numpy's pointer to an empty array is not NULL)
        up = ul.ctypes.data_as(C.c_void_p) if ul is not None else None
        if multi:
            rc = lib.cook_usage_breakdown_multi(arr, len(engines), maps, n_users, gs, int(n_groups), up, n_out if ul is not None else 0, C.byref(out))
        else:
            rc = lib.cook_usage_breakdown(engines[0]._h, gs[0], int(n_groups), up, n_out if ul is not None else 0, C.byref(out))
        if rc != 0 and cap_rows is None and usage_device_ptr is None and out.n_rows > cap:
            cap = out.n_rows
            continue
        _check_multi(engines, rc)
        break
    B, R = out.n_buckets, out.n_rows
    return dict(bucket_off=boff, bucket_group=bgroup[:B], bucket_usage=busage[:B] if busage is not None else None, row_off=roff[:B + 1],
                rows=rows[:R] if multi else rows[:R, 0], total=total[:n_out] if total is not None else None)


def usage_breakdown_multi(engines: Sequence[Engine], n_users: int, groups: Optional[Sequence[Optional[np.ndarray]]] = None, n_groups: int = 0,
                          user_maps: Optional[Sequence[Optional[np.ndarray]]] = None, users=None, usage_device_ptr: Optional[int] = None,
                          total_device_ptr: Optional[int] = None, cap_rows: Optional[int] = None) -> dict:
    """GET /usage without a pool, over the pools `engines` of one device (cook_usage_breakdown_multi): groups[i] is engine i's
    group_of_row (None: ungrouped), the ids one id space over the engines; user_maps as in user_stats_multi.  The dict of
    Engine.usage_breakdown, with rows [R, 2] = (engine index, task row)."""
    gs = [None] * len(engines) if groups is None else [np.ascontiguousarray(g, dtype=np.uint32) if g is not None else None for g in groups]
    assert len(gs) == len(engines)
    for e, g in zip(engines, gs):
        assert g is None or len(g) == getattr(e, "_tasks_n", len(g)), "group_of_row has one id per task row"
    return _usage_call(list(engines), True, int(n_users), user_maps, gs, n_groups, users, usage_device_ptr, total_device_ptr, cap_rows)


def cycle_run_rank_multi(engines: Sequence[Engine], num_considerable, user_usage_ptrs: Optional[Sequence[int]] = None,
                         n_users: int = 0):
    """cycle_run_rank of several engines (pools of one rank, same device) in ONE call: the pools' rank flows side by side on one stream,
    the same kernel of several pools in one launch (cook_cycle_run_rank_multi; same results as the calls one by one).
    num_considerable: one K for all, or one per engine.  user_usage_ptrs: device addresses of one [U, 3] float64 buffer per engine -> rank_user_usage(device_ptr=...) of each, in the same
    call; n_users > 0 without pointers: the usage comes back as a list of [U, 3] host arrays."""
    if not engines:
        return None
    lib = engines[0]._lib
    arr = (C.c_void_p * len(engines))(*[e._h for e in engines])
    ks = [int(num_considerable)] * len(engines) if np.isscalar(num_considerable) else [int(k) for k in num_considerable]
    assert len(ks) == len(engines)
    ks = (C.c_uint32 * len(engines))(*[min(k, 0xFFFFFFFF) for k in ks])
    outs = None
    if user_usage_ptrs is not None:
        uu = (C.c_void_p * len(engines))(*[C.c_void_p(int(p)) for p in user_usage_ptrs])
        rc = lib.cook_cycle_run_rank_multi(arr, len(engines), ks, uu, 1)
    elif n_users:
        outs = [np.zeros((max(1, n_users), 3), dtype=np.float64) for _ in engines]
        uu = (C.c_void_p * len(engines))(*[o.ctypes.data for o in outs])
        rc = lib.cook_cycle_run_rank_multi(arr, len(engines), ks, uu, 0)
    else:
        rc = lib.cook_cycle_run_rank_multi(arr, len(engines), ks, None, 0)
    if rc != 0:
        for e in engines:  # the message is with the engine whose flow failed
            if e._lib.cook_last_error(e._h):
                e._chk(rc)
        engines[0]._chk(rc)
    return [o[:n_users] for o in outs] if outs is not None else None


def _queue_call_multi(name: str, engines, num_considerable, steps, *parts):
    """One queue cycle of several engines through the C entry `name`: per engine the step's keywords (or None), then one list per part
    that entry takes, in ABI order (carries, finished, hosts, reservations; a list None: that part for no pool)."""
    if not engines:
        return
    n = len(engines)
    arr = (C.c_void_p * n)(*[e._h for e in engines])
    ks = [int(num_considerable)] * n if np.isscalar(num_considerable) else [int(k) for k in num_considerable]
    assert len(ks) == n
    ks = (C.c_uint32 * n)(*[min(k, 0xFFFFFFFF) for k in ks])
    steps, *parts = [list(x) if x is not None else [None] * n for x in (steps, *parts)]
    assert len(steps) == n and all(len(ps) == n for ps in parts)
    built = [[e._queue_step(**(s or {})) for e, s in zip(engines, steps)]]
    built += [[p.as_struct() if p is not None else (None, None) for p in ps] for ps in parts]
    ptrs = [(C.c_void_p * n)(*[C.addressof(st) if st is not None else None for st, _ in b]) for b in built]
    _check_multi(engines, getattr(engines[0]._lib, name)(arr, n, *ptrs, ks))


def cycle_run_queue_multi(engines: Sequence[Engine], num_considerable, steps: Optional[Sequence[Optional[dict]]] = None):
    """cycle_run_queue_rank of several engines (pools of one device) in ONE call (cook_cycle_run_queue_multi); cycle_match_multi places
    them.  steps: per engine None or the keywords of Engine.cycle_run_queue (offer_skipped, remove_mode, offers, groups)."""
    _queue_call_multi("cook_cycle_run_queue_multi", engines, num_considerable, steps)


def cycle_run_queue_carry_multi(engines: Sequence[Engine], num_considerable, steps: Optional[Sequence[Optional[dict]]] = None,
                                carries: Optional[Sequence[Optional[A.QueueCarry]]] = None):
    """cycle_run_queue_multi with one carry per engine (cook_cycle_run_queue_carry_multi; None: no carry for that pool); cycle_match_multi
    places them.  A pool whose step or carry is refused stays as it was and raises after the others have gone on."""
    _queue_call_multi("cook_cycle_run_queue_carry_multi", engines, num_considerable, steps, carries)


def cycle_run_queue_release_multi(engines: Sequence[Engine], num_considerable, steps: Optional[Sequence[Optional[dict]]] = None,
                                  carries: Optional[Sequence[Optional[A.QueueCarry]]] = None,
                                  finished: Optional[Sequence[Optional[A.Finished]]] = None):
    """cycle_run_queue_carry_multi with one list of finished tasks per engine (cook_cycle_run_queue_release_multi; None: no release for
    that pool); cycle_match_multi places them.  A pool whose step, carry or list is refused stays as it was and raises after the
    others have gone on."""
    _queue_call_multi("cook_cycle_run_queue_release_multi", engines, num_considerable, steps, carries, finished)


def cycle_run_queue_hosts_multi(engines: Sequence[Engine], num_considerable, steps: Optional[Sequence[Optional[dict]]] = None,
                                carries: Optional[Sequence[Optional[A.QueueCarry]]] = None,
                                finished: Optional[Sequence[Optional[A.Finished]]] = None,
                                hosts: Optional[Sequence[Optional[A.HostChurn]]] = None):
    """cycle_run_queue_release_multi with one host churn per engine (cook_cycle_run_queue_hosts_multi; None: no churn for that pool);
    cycle_match_multi places them.  A pool whose step, carry, list or churn is refused stays as it was and raises after the others
    have gone on."""
    _queue_call_multi("cook_cycle_run_queue_hosts_multi", engines, num_considerable, steps, carries, finished, hosts)


def cycle_run_queue_reserve_multi(engines: Sequence[Engine], num_considerable, steps: Optional[Sequence[Optional[dict]]] = None,
                                  carries: Optional[Sequence[Optional[A.QueueCarry]]] = None,
                                  finished: Optional[Sequence[Optional[A.Finished]]] = None,
                                  hosts: Optional[Sequence[Optional[A.HostChurn]]] = None,
                                  reservations: Optional[Sequence[Optional[A.Reservations]]] = None):
    """cycle_run_queue_hosts_multi with one cook_reservations per engine (cook_cycle_run_queue_reserve_multi; None: none for that
    pool); cycle_match_multi places them.  A pool whose step is refused stays as it was and raises after the others have gone on."""
    _queue_call_multi("cook_cycle_run_queue_reserve_multi", engines, num_considerable, steps, carries, finished, hosts, reservations)


def cycle_run_queue_pods_multi(engines: Sequence[Engine], num_considerable, steps: Optional[Sequence[Optional[dict]]] = None,
                               carries: Optional[Sequence[Optional[A.QueueCarry]]] = None,
                               finished: Optional[Sequence[Optional[A.Finished]]] = None,
                               pods: Optional[Sequence[Optional[A.PodDelta]]] = None,
                               reservations: Optional[Sequence[Optional[A.Reservations]]] = None, with_task_limits=False):
    """cycle_run_queue_pods of several engines in ONE call (cook_cycle_run_queue_pods_multi), the pools one after another, each placement
    deferred to cycle_match_multi.  A pool that is refused stays as it was and raises after the others have gone on."""
    if not engines:
        return
    n = len(engines)
    arr = (C.c_void_p * n)(*[e._h for e in engines])
    ks = [int(num_considerable)] * n if np.isscalar(num_considerable) else [int(k) for k in num_considerable]
    ks = (C.c_uint32 * n)(*[min(k, 0xFFFFFFFF) for k in ks])
    wl = [bool(with_task_limits)] * n if np.isscalar(with_task_limits) else list(with_task_limits)
    wl = (C.c_int32 * n)(*[int(bool(w)) for w in wl])
    steps, *parts = [list(x) if x is not None else [None] * n for x in (steps, carries, finished, pods, reservations)]
    assert len(steps) == n and all(len(ps) == n for ps in parts)
    built = [[e._queue_step(**(s or {})) for e, s in zip(engines, steps)]]
    built += [[p.as_struct() if p is not None else (None, None) for p in ps] for ps in parts]
    ptrs = [(C.c_void_p * n)(*[C.addressof(st) if st is not None else None for st, _ in b]) for b in built]
    _check_multi(engines, engines[0]._lib.cook_cycle_run_queue_pods_multi(arr, n, *ptrs, wl, ks))


def reservations_of(decisions, pending_ord=None):
    """reserve-hosts!'s filter (rebalancer.clj:419-432) over the cook_preemption rows of cook_rebalance_fetch: -> (pending_index, host)
    arrays of the decisions that preempt more than one task.  decisions: the dicts of Engine.rebalance_fetch (`tasks`: the preempted
    task list), or cook_preemption structs / dicts with task_n.  The NONE_U32 entries count too, as in (count (:task %)).
    pending_ord (optional): the selected_pending_ord of Engine.cycle_rebalance_fetch; the first array then holds pending ordinals,
    the key of Reservations, instead of indices into the selected list."""
    pend, host = [], []
    for d in decisions:
        get = (lambda k, d=d: d[k]) if isinstance(d, dict) else (lambda k, d=d: getattr(d, k))
        task_n = len(d["tasks"]) if isinstance(d, dict) and "task_n" not in d else int(get("task_n"))
        if task_n > 1:
            pend.append(int(get("pending_index")))
            host.append(int(get("host")))
    pend = np.asarray(pend, np.uint32)
    if pending_ord is not None:
        pend = np.asarray(pending_ord, np.uint32)[pend]
    return pend, np.asarray(host, np.uint32)


def cycle_match_multi(engines: Sequence[Engine]):
    """The placements of several engines (pools of one rank, same device) in lockstep rounds: one sequence of launches with
    blockIdx.z = pool instead of one stream of small kernels per pool (cook_cycle_match_multi)."""
    if not engines:
        return
    arr = (C.c_void_p * len(engines))(*[e._h for e in engines])
    lead = engines[0]
    lead._chk(lead._lib.cook_cycle_match_multi(arr, len(engines)))


def _multi_results(engines, rc, codes, results, raise_errors):
    """what the per-pool multi calls return: the engines' results, a CookError (the engine's own code and message) in the place of an engine
    that failed; raise_errors: the first of them is raised instead"""
    out = []
    for e, c, r in zip(engines, codes, results):
        out.append(r() if c == 0 else CookError(c, e._lib.cook_last_error(e._h).decode()))
    if rc != 0 and all(c == 0 for c in codes):  # the whole call was refused: nothing ran
        err = CookError(rc, "the call was refused: a NULL argument or entry, no engine, or an engine named twice")
        if raise_errors:
            raise err
        return [err for _ in engines]
    if raise_errors:
        for r in out:
            if isinstance(r, CookError):
                raise r
    return out


class _ClusterCall:
    """the arguments and outputs of one cook_cycle_autoscale_clusters call, kept alive across it"""

    def __init__(self, e, kw):
        clusters = kw["clusters"]
        self.sk = np.ascontiguousarray(kw["offer_skipped"], dtype=np.uint8) if kw.get("offer_skipped") is not None else None
        self.ex = np.ascontiguousarray(kw["exclude_tasks"] if kw.get("exclude_tasks") is not None else [], dtype=np.uint32)
        max_jobs = int(kw.get("max_jobs", 1000))
        self.p = A.CookAutoscaleParams(max_jobs, len(self.ex), float(kw.get("scale_factor", 1.0)),
                                       _p(self.sk, C.c_uint8) if self.sk is not None else None, _p(self.ex, C.c_uint32) if len(self.ex) else None)
        self.cl, self.keep = clusters.as_struct()
        self.n = clusters.n
        self.cap = int(kw["cap"]) if kw.get("cap") is not None else max(max_jobs, getattr(e, "_rank_np", 0))  # >= max(max_jobs, K)
        self.out = np.zeros(max(1, self.cap), dtype=np.uint32)
        self.off = np.zeros(self.n + 1, dtype=np.uint32)
        self.info = A.CookAutoscaleInfo()
        self.cinfo = (A.CookAutoscaleClusterInfo * max(1, self.n))()
        self.none = A.CookAutoscaleNoCluster()

    def result(self, info=None, none=None):
        info, none = info if info is not None else self.info, none if none is not None else self.none
        lists = [self.out[self.off[c]: self.off[c + 1]].copy() for c in range(self.n)]
        return (lists, info.as_dict(), [self.cinfo[c].as_dict() for c in range(self.n)],
                dict(no_cluster=none.no_cluster, first_tasks=[int(t) for t in none.first_task[: none.n_first]]))


def cycle_autoscale_clusters_multi(engines: Sequence[Engine], calls: Sequence[dict], raise_errors: bool = True) -> list:
    """cycle_autoscale_clusters of several engines (pools of one device) in ONE call (cook_cycle_autoscale_clusters_multi), as
    cycle_autoscale_multi.  calls: per engine the keywords of Engine.cycle_autoscale_clusters (`clusters` required)."""
    n = len(engines)
    if not n:
        return []
    assert len(calls) == n
    cs = [_ClusterCall(e, dict(kw)) for e, kw in zip(engines, calls)]
    arr = (C.c_void_p * n)(*[e._h for e in engines])
    pp = (C.c_void_p * n)(*[C.addressof(c.p) for c in cs])
    clp = (C.c_void_p * n)(*[C.addressof(c.cl) for c in cs])
    tp = (C.c_void_p * n)(*[c.out.ctypes.data for c in cs])
    cp = (C.c_uint32 * n)(*[c.cap for c in cs])
    op = (C.c_void_p * n)(*[c.off.ctypes.data for c in cs])
    cip = (C.c_void_p * n)(*[C.addressof(c.cinfo) for c in cs])
    info = (A.CookAutoscaleInfo * n)()
    none = (A.CookAutoscaleNoCluster * n)()
    codes = (C.c_int * n)()
    rc = engines[0]._lib.cook_cycle_autoscale_clusters_multi(arr, n, pp, clp, tp, cp, op, info, cip, none, codes)
    res = _multi_results(engines, rc, list(codes), [lambda i=i: cs[i].result(info[i], none[i]) for i in range(n)], raise_errors)
    for i, r in enumerate(res):
        if isinstance(r, CookError):
            r.info = info[i].as_dict()
    return res


def cycle_autoscale_multi(engines: Sequence[Engine], calls: Sequence[Optional[dict]], raise_errors: bool = True) -> list:
    """cycle_autoscale of several engines (pools of one device) in ONE call (cook_cycle_autoscale_multi: the pools' flows in one pool batch,
    every stream synchronisation shared).  calls: per engine the keywords of Engine.cycle_autoscale (None: the defaults).  -> per engine
    (task indices, info dict), as Engine.cycle_autoscale.  An engine that fails does not spoil the others: raise_errors=False puts its
    CookError in its place instead of raising it."""
    n = len(engines)
    if not n:
        return []
    calls = [dict(c or {}) for c in calls]
    assert len(calls) == n
    keep, ps, outs, caps = [], [], [], []
    for e, kw in zip(engines, calls):
        sk = np.ascontiguousarray(kw["offer_skipped"], dtype=np.uint8) if kw.get("offer_skipped") is not None else None
        ex = np.ascontiguousarray(kw["exclude_tasks"] if kw.get("exclude_tasks") is not None else [], dtype=np.uint32)
        max_jobs = int(kw.get("max_jobs", 1000))
        ps.append(A.CookAutoscaleParams(max_jobs, len(ex), float(kw.get("scale_factor", 1.0)), _p(sk, C.c_uint8) if sk is not None else None,
                                        _p(ex, C.c_uint32) if len(ex) else None))
        cap = int(kw["cap"]) if kw.get("cap") is not None else max(max_jobs, getattr(e, "_rank_np", 0))  # >= max(max_jobs, K)
        caps.append(cap)
        outs.append(np.zeros(max(1, cap), dtype=np.uint32))
        keep.append((sk, ex))
    arr = (C.c_void_p * n)(*[e._h for e in engines])
    pp = (C.c_void_p * n)(*[C.addressof(p) for p in ps])
    tp = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    cp = (C.c_uint32 * n)(*caps)
    info = (A.CookAutoscaleInfo * n)()
    codes = (C.c_int * n)()
    rc = engines[0]._lib.cook_cycle_autoscale_multi(arr, n, pp, tp, cp, info, codes)
    res = _multi_results(engines, rc, list(codes), [lambda i=i: (outs[i][: info[i].n_out].copy(), info[i].as_dict()) for i in range(n)], raise_errors)
    for i, r in enumerate(res):
        if isinstance(r, CookError):
            r.info = info[i].as_dict()  # (|Out| > cap: the info says how many)
    return res


def match_metrics_multi(engines: Sequence[Engine], n_users=0, n_gpu_models=0, raise_errors: bool = True) -> list:
    """match_metrics of several engines (pools of one device) in ONE call (cook_match_metrics_multi: two stream synchronisations for all of
    them, the same kernel of several pools in one launch).  n_users / n_gpu_models: one value for all, or one per engine (n_users 0: that
    engine's per-user arrays are left out).  -> per engine the dict of Engine.match_metrics; raise_errors as in cycle_autoscale_multi."""
    n = len(engines)
    if not n:
        return []
    nus = [int(n_users)] * n if np.isscalar(n_users) else [int(x) for x in n_users]
    nms = [int(n_gpu_models)] * n if np.isscalar(n_gpu_models) else [int(x) for x in n_gpu_models]
    assert len(nus) == n and len(nms) == n
    outs = [_MetricsOut(u, g) for u, g in zip(nus, nms)]
    reqs = (A.CookMetricsReq * n)(*[o.req() for o in outs])
    arr = (C.c_void_p * n)(*[e._h for e in engines])
    codes = (C.c_int * n)()
    rc = engines[0]._lib.cook_match_metrics_multi(arr, n, reqs, codes)
    return _multi_results(engines, rc, list(codes), [o.result for o in outs], raise_errors)
