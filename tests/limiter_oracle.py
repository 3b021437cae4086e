"""The oracle of the launch-rate limiters (cook_cycle_set_limiters, cook_cycle_set_clock, cook_cycle_limiters_spend): the
token bucket of include/cookmatch.h restated in plain Python over Python ints and floats (IEEE fp64), and the cycles of a pool that
holds such buckets, composed from the frozen oracle.pyoracle calls as tests/carry_oracle.py composes them.  Nothing of the engine
produces an expected value."""
from __future__ import annotations

import dataclasses
import math
from types import SimpleNamespace

import numpy as np

from cook_amd import _abi as A
from oracle import pyoracle
from tests import carry_oracle as CO
from tests import queue_cases as S

PRODUCT_MAX = 2.0 ** 62


# ---- the bucket ----------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Bucket:
    rate: float  # tokens per ms
    bucket: int
    last: int
    tokens: int = 0


def rate_of(per_minute: float) -> float:
    return float(per_minute) / 60000.0


def earn(b: Bucket, t: int) -> Bucket:
    """earn-tokens: a new Bucket (b itself when nothing changes)"""
    t1 = max(int(t), b.last)
    if t1 == b.last:
        return b
    p = float(t1 - b.last) * b.rate
    if p > PRODUCT_MAX:
        p = PRODUCT_MAX
    d = int(p)  # truncation toward zero
    if d == 0:
        return b
    return dataclasses.replace(b, last=t1, tokens=min(b.tokens + d, b.bucket))


def spend(b: Bucket, t: int, w: int) -> Bucket:
    b = earn(b, t)
    if w == 0:
        return b
    return dataclasses.replace(b, tokens=min(b.tokens - int(w), b.bucket))


def time_until(b: Bucket) -> int:
    q = float(-b.tokens) / b.rate
    if q >= PRODUCT_MAX:
        return int(PRODUCT_MAX)
    return max(0, math.ceil(q))


def in_debt(b: Bucket) -> bool:
    return b.tokens < 0


# ---- a pool's cycles -------------------------------------------------------------------------------------------------------------------
def buckets_of(lim: A.Limiters):
    return [Bucket(rate_of(pm), int(bk), int(la), int(tk)) for pm, bk, tk, la in zip(lim.per_minute, lim.bucket, lim.tokens, lim.last_update_ms)]


def cycle(k, *, state=None, eligible=None, now=None, spend_ms=None, offer_skipped=None, remove_mode=0, carry_offers=False, carry_usage=False,
          carry=False, rank=False, set_limiters=None, explicit_spend=None, offers=None):
    """one cycle of a case.  now / spend_ms: cook_cycle_set_clock in front of the cycle (now None: no clock); set_limiters: an A.Limiters
    installed in front of the cycle (False: cook_cycle_set_limiters(NULL)); explicit_spend: (spend_ms, offer_skipped) of a
    cook_cycle_limiters_spend in front of everything else of this cycle; rank: a rank cycle (cycle 0 always is one)"""
    return SimpleNamespace(k=k, state=state, eligible=eligible, now=now, spend_ms=now if spend_ms is None else spend_ms, offer_skipped=offer_skipped,
                           remove_mode=remove_mode, carry_offers=carry_offers, carry_usage=carry_usage, carry=carry, rank=rank,
                           set_limiters=set_limiters, explicit_spend=explicit_spend, offers=offers, tokens_left=None, groups=None)


def _spend_kept(B, last, offer_skipped, t, clock):
    hit = CO.kept(last.j2o, offer_skipped)
    n = np.bincount(last.jobs.user[hit], minlength=len(B)) if hit.any() else np.zeros(len(B), int)
    for u in np.flatnonzero(n):
        b = earn(B[u], t) if clock else B[u]
        B[u] = dataclasses.replace(b, tokens=min(b.tokens - int(n[u]), b.bucket))
    return int((n > 0).sum()), int(n.sum())


def oracle(params, pool, cycles):
    """-> per cycle SimpleNamespace(Q, pos, j2o, head, jobs, rate_limited, passed, tokens, last, until, view, info): tokens / last /
    until the limiter state BEHIND the cycle (None without limiters), view the tokens the filter compared with (what a host driving the
    parent's way uploads as tokens_left)."""
    J = pool.pending_jobs
    Q0, _ = pyoracle.rank(params, pool.tasks, pool.users)
    Q = Q0
    offers, state, eligible, last, out, B, spent = pool.offers, None, None, None, [], None, True
    for c, cy in enumerate(cycles):
        info = dict(earned=0, spent_users=0, in_debt=0, spent=0)
        if cy.explicit_spend is not None:
            info["spent_users"], info["spent"] = _spend_kept(B, last, cy.explicit_spend[1], cy.explicit_spend[0], True)
            spent = True
        if cy.set_limiters is False:
            B = None
        elif cy.set_limiters is not None:
            lim = cy.set_limiters
            if lim.user is None:
                spent = spent or B is None  # (a first install: the host's counts know the launches so far)
                B = buckets_of(lim)
            else:
                for x, u in enumerate(lim.user):
                    B[int(u)] = buckets_of(lim)[x]
        if cy.state is not None:
            state, eligible = cy.state, cy.eligible
        rank_cycle = c == 0 or cy.rank
        if rank_cycle:
            Q = Q0  # (the cases re-rank an unchanged task table: the fresh order again; a rank cycle never spends)
        else:
            hit = CO.kept(last.j2o, cy.offer_skipped)
            if B is not None and not spent:
                info["spent_users"], info["spent"] = _spend_kept(B, last, cy.offer_skipped, cy.spend_ms, cy.now is not None)
            if cy.carry and cy.carry_offers:
                offers = CO.carry_offers(offers, last.jobs, last.j2o, hit)
            if cy.carry and cy.carry_usage:
                state = CO.carry_usage(state, last.jobs, hit, spend=B is None)
            keep = np.ones(len(Q), bool)
            keep[last.pos[np.ones(len(hit), bool) if cy.remove_mode else hit]] = False
            Q = Q[keep]
            if cy.offers is not None:
                offers = cy.offers
        jq, queue = S._queue_of(pool, Q, eligible if state is not None else None)
        view = None
        st = state
        if B is not None and state is not None:
            view = np.array([(earn(b, cy.now) if cy.now is not None else b).tokens for b in B], np.int64)
            st = dataclasses.replace(state, tokens_left=view)
        rl = ps = None
        if st is not None:
            pos, rl, ps = pyoracle.considerable(queue, st, cy.k)
            if B is not None:
                for u in np.flatnonzero(rl + ps):
                    if cy.now is not None:
                        nb = earn(B[u], cy.now)
                        info["earned"] += int(nb is not B[u])
                        B[u] = nb
                info["in_debt"] = sum(in_debt(b) for b in B)
        else:
            pos = np.arange(min(cy.k, len(Q)), dtype=np.uint32)
        jobs = J.take(jq[pos])
        j2o, fail, head = pyoracle.match(params, jobs, offers, pool.groups)
        spent = False
        last = SimpleNamespace(Q=Q, jq=jq, pos=pos, j2o=j2o, head=head, jobs=jobs, offers=offers, state=state, queue=queue, rate_limited=rl, passed=ps,
                               tokens=None if B is None else np.array([b.tokens for b in B], np.int64),
                               last=None if B is None else np.array([b.last for b in B], np.int64),
                               until=None if B is None else np.array([time_until(b) for b in B], np.int64), view=view, info=info)
        out.append(last)
    return out
