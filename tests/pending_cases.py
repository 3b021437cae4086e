"""Cases for a placement that was SET UP (cook_cycle_run_rank) and never run, shared by the emulated and the GPU test files.  Not a test module.

An engine's match is in one of four states (cook_engine::Placement, engine.hip): nothing, window rounds set up, class-ordered walk set up,
done.  cook_cycle_match_multi runs what is set up.  Whatever changes the tables a set-up points into — another cycle, cook_cycle_update,
cook_cycle_stage — must leave "nothing" behind, or a later cook_cycle_match_multi runs the old set-up on the new tables.  Every case runs with
match_algo 3 (the set-up is a class-ordered walk) and with match_algo 2 (window rounds), on a pool of a few dozen jobs: the state logic does
not depend on K or M.

Asserted after every stale sequence: the result equals the oracle's for what was actually asked, and match_stats() shows no class-ordered
walk and no window rounds beyond those of the completed cycles."""
import dataclasses

import numpy as np
import pytest

from cook_amd import _abi as A
from cook_amd import synth
from cook_amd.engine import CookError, cycle_match_multi
from oracle import pyoracle

E_STATE = -4  # COOK_E_STATE (cookmatch.h)
ALGOS = [3, 2]
FORM = {3: 3, 2: 0}  # match_algo -> placement_form of a pool the class-ordered form takes
K_ALL = 10 ** 9
# what a placement counts in match_stats(): the window rounds' and the walk's words
COUNTED = ("rounds", "matched", "resolved", "placement_form", "cf_walked", "cf_matched", "cf_batches")


def params(algo):
    return A.default_params(good_enough_fitness=1.0, match_algo=algo)


def small_pool(seed=0x9E0, scale=1):
    """whole cpus, no gpus, no constraints: the class-ordered form takes it"""
    return synth.make_pool(seed=seed, n_pending=40 * scale, n_running=20, n_users=6, n_offers=12 * scale)


def oracle_cycle(p, pool, k=K_ALL):
    ranked, _ = pyoracle.rank(p, pool.tasks, pool.users)
    pend_ord = np.cumsum(pool.tasks.pending) - 1
    j2o, _, head = pyoracle.match(p, pool.pending_jobs.take(pend_ord[ranked[:min(k, len(ranked))]]), pool.offers, pool.groups)
    return ranked, j2o, head


def stage(e, pool):
    e.cycle_stage(pool.tasks, pool.users, pool.pending_jobs, pool.offers, pool.groups)


def full_cycle(engines, pools, p, algo, tag):
    """cycle_run_rank on each, ONE cycle_match_multi: every pool in its form and equal to the oracle -> every engine's statistics"""
    for e in engines:
        e.cycle_run_rank(K_ALL)
    cycle_match_multi(engines)
    stats = []
    for e, pool in zip(engines, pools):
        st = e.match_stats()
        assert st["placement_form"] == FORM[algo], (tag, st["placement_form"])
        ranked, j2o, head = e.cycle_fetch()
        o_ranked, o_j2o, o_head = oracle_cycle(p, pool)
        assert np.array_equal(ranked, o_ranked), tag
        assert np.array_equal(j2o, o_j2o) and head == o_head, tag
        assert (j2o >= 0).sum() > 0, (tag, "the pool places something")
        if algo == 3:
            assert st["cf_walked"] > 0 and st["cf_batches"] == (len(j2o) + 63) // 64, (tag, st)
        else:
            assert st["rounds"] > 0 and st["resolved"] == len(j2o), (tag, st)
        stats.append(st)
    return stats


def counted(e):
    st = e.match_stats()
    return {k: st[k] for k in COUNTED}


def refused(engines, tag):
    """cycle_match_multi answers COOK_E_STATE, and no engine's placement statistics move: nothing ran"""
    before = [counted(e) for e in engines]
    with pytest.raises(CookError) as err:
        cycle_match_multi(engines)
    assert err.value.code == E_STATE, (tag, err.value.code, str(err.value))
    assert [counted(e) for e in engines] == before, (tag, "a refused call ran a placement")
    with pytest.raises(CookError) as ferr:  # the lead's match is "nothing": no result to fetch either
        engines[0].cycle_fetch()
    assert ferr.value.code == E_STATE, (tag, ferr.value.code)


def run_form(make_engine, algo):
    """a complete cycle on the cases' inputs: the set-up of the sequences below really is the intended form"""
    p, pool = params(algo), small_pool()
    with make_engine(p) as e:
        stage(e, pool)
        full_cycle([e], [pool], p, algo, f"form, match_algo {algo}")


def run_then_empty_cycle(make_engine, algo):
    """1. set up, not run; a cycle with num_considerable = 0; cycle_match_multi: success, nothing considered, nothing matched, head_matched,
    not the class-ordered form, no round and no walk"""
    p, pool = params(algo), small_pool()
    with make_engine(p) as e:
        stage(e, pool)
        e.cycle_run_rank(K_ALL)  # set up
        e.cycle_run_rank(0)
        cycle_match_multi([e])
        ranked, j2o, head = e.cycle_fetch()
        st = e.match_stats()
        assert np.array_equal(ranked, oracle_cycle(p, pool)[0])
        assert len(j2o) == 0 and head is True, (len(j2o), head)
        assert st["placement_form"] != 3 and st["rounds"] == 0 and st["matched"] == 0 and st["resolved"] == 0, st
        assert st["cf_walked"] == 0 and st["cf_batches"] == 0, st
        full_cycle([e], [pool], p, algo, "the cycle behind the empty one")


def run_then_update(make_engine, algo):
    """2. set up, not run; cook_cycle_update with a delta that removes one offer; cycle_match_multi: COOK_E_STATE; the next full cycle equals
    the oracle on the updated cluster"""
    p, pool = params(algo), small_pool()
    o = pool.offers  # (synth's columns without gpus and constraints; offer 0 leaves)
    fewer = dataclasses.replace(pool, offers=A.Offers(cpus=o.cpus[1:], mem=o.mem[1:], host=o.host[1:], k8s=o.k8s[1:], run_cpus=o.run_cpus[1:],
                                                      run_mem=o.run_mem[1:], run_count=o.run_count[1:]))
    with make_engine(p) as e:
        stage(e, pool)
        e.cycle_run_rank(K_ALL)  # set up
        e.cycle_update(offers=fewer.offers)
        refused([e], f"update, match_algo {algo}")
        full_cycle([e], [fewer], p, algo, f"the cycle behind the update, match_algo {algo}")


def run_then_stage(make_engine, algo):
    """3. set up, not run; cook_cycle_stage of a pool with twice as many jobs and offers (its columns need larger buffers);
    cycle_match_multi: COOK_E_STATE; the next full cycle equals the oracle"""
    p, pool, twice = params(algo), small_pool(), small_pool(seed=0x9E1, scale=2)
    with make_engine(p) as e:
        stage(e, pool)
        e.cycle_run_rank(K_ALL)  # set up
        stage(e, twice)
        refused([e], f"stage, match_algo {algo}")
        full_cycle([e], [twice], p, algo, f"the cycle behind the stage, match_algo {algo}")


def run_one_of_two_not_set_up(make_engine, algo):
    """4. two engines, one set up, one staged only; cycle_match_multi of both: COOK_E_STATE, and the first engine's set-up is intact —
    cycle_run_rank on the second, cycle_match_multi of both: both equal the oracle"""
    p, pools = params(algo), [small_pool(), small_pool(seed=0x9E2)]
    e0, e1 = make_engine(p), make_engine(p)
    try:
        stage(e0, pools[0]), stage(e1, pools[1])
        e0.cycle_run_rank(K_ALL)  # set up
        before = counted(e0), counted(e1)
        with pytest.raises(CookError) as err:
            cycle_match_multi([e0, e1])
        assert err.value.code == E_STATE, (err.value.code, str(err.value))
        assert (counted(e0), counted(e1)) == before
        e1.cycle_run_rank(K_ALL)
        cycle_match_multi([e0, e1])  # (e0 places the set-up it was left with)
        for e, pool in zip((e0, e1), pools):
            st = e.match_stats()
            assert st["placement_form"] == FORM[algo], st["placement_form"]
            ranked, j2o, head = e.cycle_fetch()
            o_ranked, o_j2o, o_head = oracle_cycle(p, pool)
            assert np.array_equal(ranked, o_ranked) and np.array_equal(j2o, o_j2o) and head == o_head
    finally:
        e0.close(), e1.close()


SEQUENCES = {"empty_cycle": run_then_empty_cycle, "update": run_then_update, "stage": run_then_stage, "one_of_two": run_one_of_two_not_set_up}
