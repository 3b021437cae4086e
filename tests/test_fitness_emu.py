"""cook_params.fitness on a machine WITHOUT a GPU: the cook_amd/csrc sources compiled against the SIMT emulator (tests/simt_emu),
against tests/fitness_oracle.py — and that oracle against the frozen one at fitness 0."""
import numpy as np
import pytest

from cook_amd import _abi as A
from oracle import pyoracle
from tests import fitness_cases as FC
from tests import fitness_oracle as FO
from tests import golden_util as G


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd.engine import Engine
    from tests.simt_emu import build_emu
    so = build_emu.build()
    return lambda params: Engine(params, lib_path=so)


def test_known_answer(make_engine):
    FC.check_known_answer(make_engine)


def test_invalid_values(make_engine):
    FC.check_invalid(make_engine)


def test_fitness_names():
    assert [A.fitness_value(n) for n in A.FITNESS_NAMES] == list(range(6))
    assert A.fitness_value("com.netflix.fenzo.plugins.BinPackingFitnessCalculators/cpuBinPacker") == 1
    assert A.default_params(fitness="memorySpreader").fitness == 5
    with pytest.raises(ValueError):
        A.fitness_value("networkBinPacker")


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


# ---- the oracle gate: tests/fitness_oracle.py at fitness 0 IS the frozen oracle — job_to_offer, fail_code and head_matched on every case
# of these test files (both sizes) and on the match cases of tests/golden/ that it supports
_GOLDEN = G.load("match")


@pytest.mark.parametrize("case", _GOLDEN, ids=[c["name"] for c in _GOLDEN])
def test_oracle_gate_golden(case):
    J, O, _, x = G.build_match_all(case)
    if FO.supports(J, O, x["groups"]):  # (test_oracle_gate_golden_coverage counts them)
        p = A.default_params(good_enough_fitness=case["good_enough"], **x["params"])
        assert _same(FO.match(p, J, O, x["groups"], x["reserved"]), pyoracle.match(p, J, O, x["groups"], x["reserved"]))


def test_oracle_gate_golden_coverage():
    n = sum(1 for case in _GOLDEN for J, O, _, x in [G.build_match_all(case)] if FO.supports(J, O, x["groups"]))
    assert n >= 30, n  # (most of the golden vectors carry no gpu / disk request)


def test_oracle_gate_small_cases():
    for jobs, offers in (FC.known_answer()[:2], FC.pinned_case()):
        assert _same(FO.match(A.default_params(), jobs, offers), pyoracle.match(A.default_params(), jobs, offers))


@pytest.mark.parametrize("size", list(FC.SIZES))
@pytest.mark.parametrize("ge", FC.GOOD_ENOUGH)
@pytest.mark.parametrize("name", FC.POOLS + ("ports",))
def test_oracle_gate_pools(name, ge, size):
    p = A.default_params(good_enough_fitness=ge)
    assert _same(FC.want_of(name, size, 0, ge), pyoracle.match(p, *FC.case_inputs(name, size)))


@pytest.mark.parametrize("ge", FC.GOOD_ENOUGH)
@pytest.mark.parametrize("kind", FC.CONSTRAINTS)
def test_oracle_gate_constraints(kind, ge):
    p = A.default_params(good_enough_fitness=ge)
    assert _same(FC.want_of("synth", "emu", 0, ge, kind), pyoracle.match(p, *FC.constraint_case(kind)))


@pytest.mark.parametrize("size", list(FC.SIZES))
@pytest.mark.parametrize("ge", FC.GOOD_ENOUGH)
@pytest.mark.parametrize("fitness", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("name", FC.POOLS)
def test_cases_mean_something(name, fitness, ge, size):
    """on the oracle alone, for the GPU's sizes too: every parity case moves the assignment, places a quarter, leaves a job out"""
    FC.assert_meaningful(name, size, fitness, ge)


@pytest.mark.parametrize("algo", FC.ALGOS)
@pytest.mark.parametrize("ge", FC.GOOD_ENOUGH)
@pytest.mark.parametrize("fitness", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("name", FC.POOLS)
def test_parity(make_engine, name, fitness, ge, algo):
    FC.check_parity(make_engine, name, "emu", fitness, ge, algo)


def test_window_rounds_end_every_way(make_engine):
    FC.check_rounds_end_every_way(make_engine, "emu")


@pytest.mark.parametrize("fitness", [1, 2, 3, 4, 5])
def test_ports_and_scalars(make_engine, fitness):
    FC.check_parity(make_engine, "ports", "emu", fitness, 1.0, 2)


@pytest.mark.parametrize("fitness", [1, 2])
def test_touched_set_full(make_engine, fitness):
    FC.check_touched_set_full(make_engine, fitness)


def test_explain_spreader(make_engine):
    FC.check_explain_spreader(make_engine)


@pytest.mark.parametrize("algo", FC.ALGOS)
@pytest.mark.parametrize("fitness", [1, 3])
@pytest.mark.parametrize("kind", FC.CONSTRAINTS)
def test_constraints(make_engine, kind, fitness, algo):
    FC.check_parity(make_engine, "synth", "emu", fitness, 1.0, algo, constraint=kind)


def test_mixed_pools(make_engine, monkeypatch):
    monkeypatch.setenv("COOK_MATCH_SERVED", "0")  # (the multi-pool placement in its serial form: launches in lockstep)
    FC.check_mixed_pools(make_engine, "emu")
