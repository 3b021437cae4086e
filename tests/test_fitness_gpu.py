"""cook_params.fitness on the MI355X (-m gpu): the HIP build against tests/fitness_oracle.py at the shipped shapes."""
import pytest

from tests import fitness_cases as FC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd.engine import Engine
    return lambda params: Engine(params, device=0)


def test_known_answer(make_engine):
    FC.check_known_answer(make_engine)


def test_invalid_values(make_engine):
    FC.check_invalid(make_engine)


@pytest.mark.parametrize("algo", FC.ALGOS)
@pytest.mark.parametrize("ge", FC.GOOD_ENOUGH)
@pytest.mark.parametrize("fitness", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("name", FC.POOLS)
def test_parity(make_engine, name, fitness, ge, algo):
    FC.check_parity(make_engine, name, "gpu", fitness, ge, algo)


def test_window_rounds_end_every_way(make_engine):
    FC.check_rounds_end_every_way(make_engine, "gpu")


@pytest.mark.parametrize("fitness", [1, 2, 3, 4, 5])
def test_ports_and_scalars(make_engine, fitness):
    FC.check_parity(make_engine, "ports", "gpu", fitness, 1.0, 2)


@pytest.mark.parametrize("fitness", [1, 2])
def test_touched_set_full(make_engine, fitness):
    FC.check_touched_set_full(make_engine, fitness)


def test_explain_spreader(make_engine):
    FC.check_explain_spreader(make_engine)


@pytest.mark.parametrize("algo", [2, 0])
@pytest.mark.parametrize("fitness", [1, 3])
@pytest.mark.parametrize("kind", FC.CONSTRAINTS)
def test_constraints(make_engine, kind, fitness, algo):
    FC.check_parity(make_engine, "synth", "emu", fitness, 1.0, algo, constraint=kind)


def test_mixed_pools(make_engine):
    FC.check_mixed_pools(make_engine, "gpu")
