"""A placement that was set up and never run (tests/pending_cases.py), on the GPU: the form of the set-up, then the four sequences that must
not leave it behind, each with match_algo 3 and 2.  No CPU fallback: without the library or the GPU these tests FAIL."""
import pytest

from cook_amd.engine import Engine
from tests import pending_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd import build
    so = build.build()
    return lambda params: Engine(params, lib_path=so)


@pytest.mark.parametrize("algo", S.ALGOS)
def test_set_up_form(make_engine, algo):
    S.run_form(make_engine, algo)


@pytest.mark.parametrize("algo", S.ALGOS)
@pytest.mark.parametrize("name", list(S.SEQUENCES))
def test_no_stale_placement(make_engine, name, algo):
    S.SEQUENCES[name](make_engine, algo)
