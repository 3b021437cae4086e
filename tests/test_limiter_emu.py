"""The launch-rate limiters kept on the device (cook_cycle_set_limiters, cook_cycle_set_clock, cook_cycle_limiters_spend,
cook_cycle_fetch_limiters) on a machine WITHOUT a GPU: the cook_amd/csrc sources compiled against the SIMT emulator (tests/simt_emu),
every cycle against the oracle of tests/limiter_oracle.py (cases in tests/limiter_cases.py); and that oracle against the reference's own
token-bucket cases (tests/golden/token_bucket_filter.json)."""
import json
import os

import pytest

from cook_amd.engine import Engine
from tests import limiter_cases as X
from tests import limiter_oracle as O

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "token_bucket_filter.json")))


@pytest.fixture(scope="module")
def make_engine():
    from tests.simt_emu import build_emu
    so = build_emu.build()
    return lambda params: Engine(params, lib_path=so)


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: c["name"].replace(" ", "_").replace(":", ""))
def test_limiter_oracle_golden(case):
    """the reference's token-bucket tests through the Python restatement: every expected value exactly"""
    rate, bucket, t0 = case["create"]
    made = O.Bucket(float(rate), int(bucket), int(t0), 0)
    results = []
    for x, st in enumerate(case["steps"]):
        at = st.get("from", x - 1)
        b = made if at < 0 else results[at]
        if st["op"] == "earn":
            b = O.earn(b, st["t"])
        elif st["op"] == "spend":
            b = O.spend(b, st["t"], st["w"])
        else:
            for t in range(st["start"], st["stop"], st["step"]):
                b = O.earn(b, t)
        results.append(b)
        got = dict(tokens=b.tokens, last=b.last, in_debt=O.in_debt(b), time_until=O.time_until(b))
        for key, want in st.get("expect", {}).items():
            assert got[key] == want and type(got[key]) is type(want), (case["name"], x, key, got[key], want)


def test_limiter_oracle_golden_summary():
    """the figures the fixture must hold, as the reference's tests state them"""
    by = {c["name"]: c for c in GOLDEN["cases"]}
    tok = lambda name: [s["expect"]["tokens"] for s in by[name]["steps"] if "tokens" in s.get("expect", {})]
    assert tok("test-spend-tokens") == tok("test-take-fraction") == [-130, -80, -33, -36, 4, 95]
    assert tok("test-fractional-token: maxing out the bucket") == [4] and tok("test-fractional-token: not maxing the bucket") == [30]
    assert [s["expect"]["time_until"] for s in by["test-time-until"]["steps"][1:]] == [13, 3, 3, 0]
    assert [s["expect"]["last"] for s in by["test-negative-tokens: out of order"]["steps"][2:7]] == [5, 15, 15, 15, 20]


def test_limiter_oracle_fraction_rule():
    X.check_fraction_rule()


def test_limiter_by_hand(make_engine):
    X.check_by_hand(make_engine)


@pytest.mark.parametrize("users,k", X.CASES)
def test_limiter_differential(make_engine, users, k):
    X.check_differential(make_engine, users, k)


def test_limiter_earn_set(make_engine):
    X.check_earn_set(make_engine)


@pytest.mark.parametrize("how", ["none", "backwards", "fraction"])
def test_limiter_clock(make_engine, how):
    X.check_clock(make_engine, how)


def test_limiter_spend(make_engine):
    X.check_spend(make_engine)


@pytest.mark.parametrize("n", [1, 65])
def test_limiter_listed_replace(make_engine, n):
    X.check_listed(make_engine, n)


def test_limiter_persistence(make_engine):
    X.check_persistence(make_engine)


def test_limiter_drop(make_engine):
    X.check_drop(make_engine)


def test_limiter_late_install(make_engine):
    X.check_late_install(make_engine)


def test_limiter_multi(make_engine, multi_mode):
    X.check_multi(make_engine)


@pytest.mark.parametrize("algo,form", [(1, 1), (3, 3)])
def test_limiter_placement_forms(make_engine, algo, form):
    X.check_forms(make_engine, algo, form)


def test_limiter_edges(make_engine):
    X.check_edges(make_engine)


def test_limiter_refusals(make_engine):
    X.check_refusals(make_engine)
