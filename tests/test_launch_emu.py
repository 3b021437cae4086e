"""cook_match_launch_resources on a machine WITHOUT a GPU: the cook_amd/csrc sources compiled against the SIMT emulator (tests/simt_emu),
every case of tests/launch_cases.py against the oracle of tests/launch_oracle.py; and, with no engine at all, the oracle against the
values of the reference's own tests (tests/golden/launch_resources.json)."""
import pytest

from cook_amd.engine import Engine
from tests import launch_cases as K
from tests import launch_oracle as O

G = K.GOLDEN


# ---- the oracle alone ------------------------------------------------------------------------------------------------------------------
def test_oracle_reproduces_the_reference_tests():
    g = G["resources_by_role"]
    assert O.resources_by_role(g["offers"]) == g["expect"]
    assert list(O.resources_by_role(g["offers"])) == ["mem", "cpus", "ports"]
    g = G["take_resources"]
    r = O.take_resources(g["resources"], g["name"], g["amount"])
    assert r["amount-still-needed"] == g["amount_still_needed"] and r["mesos-messages"] == g["mesos_messages"]
    assert r["remaining-resources"] == g["remaining_resources"]
    g = G["range_contains"]
    assert [O.range_contains(v, g["range"]) for v, _ in g["cases"]] == [w for _, w in g["cases"]]
    g = G["role_containing_port"]
    assert [O.role_containing_port(g["avail"], p) for p, _ in g["cases"]] == [w for _, w in g["cases"]]
    g = G["take_ports"]
    assert O.take_ports(g["resources"], g["ports_needed"]) == g["expect"]
    g = G["take_scalar_resources_for_task"]
    r = O.take_all_scalar_resources_for_task(g["available"], g["scalar_requests"])
    assert r["remaining-resources"] == g["remaining_resources"] and r["mesos-messages"] == g["mesos_messages"]
    g = G["add_scalar_resources_to_task_infos"]
    out = O.add_scalar_resources_to_task_infos(g["available"], [{"scalar-requests": t["scalar_requests"]} for t in g["tasks"]])
    assert [t["scalar-resource-messages"] for t in out] == g["scalar_resource_messages"]


def test_port_cursor_rule():
    lease = [{"begin": 203, "end": 204}, {"begin": 201, "end": 202}, {"begin": 300, "end": 300}]
    assert O.assign_ports(lease, [2, 0, 3]) == [[203, 204], [], [201, 202, 300]]
    assert O.assign_ports(lease, [1, 3]) == [[203], [201, 202, 204]]
    assert O.assign_ports(lease, [5, 1]) is None and O.assign_ports([], [0, 0]) == [[], []]


def test_random_cases_hold_what_they_are_for():
    K.check_random_precondition()


# ---- the engine, emulated --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def make_engine():
    from tests.simt_emu import build_emu
    so = build_emu.build()
    return lambda params: Engine(params, lib_path=so)


def test_launch_golden(make_engine):
    K.check_golden(make_engine)


def test_launch_range_boundaries(make_engine):
    K.check_range_boundaries(make_engine)


def test_launch_single_port_ranges(make_engine):
    K.check_single_port_ranges(make_engine)


def test_launch_segment_lengths(make_engine):
    K.check_segment_lengths(make_engine)


def test_launch_one_offer_none_kept_k1(make_engine):
    K.check_one_offer_none_kept_k1(make_engine)


def test_launch_roles(make_engine):
    K.check_roles(make_engine)


def test_launch_offer_skipped(make_engine):
    K.check_offer_skipped(make_engine)


def test_launch_call_forms(make_engine):
    K.check_call_forms(make_engine)


@pytest.mark.parametrize("seed", K.SEEDS)
def test_launch_random(make_engine, seed):
    K.check_random(make_engine, seed)


def test_launch_refusals(make_engine):
    K.check_refusals(make_engine)


def test_launch_binding_finds_room(make_engine):
    K.check_binding_finds_room(make_engine)


def test_launch_no_jobs(make_engine):
    K.check_no_jobs(make_engine)
