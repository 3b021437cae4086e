"""The carry (cook_cycle_run_queue_carry*) on a machine WITHOUT a GPU: the cook_amd/csrc sources compiled against the SIMT emulator
(tests/simt_emu), every cycle against the oracle of tests/carry_oracle.py (cases in tests/carry_cases.py)."""
import os
import subprocess
import sys

import pytest

from cook_amd import _abi as A
from cook_amd.engine import EXPORTS, Engine
from tests import carry_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def make_engine():
    from tests.simt_emu import build_emu
    so = build_emu.build()
    return lambda params: Engine(params, lib_path=so)


def test_carry_base(make_engine):
    K.check_base(make_engine)


def test_carry_non_dyadic(make_engine):
    K.check_base(make_engine, fractional=True)


def test_carry_segment_lengths(make_engine):
    K.check_segment_lengths(make_engine)


@pytest.mark.parametrize("null_cols", [False, True])
def test_carry_every_column(make_engine, null_cols):
    K.check_columns(make_engine, null_cols=null_cols)


def test_carry_skipped_offers_and_remove_all(make_engine):
    K.check_skipped(make_engine)


def test_carry_tokens(make_engine):
    K.check_tokens(make_engine)


def test_carry_split_equivalence(make_engine):
    K.check_split(make_engine)


def test_carry_class_ordered_walk(make_engine):
    K.check_classfit(make_engine)


def test_carry_multi(make_engine, multi_mode):
    K.check_multi(make_engine)


def test_carry_built_offers_in_place(make_engine):
    K.check_built_offers(make_engine)


def test_carry_refusals_and_persistence(make_engine):
    K.check_refusals(make_engine)


def test_carry_abi(make_engine, tmp_path):
    assert "cook_cycle_run_queue_carry" in EXPORTS and "cook_cycle_run_queue_carry_multi" in EXPORTS
    with make_engine(A.default_params()) as e:  # (load_library resolves every prototype of the header in the library)
        assert e._lib.cook_abi_version() == A.ABI_VERSION == 4
    subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "gen_protos.py"), "--check"])
    text, want = K.struct_size_sources()
    src = tmp_path / "sz.c"
    src.write_text(text)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want
