"""The rank's sorts and scans at their tile and launch-path edges (tests/sort_scan_edges_cases.py), on the SIMT emulator with the emulated
suite's small launch shapes: every radix tile and path edge of the position probe, the key shapes, the several-user pools, the segmented
scan's head placements, excl_scan_u32_single through the rebalancer's host table and the tie tiles at their capacity.
The segmented scan's fused / blocksums switch needs SS_THREADS tiles on either build: its integer pair runs here (18 s a case).
test_sort_scan_edges_gpu.py runs the same cases at the shipped shapes, the switch's fractional pair and the longer host tables."""
import pytest

from cook_amd.engine import Engine
from tests import sort_scan_edges_cases as S


@pytest.fixture(scope="module")
def make_engine():
    from tests.simt_emu import build_emu
    so = build_emu.build()
    return lambda params: Engine(params, lib_path=so)


def test_the_constants_are_the_emulated_ones(make_engine):
    sh = S.shapes(make_engine)
    assert not sh.ship and sh.rs_fused_large < 100_000 and sh.TS_CAP < 8192, sh


@pytest.mark.parametrize("size", S.PROBE_SIZES + S.PROBE_SWITCH)
def test_position_probe_at_radix_edges(make_engine, size):
    """one user: DRU == position in the per-user order == numpy's lexsort; radix_scan present exactly above RS_FUSED_BLOCKS_LARGE large tiles"""
    S.run_probe_size(make_engine, size)


@pytest.mark.parametrize("kind", S.PROBE_KINDS)
def test_position_probe_key_shapes(make_engine, kind):
    """radix_sort_masked's digit placement: the number of passes is what the varying bits ask for"""
    S.run_probe_kind(make_engine, kind)


@pytest.mark.parametrize("flavour", S.FLAVOURS)
@pytest.mark.parametrize("size", S.SEVERAL_USERS_SIZES)
def test_several_users_at_radix_edges(make_engine, size, flavour):
    S.run_several_users(make_engine, size, flavour)


@pytest.mark.parametrize("fractional", [False, True])
def test_seg_scan_heads_on_tile_ends(make_engine, fractional):
    S.run_scan_heads(make_engine, fractional)


@pytest.mark.parametrize("which", S.SCAN_SWITCH)
def test_seg_scan_fused_blocksums_switch(make_engine, which):
    """SS_THREADS tiles / one item more: seg_scan_blocksums absent / present.  SS_THREADS is the same number in both builds, so this is
    262 144 tasks here too: about 18 s a case on the emulator.  The integer pair runs here, the fractional pair in the GPU file only."""
    S.run_scan_switch(make_engine, which)


@pytest.mark.parametrize("name", ["step-1", "step", "step+1", "super+1"])
def test_excl_scan_single_through_the_host_table(make_engine, name):
    """SCAN1_* are the same numbers on both builds, so the host tables are as long here as on the GPU, and a pending job costs the emulator
    a pass over all of them (0.4 s per job and 8 192 hosts): the step's three sizes (step-1 has a scalar tail of seven entries, with two
    big hosts in it) and the first size with a second super-step run here, the other four (up to two super-steps + 1) in the GPU file"""
    S.run_hbase_case(make_engine, name)


@pytest.mark.parametrize("name", S.TIE_CASES)
def test_tie_tiles_at_capacity(make_engine, monkeypatch, name):
    S.run_tie_case(make_engine, monkeypatch, name)


def test_tie_tiles_all_single_items(make_engine, monkeypatch):
    S.run_all_singles(make_engine, monkeypatch)
