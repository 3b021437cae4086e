"""The rank's sorts and scans at their tile and launch-path edges (tests/sort_scan_edges_cases.py), on the GPU at the shipped launch shapes:
the cases of test_sort_scan_edges_emu.py at the sizes the shipped constants give, all eight host-table lengths of excl_scan_u32_single, the
segmented scan's fused / blocksums switch, and the three-launch radix pass at the smallest size at which it exists.  No CPU fallback:
without the library or the GPU these tests FAIL."""
import pytest

from cook_amd.engine import Engine
from tests import sort_scan_edges_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make_engine():
    from cook_amd import build
    so = build.build()
    return lambda params: Engine(params, lib_path=so)


def test_the_constants_are_the_shipped_ones(make_engine):
    sh = S.shapes(make_engine)
    assert sh.ship and "hip gfx950" in sh.version, sh


@pytest.mark.parametrize("size", S.PROBE_SIZES)
def test_position_probe_at_radix_edges(make_engine, size):
    """one user: DRU == position in the per-user order == numpy's lexsort, at every tile end and at the switch from small to large tiles"""
    S.run_probe_size(make_engine, size)


@pytest.mark.parametrize("size", S.PROBE_SWITCH)
def test_position_probe_at_the_three_launch_switch(make_engine, size):
    """RS_FUSED_BLOCKS_LARGE large tiles and one item more: the smallest size at which the shipped three-launch pass (radix_hist,
    excl_scan_u32_single over 256 entries per tile = two full super-steps + 256, radix_scatter) exists.  radix_scan absent up to the
    threshold, present above it.  Against the numpy reference only.  Measured on an MI355X: 0.017 - 0.034 s in the engine's call at each of
    the three sizes, 4.1 s for the three tests together (most of it numpy's lexsort of 2 M keys), so all three stay."""
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


@pytest.mark.parametrize("fractional", [False, True])
@pytest.mark.parametrize("which", S.SCAN_SWITCH)
def test_seg_scan_fused_blocksums_switch(make_engine, which, fractional):
    """SS_THREADS tiles / one item more: seg_scan_blocksums absent / present.  (The emulated file runs the integer pair as well.)"""
    S.run_scan_switch(make_engine, which, fractional)


@pytest.mark.parametrize("name", S.HBASE_CASES)
def test_excl_scan_single_through_the_host_table(make_engine, name):
    S.run_hbase_case(make_engine, name)


@pytest.mark.parametrize("name", S.TIE_CASES)
def test_tie_tiles_at_capacity(make_engine, monkeypatch, name):
    S.run_tie_case(make_engine, monkeypatch, name)


def test_tie_tiles_all_single_items(make_engine, monkeypatch):
    S.run_all_singles(make_engine, monkeypatch)
