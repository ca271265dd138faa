"""CPU-only checks of the mixed-height tile planner (hkp_conv_x3_mix_plan, the
regions of a HKP_TILE_MIX_A3 launch) and of the BN partial layout query that goes
with it (hkp_conv_x3_stat_layout): host arithmetic, no GPU."""
import ctypes

import pytest

HEIGHTS = (256, 192, 160)
COST = (16, 12, 10)                      # 16-row blocks per tile


def _plan(m, n_tiles, cus):
    from hkp import _lib
    out = (ctypes.c_int32 * _lib.HKP_MIX_PLAN_LEN)()
    n = _lib.lib().hkp_conv_x3_mix_plan(m, n_tiles, cus, out)
    assert n >= 0
    v = list(out)
    return dict(n=n, cost=v[0], rounds=v[1:4], mt=v[4:7], m_base=v[7:10], part_base=v[10:13], part_tiles=v[13])


M_GRID = [1, 79, 160, 4551, 40000, 57344, 60000, 76800, 115200, 153599, 153600, 153601, 307200, 1 << 20,
          (1 << 24) + 12345]


@pytest.mark.parametrize("cus", [64, 256, 304])
@pytest.mark.parametrize("n_tiles", [1, 2, 4])
def test_mix_plan_regions(n_tiles, cus):
    """The regions tile [0, M) exactly once, every region but the last is whole
    rounds of full tiles, the cost is the blocks the rounds add up to and no more
    than a uniform grid's of any of the three heights, and the BN partial segments
    hold ceil(region rows / (height / 2)) tiles each."""
    per_round = cus // n_tiles
    for m in M_GRID:
        p = _plan(m, n_tiles, cus)
        live = [r for r in range(3) if p["mt"][r] > 0]
        assert p["n"] == len(live) >= 1, (m, p)
        last = live[-1]
        row, pt = 0, 0
        for r in range(3):
            assert p["m_base"][r] == row and p["part_base"][r] == pt, (m, r, p)
            bm, mt = HEIGHTS[r], p["mt"][r]
            if r == last:
                rows = m - row
                assert (mt - 1) * bm < rows <= mt * bm, (m, r, p)             # only the tiles it needs
                assert mt <= p["rounds"][r] * per_round, (m, r, p)
            else:
                rows = mt * bm
                assert mt == p["rounds"][r] * per_round, (m, r, p)            # whole rounds of full tiles
                assert r < last or mt == 0, (m, r, p)
            row += rows
            pt += -(-rows // (bm // 2))
        assert row == m and pt == p["part_tiles"], (m, p)
        assert p["cost"] == sum(c * a for c, a in zip(COST, p["rounds"])), (m, p)
        assert per_round * sum(h * a for h, a in zip(HEIGHTS, p["rounds"])) >= m, (m, p)
        for bm, c in zip(HEIGHTS, COST):                                      # the uniform grids
            rounds = -(-(-(-m // bm)) // per_round)
            assert p["cost"] <= c * rounds, (m, bm, p)


def test_mix_plan_c2_shapes():
    """The C2 shapes (M = 153,600 on 256 CUs): layer3 (one column tile) runs 256 + 192 + 160 rows
    per CU, layer4 (two column tiles) four rounds of 256 and one of 192."""
    p = _plan(153600, 1, 256)
    assert p["rounds"] == [1, 1, 1] and p["mt"] == [256, 256, 244] and p["cost"] == 38
    assert p["m_base"] == [0, 65536, 114688]
    p = _plan(153600, 2, 256)
    assert p["rounds"] == [4, 1, 0] and p["mt"] == [512, 118, 0] and p["cost"] == 76
    assert _plan(100, 8, 4)["n"] == 0                                         # more column tiles than CUs: no plan


def test_stat_layout_segments():
    """hkp_conv_x3_stat_layout: a mix launch's list has one segment per non-empty
    region, ceil(region rows / stat rows) tiles each (the planner's regions on this
    device's CU count: 256 without a GPU); the uniform bodies have one segment, and a
    192- / 160-row policy the halo body takes reports the halo body's 128 rows."""
    from hkp import _lib, ops
    from hkp._lib import HKP_KOP_FWD_X3, ConvDesc
    d = ConvDesc(32, 60, 80, 256, 256, 3, 3, 1, 2, 2, 0, _lib.HKP_TILE_MIX_A3)
    assert ops.kernel_name(d, HKP_KOP_FWD_X3) == "conv_x3_a3_mix_kernel<3>"
    assert ops.kernel_name(d, _lib.HKP_KOP_FWD_X3_W16) == "conv_x3_a3_mix_kernel<2>"
    segs = ops.conv_stat_layout(d, HKP_KOP_FWD_X3)
    name = ops.kernel_name(ConvDesc(32, 60, 80, 256, 256, 3, 3, 1, 2, 2, 0, 0), HKP_KOP_FWD_X3)
    assert name == "conv_x3_a3_kernel<3>"                                     # AUTO never picks the mix
    m = 32 * 60 * 80
    # the planner the launcher uses runs on the device's CU count; check against it
    for cus in (256, 304, 64, 128, 120, 104, 80):
        p = _plan(m, 1, cus)
        ends = p["m_base"][1:] + [m]                                          # a region ends where the next begins
        want = tuple((HEIGHTS[r] // 2, -(-(ends[r] - p["m_base"][r]) // (HEIGHTS[r] // 2)))
                     for r in range(3) if p["mt"][r])
        if want == segs:
            break
    else:
        raise AssertionError("segments %s match no CU count's plan" % (segs,))
    assert sum(r * t for r, t in segs[:-1]) < m <= sum(r * t for r, t in segs)
    # one round deep (150 tiles): plans as AUTO, one segment of 128-row tiles
    d1 = ConvDesc(2, 120, 160, 64, 256, 1, 1, 1, 0, 1, 0, _lib.HKP_TILE_MIX_A3)
    assert "mix" not in ops.kernel_name(d1, HKP_KOP_FWD_X3)
    assert ops.conv_stat_layout(d1, HKP_KOP_FWD_X3) == ((128, 300),)
    # uniform 192- / 160-row grids: 96- / 80-row partials ...
    for tile, rows in ((_lib.HKP_TILE_192_A3, 96), (_lib.HKP_TILE_160_A3, 80)):
        du = ConvDesc(8, 60, 80, 256, 256, 3, 3, 1, 2, 2, 0, tile)
        assert ops.conv_stat_layout(du, HKP_KOP_FWD_X3) == ((rows, -(-38400 // rows)),)
        assert _lib.lib().hkp_conv_x3_stat_tile_rows(ctypes.byref(du), HKP_KOP_FWD_X3) == rows
        # ... but a 64-channel 3x3 the halo-tile body takes writes 128-row partials
        dh = ConvDesc(1, 32, 64, 64, 64, 3, 3, 1, 1, 1, 0, tile)
        assert ops.kernel_name(dh, HKP_KOP_FWD_X3) == "conv_x3_halo_kernel<3>"
        assert ops.conv_stat_layout(dh, HKP_KOP_FWD_X3) == ((128, 16),)
        assert _lib.lib().hkp_conv_x3_stat_tile_rows(ctypes.byref(dh), HKP_KOP_FWD_X3) == 128
