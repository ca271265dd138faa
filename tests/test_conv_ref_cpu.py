"""CPU-only: the case tables of tests/_conv_ref.py reach every dispatch branch of the
exact-fp32 convs (csrc/conv_fwd.hip, csrc/conv_bwd.hip), judged by the library's own
planner; the references agree with a direct loop; and the C ABI's rejections, which
all return before a launch (dummy non-null pointers, as test_abi_cpu.py does)."""
import ctypes

import pytest
import torch

import _conv_ref as ref
from _conv_ref import Case

ALL_ROWS = [(name, c) for name, rows in ref.TABLES.items() for c in rows]
P = ctypes.c_void_p(16)       # a non-null pointer no rejected call dereferences


def _layout(table):
    return "nchw" if table.endswith("stem") else "nhwc"


def lib_splits(c, layout):
    """The split count hkp_conv2d_bwd_filter will use, from the workspace it asks for."""
    from hkp import _lib
    nbytes = _lib.lib().hkp_conv_bwd_filter_workspace(ctypes.byref(ref.desc(c, layout)))
    slab = 4 * c.cout * c.r * c.s * c.cin
    assert nbytes > 0 and nbytes % slab == 0, (c, nbytes)
    return nbytes // slab


# ------------------------------------------------------------------ the tables ----

@pytest.mark.parametrize("table,c", ALL_ROWS, ids=lambda v: v if isinstance(v, str) else ref.case_id(v))
def test_rows_are_exact_on_integers(table, c):
    """9 L + 3 < 2^24 for the forward, dgrad and wgrad reduction of every row, the
    output is not empty, and int_tensors holds integers in its ranges."""
    assert ref.int_exact(c)
    assert min(ref.out_hw(c)) > 0
    t = ref.int_tensors(c, 1)
    for name, lim in (("x", 3), ("dy", 3), ("add", 3), ("w", 2)):
        v = t[name]
        assert v.dtype == torch.float32 and torch.equal(v, v.round()) and v.abs().max() <= lim, name
    assert t["w"].abs().max() == 2 or t["w"].numel() < 32


def test_library_agrees_on_geometry_and_stat_tiles():
    from hkp import _lib
    ho, wo = ctypes.c_int32(), ctypes.c_int32()
    for table, c in ALL_ROWS:
        d = ref.desc(c, _layout(table))
        _lib.call("hkp_conv_out_hw", ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo))
        assert (ho.value, wo.value) == ref.out_hw(c), c
        if table.startswith("fwd"):
            m = ref.out_pixels(c)
            assert _lib.lib().hkp_conv_stat_tiles(ctypes.byref(d)) == (m + 127) // 128, c


def test_forward_rows_named_edges():
    """The row-count edges the forward table is there for: M = 1, 127, 128, 129 (a last
    tile of one row), both widths in both layouts, one and three chunks per tap,
    rectangular filters both ways."""
    ms = {ref.out_pixels(c) for c in ref.FWD_NHWC}
    assert {1, 127, 128, 129} <= ms
    assert any(ref.out_pixels(c) % 128 == 1 and ref.out_pixels(c) > 128 for c in ref.FWD_STEM + ref.FWD_NHWC)
    for rows in (ref.FWD_NHWC, ref.FWD_STEM):
        assert {c.cout % 128 == 0 for c in rows} == {True, False}
        assert all(c.cout % 64 == 0 for c in rows)
    assert {c.cin // 32 for c in ref.FWD_NHWC} >= {1, 2, 3} and all(c.cin % 32 == 0 for c in ref.FWD_NHWC)
    assert any(c.r < c.s for c in ref.FWD_NHWC) and any(c.r > c.s for c in ref.FWD_NHWC)
    assert any(c.pad > c.dil * (c.r - 1) // 2 and c.r > 1 for c in ref.FWD_NHWC)
    assert any(c.h <= c.dil and c.w <= c.dil and c.r == 3 for c in ref.FWD_NHWC)      # only the centre tap is live
    # stem: C 1 and the cap 8; Kreal below one chunk, and ending inside a float4
    kreal = [c.cin * c.r * c.s for c in ref.FWD_STEM]
    assert {1, 8} <= {c.cin for c in ref.FWD_STEM} and all(c.cin <= 8 for c in ref.FWD_STEM)
    assert any(k < 32 for k in kreal) and any(k % 4 for k in kreal) and any(k % 4 == 0 and k % 32 for k in kreal)


def test_dgrad_rows_reach_every_instantiation():
    """hkp_conv2d_bwd_data launches <128, BN, MODE_FWD> at stride 1 and <128, BN,
    MODE_DGRAD> above it, BN = 128 where Cin % 128 == 0, else 64."""
    got = {(c.cin % 128 == 0, c.stride > 1) for c in ref.DGRAD}
    assert got == {(a, b) for a in (True, False) for b in (True, False)}
    assert {c.cout // 32 for c in ref.DGRAD} >= {1, 3}                 # cchunks with the roles swapped
    assert all(c.cin % 64 == 0 and c.cout % 32 == 0 for c in ref.DGRAD)
    assert all(c.r == c.s and c.pad <= c.dil * (c.r - 1) for c in ref.DGRAD)   # what the library takes
    assert any(c.stride == 2 and c.dil == 2 for c in ref.DGRAD) and any(c.stride == 3 for c in ref.DGRAD)
    assert any(c.stride == 2 and c.r == 1 and c.h % 2 == 0 and c.w % 2 == 0 for c in ref.DGRAD)
    assert any(c.stride == 2 and c.r == 1 and c.h % 2 == 1 and c.w % 2 == 1 for c in ref.DGRAD)


def test_wgrad_rows_reach_every_template_and_split_count():
    """All six conv_wgrad_kernel instantiations, and — from the library's own planner —
    1, 2, 3, 4, 5 and >= 9 splits (split_reduce_kernel sums slab q, q + 4, ... in four
    lanes: one to four splits leave lanes empty, five give lane 0 a second slab, nine a
    third), a last split shorter than one 32-pixel stage and one that ends inside a
    stage.  With two or more splits of a multiple of 32 pixels each, the last split's
    length is M mod 32 whatever the planner's rows per split, so a ragged last stage
    is M % 32 != 0."""
    nhwc = {(c.cout % 128 == 0, c.cin % 128 == 0) for c in ref.WGRAD_NHWC}
    assert nhwc == {(a, b) for a in (True, False) for b in (True, False)}
    assert {c.cout % 128 == 0 for c in ref.WGRAD_STEM} == {True, False}
    assert all(c.cout % 64 == 0 and c.cin % 64 == 0 for c in ref.WGRAD_NHWC)
    assert all(c.cout % 64 == 0 and c.cin <= 8 for c in ref.WGRAD_STEM)
    counts = {}
    for table in ("wgrad_nhwc", "wgrad_stem"):
        for c in ref.TABLES[table]:
            counts[(table, c)] = lib_splits(c, _layout(table))
    print(sorted((ref.case_id(c), sp) for (_, c), sp in counts.items()))
    seen = set(counts.values())
    assert {1, 2, 3, 4, 5} <= seen and any(sp >= 9 for sp in seen), sorted(seen)
    nh = {c: sp for (t, c), sp in counts.items() if t == "wgrad_nhwc"}
    assert {1, 2, 3, 4, 5} <= set(nh.values()) and any(sp >= 9 for sp in nh.values())
    assert any(sp == 1 and ref.out_pixels(c) < ref.WG_STAGE for c, sp in nh.items())
    assert any(sp == 1 and ref.out_pixels(c) % ref.WG_STAGE == 0 for c, sp in nh.items())    # exactly full
    assert any(sp >= 2 and ref.out_pixels(c) % ref.WG_STAGE for c, sp in nh.items())
    assert any(sp >= 2 for (t, _), sp in counts.items() if t == "wgrad_stem")
    assert any(c.r < c.s for c in ref.WGRAD_NHWC) and any(c.r > c.s for c in ref.WGRAD_NHWC)
    # the stem's column tiles: Kreal below one 64-wide tile, and a ragged last tile
    kreal = [c.cin * c.r * c.s for c in ref.WGRAD_STEM]
    assert any(k < 64 for k in kreal) and any(k > 64 and k % 64 for k in kreal)


def test_flip_shapes_take_a_second_grid_trip():
    n = [k * r * s * c for k, r, s, c in ref.FLIP_SHAPES]
    assert max(n) > 4096 * 256 and min(n) < 4096 * 256
    assert any(r != s for _, r, s, _ in ref.FLIP_SHAPES)


# -------------------------------------------------------------- the references ----

def test_references_match_a_direct_loop():
    """fwd64 / dgrad64 / wgrad64 against the defining sums written out, on a strided,
    dilated, rectangular-filter case: integers, so all three are exact."""
    c = Case(2, 7, 6, 3, 4, 2, 3, 2, 2, 2)
    t = ref.int_tensors(c, 5)
    x, w, dy = t["x"].double(), t["w"].double(), t["dy"].double()
    ho, wo = ref.out_hw(c)
    y = torch.zeros(c.n, c.cout, ho, wo, dtype=torch.float64)
    dx = torch.zeros_like(x)
    dw = torch.zeros_like(w)
    for oh in range(ho):
        for ow in range(wo):
            for r in range(c.r):
                for s in range(c.s):
                    hi, wi = oh * c.stride - c.pad + r * c.dil, ow * c.stride - c.pad + s * c.dil
                    if 0 <= hi < c.h and 0 <= wi < c.w:
                        y[:, :, oh, ow] += x[:, :, hi, wi] @ w[:, :, r, s].T
                        dx[:, :, hi, wi] += dy[:, :, oh, ow] @ w[:, :, r, s]
                        dw[:, :, r, s] += dy[:, :, oh, ow].T @ x[:, :, hi, wi]
    assert torch.equal(ref.fwd64(t["x"], t["w"], c), y)
    assert torch.equal(ref.dgrad64(t["dy"], t["w"], c), dx)
    assert torch.equal(ref.dgrad64(t["dy"], t["w"], c, t["add"]), dx + t["add"].double())
    assert torch.equal(ref.wgrad64(t["x"], t["dy"], c), dw)


def test_tile_partials_and_bounds():
    y = torch.arange(130 * 2, dtype=torch.float64).reshape(130, 2)
    s, m2, mu, cnt = ref.tile_partials64(y)
    assert cnt == [128, 2] and s.shape == (2, 2)
    assert torch.equal(s[0], y[:128].sum(0)) and torch.equal(mu[1], y[128:].mean(0))
    assert torch.allclose(m2[0], y[:128].var(0, unbiased=False) * 128, rtol=1e-14)
    assert torch.equal(m2[1], torch.full((2,), 2.0, dtype=torch.float64))
    assert float(ref.err_bound(10, torch.tensor(2.0))) == 12 * 2.0 ** -24 * 2.0
    # (cnt + 2) u relative, plus the mean's rounding
    b = ref.m2_bound(128, torch.tensor(1.0), torch.tensor(0.0))
    assert 130 * ref.U <= float(b) < 130.01 * ref.U
    assert float(ref.m2_bound(4, torch.tensor(0.0), torch.tensor(3.0))) >= 4 * (2 * ref.U * 3) ** 2


# ------------------------------------------------------------ C-ABI rejections ----

NHWC, NCHW = 0, 1


def _d(*a):
    from hkp import _lib
    return _lib.ConvDesc(*a)


def _rejects(fn, d, match, *args):
    from hkp import _lib
    with pytest.raises(_lib.HkpError, match=match):
        _lib.call(fn, ctypes.byref(d), *args)


FWD_REJECTS = [
    ((1, 8, 8, 64, 96, 3, 3, 1, 1, 1, NHWC), "Cout=96 must be a multiple of 64"),
    ((1, 8, 8, 48, 64, 3, 3, 1, 1, 1, NHWC), "NHWC Cin=48 must be a multiple of 32"),
    ((1, 8, 8, 9, 64, 7, 7, 2, 3, 1, NCHW), r"stem \(Cin<=8\), got 9"),
    ((1, 8, 8, 64, 64, 3, 3, 1, 1, 1, 2), "bad layout 2"),
    ((1, 2, 2, 64, 64, 3, 3, 1, 0, 1, NHWC), "empty output"),
    ((1, 2, 9, 64, 64, 3, 3, 2, 0, 1, NHWC), "empty output"),     # extent -1: C's -1 / 2 + 1 would be one row
    ((1, 9, 3, 64, 64, 1, 3, 3, 0, 2, NHWC), "empty output"),     # the same in the width, extent -2 at stride 3
    ((1, 8, 8, 64, 64, 3, 3, 0, 1, 1, NHWC), "bad stride/dilation/pad"),
    ((1, 8, 8, 64, 64, 3, 3, 1, 1, 0, NHWC), "bad stride/dilation/pad"),
    ((1, 8, 8, 64, 64, 3, 3, 1, -1, 1, NHWC), "bad stride/dilation/pad"),
    ((0, 8, 8, 64, 64, 3, 3, 1, 1, 1, NHWC), "non-positive size"),
]


@pytest.mark.parametrize("args,match", FWD_REJECTS, ids=[m for _, m in FWD_REJECTS])
def test_fwd_rejects(args, match):
    _rejects("hkp_conv2d_fwd", _d(*args), match, P, P, P, None, None)


def test_fwd_rejects_null_tensors():
    d = _d(1, 8, 8, 64, 64, 3, 3, 1, 1, 1, NHWC)
    for a in ((None, P, P), (P, None, P), (P, P, None)):
        _rejects("hkp_conv2d_fwd", d, "null tensor", *a, None, None)
    from hkp import _lib
    assert _lib.lib().hkp_conv2d_fwd(None, P, P, P, None, None) != 0
    assert "null descriptor" in _lib.lib().hkp_last_error().decode()


def test_empty_output_has_no_geometry():
    """A footprint larger than the padded image has no output at any stride: no size,
    no statistic tiles, no wgrad workspace."""
    from hkp import _lib
    L = _lib.lib()
    for stride in (1, 2, 3, 4):
        d = _d(1, 2, 9, 64, 64, 3, 3, stride, 0, 1, NHWC)
        ho, wo = ctypes.c_int32(7), ctypes.c_int32(7)
        assert L.hkp_conv_out_hw(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo)) != 0
        assert (ho.value, wo.value) == (7, 7)
        assert L.hkp_conv_stat_tiles(ctypes.byref(d)) == -1
        assert L.hkp_conv_bwd_filter_workspace(ctypes.byref(d)) == -1
    d = _d(1, 3, 9, 64, 64, 3, 3, 2, 0, 1, NHWC)               # extent 0: one output row
    assert L.hkp_conv_out_hw(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo)) == 0
    assert (ho.value, wo.value) == (1, 4)


DGRAD_REJECTS = [
    ((1, 8, 8, 96, 64, 3, 3, 1, 1, 1, NHWC), "Cin%64==0"),
    ((1, 8, 8, 64, 48, 3, 3, 1, 1, 1, NHWC), "Cout%32==0"),
    ((1, 8, 8, 3, 64, 7, 7, 2, 3, 1, NCHW), "NHWC convs only"),
    ((1, 8, 8, 64, 64, 3, 3, 1, 3, 1, NHWC), "asymmetric padding"),       # pad > dil * (r - 1)
    ((1, 8, 8, 64, 64, 1, 3, 1, 1, 1, NHWC), "asymmetric padding"),       # R != S
    ((1, 8, 8, 64, 64, 3, 1, 1, 1, 1, NHWC), "asymmetric padding"),
    ((1, 8, 8, 64, 64, 1, 3, 1, 0, 1, NHWC), "asymmetric padding"),       # R != S even without padding
    ((1, 2, 2, 64, 64, 3, 3, 1, 0, 1, NHWC), "empty output"),
    ((1, 8, 8, 64, 64, 3, 3, 0, 1, 1, NHWC), "bad stride/dilation/pad"),
]


@pytest.mark.parametrize("args,match", DGRAD_REJECTS, ids=["%s-%d" % (m, i) for i, (_, m) in enumerate(DGRAD_REJECTS)])
def test_dgrad_rejects(args, match):
    _rejects("hkp_conv2d_bwd_data", _d(*args), match, P, P, None, P, None)


def test_dgrad_rejects_null_tensors():
    d = _d(1, 8, 8, 64, 64, 3, 3, 1, 1, 1, NHWC)
    for a in ((None, P, None, P), (P, None, None, P), (P, P, P, None)):
        _rejects("hkp_conv2d_bwd_data", d, "null tensor", *a, None)


def test_wgrad_rejects():
    big = ctypes.c_int64(1 << 40)
    for args, match in [((1, 8, 8, 64, 96, 3, 3, 1, 1, 1, NHWC), "Cout=96 must be a multiple of 64"),
                        ((1, 8, 8, 96, 64, 3, 3, 1, 1, 1, NHWC), "NHWC Cin=96 must be a multiple of 64"),
                        ((1, 8, 8, 32, 64, 3, 3, 1, 1, 1, NHWC), "NHWC Cin=32 must be a multiple of 64"),
                        ((1, 8, 8, 9, 64, 7, 7, 2, 3, 1, NCHW), r"stem \(Cin<=8\)"),
                        ((1, 2, 2, 64, 64, 3, 3, 1, 0, 1, NHWC), "empty output"),
                        ((1, 8, 8, 64, 64, 3, 3, 0, 1, 1, NHWC), "bad stride/dilation/pad")]:
        _rejects("hkp_conv2d_bwd_filter", _d(*args), match, P, P, P, 0, P, big, None)
    from hkp import _lib
    for c, layout in [(ref.WGRAD_NHWC[0], "nhwc"), (ref.WGRAD_NHWC[7], "nhwc"), (ref.WGRAD_STEM[3], "nchw")]:
        d = ref.desc(c, layout)
        need = _lib.lib().hkp_conv_bwd_filter_workspace(ctypes.byref(d))
        assert need >= 4 * c.cout * c.r * c.s * c.cin
        _rejects("hkp_conv2d_bwd_filter", d, "workspace %d < %d bytes" % (need - 1, need), P, P, P, 0, P,
                 ctypes.c_int64(need - 1), None)
        _rejects("hkp_conv2d_bwd_filter", d, "null tensor", P, P, P, 0, None, ctypes.c_int64(need), None)
        for a in ((None, P, P), (P, None, P), (P, P, None)):
            _rejects("hkp_conv2d_bwd_filter", d, "null tensor", *a, 0, P, ctypes.c_int64(need), None)


def test_flip_rejects():
    _rejects("hkp_conv_weight_flip", _d(1, 1, 1, 64, 64, 3, 3, 1, 0, 1, NCHW), "KRSC weights only", P, P, None)
    _rejects("hkp_conv_weight_flip", _d(1, 1, 1, 64, 64, 3, 3, 1, 0, 1, NHWC), "null argument", None, P, None)
    _rejects("hkp_conv_weight_flip", _d(1, 1, 1, 64, 64, 3, 3, 1, 0, 1, NHWC), "null argument", P, None, None)


# -------------------------------------------------- wrapper checks (no tensor) ----

def test_conv_out_hw_rejects_like_the_library():
    """ops.conv_out_hw sizes every wrapper's output: it must refuse what conv_geometry
    refuses, not floor-divide a negative extent into a size of zero."""
    from hkp import ops
    from hkp._lib import HkpError
    assert ops.conv_out_hw(30, 40, 3, 3, 2, 1, 1) == (15, 20)
    assert ops.conv_out_hw(3, 9, 3, 3, 2, 0, 1) == (1, 4)
    for a, match in [((8, 8, 3, 3, 0, 1, 1), "bad stride"), ((8, 8, 3, 3, 1, 1, 0), "bad stride"),
                     ((8, 8, 3, 3, 1, -1, 1), "bad stride"), ((2, 9, 3, 3, 1, 0, 1), "empty output"),
                     ((2, 9, 3, 3, 2, 0, 1), "empty output"), ((9, 3, 1, 3, 3, 0, 2), "empty output")]:
        with pytest.raises(HkpError, match=match):
            ops.conv_out_hw(*a)
