"""tests/_x3_ref.py checked without a GPU: the packing helpers round-trip, ref64 equals four
nested Python loops over exactly the products each mode keeps, every row of the exact GPU
tests meets the 2^24 condition (no exceptions list), the planner names the kernel and form
each row claims (on 256 CUs, asked without a device), and the rows reach every HKP_X3K_* id
and both wgrad bodies."""
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "hulk-keypoints_amd"), os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _x3_ref as R  # noqa: E402
import test_gpu_precision as prec  # noqa: E402
import test_gpu_x3_exact as exact  # noqa: E402
import test_gpu_x3_launch_bits as bits  # noqa: E402
from hkp import _lib, ops  # noqa: E402

CUS = 256


def _ints(*shape, seed, a=9):
    return torch.randint(-a, a + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def test_pack_round_trips():
    hi, lo = _ints(2, 64, 3, 5, seed=1), _ints(2, 64, 3, 5, seed=2)
    t = R.pack_act(hi, lo)
    assert t.dtype == torch.float16 and tuple(t.shape) == (2, 3, 5, 128) and t._hkp_split_passes == 3
    # the layout itself: [.., C/32, hi32 | lo32]
    assert torch.equal(t[1, 2, 4, 64:96].float(), hi[1, 32:64, 2, 4])
    assert torch.equal(t[1, 2, 4, 96:128].float(), lo[1, 32:64, 2, 4])
    assert all(torch.equal(a, b) for a, b in zip(R.unpack_act(t), (hi, lo)))
    t1 = R.pack_act(hi, lo, 1)
    assert tuple(t1.shape) == (2, 3, 5, 64) and t1._hkp_split_passes == 1 and torch.equal(R.unpack_act(t1, 1)[0], hi)
    hw, lw = _ints(64, 32, 3, 3, seed=3), _ints(64, 32, 3, 3, seed=4)
    w = R.pack_w(hw, lw)
    assert tuple(w.shape) == (64, 3, 3, 64) and torch.equal(w[5, 1, 2, :32].float(), hw[5, :, 1, 2])
    assert torch.equal(w[5, 1, 2, 32:].float(), lw[5, :, 1, 2])
    assert all(torch.equal(a, b) for a, b in zip(R.unpack_w(w), (hw, lw)))
    assert torch.equal(R.unpack_w(R.pack_w(hw, lw, 1), 1)[0], hw)
    f = R.pack_w_flip(hw, lw)                                        # [C, R, S, 2K], tap (i, j) = (R-1-i, S-1-j)
    assert tuple(f.shape) == (32, 3, 3, 128) and torch.equal(f[7, 0, 2, :32].float(), hw[:32, 7, 2, 0])
    assert torch.equal(f[7, 0, 2, 96:128].float(), lw[32:, 7, 2, 0])
    assert all(torch.equal(a, b) for a, b in zip(R.unpack_w_flip(f), (hw, lw)))
    # the same layouts as the GPU tests' own unpacker
    assert all(torch.equal(a, b) for a, b in zip(R.unpack_x3(t), prec._unpack_x3(t)))


def test_phase_slices_are_the_phase_taps():
    for k, pad in ((3, 1), (1, 0), (3, 0), (7, 3)):
        for ph in range(4):
            rows, cols = R.phase_slices(k, pad, ph)
            assert len(rows) == max(0, ops.phase_taps(k, pad, ph >> 1)), (k, pad, ph)
            assert len(cols) == max(0, ops.phase_taps(k, pad, ph & 1)), (k, pad, ph)


def test_pow2_scale():
    assert R.pow2_scale(0.0) == 1.0 and R.pow2_scale(2.0 ** 10) == 8.0 and R.pow2_scale(2.0 ** 10 - 1) == 16.0
    assert R.pow2_scale(1e-9) * 1e-9 >= 2 ** 13 and R.pow2_scale(1e-9) * 1e-9 < 2 ** 14


def _loops(p, shape, op, P):
    """Four nested loops (output pixel, channel, tap, channel) over the products mode P keeps."""
    n, h, w, cin, cout, k, st, pad, dil = shape
    ho, wo = R.out_hw(shape)
    keep = {3: ((0, 0), (0, 1), (1, 0)), 2: ((0, 0), (1, 0)), 4: ((0, 0), (0, 1)), 1: ((0, 0),)}[P]
    if op == "fwd":
        a, b = (p["hx"], p["lx"]), (p["hw"], p["lw"])
        out = torch.zeros(n, cout, ho, wo, dtype=torch.float64)
    elif op == "dgrad":
        a, b = (p["hdy"], p["ldy"]), (p["hw"], p["lw"])
        out = torch.zeros(n, cin, h, w, dtype=torch.float64)
    else:
        a, b = (p["hx"], p["lx"]), (p["hdy"], p["ldy"])
        out = torch.zeros(cout, cin, k, k, dtype=torch.float64)
    for i in range(n):
        for oy in range(ho):
            for ox in range(wo):
                for r in range(k):
                    for s in range(k):
                        iy, ix = oy * st - pad + r * dil, ox * st - pad + s * dil
                        if not (0 <= iy < h and 0 <= ix < w):
                            continue
                        for ai, bi in keep:
                            if op == "fwd":      # [cout, cin] @ [cin]
                                out[i, :, oy, ox] += b[bi][:, :, r, s].double() @ a[ai][i, :, iy, ix].double()
                            elif op == "dgrad":
                                out[i, :, iy, ix] += b[bi][:, :, r, s].double().t() @ a[ai][i, :, oy, ox].double()
                            else:
                                out[:, :, r, s] += torch.outer(b[bi][i, :, oy, ox].double(), a[ai][i, :, iy, ix].double())
    return out


@pytest.mark.parametrize("shape", [(2, 5, 4, 32, 64, 3, 1, 1, 1), (1, 7, 6, 32, 64, 3, 2, 1, 1), (1, 6, 5, 32, 64, 3, 1, 2, 2),
                                   (1, 4, 5, 32, 64, 1, 2, 0, 1)], ids=R.case_id)
def test_ref64_equals_the_loops(shape):
    fwd = R.int_planes(shape, 3, "fwd")
    for P in (3, 2, 4, 1):
        want = _loops(fwd, shape, "fwd", P) * fwd["inv"].double().view(1, -1, 1, 1)
        assert torch.equal(R.ref64(fwd, shape, "fwd", P), want), P
    assert not torch.equal(R.ref64(fwd, shape, "fwd", 3), R.ref64(fwd, shape, "fwd", 2))     # lo is not hi's remainder
    dg = R.int_planes(shape, 4, "dgrad")
    want = _loops(dg, shape, "dgrad", 3) * dg["inv"].double().view(1, -1, 1, 1) / 8 + dg["add"].double()
    assert torch.equal(R.ref64(dg, shape, "dgrad", gscale=8.0), want)
    wg = R.int_planes(shape, 5, "wgrad")
    assert torch.equal(R.ref64(wg, shape, "wgrad", gscale=8.0), _loops(wg, shape, "wgrad", 3) / 8)


def test_int_planes_are_what_the_docstring_says():
    shape = (2, 9, 11, 64, 128, 3, 1, 1, 1)
    p = R.int_planes(shape, 7, "fwd")
    assert float(p["hx"].abs().max()) == 3 and float(p["lx"].abs().max()) == 2 and float(p["lw"].abs().max()) == 2
    assert int((p["lx"].abs().amax((0, 2, 3)) == 0).sum()) >= 1 and int((p["lw"].abs().amax((0, 2, 3)) == 0).sum()) >= 1
    assert int(((p["hw"].abs() + p["lw"].abs()).amax((1, 2, 3)) == 0).sum()) >= 1
    m, _ = torch.frexp(p["inv"])
    assert bool((m == 0.5).all()) and float(p["inv"].min()) >= 0.25 and float(p["inv"].max()) <= 4
    assert not torch.equal(p["lx"], (p["hx"] - p["hx"].half().float()))                      # unrelated planes
    d = R.int_planes(shape, 7, "dgrad")
    assert float(d["add"].abs().max()) == 3 and d["inv"].numel() == 64


def test_stat_tiles_group_rows_as_the_bodies_do():
    y = torch.arange(2 * 3 * 8 * 64, dtype=torch.float64).reshape(2, 8, 64, 3).permute(0, 3, 1, 2)   # NCHW view of NHWC
    s, m2, mu, cnt, ymax, nominal = R.stat_tiles64(y, ("patch",))
    assert cnt == [128] * 8 and nominal == cnt
    # tile 1 = the second half (patch rows 4-7) of the first patch (columns 0-31) of image 0
    want = y[0, :, 4:8, 0:32].reshape(3, -1)
    assert torch.equal(s[1], want.sum(1)) and torch.equal(ymax[1], want.abs().amax(1))
    # tile 2 = the first half of the patch at columns 32-63
    assert torch.equal(s[2], y[0, :, 0:4, 32:64].reshape(3, -1).sum(1))
    ym = R.rows(y)
    s, m2, mu, cnt, _, nominal = R.stat_tiles64(y, ("raster", ((128, 2), (96, 2), (80, 8))))   # a mix launch's three regions
    assert cnt == [128, 128, 96, 96] + [80] * 7 + [16] and sum(cnt) == ym.shape[0]
    assert nominal == [128, 128, 96, 96] + [80] * 8
    assert torch.equal(s[2], ym[256:352].sum(0)) and torch.equal(s[-1], ym[-16:].sum(0))
    t = ym[352:448]
    assert torch.allclose(m2[3], ((t - t.mean(0)) ** 2).sum(0))
    with pytest.raises(AssertionError):
        R.stat_tiles64(y, ("raster", ((128, 2),)))


def test_bounds():
    absref = torch.tensor([2.0, 0.0])
    assert torch.equal(R.err_bound_x3(3, 576, absref), (3 * 576 + 2) * 2.0 ** -24 * absref)
    import _conv_ref
    m2 = torch.tensor([12800.0, 0.0], dtype=torch.float64)
    mean, ymax = torch.tensor([3.0, 5.0], dtype=torch.float64), torch.tensor([30.0, 5.0], dtype=torch.float64)
    # the direct bodies take _conv_ref.m2_bound as it stands
    assert torch.equal(R.m2_bound_x3(128, m2, mean, ymax, ("direct",)), _conv_ref.m2_bound(128, m2, mean))
    # the merged bodies: gamma at the leaf's size (16 + 2 + 18), plus the merges' 3 sqrt(cnt M2) 8 u Y
    b = R.m2_bound_x3(128, m2, mean, ymax, ("merged", 16, 3))
    lead = 36 * R.U * 12800 + 3 * (128 * 12800) ** 0.5 * 8 * R.U * 30
    assert lead < float(b[0]) < 1.001 * lead + 1e-9
    assert float(b[1]) > 0                             # a constant column still allows the means' roundings
    # a ragged tile shorter than a leaf: the index is the tile's own count
    short, full = (R.m2_bound_x3(c, m2, mean, ymax, ("merged", 16, 3))[0] for c in (5, 16))
    assert float(short) < float(full)
    y, by = torch.tensor([100.0], dtype=torch.float64), torch.tensor([1e-3], dtype=torch.float64)
    one = torch.ones(1, dtype=torch.float64)
    fb = R.f16bn_bound(y, by, 0.5 * one, one, 3 * one)
    assert float(fb) > 0.5 * (1e-3 + 2.0 ** -11 * 100) + 2.0 ** -11 * 54 and float(fb) < 0.06


def test_stat_body_reads_the_kernel_name():
    assert R.stat_body("conv_x3_kernel<128, false, false, 32, false, 3>", 128) == ("direct",)
    assert R.stat_body("conv_x3_kernel<64, false, false, 32, true, 1>", 128) == ("direct",)
    assert R.stat_body("conv_x3_kernel<64, false, true, 16, false, 3>", 128) == ("merged", 16, 3)
    assert R.stat_body("conv_x3_kernel<64, true, true, 16, false, 3>", 128) == ("merged", 16, 3)
    assert R.stat_body("conv_x3_a3_kernel<3>", 128) == ("merged", 16, 3)
    assert R.stat_body("conv_x3_a3_192_kernel<3>", 96) == ("merged", 12, 3)
    assert R.stat_body("conv_x3_a3_160_kernel<3>", 80) == ("merged", 20, 2)
    assert R.stat_body("conv_x3_a3_mix_kernel<3>", 96) == ("merged", 12, 3)
    assert R.stat_body("conv_x3_duo_kernel<1>", 128) == ("merged", 32, 2)
    assert R.stat_body("conv_x3_halo_bnin_kernel<3>", 128) == ("merged", 16, 3)
    assert R.stat_body("conv_x3_stem_patch_kernel<1>", 128) == ("merged", 16, 3)
    # every first launch the rows name is one of these, and both kinds are reached
    kinds = set()
    for r, _ in exact.FWD_ROWS:
        plan = bits._plans(r.name, r.entry, r.shape, r.tile, r.sk, CUS) if r.name in exact.WANT else \
            R.plans(r.entry, r.shape, r.tile, r.sk, CUS)
        for rows_, _t in plan[0]["segments"]:
            kinds.add(R.stat_body(plan[0]["name"], rows_))
    assert kinds == {("direct",), ("merged", 16, 3), ("merged", 12, 3), ("merged", 20, 2), ("merged", 32, 2)}, kinds


# ---------------------------------------------------------------- the rows ----

def _all_rows():
    """(row, op) of every exact GPU test."""
    out = [(r, "fwd") for r, _ in exact.FWD_ROWS] + [(r, "dgrad") for r, _ in exact.DGRAD_ROWS]
    out += [(R.Row(R.case_id(s), "dgrad_s2", s, 0, True, R.HI, R.LO), "dgrad") for s in exact.S2_ROWS]
    out += [(R.Row(R.case_id(s), "wgrad", s, c, True, R.HI, R.LO), "wgrad") for s in exact.WG_ROWS for c in R.WG_CUS]
    out += [(r, "fwd") for r in exact._of("f16bn")]
    return out


def test_the_tables_have_every_row():
    """The edge rows are generated from the plan when the module is imported; their number
    per entry and shape is pinned here so that an entry that stops accepting a shape, or a
    policy that stops naming its body, cannot shrink the GPU suite without a word."""
    count = {}
    for r, body in exact.FWD_ROWS + exact.DGRAD_ROWS:
        if body is not None:
            count[(r.entry, r.shape)] = count.get((r.entry, r.shape), 0) + 1
    e = R.EDGE_SHAPES
    per_shape = {e[0]: 2, e[1]: 2, e[2]: 2, e[3]: 5, e[4]: 2, e[5]: 5, e[6]: 2, e[7]: 3, e[8]: 2, e[9]: 3}
    want = {(entry, s): c for entry in ("x3", "w16", "x16") for s, c in per_shape.items()}
    want.update({("f16", s): c for s, c in per_shape.items() if s[3] % 64 == 0})
    want.update({("dgrad", s): c for s, c in {e[2]: 2, e[3]: 2, e[7]: 3, e[8]: 2, e[9]: 3}.items()})
    assert count == want, sorted(set(count.items()) ^ set(want.items()))
    assert len(exact.CATALOGUE) == 33 and len(exact.FWD_ROWS) == 127 and len(exact.DGRAD_ROWS) == 14
    assert len(exact.S2_ROWS) == 5 and len(exact.WG_ROWS) == 27 and len(exact.BNIN_ROWS) == 4
    assert len(exact.STEM_ROWS) == 7 and len(exact.FLOAT_ROWS) == 29
    assert not R.accepts("f16", e[0]) and not R.accepts("dgrad", e[5]) and R.accepts("dgrad", e[2])


def test_every_row_is_exact():
    rows = _all_rows()
    assert len(rows) == 127 + 14 + 5 + 27 * 4 + 1
    bad = [(r.name, op) for r, op in rows if not R.int_exact(r, op)]
    assert not bad, bad
    # the check bites: a layer4-sized reduction with wide ranges fails it
    assert not R.int_exact(R.Row("wide", "x3", (1, 8, 8, 512, 512, 3, 1, 1, 1), 0, True, 60, 60), "fwd")
    assert R.int_exact(R.Row("narrow", "x3", (1, 8, 8, 512, 512, 3, 1, 1, 1), 0, True, 3, 2), "fwd")


def test_the_planner_names_what_each_row_claims():
    """Catalogue rows: the kernels and forms test_gpu_x3_launch_bits lists for 256 CUs.  Edge
    rows: the body they were deduplicated by, again from the plan, and under another policy of
    the same shape a different one (the row's name says which policy)."""
    for r in exact.CATALOGUE:
        if r.entry == "dgrad_s2":
            continue
        plan = bits._plans(r.name, r.entry, r.shape, r.tile, r.sk, CUS)
        if exact.WANT[r.name] is not None:
            assert [l["name"] for l in plan] == exact.WANT[r.name], r.name
        for key, val in bits.FORMS.get(r.name, {}).items():
            assert plan[0][key] == val, (r.name, key)
    for rows in (exact.FWD_ROWS, exact.DGRAD_ROWS):
        seen = {}
        for r, body in rows:
            if body is None:
                continue
            assert R.body_of(R.plans(r.entry, r.shape, r.tile, r.sk, CUS)) == body, r.name
            assert body not in seen.setdefault((r.entry, r.shape), set()), r.name     # one row per body
            seen[(r.entry, r.shape)].add(body)
    # the rows the issue names land where it says
    def name(entry, shape, tile):
        return R.plans(entry, shape, tile, True, CUS)[0]["name"]
    assert name("x3", (1, 16, 64, 64, 64, 3, 1, 1, 1), 0) == "conv_x3_halo_kernel<3>"
    assert name("x3", (1, 8, 32, 64, 64, 3, 1, 1, 1), 0) == "conv_x3_halo_kernel<3>"
    assert "halo" not in name("x3", (1, 17, 64, 64, 64, 3, 1, 1, 1), 0)
    assert R.plans("x3", (1, 1, 1, 32, 64, 1, 1, 0, 1), 0, True, CUS)[0]["nks"] == 1
    assert R.plans("f16", (1, 1, 1, 32, 64, 1, 1, 0, 1), 0, True, CUS) == []          # 64-channel lines
    for e, s, t in exact.STEM_ROWS:
        patch = t == 0 and not (R.out_hw(s)[0] % R.PATCH_H or R.out_hw(s)[1] % R.PATCH_W)
        got = ops.launch_plan(R.desc(s, t, "nchw"), R.kop(e), True, CUS)[0]["name"]
        assert got.startswith("conv_x3_stem_patch_kernel") == patch, (e, s, t, got)


def test_the_rows_reach_every_kernel_and_both_wgrad_bodies():
    seen = set()
    for r, _ in exact.FWD_ROWS + exact.DGRAD_ROWS:
        if r.name in exact.WANT:
            seen |= {l["kernel"] for l in bits._plans(r.name, r.entry, r.shape, r.tile, r.sk, CUS)}
        else:
            seen |= {l["kernel"] for l in R.plans(r.entry, r.shape, r.tile, r.sk, CUS)}
    for r in exact.BNIN_ROWS:
        seen |= {l["kernel"] for l in bits._plans(r.name, r.entry, r.shape, r.tile, r.sk, CUS)}
    for e, s, t in exact.STEM_ROWS + [("stem_u8", bits.STEM, 0)]:
        seen |= {l["kernel"] for l in ops.launch_plan(R.desc(s, t, "nchw"), R.kop(e), True, CUS)}
    assert seen == set(range(_lib.HKP_X3K_COUNT)), sorted(set(range(_lib.HKP_X3K_COUNT)) - seen)
    wg = {ops.kernel_name(R.desc(s, c), _lib.HKP_KOP_WGRAD_X3) for s in exact.WG_ROWS for c in R.WG_CUS}
    assert wg == {"wgrad_x3_halo_kernel", "wgrad_x3_kernel<64>", "wgrad_x3_kernel<128>", "wgrad_x3_kernel<256>"}, wg
