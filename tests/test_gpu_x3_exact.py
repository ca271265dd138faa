"""The f16x3 / plain-fp16 convs (csrc/conv_x3.hip and its x3_*.h bodies, csrc/wgrad_x3.hip, the
packers of csrc/pack_x3.hip) at every kernel form, exact on integer
planes: hand-built UNRELATED hi / lo planes of small integers make every product and every
partial sum an integer below 2^24 whatever the body, so the output must equal the fp64
reference of exactly the products the mode keeps BIT FOR BIT (tests/_x3_ref.py has the
argument, the references and the bounds); a wrong tap, plane, channel group, row or column
at a single element is reported with its index.  The rows are the catalogue of
test_gpu_x3_launch_bits.CASES (every kernel id and launch form on 256 CUs) plus the edge
rows of _x3_ref under every tile policy the plan tells apart.  One float-data test judges
the catalogue rows elementwise by the a-priori dot-product bound and prints the ratios.

A row's body depends on the CU count: each test asserts that the plan on THIS device names
the body the row was listed for (on 256 CUs) and fails — it does not skip — otherwise."""
import functools
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
import test_gpu_x3_launch_bits as bits  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 20
SENTINEL = -12345.6796875      # exact in fp32; no integer-plane result (a multiple of 1/4) equals it
GUARD = 4096
AMAX = 2.0 ** 10               # the gradient scale is then pow2_scale(2^10) = 2^3 (max -> [2^13, 2^14))

CATALOGUE = [R.Row(name, entry, shape, tile, sk, R.HI, R.LO) for name, entry, shape, tile, sk, _ in bits.CASES]
WANT = {c[0]: c[5] for c in bits.CASES}


def _of(*entries):
    return [r for r in CATALOGUE if r.entry in entries]


# (row, the body the plan names on 256 CUs or None: the catalogue's own `want` list)
FWD_ROWS = [(r, None) for r in _of(*R.FWD_ENTRIES)] + R.edge_rows()
DGRAD_ROWS = [(r, None) for r in _of("dgrad")] + R.edge_rows(("dgrad",))
S2_ROWS = [(n, h, w, ci, co, k, 2, pad, 1) for n, h, w, ci, co, k, pad in prec.STRIDED_CASES] + \
    [r.shape for r in _of("dgrad_s2")]
WG_ROWS = list(dict.fromkeys(list(prec.WG_X3_CASES) + R.WG_EDGE))
BNIN_ROWS = _of("x3_bnin", "f16_bnin") + [R.Row("bnin-" + R.case_id(s), "x3_bnin", s, 0, True, R.HI, R.LO)
                                          for s in R.EDGE_SHAPES if s[1:3] in ((16, 64), (8, 32))]


def _ids(rows):
    return [r[0].name for r in rows]


def _first_diff(got, ref, names):
    """The first differing index of two equal-shaped CPU tensors, as text."""
    bad = (got != ref) | (got.isnan() != ref.isnan())
    if not bool(bad.any()):
        return None
    idx = tuple(int(v) for v in bad.nonzero()[0])
    return "%d of %d elements differ; first at (%s) = %s: got %r, reference %r" % (
        int(bad.sum()), bad.numel(), ",".join(names), idx, got[idx].item(), ref[idx].item())


def _check_body(row, want_body, cuda_device):
    """The plan on this device names the body the row is listed for."""
    if row.entry.endswith("_bnin") or want_body is None and row.name in WANT:
        plan = bits._plans(row.name, row.entry, row.shape, row.tile, row.sk, 0)
        if WANT.get(row.name) is not None:
            assert [l["name"] for l in plan] == WANT[row.name], \
                "%s: this device plans %s" % (row.name, [l["name"] for l in plan])
        for key, val in bits.FORMS.get(row.name, {}).items():
            assert plan[0][key] == val, (row.name, key, plan[0][key])
        if row.entry.endswith("_bnin"):
            assert [l["name"] for l in plan] == ["conv_x3_halo_bnin_kernel<%d>" % R.PRODUCTS[row.entry]], \
                "%s: this device plans %s" % (row.name, [l["name"] for l in plan])
        return plan
    plan = R.plans(row.entry, row.shape, row.tile, row.sk, 0)
    assert plan, "%s: the entry rejects the row on this device" % row.name
    if want_body is not None:
        assert R.body_of(plan) == want_body, "%s: this device plans %s" % (row.name, R.body_of(plan))
    return plan


def _guarded(shape, dev):
    """A view of `shape` inside a sentinel-filled buffer with GUARD elements on either side."""
    n = 1
    for v in shape:
        n *= v
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=dev, dtype=torch.float32)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


@functools.lru_cache(maxsize=2)
def _fwd_ref(shape, P, hi, lo):
    """(y reference as fp32 NHWC — exact: asserted —, tile statistics come from the fp64 one)."""
    p = R.int_planes(shape, SEED, "fwd", hi, lo)
    y64 = R.ref64(p, shape, "fwd", P)
    y32 = y64.float()
    assert torch.equal(y32.double(), y64)
    return R.nhwc(y32), y64


def _run_fwd(ops, row, ops_in, stats=True, out=None, part_out=None):
    xs, wp = ops_in
    n, h, w, cin, cout, k, st, pad, dil = row.shape
    if row.entry == "f16":
        return ops.conv2d_fwd_f16(xs, wp, st, pad, dil, stats=stats, sk=row.sk, tile=row.tile)
    return ops.conv2d_fwd_x3(xs, wp, st, pad, dil, stats=stats, out=out, part_out=part_out, sk=row.sk,
                             tile=row.tile, products=R.PRODUCTS[row.entry])


def _layout(plan):
    name = plan[0]["name"]
    if "halo" in name or "stem_patch" in name:
        return ("patch",)
    return ("raster", plan[0]["segments"])


def _check_partials(ops, part, y64, plan, what):
    """sum plane == the fp64 tile sum bit for bit; M2 within m2_bound_x3 for the body the
    plan names (_conv_ref.m2_bound where the squares are taken about the tile's own mean, the
    bound extended by the merges' roundings where sub-tiles are merged), exactly +0 on one-row
    tiles.  Returns the largest err / bound."""
    layout = _layout(plan)
    if layout[0] == "raster":
        segs = ops.stat_segments(part) or ((ops.stat_tile_rows(part), part.shape[0]),)
        assert tuple(segs) == tuple(layout[1]), (what, segs, layout[1])
    s, m2, mu, cnt, ymax, nominal = R.stat_tiles64(y64, layout)
    # the body that writes the partials: the first launch's (a split-K tail kernel that follows
    # it is conv_x3_tile's 16x16x32 form, as the 256-wide main kernel is)
    name = plan[0]["name"]
    got = part.cpu()
    assert got.shape[0] == s.shape[0], (what, got.shape, s.shape)
    diff = _first_diff(got[:, :, 0].double(), s, ("tile", "k"))
    assert diff is None, "%s: BN tile sums: %s" % (what, diff)
    worst = 0.0
    for t, c in enumerate(cnt):
        q = got[t, :, 1].double()
        if c == 1:
            assert bool((q == 0).all()) and not bool(torch.signbit(q).any()), "%s: one-row tile %d: M2 %s" % (
                what, t, q[q != 0][:4])
            continue
        bound = R.m2_bound_x3(c, m2[t], mu[t], ymax[t], R.stat_body(name, nominal[t]))
        err = (q - m2[t]).abs()
        ok = err <= bound
        assert bool(ok.all()), "%s: M2 of tile %d, k=%d: got %r, reference %r, bound %r" % (
            what, t, int((~ok).nonzero()[0]), q[~ok][0].item(), m2[t][~ok][0].item(), bound[~ok][0].item())
        live = bound > 0
        if bool(live.any()):
            worst = max(worst, float((err[live] / bound[live]).max()))
    return worst


@pytest.mark.parametrize("row,body", FWD_ROWS, ids=_ids(FWD_ROWS))
def test_forward_exact(cuda_device, row, body):
    """x3 / w16 / x16 / plain f16 forward on hand-built integer planes: y, the BN tile sums
    and (within its bound) M2, twice with the same bits, into guarded views, stats=False."""
    from hkp import ops
    dev = cuda_device
    assert R.int_exact(row, "fwd")
    plan = _check_body(row, body, dev)
    P = R.PRODUCTS[row.entry]
    p = R.int_planes(row.shape, SEED, "fwd", row.hi, row.lo)
    ref, y64 = _fwd_ref(row.shape, P, row.hi, row.lo)
    xs = R.pack_act(p["hx"], p["lx"], P).to(dev)
    xs._hkp_split_passes = 1 if P == 1 else 3
    wp = ops.PackedWeight(R.pack_w(p["hw"], p["lw"], P).to(dev), p["inv"].to(dev))
    names = ("n", "h", "w", "k")
    if P == 1:
        y, part = _run_fwd(ops, row, (xs, wp))
        y2, part2 = _run_fwd(ops, row, (xs, wp))
        ref = ref.half()                                 # ref is exact in fp32: one rounding
        ybuf = pbuf = None
    else:
        tiles = sum(t for _, t in plan[0]["segments"])
        ybuf, yv = _guarded(tuple(ref.shape), dev)
        pbuf, pv = _guarded((tiles, row.shape[4], 2), dev)
        y, part = _run_fwd(ops, row, (xs, wp), out=yv, part_out=pv)
        y2, part2 = _run_fwd(ops, row, (xs, wp))
    diff = _first_diff(y.cpu(), ref, names)
    assert diff is None, "%s: %s" % (row.name, diff)
    assert torch.equal(y2, y) and torch.equal(part2, part), "%s: two runs differ" % row.name
    if ybuf is not None:
        assert _guards_intact(ybuf) and _guards_intact(pbuf), "%s: a store outside the output" % row.name
    print("M2RATIO %s %s %.3g" % (row.entry, row.name, _check_partials(ops, part, y64, plan, row.name)))
    y3, p3 = _run_fwd(ops, row, (xs, wp), stats=False)
    assert p3 is None and torch.equal(y3, y), "%s: stats=False changes y" % row.name


def test_f16bn_exact(cuda_device):
    """The fused-BN fp16 epilogue: out = f16(relu(f16(acc) * s + t + res)) with power-of-two
    s and integer t, res — every step after the first rounding is exact in fp32."""
    from hkp import ops
    (row,) = _of("f16bn")
    dev = cuda_device
    _check_body(row, None, dev)
    n, h, w, cin, cout, k, st, pad, dil = row.shape
    p = R.int_planes(row.shape, SEED, "fwd", row.hi, row.lo)
    g = torch.Generator().manual_seed(SEED + 1)
    s = 2.0 ** torch.randint(-1, 2, (cout,), generator=g).float() * (1 - 2 * torch.randint(0, 2, (cout,), generator=g))
    t = torch.randint(-40, 41, (cout,), generator=g).float()
    ho, wo = R.out_hw(row.shape)
    res = torch.randint(-40, 41, (n, ho, wo, cout), generator=g).half()
    y16 = R.nhwc(R.ref64(p, row.shape, "fwd", 1)).float().half().double()
    ref = torch.relu(y16 * s.double() + t.double() + res.double()).float().half()
    x16 = R.pack_act(p["hx"], p["lx"], 1).to(dev)
    x16._hkp_split_passes = 1
    wp = ops.PackedWeight(R.pack_w(p["hw"], p["lw"], 1).to(dev), p["inv"].to(dev))
    outs = [ops.conv2d_fwd_f16_bn(x16, wp, torch.cat([s, t]).to(dev), res=res.to(dev), relu=True, stride=st, pad=pad,
                                  dil=dil, sk=row.sk, tile=row.tile) for _ in range(2)]
    diff = _first_diff(outs[0].cpu(), ref, ("n", "h", "w", "k"))
    assert diff is None, diff
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------- dgrad ----

def _amax_bits(dev):
    return torch.tensor([AMAX], dtype=torch.float32).view(torch.int32).to(dev)


@pytest.mark.parametrize("row,body", DGRAD_ROWS, ids=_ids(DGRAD_ROWS))
def test_dgrad_exact(cuda_device, row, body):
    """Stride-1 dgrad on hand-built dy planes and a hand-built flipped pack, without a
    gradient scale and with amax = 2^10 (dx = acc / 8): dx bit-equal, addend included."""
    from hkp import ops
    dev = cuda_device
    assert R.int_exact(row, "dgrad")
    _check_body(row, body, dev)
    n, h, w, cin, cout, k, st, pad, dil = row.shape
    p = R.int_planes(row.shape, SEED, "dgrad", row.hi, row.lo)
    dys = R.pack_act(p["hdy"], p["ldy"]).to(dev)
    wfp = ops.PackedWeight(R.pack_w_flip(p["hw"], p["lw"]).to(dev), p["inv"].to(dev))
    add = R.nhwc(p["add"]).to(dev)
    noadd = {q: v for q, v in p.items() if q != "add"}
    base = R.nhwc(R.ref64(noadd, row.shape, "dgrad"))                # inv[c] * acc
    for amax, gscale in ((None, 1.0), (_amax_bits(dev), R.pow2_scale(AMAX))):
        ref = (base / gscale + add.cpu().double()).float()
        dx = [ops.conv2d_bwd_data_x3(dys, wfp, (n, h, w, cin), pad, dil, add=add, amax=amax, sk=row.sk,
                                     tile=row.tile) for _ in range(2)]
        diff = _first_diff(dx[0].cpu(), ref, ("n", "h", "w", "c"))
        assert diff is None, "%s (gradient scale %g): %s" % (row.name, gscale, diff)
        assert torch.equal(dx[0], dx[1])
    dx0 = ops.conv2d_bwd_data_x3(dys, wfp, (n, h, w, cin), pad, dil, sk=row.sk, tile=row.tile)
    diff = _first_diff(dx0.cpu(), base.float(), ("n", "h", "w", "c"))
    assert diff is None, "%s (no addend): %s" % (row.name, diff)


@pytest.mark.parametrize("shape", S2_ROWS, ids=[R.case_id(s) for s in S2_ROWS])
def test_dgrad_strided_exact(cuda_device, shape):
    """Stride-2 dgrad, one stride-1 conv per output phase on slices of the hand-built flipped
    pack: dx bit-equal, and equal to the addend wherever no gradient arrives (the add-only
    phases of a 1x1 stride-2 conv are three quarters of dx)."""
    from hkp import ops
    dev = cuda_device
    row = R.Row(R.case_id(shape), "dgrad_s2", shape, 0, True, R.HI, R.LO)
    assert R.int_exact(row, "dgrad")
    n, h, w, cin, cout, k, st, pad, dil = shape
    p = R.int_planes(shape, SEED, "dgrad")
    dys = R.pack_act(p["hdy"], p["ldy"]).to(dev)
    flipped = R.pack_w_flip(p["hw"], p["lw"])                       # [C, R, S, 2K]
    inv = p["inv"].to(dev)
    packs = []
    for ph in range(4):
        rws, cls = R.phase_slices(k, pad, ph)
        packs.append(ops.PackedWeight(flipped[:, rws][:, :, cls].contiguous().to(dev), inv) if rws and cls else None)
    for ph, pk in enumerate(packs):
        assert (pk is None) == (min(ops.phase_taps(k, pad, ph >> 1), ops.phase_taps(k, pad, ph & 1)) <= 0)
    add = R.nhwc(p["add"]).to(dev)
    base = R.nhwc(R.ref64({q: v for q, v in p.items() if q != "add"}, shape, "dgrad"))
    for amax, gscale in ((None, 1.0), (_amax_bits(dev), R.pow2_scale(AMAX))):
        ref = (base / gscale + add.cpu().double()).float()
        dx = [ops.conv2d_bwd_data_x3_strided(dys, packs, (n, h, w, cin), (cout, k, k, cin), pad, add=add, amax=amax)
              for _ in range(2)]
        diff = _first_diff(dx[0].cpu(), ref, ("n", "h", "w", "c"))
        assert diff is None, "%s (gradient scale %g): %s" % (row.name, gscale, diff)
        assert torch.equal(dx[0], dx[1])
    if k == 1:                                                       # no gradient reaches odd rows / columns
        got = dx[0].cpu()
        assert torch.equal(got[:, 1::2], add.cpu()[:, 1::2]) and torch.equal(got[:, :, 1::2], add.cpu()[:, :, 1::2])


# ---------------------------------------------------------------------- wgrad ----

@functools.lru_cache(maxsize=1)
def _wg_ref(shape):
    return R.nhwc(R.ref64(R.int_planes(shape, SEED, "wgrad"), shape, "wgrad"))


@pytest.mark.parametrize("cus", R.WG_CUS)
@pytest.mark.parametrize("shape", WG_ROWS, ids=[R.case_id(s) for s in WG_ROWS])
def test_wgrad_exact(cuda_device, shape, cus):
    """wgrad on hand-built x and dy planes, on both bodies and every CU budget: dw bit-equal
    (the pixel splits' slabs are sums of integers too), with and without a gradient scale."""
    from hkp import _lib, ops
    dev = cuda_device
    row = R.Row(R.case_id(shape), "wgrad", shape, cus, True, R.HI, R.LO)
    assert R.int_exact(row, "wgrad")
    n, h, w, cin, cout, k, st, pad, dil = shape
    name = ops.kernel_name(R.desc(shape, cus), _lib.HKP_KOP_WGRAD_X3)
    halo = prec._wg_halo(shape) and cus != -1
    assert name == "wgrad_x3_halo_kernel" if halo else name.startswith("wgrad_x3_kernel<"), name
    p = R.int_planes(shape, SEED, "wgrad")
    xs, dys = R.pack_act(p["hx"], p["lx"]).to(dev), R.pack_act(p["hdy"], p["ldy"]).to(dev)
    for amax, gscale in ((None, 1.0), (_amax_bits(dev), R.pow2_scale(AMAX))):
        ref = (_wg_ref(shape) / gscale).float()
        dw = [ops.conv2d_bwd_filter_x3(xs, dys, (cout, k, k, cin), st, pad, dil, amax=amax, cus=cus) for _ in range(2)]
        diff = _first_diff(dw[0].cpu(), ref, ("k", "r", "s", "c"))
        assert diff is None, "%s cus %d (gradient scale %g): %s" % (row.name, cus, gscale, diff)
        assert torch.equal(dw[0], dw[1])


# ------------------------------------------------------------- fused input BN ----

@pytest.mark.parametrize("row", BNIN_ROWS, ids=[r.name for r in BNIN_ROWS])
def test_fused_input_bn_exact(cuda_device, row):
    """conv2d_fwd_bnin splits relu(y_in * a + b) inside the kernel, so it is driven through
    real values: integers with x odd in [2049, 4095] (f16x3: hi = f16(x) is even, lo = +-1 or
    0, hi + lo == x) or x a small integer with negatives the ReLU clears (plain fp16), b != 0.
    y bit-equal to the reference of the torch-side split: padded taps contribute exactly 0,
    not b."""
    from hkp import ops
    dev = cuda_device
    _check_body(row, None, dev)
    n, h, w, cin, cout, k, st, pad, dil = row.shape
    f16 = row.entry == "f16_bnin"
    P = 1 if f16 else 3
    g = torch.Generator().manual_seed(SEED + 2)
    a = torch.tensor([1.0, 2.0, -1.0])[torch.randint(0, 3, (cin,), generator=g)]
    if f16:
        b = (torch.randint(1, 4, (cin,), generator=g) * (1 - 2 * torch.randint(0, 2, (cin,), generator=g))).float()
        y_in = torch.randint(-8, 9, (n, h, w, cin), generator=g).float()
        x = torch.relu(y_in * a + b)
        assert bool((x == 0).any()) and float(x.max()) <= 2048
        hi, lo = x.half().float(), torch.zeros_like(x)
        hw_, lw_ = 2, 0
    else:
        b = (2 * torch.randint(1, 40, (cin,), generator=g) + 1).float() * (1 - 2 * torch.randint(0, 2, (cin,), generator=g))
        x = (2 * torch.randint(1024, 2048, (n, h, w, cin), generator=g) + 1).float()       # odd, 2049 .. 4095
        y_in = (x - b) / a                                                                  # x - b is even: exact
        assert torch.equal(torch.relu(y_in * a + b), x) and bool((b != 0).all())
        hi = x.half().float()
        lo = (x - hi).half().float()
        assert torch.equal(hi + lo, x) and bool((lo != 0).any()) and bool((hi % 2 == 0).all())
        hw_, lw_ = 2, 1
    # |x| <= 4096: (hw + lw) * 4096 L + hw L < 2^24 is the 2^24 condition of this test's ranges
    assert ((hw_ + lw_) * 4096 + hw_) * R.red_len(row.shape, "fwd") < 2 ** 24
    pw = R.int_planes(row.shape, SEED, "fwd", hw_, max(lw_, 1))
    lw = pw["lw"] if lw_ else torch.zeros_like(pw["lw"])
    planes = dict(hx=R.nchw(hi), lx=R.nchw(lo), hw=pw["hw"], lw=lw, inv=pw["inv"])
    y64 = R.ref64(planes, row.shape, "fwd", P)
    ref = R.nhwc(y64.float())
    assert torch.equal(R.nhwc(y64), ref.double())
    wp = ops.PackedWeight(R.pack_w(pw["hw"], lw, P).to(dev), pw["inv"].to(dev))
    yin_d = (y_in.half() if f16 else y_in).to(dev)
    ss = torch.cat([a, b]).to(dev)
    got = [ops.conv2d_fwd_bnin(yin_d, ss, wp, st, pad, dil, sk=row.sk, tile=row.tile)[0] for _ in range(2)]
    diff = _first_diff(got[0].cpu(), ref.half() if f16 else ref, ("n", "h", "w", "k"))
    assert diff is None, "%s: %s" % (row.name, diff)
    assert torch.equal(got[0], got[1])


# ----------------------------------------------------------------------- stem ----

def _stem_inputs(family, shape):
    """(A) x in {0..3}, w 14-bit integers with every filter's max in [8192, 16383]: the pack's
    scale is 1, lo_w in [-4, 4], lx == 0, so the three products are x * w exactly and the worst
    sum 147 * 3 * 16383 < 2^24.  (B) x odd 12-bit integers (hi + lo == x, lo != 0 on many),
    w in {-1, 0, 1}, scaled to +-2^13 by the pack: every partial sum is 2^13 times an integer
    below 147 * 4095, hence exact.  (C) x in {0..3}, w in {-1, 0, 1}: |y| <= 3 * 147, so the
    BN tile sums (128 rows) are exact too — A and B pin y, C pins the partials."""
    n, h, w, c, cout = shape[:5]
    g = torch.Generator().manual_seed(SEED + 3)
    if family == "C":
        x = torch.randint(0, 4, (n, c, h, w), generator=g).float()
        wt = torch.randint(-1, 2, (cout, c, 7, 7), generator=g).float()
    elif family == "A":
        x = torch.randint(0, 4, (n, c, h, w), generator=g).float()
        wt = torch.randint(-16383, 16384, (cout, c, 7, 7), generator=g).float()
        wt[:, 0, 0, 0] = torch.randint(8192, 16384, (cout,), generator=g).float()
    else:
        x = (2 * torch.randint(0, 2048, (n, c, h, w), generator=g) + 1).float()
        wt = torch.randint(-1, 2, (cout, c, 7, 7), generator=g).float()
    return x, wt


STEM_ROWS = [(entry, shape, tile) for shape in R.STEM_SHAPES for entry, tile in
             (("stem_planes", 0), ("stem_image", 0), ("stem_planes", 6))      # 6: HKP_TILE_64_PAIR
             if not (entry == "stem_image" and (R.out_hw(shape)[0] % R.PATCH_H or R.out_hw(shape)[1] % R.PATCH_W))]


@pytest.mark.parametrize("family", ["A", "B", "C"])
@pytest.mark.parametrize("entry,shape,tile", STEM_ROWS,
                         ids=["%s-%s-t%d" % (e, R.case_id(s), t) for e, s, t in STEM_ROWS])
def test_stem_exact(cuda_device, entry, shape, tile, family):
    """The stem's fp32-image entries (packed planes, image-direct, the one-tile pair body)
    through the real weight packer on integer families A and B, each keeping one cross term
    alive: y bit-equal to the fp64 conv; on family C also the BN tile sums, M2 within its
    bound."""
    from hkp import ops
    dev = cuda_device
    n, h, w, c, cout = shape[:5]
    x, wt = _stem_inputs(family, shape)
    y64 = torch.nn.functional.conv2d(x.double(), wt.double(), None, 2, 3)
    plan = ops.launch_plan(R.desc(shape, tile, "nchw"), R.kop(entry), True, 0)
    patch = not (R.out_hw(shape)[0] % R.PATCH_H or R.out_hw(shape)[1] % R.PATCH_W) and tile == 0
    want = {"stem_planes": "conv_x3_stem_patch_kernel<0>", "stem_image": "conv_x3_stem_patch_kernel<1>"}[entry] \
        if patch else "conv_x3_kernel<64, true, true, 16, false, 3>"
    assert [l["name"] for l in plan] == [want], plan
    wp = ops.stem_weight_pack_x3(wt.to(dev))
    if family == "A":
        assert bool((wp.inv_scale == 1).all())
    outs = [ops.conv2d_fwd_stem_x3(x.to(dev), wp, cout, tile=tile, image_direct=entry == "stem_image") for _ in range(2)]
    y, part = outs[0]
    ref = R.nhwc(y64.float())
    diff = _first_diff(y.cpu(), ref, ("n", "h", "w", "k"))
    assert diff is None, "%s %s family %s: %s" % (entry, R.case_id(shape), family, diff)
    assert torch.equal(outs[1][0], y) and torch.equal(outs[1][1], part)
    pbuf, pv = _guarded(tuple(part.shape), dev)
    _, part_g = ops.conv2d_fwd_stem_x3(x.to(dev), wp, cout, part_out=pv, tile=tile, image_direct=entry == "stem_image")
    assert torch.equal(part_g, part) and _guards_intact(pbuf)
    if family == "C":
        assert 128 * 3 * 49 * c < 2 ** 24
        print("M2RATIO %s %s-%s %.3g" % (entry, R.case_id(shape), family,
                                         _check_partials(ops, part, y64, plan, entry + R.case_id(shape))))
    y0, p0 = ops.conv2d_fwd_stem_x3(x.to(dev), wp, cout, stats=False, tile=tile, image_direct=entry == "stem_image")
    assert p0 is None and torch.equal(y0, y)


def test_stem_u8_equals_the_image_entry(cuda_device):
    """The u8 entry divides by 255 and is not exact: it must equal the fp32-image entry fed
    u8.float() / 255, bit for bit (y and partials)."""
    from hkp import ops
    dev = cuda_device
    shape = bits.STEM
    n, h, w, c, cout = shape[:5]
    g = torch.Generator().manual_seed(SEED + 4)
    img = torch.randint(0, 256, (n, h, w, c), generator=g, dtype=torch.uint8)
    wt = torch.randn(cout, c, 7, 7, generator=g) * 0.1
    wp = ops.stem_weight_pack_x3(wt.to(dev))
    assert [l["name"] for l in ops.launch_plan(R.desc(shape, 0, "nchw"), R.kop("stem_u8"), True, 0)] == \
        ["conv_x3_stem_patch_kernel<2>"]
    yu, pu = ops.conv2d_fwd_stem_x3(img.to(dev), wp, cout)
    yf, pf = ops.conv2d_fwd_stem_x3((R.nchw(img.float()) / 255).to(dev), wp, cout)
    diff = _first_diff(yu.cpu(), yf.cpu(), ("n", "h", "w", "k"))
    assert diff is None, diff
    assert torch.equal(pu, pf)


# ------------------------------------------------- through the real producers ----

PROD_SHAPE = (1, 9, 14, 32, 192, 3, 1, 2, 2)        # L = 288: family A's 3 * 16383 L < 2^24
PROD_BWD = (2, 7, 9, 64, 64, 3, 1, 1, 1)            # dgrad L = 576, wgrad L = 126


def _family(family, g, xshape, wshape):
    if family == "A":
        x = torch.randint(0, 4, xshape, generator=g).float()
        wt = torch.randint(-16383, 16384, wshape, generator=g).float()
        wt[:, 0, 0, 0] = torch.randint(8192, 16384, (wshape[0],), generator=g).float()
    else:
        x = (2 * torch.randint(0, 2048, xshape, generator=g) + 1).float()
        x = x * (1 - 2 * torch.randint(0, 2, xshape, generator=g))
        wt = torch.randint(-1, 2, wshape, generator=g).float()
    return x, wt


@pytest.mark.parametrize("family", ["A", "B"])
def test_forward_through_the_producers(cuda_device, family):
    """bn_apply(split=3) and weight_pack_x3 on the stem test's two integer families: the
    three products are x * w exactly, so y equals the fp64 conv of the fp32 values — the
    hand-built planes of the tests above are what training feeds."""
    from hkp import ops
    dev = cuda_device
    n, h, w, cin, cout, k, st, pad, dil = PROD_SHAPE
    x, wt = _family(family, torch.Generator().manual_seed(SEED + 5), (n, cin, h, w), (cout, cin, k, k))
    worst = (3 * 16383 if family == "A" else 4095) * k * k * cin
    assert worst < 2 ** 24
    y64 = torch.nn.functional.conv2d(x.double(), wt.double(), None, st, pad, dil)
    ident = torch.cat([torch.ones(cin), torch.zeros(cin)]).to(dev)
    xs = ops.bn_apply(R.nhwc(x).to(dev), ident, relu=False, split=3, keep_fp32=False)
    y, _ = ops.conv2d_fwd_x3(xs, ops.weight_pack_x3(R.nhwc(wt).to(dev)), st, pad, dil)
    diff = _first_diff(y.cpu(), R.nhwc(y64.float()), ("n", "h", "w", "k"))
    assert diff is None, diff


@pytest.mark.parametrize("entry,family", [("w16", "B"), ("x16", "A")])
def test_product_subsets_through_the_producers(cuda_device, entry, family):
    """HKP_X3_W16 keeps (hx + lx) * hw: family B's weights (+-2^13 after the pack, lw == 0) lose
    nothing.  HKP_X3_X16 keeps hx * (hw + lw): family A's activations ({0..3}, lx == 0) lose
    nothing.  Either way y equals the fp64 conv of the fp32 values, through bn_apply(split=3)
    and weight_pack_x3."""
    from hkp import ops
    dev = cuda_device
    n, h, w, cin, cout, k, st, pad, dil = PROD_SHAPE
    x, wt = _family(family, torch.Generator().manual_seed(SEED + 7), (n, cin, h, w), (cout, cin, k, k))
    assert (3 * 16383 if family == "A" else 4095) * k * k * cin < 2 ** 24
    y64 = torch.nn.functional.conv2d(x.double(), wt.double(), None, st, pad, dil)
    ident = torch.cat([torch.ones(cin), torch.zeros(cin)]).to(dev)
    xs = ops.bn_apply(R.nhwc(x).to(dev), ident, relu=False, split=3, keep_fp32=False)
    wp = ops.weight_pack_x3(R.nhwc(wt).to(dev))
    y, _ = ops.conv2d_fwd_x3(xs, wp, st, pad, dil, products=R.PRODUCTS[entry])
    diff = _first_diff(y.cpu(), R.nhwc(y64.float()), ("n", "h", "w", "k"))
    assert diff is None, "%s: %s" % (entry, diff)
    # and the subset matters on the other family: the dropped product is alive there
    x2, w2 = _family("A" if family == "B" else "B", torch.Generator().manual_seed(SEED + 7), (n, cin, h, w),
                     (cout, cin, k, k))
    xs2 = ops.bn_apply(R.nhwc(x2).to(dev), ident, relu=False, split=3, keep_fp32=False)
    wp2 = ops.weight_pack_x3(R.nhwc(w2).to(dev))
    full, _ = ops.conv2d_fwd_x3(xs2, wp2, st, pad, dil)
    part, _ = ops.conv2d_fwd_x3(xs2, wp2, st, pad, dil, products=R.PRODUCTS[entry])
    assert not torch.equal(full, part)


def _bwd_inputs(dev):
    """Family B on PROD_BWD: odd 12-bit gradients against weights in {-1, 0, 1}, split with
    their absmax scale."""
    from hkp import ops
    n, h, w, cin, cout, k, st, pad, dil = PROD_BWD
    g = torch.Generator().manual_seed(SEED + 6)
    ho, wo = R.out_hw(PROD_BWD)
    dy, wt = _family("B", g, (n, cout, ho, wo), (cout, cin, k, k))
    assert 4095 * k * k * cout < 2 ** 24 and 4095 * n * ho * wo < 2 ** 24
    amax = ops.absmax(R.nhwc(dy).to(dev))
    return g, dy, wt, amax, ops.split_pack_x3(R.nhwc(dy).to(dev), amax)


def test_dgrad_through_the_producers(cuda_device):
    """split_pack_x3 (with the absmax scale) and weight_flip_pack_x3: dx equals the fp64
    gradient of the fp32 values exactly."""
    from hkp import ops
    dev = cuda_device
    n, h, w, cin, cout, k, st, pad, dil = PROD_BWD
    g, dy, wt, amax, dys = _bwd_inputs(dev)
    add = torch.randint(-3, 4, (n, cin, h, w), generator=g).float()
    dx = ops.conv2d_bwd_data_x3(dys, ops.weight_flip_pack_x3(R.nhwc(wt).to(dev)), (n, h, w, cin), pad, dil,
                                add=R.nhwc(add).to(dev), amax=amax)
    ref = torch.nn.grad.conv2d_input((n, cin, h, w), wt.double(), dy.double(), st, pad, dil) + add.double()
    diff = _first_diff(dx.cpu(), R.nhwc(ref.float()), ("n", "h", "w", "c"))
    assert diff is None, diff


def test_strided_dgrad_through_the_producers(cuda_device):
    """The same gradient through a stride-2 conv of (2h - 1) x (2w - 1) inputs: the batched
    phase packer (weight_phase_pack_x3)."""
    from hkp import ops
    dev = cuda_device
    n, h, w, cin, cout, k, st, pad, dil = PROD_BWD
    g, dy, wt, amax, dys = _bwd_inputs(dev)
    h2, w2 = 2 * h - 1, 2 * w - 1
    assert R.out_hw((n, h2, w2, cin, cout, k, 2, pad, 1)) == R.out_hw(PROD_BWD)
    add2 = torch.randint(-3, 4, (n, cin, h2, w2), generator=g).float()
    dx2 = ops.conv2d_bwd_data_x3_strided(dys, ops.weight_phase_pack_x3(R.nhwc(wt).to(dev), pad), (n, h2, w2, cin),
                                         (cout, k, k, cin), pad, add=R.nhwc(add2).to(dev), amax=amax)
    ref2 = torch.nn.grad.conv2d_input((n, cin, h2, w2), wt.double(), dy.double(), 2, pad, 1) + add2.double()
    diff = _first_diff(dx2.cpu(), R.nhwc(ref2.float()), ("n", "h", "w", "c"))
    assert diff is None, diff


def test_wgrad_through_the_producers(cuda_device):
    """x odd 12-bit (hi + lo == x), dy in {-1, 0, 1} scaled to +-2^13 by its absmax, both
    through split_pack_x3: dw equals the fp64 gradient exactly."""
    from hkp import ops
    dev = cuda_device
    n, h, w, cin, cout, k, st, pad, dil = PROD_BWD
    ho, wo = R.out_hw(PROD_BWD)
    assert 4095 * n * ho * wo < 2 ** 24
    x, dyw = _family("B", torch.Generator().manual_seed(SEED + 8), (n, cin, h, w), (n, cout, ho, wo))
    dyw_d = R.nhwc(dyw).to(dev)
    amax_w = ops.absmax(dyw_d)
    dw = ops.conv2d_bwd_filter_x3(ops.split_pack_x3(R.nhwc(x).to(dev)), ops.split_pack_x3(dyw_d, amax_w),
                                  (cout, k, k, cin), st, pad, dil, amax=amax_w)
    refw = torch.nn.grad.conv2d_weight(x.double(), (cout, cin, k, k), dyw.double(), st, pad, dil)
    diff = _first_diff(dw.cpu(), R.nhwc(refw.float()), ("k", "r", "s", "c"))
    assert diff is None, diff


def test_f16_forward_through_the_producers(cuda_device):
    """bn_apply(split=1) and weight_pack_f16 on x in {0..3}, w in {-1, 0, 1}: y is the fp64
    conv rounded once to fp16."""
    from hkp import ops
    dev = cuda_device
    n, h, w, cin, cout, k, st, pad, dil = PROD_BWD
    g = torch.Generator().manual_seed(SEED + 9)
    x1 = torch.randint(0, 4, (n, cin, h, w), generator=g).float()
    wt = torch.randint(-1, 2, (cout, cin, k, k), generator=g).float()
    ident = torch.cat([torch.ones(cin), torch.zeros(cin)]).to(dev)
    x16 = ops.bn_apply(R.nhwc(x1).to(dev), ident, relu=False, split=1, keep_fp32=False)
    y16, _ = ops.conv2d_fwd_f16(x16, ops.weight_pack_f16(R.nhwc(wt).to(dev)), st, pad, dil)
    refy = torch.nn.functional.conv2d(x1.double(), wt.double(), None, st, pad, dil)
    diff = _first_diff(y16.cpu(), R.nhwc(refy.float()).half(), ("n", "h", "w", "k"))
    assert diff is None, diff


# ------------------------------------------------------- float data, a-priori bound ----

# the stem rows are left to their exact tests: the stem's split planes never leave the wrapper
# in a layout the reference reads
FLOAT_ROWS = [r for r in CATALOGUE if not r.entry.startswith("stem")]


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("row", FLOAT_ROWS, ids=[r.name for r in FLOAT_ROWS])
def test_float_data_within_the_dot_product_bound(cuda_device, row):
    """relu'd N(0,1) activations and He-scaled weights through the real producers; the planes
    are read back from the device and the reference is ref64 of THOSE planes, so what is
    judged is the kernel's accumulation alone: |y - ref| <= err_bound_x3 elementwise (plus
    one fp16 rounding for the plain-fp16 output, and f16bn_bound's affine step and second
    rounding for the fused-BN epilogue).  No tolerance is fitted: RATIO is printed."""
    from hkp import ops
    dev = cuda_device
    if row.entry != "dgrad_s2":                        # (four stride-1 launches: the plan has no descriptor for them)
        _check_body(row, None, dev)
    n, h, w, cin, cout, k, st, pad, dil = row.shape
    P = R.PRODUCTS[row.entry]
    ho, wo = R.out_hw(row.shape)
    wt = (_randn(cout, k, k, cin, seed=2) * (2.0 / (k * k * cout)) ** 0.5).to(dev)
    if row.entry in ("dgrad", "dgrad_s2"):
        dy = _randn(n, ho, wo, cout, seed=11).to(dev)
        add = _randn(n, h, w, cin, seed=12)
        amax = ops.absmax(dy)
        dys, wfp = ops.split_pack_x3(dy, amax), ops.weight_flip_pack_x3(wt)
        if row.entry == "dgrad":
            got = ops.conv2d_bwd_data_x3(dys, wfp, (n, h, w, cin), pad, dil, add=add.to(dev), amax=amax, sk=row.sk,
                                         tile=row.tile).cpu()
        else:                                          # the phase packs are slices of wfp (test_x3_dgrad_strided)
            got = ops.conv2d_bwd_data_x3_strided(dys, ops.weight_phase_pack_x3(wt, pad), (n, h, w, cin),
                                                 (cout, k, k, cin), pad, add=add.to(dev), amax=amax, sk=row.sk,
                                                 tile=row.tile).cpu()
        gscale = R.pow2_scale(float(amax.cpu().view(torch.float32)))
        hdy, ldy = R.unpack_act(dys.cpu())
        hw, lw = R.unpack_w_flip(wfp.split.cpu())
        p = dict(hdy=hdy, ldy=ldy, hw=hw, lw=lw, inv=wfp.inv_scale.cpu(), add=R.nchw(add))
        op, L = "dgrad", R.red_len(row.shape, "dgrad")
        P = 3
    else:
        wp = ops.weight_pack_f16(wt) if P == 1 else ops.weight_pack_x3(wt)
        if row.entry.endswith("_bnin"):                # the in-kernel split is bn_apply's, bit for bit
            y_in = (_randn(n, h, w, cin, seed=8) * 3 + 1).to(dev)
            in_ss = torch.cat([_randn(cin, seed=9) * 0.7, _randn(cin, seed=10) * 2.0]).to(dev)
            if P == 1:
                y_in = y_in.half()
                xs = ops.bn_apply_f16(y_in, in_ss, relu=True)
            else:
                xs = ops.bn_apply(y_in, in_ss, relu=True, split=3, keep_fp32=False)
            got = ops.conv2d_fwd_bnin(y_in, in_ss, wp, st, pad, dil, sk=row.sk, tile=row.tile)[0].cpu()
        else:
            x = torch.relu(_randn(n, h, w, cin, seed=1)).to(dev)
            ident = torch.cat([torch.ones(cin), torch.zeros(cin)]).to(dev)
            xs = ops.bn_apply(x, ident, relu=False, split=1 if P == 1 else 3, keep_fp32=False)
            if row.entry == "f16bn":                   # bits.run_case's scale, shift and residual
                bn_s, bn_t = _randn(cout, seed=5) * 0.7, _randn(cout, seed=6)
                res = _randn(n, ho, wo, cout, seed=7).half()
                got = ops.conv2d_fwd_f16_bn(xs, wp, torch.cat([bn_s, bn_t]).to(dev), res=res.to(dev), relu=True,
                                            stride=st, pad=pad, dil=dil, sk=row.sk, tile=row.tile).cpu()
            else:
                got = _run_fwd(ops, row, (xs, wp))[0].cpu()
        hx, lx = R.unpack_act(xs.cpu(), P)
        hw, lw = R.unpack_w(wp.split.cpu(), P)
        p = dict(hx=hx, lx=lx, hw=hw, lw=lw, inv=wp.inv_scale.cpu())
        op, L = "fwd", R.red_len(row.shape, "fwd")
    ref = R.nhwc(R.ref64(p, row.shape, op, P, gscale=gscale if op == "dgrad" else 1.0))
    bound = R.err_bound_x3(R.NPROD[P], L, R.nhwc(R.ref64(R.abs_planes(p), row.shape, op, P,
                                                         gscale=gscale if op == "dgrad" else 1.0)))
    if row.entry == "f16bn":
        bound = R.f16bn_bound(ref, bound, bn_s.double(), bn_t.double(), res.double())
        ref = torch.relu(ref * bn_s.double() + bn_t.double() + res.double())
    elif P == 1:
        bound = bound + R.f16_round_bound(ref, bound)
    err = (got.double() - ref).abs()
    live = bound > 0
    ratio = float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0
    print("RATIO %s %s %.3g" % (row.entry, row.name, ratio))
    bad = err > bound
    assert not bool(bad.any()), "%s: %d elements past the bound; first at %s: err %g, bound %g (ratio %.3g)" % (
        row.name, int(bad.sum()), tuple(int(v) for v in bad.nonzero()[0]), err[bad][0].item(), bound[bad][0].item(),
        ratio)
