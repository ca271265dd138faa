"""The exact-fp32 MFMA convs (hkp_conv2d_fwd, hkp_conv2d_bwd_data, hkp_conv2d_bwd_filter,
hkp_conv_weight_flip; csrc/conv_fwd.hip, csrc/conv_bwd.hip) at their dispatch edges.

The rows of tests/_conv_ref.py drive every template instantiation and every split
count of the reduce at the smallest shapes that reach them (test_conv_ref_cpu.py holds
the tables to the library's planner).  Each row is checked two ways:

* integer inputs: y, dx, dw, the BN tile sums and the flip equal the fp64 reference
  bit for bit (every product and partial sum is an integer below 2^24, exact in any
  order), the tile M2 lies within _conv_ref.m2_bound of the fp64 one and is exactly 0
  where a tile has one row, and dx is exactly the addend where no gradient arrives;
* float inputs: |got - ref64| <= _conv_ref.err_bound(L, |conv|(|a|, |b|)) elementwise,
  the a-priori bound of an fp32 dot product of length L; the largest err / bound of
  each test is printed ("RATIO ...").

Every call is made twice and must give the same bits (fixed-order split reduce, no
atomics).  Wherever an `out=` exists the output is a view into the middle of a
sentinel-filled buffer whose 4096 floats on either side must still hold the sentinel:
a stray store shows without a fault.  The rejections at the end all return before a
launch; the mismatched calls there are safe only because hkp/ops.py refuses them.
"""
import pytest
import torch

import _conv_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 4096                  # floats on either side of a guarded output
SENT = -7777.25               # no integer, so a sentinel left in an integer result shows as well


def _rows(table):
    return pytest.mark.parametrize("c", ref.TABLES[table], ids=ref.case_id)


def _seed(table, c):
    return 100 + 37 * sorted(ref.TABLES).index(table) + ref.TABLES[table].index(c)


def _guarded(shape, dev, fill=None):
    """(buffer, view): a contiguous view of `shape` GUARD floats into a sentinel-filled
    buffer; the view itself holds the sentinel too, or `fill` (a CPU tensor)."""
    n = 1
    for v in shape:
        n *= v
    buf = torch.full((n + 2 * GUARD,), SENT, device=dev, dtype=torch.float32)
    view = buf[GUARD:GUARD + n].view(shape)
    if fill is not None:
        view.copy_(fill)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 4 * GUARD
    return buf, view


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())


def _ratio(entry, c, got, ref64, bound):
    """Prints the largest err / bound, then asserts the elementwise bound (and err == 0
    where the bound is 0)."""
    err = (got.double() - ref64).abs()
    pos = bound > 0
    r = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    print("RATIO %-28s %-36s %.4f" % (entry, ref.case_id(c), r))
    bad = (err > bound).nonzero()
    assert bad.numel() == 0, "%s %s: %d elements past the bound (largest ratio %.3f), first %s" % (
        entry, ref.case_id(c), bad.shape[0], r, bad[:4].tolist())


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------- forward ----

def _fwd_args(c, layout, t, dev):
    if layout == "nhwc":
        return ref.nhwc(t["x"]).to(dev), ref.krsc(t["w"]).to(dev)
    return t["x"].to(dev), t["w"].to(dev)


def _fwd_int(c, layout, seed, dev):
    """Integer inputs: y and the tile sums in every bit; M2 within m2_bound(cnt, M2, mean)
    — gamma_{cnt+2} relative plus cnt (2u |mean|)^2 for the fp32 tile mean, u = 2^-24,
    derived in tests/_conv_ref.py — and exactly 0 where the tile has one row, whose sum
    is then y itself; out= against an allocated output, stats on against off, twice."""
    from hkp import ops
    t = ref.int_tensors(c, seed)
    x, w = _fwd_args(c, layout, t, dev)
    y64 = ref.nhwc(ref.fwd64(t["x"], t["w"], c))
    assert torch.equal(y64.float().double(), y64)
    buf, out = _guarded(tuple(y64.shape), dev)
    y, part = ops.conv2d_fwd(x, w, c.stride, c.pad, c.dil, layout=layout, stats=True, out=out)
    assert y is out
    yc, pc = y.cpu(), part.cpu()
    bad = (yc != y64.float()).nonzero()
    assert bad.numel() == 0, "y differs at %d of %d, first (n, h, w, k) %s" % (bad.shape[0], yc.numel(), bad[:4].tolist())
    assert _guards_intact(buf)

    sums, m2, mu, cnts = ref.tile_partials64(y64.reshape(-1, c.cout))
    assert tuple(pc.shape) == (len(cnts), c.cout, 2)
    assert sums.abs().max() < 2 ** 24
    assert torch.equal(pc[:, :, 0].double(), sums), (pc[:, :, 0].double() != sums).nonzero()[:4].tolist()
    worst = 0.0
    for ti, cnt in enumerate(cnts):
        q = pc[ti, :, 1].double()
        if cnt == 1:
            assert (pc[ti, :, 1] == 0).all() and not torch.signbit(pc[ti, :, 1]).any()
            assert torch.equal(pc[ti, :, 0], yc.reshape(-1, c.cout)[ti * ref.TILE_ROWS])
            continue
        bound = ref.m2_bound(cnt, m2[ti], mu[ti])
        err = (q - m2[ti]).abs()
        pos = bound > 0
        if pos.any():
            worst = max(worst, float((err[pos] / bound[pos]).max()))
        assert not (err > bound).any(), "tile %d (cnt %d): M2 err/bound %.3f" % (ti, cnt, worst)
    print("M2RATIO %-26s %-36s %.4f" % ("conv2d_fwd/" + layout, ref.case_id(c), worst))

    y2, part2 = ops.conv2d_fwd(x, w, c.stride, c.pad, c.dil, layout=layout)          # allocated output, again
    assert _same_bits(y2, y) and _same_bits(part2, part)
    y3, part3 = ops.conv2d_fwd(x, w, c.stride, c.pad, c.dil, layout=layout, stats=False)
    assert part3 is None and _same_bits(y3, y)


def _fwd_float(c, layout, seed, dev):
    from hkp import ops
    t = ref.float_tensors(c, seed)
    x, w = _fwd_args(c, layout, t, dev)
    y64 = ref.nhwc(ref.fwd64(t["x"], t["w"], c))
    absref = ref.nhwc(ref.fwd64(t["x"].abs(), t["w"].abs(), c))
    buf, out = _guarded(tuple(y64.shape), dev)
    y, _ = ops.conv2d_fwd(x, w, c.stride, c.pad, c.dil, layout=layout, out=out)
    _ratio("conv2d_fwd/" + layout, c, y.cpu(), y64, ref.err_bound(ref.red_len(c, "fwd"), absref))
    assert _guards_intact(buf)
    y2, _ = ops.conv2d_fwd(x, w, c.stride, c.pad, c.dil, layout=layout, stats=False)
    assert _same_bits(y2, y)


@_rows("fwd_nhwc")
def test_fwd_nhwc_int_exact(cuda_device, c):
    _fwd_int(c, "nhwc", _seed("fwd_nhwc", c), cuda_device)


@_rows("fwd_nhwc")
def test_fwd_nhwc_float_bound(cuda_device, c):
    _fwd_float(c, "nhwc", _seed("fwd_nhwc", c), cuda_device)


@_rows("fwd_stem")
def test_fwd_stem_int_exact(cuda_device, c):
    _fwd_int(c, "nchw", _seed("fwd_stem", c), cuda_device)


@_rows("fwd_stem")
def test_fwd_stem_float_bound(cuda_device, c):
    _fwd_float(c, "nchw", _seed("fwd_stem", c), cuda_device)


# --------------------------------------------------------------------- dgrad ----

def _no_gradient(c):
    """dx positions [n, h, w, c] no tap reaches: there dx is the addend (or 0) exactly."""
    ho, wo = ref.out_hw(c)
    reach = ref.dgrad64(torch.ones(c.n, c.cout, ho, wo), torch.ones(c.cout, c.cin, c.r, c.s), c)
    return ref.nhwc(reach) == 0


def _dgrad(c, t, dev, with_add):
    from hkp import ops
    dy = ref.nhwc(t["dy"]).to(dev)
    wf = ops.conv_weight_flip(ref.krsc(t["w"]).to(dev))
    add = ref.nhwc(t["add"]).to(dev) if with_add else None
    shape = (c.n, c.h, c.w, c.cin)
    dx = ops.conv2d_bwd_data(dy, wf, shape, c.stride, c.pad, c.dil, add=add)
    dx2 = ops.conv2d_bwd_data(dy, wf, shape, c.stride, c.pad, c.dil, add=add)
    assert tuple(dx.shape) == shape and _same_bits(dx, dx2)
    if with_add:
        assert torch.equal(add.cpu(), ref.nhwc(t["add"]))                # the addend is read, not written
    dxc = dx.cpu()
    dead = _no_gradient(c)
    if c.stride == 2 and c.r == 1:                                       # rows and columns no dy pixel maps to
        assert dead[:, 1::2].all() and dead[:, :, 1::2].all() and not dead[:, ::2, ::2].any()
        if c.h % 2 == 0:
            assert dead[:, -1].all() and dead[:, :, -1].all()
    want = ref.nhwc(t["add"]) if with_add else torch.zeros(shape)
    assert _same_bits(dxc[dead], want[dead]), "dx is not the addend where no gradient arrives"
    return dxc


@pytest.mark.parametrize("with_add", [True, False], ids=["add", "noadd"])
@_rows("dgrad")
def test_dgrad_int_exact(cuda_device, c, with_add):
    """dx == the fp64 transposed conv (+ add) in every bit, twice; exact addend / zero
    where the stride leaves a dx pixel without gradient."""
    t = ref.int_tensors(c, _seed("dgrad", c))
    dx64 = ref.nhwc(ref.dgrad64(t["dy"], t["w"], c, t["add"] if with_add else None))
    dx = _dgrad(c, t, cuda_device, with_add)
    bad = (dx != dx64.float()).nonzero()
    assert bad.numel() == 0, "dx differs at %d of %d, first (n, h, w, c) %s" % (bad.shape[0], dx.numel(), bad[:4].tolist())


@pytest.mark.parametrize("with_add", [True, False], ids=["add", "noadd"])
@_rows("dgrad")
def test_dgrad_float_bound(cuda_device, c, with_add):
    t = ref.float_tensors(c, _seed("dgrad", c))
    add = t["add"] if with_add else None
    dx64 = ref.nhwc(ref.dgrad64(t["dy"], t["w"], c, add))
    absref = ref.nhwc(ref.dgrad64(t["dy"].abs(), t["w"].abs(), c, None if add is None else add.abs()))
    dx = _dgrad(c, t, cuda_device, with_add)
    _ratio("conv2d_bwd_data", c, dx, dx64, ref.err_bound(ref.red_len(c, "dgrad"), absref))


# --------------------------------------------------------------------- wgrad ----

def _wgrad_args(c, layout, t, dev):
    """(x, dy, w_shape, to_layout): to_layout maps an OIHW reference to dw's layout."""
    dy = ref.nhwc(t["dy"]).to(dev)
    if layout == "nhwc":
        return ref.nhwc(t["x"]).to(dev), dy, (c.cout, c.r, c.s, c.cin), ref.krsc
    return t["x"].to(dev), dy, (c.cout, c.cin, c.r, c.s), lambda w: w.contiguous()


def _wgrad_int(c, layout, seed, dev):
    """dw == the fp64 reference in every bit: plain (twice); into a prefilled out= with
    accumulate=False (the prefill is gone); with accumulate=True (exactly prefill + dw:
    |dw| + 3 stays below 2^24).  The guards around out= keep their sentinel."""
    from hkp import ops
    t = ref.int_tensors(c, seed)
    x, dy, w_shape, lay = _wgrad_args(c, layout, t, dev)
    dw64 = lay(ref.wgrad64(t["x"], t["dy"], c))
    want = dw64.float()
    assert torch.equal(want.double(), dw64)
    a = (c.stride, c.pad, c.dil)
    dw = ops.conv2d_bwd_filter(x, dy, w_shape, *a, layout=layout)
    bad = (dw.cpu() != want).nonzero()
    assert bad.numel() == 0, "dw differs at %d of %d, first %s" % (bad.shape[0], want.numel(), bad[:4].tolist())
    assert _same_bits(ops.conv2d_bwd_filter(x, dy, w_shape, *a, layout=layout), dw)
    pre = torch.randint(-3, 4, w_shape, generator=torch.Generator().manual_seed(seed + 1)).float()
    for accumulate in (False, True):
        buf, out = _guarded(w_shape, dev, fill=pre)
        got = ops.conv2d_bwd_filter(x, dy, w_shape, *a, layout=layout, out=out, accumulate=accumulate)
        assert got is out
        exp = want + pre if accumulate else want
        bad = (out.cpu() != exp).nonzero()
        assert bad.numel() == 0, "accumulate=%s: dw differs at %d, first %s" % (accumulate, bad.shape[0], bad[:4].tolist())
        assert _guards_intact(buf)


def _wgrad_float(c, layout, seed, dev):
    from hkp import ops
    t = ref.float_tensors(c, seed)
    x, dy, w_shape, lay = _wgrad_args(c, layout, t, dev)
    dw64 = lay(ref.wgrad64(t["x"], t["dy"], c))
    absref = lay(ref.wgrad64(t["x"].abs(), t["dy"].abs(), c))
    a = (c.stride, c.pad, c.dil)
    buf, out = _guarded(w_shape, dev)
    dw = ops.conv2d_bwd_filter(x, dy, w_shape, *a, layout=layout, out=out)
    _ratio("conv2d_bwd_filter/" + layout, c, dw.cpu(), dw64, ref.err_bound(ref.red_len(c, "wgrad"), absref))
    assert _guards_intact(buf)
    assert _same_bits(ops.conv2d_bwd_filter(x, dy, w_shape, *a, layout=layout), dw)
    # accumulate is one fp32 addition of the reduced sum to what out= held
    pre = torch.randn(w_shape, generator=torch.Generator().manual_seed(seed + 1)).to(dev)
    acc = ops.conv2d_bwd_filter(x, dy, w_shape, *a, layout=layout, out=pre.clone(), accumulate=True)
    assert _same_bits(acc, pre + dw)


@_rows("wgrad_nhwc")
def test_wgrad_nhwc_int_exact(cuda_device, c):
    _wgrad_int(c, "nhwc", _seed("wgrad_nhwc", c), cuda_device)


@_rows("wgrad_nhwc")
def test_wgrad_nhwc_float_bound(cuda_device, c):
    _wgrad_float(c, "nhwc", _seed("wgrad_nhwc", c), cuda_device)


@_rows("wgrad_stem")
def test_wgrad_stem_int_exact(cuda_device, c):
    _wgrad_int(c, "nchw", _seed("wgrad_stem", c), cuda_device)


@_rows("wgrad_stem")
def test_wgrad_stem_float_bound(cuda_device, c):
    _wgrad_float(c, "nchw", _seed("wgrad_stem", c), cuda_device)


# ---------------------------------------------------------------------- flip ----

@pytest.mark.parametrize("shape", ref.FLIP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_weight_flip_is_a_pure_copy(cuda_device, shape):
    """KRSC -> flipped CRSK moves bits and nothing else, on arbitrary floats (a NaN and
    a -0.0 among them), past the first grid-stride trip too."""
    from hkp import ops
    w = torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape))).to(cuda_device)
    w.view(-1)[0], w.view(-1)[-1] = float("nan"), -0.0
    want = w.flip(1, 2).permute(3, 1, 2, 0).contiguous()
    wf = ops.conv_weight_flip(w)
    assert tuple(wf.shape) == (shape[3], shape[1], shape[2], shape[0])
    assert _same_bits(wf, want) and _same_bits(ops.conv_weight_flip(w), wf)


# ---------------------------------------------------------------- rejections ----

def _t(dev, *shape):
    return torch.ones(shape, device=dev, dtype=torch.float32)


def test_bwd_data_rejects_mismatched_shapes(cuda_device):
    """conv2d_bwd_data builds its descriptor's Cin from x_shape: one that is not w_flip's
    would have the kernel read past w_flip (and dx be sized for it)."""
    from hkp import ops
    from hkp._lib import HkpError
    dev = cuda_device
    dy, wf = _t(dev, 1, 8, 8, 64), _t(dev, 64, 3, 3, 64)
    free = torch.cuda.memory_allocated(dev)
    with pytest.raises(HkpError, match="w_flip Cin 64 != x_shape C 128"):
        ops.conv2d_bwd_data(dy, wf, (1, 8, 8, 128), 1, 1, 1)
    for bad in ((1, 8, 8), (1, 8, 8, 64, 1), (1, 0, 8, 64), (1, 8, -8, 64), (1, 8, 8, 64.0), (1, 8, 8, None), None, 64):
        with pytest.raises(HkpError, match="four positive ints"):
            ops.conv2d_bwd_data(dy, wf, bad, 1, 1, 1)
    assert torch.cuda.memory_allocated(dev) == free                      # nothing was allocated
    dx = ops.conv2d_bwd_data(dy, wf, torch.Size((1, 8, 8, 64)), 1, 1, 1)  # a torch.Size is four ints
    assert tuple(dx.shape) == (1, 8, 8, 64)


def test_bwd_filter_rejects_mismatched_shapes(cuda_device):
    """conv2d_bwd_filter: w_shape's Cin against x's (the kernel writes k*r*s*C(x) floats
    into a dw sized from w_shape), out= of another shape, accumulate without out=.  The
    out= buffers keep their sentinel: nothing was launched."""
    from hkp import ops
    from hkp._lib import HkpError
    dev = cuda_device
    x, dy = _t(dev, 1, 8, 8, 128), _t(dev, 1, 8, 8, 64)

    def refused(match, xx, dyy, w_shape, out_shape=None, **kw):
        buf = out = None
        if out_shape is not None:
            buf, out = _guarded(out_shape, dev)
        with pytest.raises(HkpError, match=match):
            ops.conv2d_bwd_filter(xx, dyy, w_shape, 1, kw.pop("pad", 1), 1, out=out, **kw)
        if buf is not None:
            assert bool((buf == SENT).all())

    refused("w_shape Cin 64 != input C 128", x, dy, (64, 3, 3, 64))                     # dw half the size written
    refused("w_shape Cin 64 != input C 128", x, dy, (64, 3, 3, 64), (64, 3, 3, 64))
    refused("w_shape Cin 256 != input C 128", x, dy, (64, 3, 3, 256), (64, 3, 3, 256))
    xs, dys = _t(dev, 1, 3, 16, 16), _t(dev, 1, 8, 8, 64)
    refused("w_shape Cin 8 != input C 3", xs, dys, (64, 8, 7, 7), (64, 8, 7, 7), pad=3, layout="nchw")
    refused("w_shape Cin 7 != input C 3", xs, dys, (64, 7, 7, 3), pad=3, layout="nchw")  # KRSC by mistake
    for shape in ((64, 3, 3, 64), (64, 3, 3, 256), (64, 9, 128), (64 * 9 * 128,), (128, 3, 3, 64), (64, 128, 3, 3)):
        refused("out shape", x, dy, (64, 3, 3, 128), shape)
        refused("out shape", x, dy, (64, 3, 3, 128), shape, accumulate=True)
    refused("accumulate=True needs out=", x, dy, (64, 3, 3, 128), accumulate=True)
    for bad in ((64, 3, 3), (64, 3, 3, 128, 1), (64, 3, 3, 128.0), (64, 0, 3, 128), None):
        refused("four positive ints", x, dy, bad)
    with pytest.raises(HkpError, match="expected torch.float32"):
        ops.conv2d_bwd_filter(x, dy, (64, 3, 3, 128), 1, 1, 1, out=torch.zeros(64, 3, 3, 128, device=dev, dtype=torch.float64))
    with pytest.raises(HkpError, match="contiguous"):
        ops.conv2d_bwd_filter(x, dy, (64, 3, 3, 128), 1, 1, 1, out=_t(dev, 128, 3, 3, 64).permute(3, 1, 2, 0))
    # and the well-formed call right after them
    buf, out = _guarded((64, 3, 3, 128), dev)
    ops.conv2d_bwd_filter(x, dy, (64, 3, 3, 128), 1, 1, 1, out=out)
    assert _guards_intact(buf) and not bool((out == SENT).any())


def test_library_rejections_through_the_wrappers(cuda_device):
    """The library's own refusals (test_conv_ref_cpu.py has them at the C ABI) as the
    wrappers surface them, with real tensors; a given out= keeps its sentinel."""
    from hkp import ops
    from hkp._lib import HkpError
    dev = cuda_device

    def fwd(match, x, w, out_shape, **kw):
        buf, out = _guarded(out_shape, dev)
        with pytest.raises(HkpError, match=match):
            ops.conv2d_fwd(x, w, kw.pop("stride", 1), kw.pop("pad", 1), kw.pop("dil", 1), out=out, **kw)
        assert bool((buf == SENT).all())

    fwd("Cout=96 must be a multiple of 64", _t(dev, 1, 8, 8, 64), _t(dev, 96, 3, 3, 64), (1, 8, 8, 96))
    fwd("NHWC Cin=48 must be a multiple of 32", _t(dev, 1, 8, 8, 48), _t(dev, 64, 3, 3, 48), (1, 8, 8, 64))
    fwd(r"stem \(Cin<=8\), got 9", _t(dev, 1, 9, 8, 8), _t(dev, 64, 9, 3, 3), (1, 8, 8, 64), layout="nchw")
    fwd("weight Cin 32 != input C 64", _t(dev, 1, 8, 8, 64), _t(dev, 64, 3, 3, 32), (1, 8, 8, 64))
    fwd("empty output", _t(dev, 1, 2, 2, 64), _t(dev, 64, 3, 3, 64), (1, 1, 1, 64), pad=0)
    fwd("empty output", _t(dev, 1, 2, 9, 64), _t(dev, 64, 3, 3, 64), (1, 1, 4, 64), pad=0, stride=2)
    fwd("bad stride/dilation/pad", _t(dev, 1, 8, 8, 64), _t(dev, 64, 3, 3, 64), (1, 8, 8, 64), stride=0)
    fwd("out shape", _t(dev, 1, 8, 8, 64), _t(dev, 64, 3, 3, 64), (1, 8, 8, 128))

    def dgrad(match, dy, wf, x_shape, pad=1):
        with pytest.raises(HkpError, match=match):
            ops.conv2d_bwd_data(dy, wf, x_shape, 1, pad, 1)

    dgrad("Cin%64==0", _t(dev, 1, 8, 8, 64), _t(dev, 96, 3, 3, 64), (1, 8, 8, 96))
    dgrad("Cout%32==0", _t(dev, 1, 8, 8, 48), _t(dev, 64, 3, 3, 48), (1, 8, 8, 64))
    dgrad("asymmetric padding", _t(dev, 1, 12, 12, 64), _t(dev, 64, 3, 3, 64), (1, 8, 8, 64), pad=3)
    dgrad("asymmetric padding", _t(dev, 1, 10, 8, 64), _t(dev, 64, 1, 3, 64), (1, 8, 8, 64))

    def wgrad(match, x, dy, w_shape, **kw):
        buf, out = _guarded(w_shape, dev)
        with pytest.raises(HkpError, match=match):
            ops.conv2d_bwd_filter(x, dy, w_shape, 1, kw.pop("pad", 1), 1, out=out, **kw)
        assert bool((buf == SENT).all())

    wgrad("Cout=96 must be a multiple of 64", _t(dev, 1, 8, 8, 64), _t(dev, 1, 8, 8, 96), (96, 3, 3, 64))
    wgrad("NHWC Cin=32 must be a multiple of 64", _t(dev, 1, 8, 8, 32), _t(dev, 1, 8, 8, 64), (64, 3, 3, 32))
    wgrad(r"stem \(Cin<=8\)", _t(dev, 1, 9, 16, 16), _t(dev, 1, 16, 16, 64), (64, 9, 3, 3), layout="nchw")
    wgrad("dy shape", _t(dev, 1, 8, 8, 64), _t(dev, 1, 8, 7, 64), (64, 3, 3, 64))
    wgrad("empty output", _t(dev, 1, 2, 2, 64), _t(dev, 1, 1, 1, 64), (64, 3, 3, 64), pad=0)
