"""Per-pixel ignore masks without a GPU: the float64 reference of tests/_masks_ref.py against
_planes_ref.py where the two agree by definition and against central differences, the
top-k tests' precondition on the very inputs the GPU tests use, the rasteriser's
restatement on hand cases, flip_lut, peaks_drop_masked on CPU tensors against the loop
version, the Python-side rejections (all before a tensor is touched) and the C ABI's
argument checks (which return before any launch)."""
import ctypes

import numpy as np
import pytest
import torch

import _instances_ref as iref
import _masks_ref as mref
import _planes_ref as pref

NAN = float("nan")
KINDS = [("bce", 2.0), ("mse", 2.0), ("qfl", 2.0), ("qfl", 1.5)]


def _case():
    n, k, m, H, W = 2, 4, 2, 9, 11
    g = torch.Generator().manual_seed(5)
    p = torch.rand(n, k, H, W, generator=g) * 0.98 + 0.01
    pts = torch.zeros(n, k, m, 3)
    pts[..., 0] = torch.rand(n, k, m, generator=g) * W
    pts[..., 1] = torch.rand(n, k, m, generator=g) * H
    pts[..., 2] = 1.0
    pts[0, 1, :, 2] = 0.0                                  # an absent plane
    y = torch.from_numpy(iref.gauss_target_multi(pts.numpy(), H, W, 3.0)).double()
    w = torch.rand(n, k, generator=g) * 1.5 + 0.25
    return (n, k, m, H, W), p, y, pts, w


# ------------------------------------------------------- the reference against planes_ref ----

@pytest.mark.parametrize("norm", ["elements", "instances"])
@pytest.mark.parametrize("absent", ["zero", "ignore"])
def test_all_zero_mask_is_planes_ref(absent, norm):
    shape, p, y, pts, w = _case()
    zero = torch.zeros(shape[0], shape[3], shape[4], dtype=torch.uint8)
    for kind, beta in KINDS:
        for weights in (None, w):
            for topk in (None, 2):
                a = mref.masked_ref(p, y, pts, zero, kind, absent, norm, beta, weights, topk)
                b = pref.planes_ref(p, y, pts, kind, absent, norm, beta, weights, topk)
                assert a["loss"] == b["loss"] and torch.equal(a["dheat"], b["dheat"]) and torch.equal(a["S"], b["S"])
                assert torch.equal(a["used"], b["used"]) and a["elements"] == b["elements"]
                assert torch.equal(a["plane_pixels"], b["eligible"].long() * shape[3] * shape[4])


@pytest.mark.parametrize("norm", ["elements", "instances"])
@pytest.mark.parametrize("absent", ["zero", "ignore"])
def test_whole_plane_mask_is_weight_zero(absent, norm):
    shape, p, y, pts, w = _case()
    off = torch.zeros(shape[:2], dtype=torch.bool)
    off[0, 2] = off[1, 0] = off[1, 3] = True
    mask = mref.plane_mask(shape, off)
    assert mask[0].unique().tolist() == [4] and mask[1].unique().tolist() == [9]
    for kind, beta in KINDS:
        for weights in (None, w):
            w0 = torch.where(off, torch.zeros(()), torch.ones(shape[:2]) if weights is None else weights)
            for topk in (None, 2):
                a = mref.masked_ref(p, y, pts, mask, kind, absent, norm, beta, weights, topk)
                b = pref.planes_ref(p, y, pts, kind, absent, norm, beta, w0, topk)
                assert a["loss"] == b["loss"] and torch.equal(a["dheat"], b["dheat"]) and torch.equal(a["S"], b["S"])
                assert torch.equal(a["used"], b["used"]) and not a["used"][off].any()
                assert (a["plane_loss"][off] == -1).all() and (a["plane_pixels"][off] == 0).all()


def test_reference_gradient_against_central_differences():
    shape, p, y, pts, w = _case()
    n, k, m, H, W = shape
    mask = mref.seeded_mask(shape)
    h = 1e-3
    for kind, beta in KINDS:
        for norm in ("elements", "instances"):
            ref = mref.masked_ref(p, y, pts, mask, kind, "ignore", norm, beta, w)
            keep = ref["keep"]
            assert ((ref["dheat"] == 0) | keep).all()                       # +0 under every masked pixel
            assert ref["D"] == (float(ref["elements"]) if norm == "elements" else ref["D"])
            for (b, c, yy, xx) in ((0, 0, 1, 2), (0, 2, 3, 3), (0, 3, 8, 10), (1, 1, 4, 5), (0, 2, H // 2, 0)):
                hi, lo = p.clone(), p.clone()
                hi[b, c, yy, xx] += h
                lo[b, c, yy, xx] -= h
                num = (mref.masked_ref(hi, y, pts, mask, kind, "ignore", norm, beta, w)["loss"]
                       - mref.masked_ref(lo, y, pts, mask, kind, "ignore", norm, beta, w)["loss"]) / \
                    (float(hi[b, c, yy, xx]) - float(lo[b, c, yy, xx]))
                got = float(ref["dheat"][b, c, yy, xx])
                if not (keep[b, c, yy, xx] and ref["used"][b, c]):
                    assert got == 0.0 and num == 0.0
                else:
                    assert abs(got - num) <= 2e-3 * abs(num) + 1e-12, (kind, norm, b, c, got, num)


def test_mean_ranking_differs_from_sum_ranking():
    """w * S / n, not w * S: a plane that keeps a tenth of its pixels and has the larger mean
    leads, although its sum is smaller."""
    S = torch.tensor([[10.0, 4.0, 1.0]], dtype=torch.float64)
    npix = torch.tensor([[100, 10, 0]])
    el = torch.tensor([[True, True, False]])
    assert mref.select(S, npix, None, el, 1).tolist() == [[False, True, False]]
    assert pref.select(S, None, el, 1).tolist() == [[True, False, False]]
    assert mref.select(S, npix, torch.tensor([[5.0, 1.0, 1.0]]), el, 1).tolist() == [[True, False, False]]


@pytest.mark.parametrize("shape", mref.TOPK_SHAPES)
def test_topk_precondition_of_the_gpu_inputs(shape):
    """The GPU top-k tests compare a selection: on their inputs (the same generator) no two
    neighbouring ranks are closer than the planes tests' 8e-4."""
    n, k, m, H, W = shape
    for absent in ("zero", "ignore"):
        p, pts, mask = mref.topk_inputs(shape, absent)
        for sigma in (8.0,):
            y = torch.from_numpy(iref.gauss_target_multi(pts.numpy(), H, W, sigma)).double()
            for kind in ("bce", "mse"):
                for w in (None, mref.topk_weights(shape)):
                    ref = mref.masked_ref(p, y, pts, mask, kind, absent, "elements", 2.0, w)
                    gap = mref.rank_gap(ref["S"], ref["plane_pixels"], w, ref["eligible"])
                    print("%s %s %s weights %s: smallest relative rank gap %.3e" % (shape, absent, kind,
                                                                                     w is not None, gap))
                    assert gap >= mref.TOPK_MIN_GAP


# ------------------------------------------------------------------------- rasteriser ----

def _raster(recs, H=12, W=14):
    from hkp import masks
    return mref.regions_ref(masks.pack([recs]).numpy(), H, W)[0]


def test_rasteriser_restatement_hand_cases():
    from hkp import masks
    # a box: both ends included, a pixel exactly on the edge is inside
    m = _raster([masks.box(2, 3, 5, 4, (0, 2))])
    want = np.zeros((12, 14), dtype=np.uint8)
    want[3:5, 2:6] = 5
    assert np.array_equal(m, want)
    m = _raster([masks.box(1.5, 2.0, 3.0, 2.5, 1)])          # fractional bounds: x in {2, 3}, y = 2
    assert m.sum() == 2 * 2 and m[2, 2] == 2 and m[2, 3] == 2
    # a disc of radius 5 about (6, 6): (3, 4) away is exactly r^2 and inside, (4, 4) is not
    m = _raster([masks.disc(6, 6, 5, 3)])
    assert m[6 + 4, 6 + 3] == 8 and m[6 - 3, 6 - 4] == 8 and m[6, 11] == 8 and m[6, 1] == 8
    assert m[6 + 4, 6 + 4] == 0 and m[6, 12] == 0
    yy, xx = np.mgrid[0:12, 0:14]
    assert np.array_equal(m != 0, (xx - 6) ** 2 + (yy - 6) ** 2 <= 25)
    # r = 0: the centre pixel alone, and nothing when the centre is between pixels
    m = _raster([masks.disc(4, 7, 0, 0)])
    assert m.sum() == 1 and m[7, 4] == 1
    assert _raster([masks.disc(4.5, 7, 0, 0)]).sum() == 0
    # a NaN bound is never inside
    for rec in (masks.box(NAN, 0, 5, 5), masks.box(0, 0, 5, NAN), masks.disc(NAN, 3, 4), masks.disc(3, 3, NAN)):
        assert _raster([rec]).sum() == 0
    # an unknown kind is an empty slot, whatever it holds
    regs = masks.pack([[masks.box(0, 0, 1, 1, 0)]], R=4).numpy()
    regs[0, 1] = (3.0, NAN, NAN, NAN, NAN, NAN)
    regs[0, 2] = (NAN, 0.0, 0.0, 13.0, 11.0, 255.0)
    regs[0, 3] = (0.0, 0.0, 0.0, 13.0, 11.0, 255.0)
    m = mref.regions_ref(regs, 12, 14)[0]
    assert m.sum() == 4 and (m[:2, :2] == 1).all()
    # overlapping regions: the bits OR together
    m = _raster([masks.box(0, 0, 5, 5, 0), masks.disc(5, 5, 2, (1, 7)), masks.box(4, 4, 13, 11, None)])
    assert m[0, 0] == 1 and m[5, 7] == 0xFF and m[5, 5] == 0xFF and m[3, 5] == 1 | 2 | 128 and m[11, 0] == 0
    assert m[5, 3] == 1 | 2 | 128 and m[4, 3] == 1 and m[6, 3] == 0


def test_region_builders():
    from hkp import masks
    from hkp._lib import HkpError
    assert masks.class_bits(None) == 0xFF and masks.class_bits("all") == 0xFF
    assert masks.class_bits(3) == 8 and masks.class_bits((0, 7)) == 129 and masks.class_bits(()) == 0
    for bad in (8, -1, True, 1.0, (0, 9)):
        with pytest.raises(HkpError, match="class_bits"):
            masks.class_bits(bad)
    assert masks.box(1, 2, 3, 4, 1) == (1.0, 1.0, 2.0, 3.0, 4.0, 2.0)
    assert masks.disc(1, 2, 3, (0, 1)) == (2.0, 1.0, 2.0, 3.0, 0.0, 3.0)
    t = masks.pack([[masks.box(1, 2, 3, 4)], []], R=3)
    assert t.dtype == torch.float32 and tuple(t.shape) == (2, 3, 6)
    assert t[0, 0].tolist() == [1.0, 1.0, 2.0, 3.0, 4.0, 255.0] and (t[0, 1:] == 0).all() and (t[1] == 0).all()
    assert tuple(masks.pack([[], []]).shape) == (2, 1, 6)
    with pytest.raises(HkpError, match="outside 1..64"):
        masks.pack([[masks.box(0, 0, 1, 1)] * 65])
    with pytest.raises(HkpError, match="longest"):
        masks.pack([[masks.box(0, 0, 1, 1)] * 3], R=2)


# --------------------------------------------------------------------------- flip_lut ----

def test_flip_lut():
    from hkp import masks
    ident = masks.flip_lut(())
    assert ident.dtype == torch.uint8 and ident.tolist() == list(range(256))
    for pairs in (((0, 1),), ((0, 1), (2, 5)), ((3, 7),)):
        lut = masks.flip_lut(pairs)
        assert np.array_equal(lut.numpy(), mref.flip_lut(pairs))
        assert lut[lut.long()].tolist() == list(range(256))                  # an involution
        touched = 0
        for a, b in pairs:
            touched |= (1 << a) | (1 << b)
            assert lut[1 << a].item() == 1 << b and lut[1 << b].item() == 1 << a
        v = torch.arange(256)
        assert torch.equal(lut.long() & ~touched, v & ~touched)              # the other bits are kept
        assert lut[255].item() == 255 and lut[0].item() == 0
    with pytest.raises(masks.HkpError, match="flip_lut"):
        masks.flip_lut(((0, 8),))


# ------------------------------------------------------------------ peaks_drop_masked ----

def _peaks_case():
    n, k, p, H, W = 2, 3, 4, 6, 8
    mask = torch.zeros(n, H, W, dtype=torch.uint8)
    mask[0, 2, 3] = 1 | 4                                    # classes 0 and 2 at (x 3, y 2)
    mask[0, 5, 7] = 2
    mask[0, 0, 0] = 1
    mask[1] = 0xFF
    peaks = torch.full((n, k, p, 3), -1.0)
    peaks[..., 2] = 0.0
    counts = torch.zeros(n, k, dtype=torch.int32)

    def put(b, c, rows, count=None):
        for j, r in enumerate(rows):
            peaks[b, c, j] = torch.tensor(r)
        counts[b, c] = len(rows) if count is None else count

    # class 0: dropped, kept, dropped (x.5 rounds up into the masked pixel), kept
    put(0, 0, [(3.0, 2.0, 0.9), (4.0, 2.0, 0.8), (2.5, 1.5, 0.7), (2.49, 2.0, 0.6)])
    # class 1: bit 1 only at (7, 5): clamped from outside the frame; NaN is kept; counts = P + 3
    put(0, 1, [(9.0, 7.5, 0.9), (NAN, 5.0, 0.8), (3.0, 2.0, 0.7), (7.4, 4.5, 0.6)], count=7)
    # class 2: counts = -1, nothing is looked at
    put(0, 2, [(3.0, 2.0, 0.9)], count=-1)
    # image 1: everything dropped; a non-finite coordinate is kept; two of four slots valid
    put(1, 0, [(1.0, 1.0, 0.5), (2.0, 2.0, 0.4), (3.0, 3.0, 0.3)])
    put(1, 1, [(float("inf"), 1.0, 0.5), (2.0, 2.0, 0.4)])
    put(1, 2, [(-0.6, -3.0, 0.5), (2.0, 2.0, 0.4), (5.0, 5.0, 0.3), (6.0, 1.0, 0.2)], count=2)
    return peaks, counts, mask


def test_peaks_drop_masked_against_the_loops():
    from hkp import masks
    peaks, counts, mask = _peaks_case()
    before = (peaks.clone(), counts.clone(), mask.clone())
    got_p, got_c = masks.peaks_drop_masked(peaks, counts, mask)
    want_p, want_c = mref.peaks_drop_masked(peaks, counts, mask)
    assert got_c.dtype == torch.int32 and got_p.dtype == torch.float32
    assert torch.equal(got_c, want_c)
    assert np.array_equal(got_p.numpy().view(np.int32), want_p.numpy().view(np.int32))      # NaN and all
    assert got_c.tolist() == [[2, 2, 0], [0, 1, 0]]
    # order kept, freed slots filled
    assert got_p[0, 0, 0].tolist() == pytest.approx([4.0, 2.0, 0.8]) and got_p[0, 0, 1, 0].item() == pytest.approx(2.49)
    assert got_p[0, 0, 2:].tolist() == [[-1.0, -1.0, 0.0]] * 2
    assert np.isnan(got_p[0, 1, 0, 0].item()) and got_p[0, 1, 1].tolist() == pytest.approx([3.0, 2.0, 0.7])
    assert (got_p[0, 2] == torch.tensor([-1.0, -1.0, 0.0])).all() and (got_p[1, 0] == torch.tensor([-1.0, -1.0, 0.0])).all()
    assert got_p[1, 1, 0, 0].item() == float("inf")
    # the inputs are left as they were
    assert np.array_equal(peaks.numpy().view(np.int32), before[0].numpy().view(np.int32))
    assert torch.equal(counts, before[1]) and torch.equal(mask, before[2])
    # no mask bit: the valid slots come back, the others cleared
    none_p, none_c = masks.peaks_drop_masked(peaks, counts, torch.zeros_like(mask))
    assert none_c.tolist() == [[4, 4, 0], [3, 2, 2]]
    assert np.array_equal(none_p[0, 0].numpy().view(np.int32), peaks[0, 0].numpy().view(np.int32))
    # random batches
    g = torch.Generator().manual_seed(3)
    for _ in range(5):
        pk = torch.rand(3, 4, 5, 3, generator=g) * torch.tensor([12.0, 9.0, 1.0]) - torch.tensor([1.0, 1.0, 0.0])
        pk[..., :2] = (pk[..., :2] * 2).round() / 2                          # halves: the x.5 rule at work
        cn = torch.randint(-1, 8, (3, 4), generator=g, dtype=torch.int32)
        mk = torch.randint(0, 256, (3, 7, 10), generator=g, dtype=torch.uint8)
        a, b = masks.peaks_drop_masked(pk, cn, mk), mref.peaks_drop_masked(pk, cn, mk)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_peaks_drop_masked_rejections():
    from hkp import masks
    peaks, counts, mask = _peaks_case()
    for args in ((peaks.double(), counts, mask), (peaks[..., :2], counts, mask), (peaks, counts.long(), mask),
                 (peaks, counts[:1], mask), (peaks, counts, mask.int()), (peaks, counts, mask[:1]),
                 (peaks, counts, mask[0]), (peaks.numpy(), counts, mask),
                 (torch.zeros(2, 9, 4, 3), torch.zeros(2, 9, dtype=torch.int32), mask)):
        with pytest.raises(masks.HkpError, match="peaks_drop_masked"):
            masks.peaks_drop_masked(*args)


def test_metrics_without_a_mask_call_what_they_called(monkeypatch):
    from hkp import masks, metrics, ops
    seen = []
    monkeypatch.setattr(ops, "peaks_match", lambda *a, **kw: seen.append((a, kw)))
    monkeypatch.setattr(masks, "peaks_drop_masked", lambda *a: seen.append("drop") or (a[0], a[1]))
    peaks, counts, mask = _peaks_case()
    labels = torch.zeros(2, 3, 2)
    km = metrics.KeypointMetrics(3, (2, 4), bins=16)
    km.update(peaks, counts, labels)
    assert len(seen) == 1 and seen[0][0][0] is peaks and seen[0][0][1] is counts and seen[0][0][2] is labels
    assert seen[0][1] == {"bins": 16}
    del seen[:]
    km.update(peaks, counts, labels, mask=mask)
    assert seen[0] == "drop" and len(seen) == 2


# ------------------------------------------------------------------------- rejections ----

def test_python_rejections_before_a_tensor_is_touched():
    """Every tensor here is on the CPU: the mask's checks come before the device check of
    heat, and nothing is computed."""
    from hkp import autograd as hkp_autograd
    from hkp import ops
    from hkp._lib import HkpError
    heat, pts = torch.rand(2, 3, 4, 8), torch.zeros(2, 3, 1, 3)
    uv = torch.zeros(2, 3, 2)
    good = torch.zeros(2, 4, 8, dtype=torch.uint8)
    calls = (lambda m: ops.heat_loss_masked(heat, pts, m), lambda m: ops.heat_loss_multi(heat, pts, mask=m),
             lambda m: ops.heat_loss(heat, uv=uv, mask=m), lambda m: hkp_autograd.heatmap_loss(heat, pts=pts, mask=m),
             lambda m: hkp_autograd.heatmap_loss(heat, uv=uv, mask=m))
    for fn in calls:
        with pytest.raises(HkpError, match="mask must be uint8"):
            fn(good.int())                                               # dtype
        with pytest.raises(HkpError, match="mask must be uint8"):
            fn(good[0])                                                  # dims
        with pytest.raises(HkpError, match="mask must be a uint8 tensor"):
            fn(good.numpy())
        with pytest.raises(HkpError, match=r"mask must be uint8 \[2,4,8\]"):
            fn(torch.zeros(2, 8, 4, dtype=torch.uint8))                  # shape
        with pytest.raises(HkpError, match=r"mask must be uint8 \[2,4,8\] on cpu, got .* on meta"):
            fn(good.to("meta"))                                          # device
        with pytest.raises(HkpError, match="mask must be contiguous"):
            fn(torch.zeros(2, 8, 4, dtype=torch.uint8).transpose(1, 2))
        with pytest.raises(HkpError, match="must be on the GPU"):        # ... and only then heat's device
            fn(good)
    wide, wide_pts = torch.rand(1, 9, 4, 8), torch.zeros(1, 9, 1, 3)
    with pytest.raises(HkpError, match="8 class bits, heat has K = 9"):
        ops.heat_loss_masked(wide, wide_pts, good[:1])
    with pytest.raises(HkpError, match="8 class bits, heat has K = 9"):
        hkp_autograd.heatmap_loss(wide, pts=wide_pts, mask=good[:1])
    with pytest.raises(HkpError, match="mask is required"):
        ops.heat_loss_masked(heat, pts, None)
    # a mask with a dense target
    with pytest.raises(HkpError, match="dense target is not supported"):
        ops.heat_loss(heat, target=heat.double(), mask=good)
    with pytest.raises(HkpError, match="dense target is not supported"):
        hkp_autograd.heatmap_loss(heat, target=heat.double(), mask=good)
    # the rasteriser and the warp
    regs = torch.zeros(2, 3, 6)
    for bad, what in ((regs.double(), "must be float32"), (regs[0], r"\[N,R,6\]"), (regs.numpy(), "got ndarray"),
                      (torch.zeros(2, 65, 6), "1 <= R <= 64"), (torch.zeros(2, 3, 5), r"\[N,R,6\]"),
                      (regs, "must be on the GPU")):
        with pytest.raises(HkpError, match=what):
            ops.mask_regions_u8(bad, 4, 8)
    for H, W in ((0, 8), (4, 4097), (4097, 4)):
        with pytest.raises(HkpError, match="1..4096"):
            ops.mask_regions_u8(regs, H, W)
    for fill in (-1, 256, 1.0, True):
        with pytest.raises(HkpError, match="fill is an integer"):
            ops.warp_mask_u8(good, None, fill=fill)
    with pytest.raises(HkpError, match="must be on the GPU"):
        ops.warp_mask_u8(good, None)


def test_trainer_rejects_a_mask_before_the_forward():
    from hkp import ops, train
    from src.model import KeypointsGauss
    tr = train.Trainer(KeypointsGauss(3, backbone="resnet18", pretrained=False))
    assert tr.plane_pixels is None
    x = torch.zeros(1, 3, 32, 32)
    good = torch.zeros(1, 32, 32, dtype=torch.uint8)
    with pytest.raises(ops.HkpError, match="dense target is not supported"):
        tr.forward_backward(x, target=torch.zeros(1, 3, 32, 32, dtype=torch.float64), mask=good)
    with pytest.raises(ops.HkpError, match="mask must be uint8"):
        tr.forward_backward(x, uv=torch.zeros(1, 3, 2), mask=good.float())
    tr9 = train.Trainer(KeypointsGauss(9, backbone="resnet18", pretrained=False))
    with pytest.raises(ops.HkpError, match="8 class bits"):
        tr9.step(x, uv=torch.zeros(1, 9, 2), mask=good)


def test_c_abi_rejects_before_any_launch():
    """No device pointer here is real: every one of these returns HKP_ERR_BAD_ARG first."""
    from hkp import _lib
    L = _lib.lib()
    for name in ("hkp_heat_loss_masked", "hkp_heat_loss_masked_workspace", "hkp_mask_regions_u8", "hkp_warp_mask_u8"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    base = L.hkp_heat_loss_planes_workspace(2, 3, 5, 7)
    assert L.hkp_heat_loss_masked_workspace(2, 3, 5, 7) >= base + (6 + 2 * 64 * 8) * 4
    assert L.hkp_heat_loss_masked_workspace(2, 3, 5, 7) % 8 == 0
    assert L.hkp_heat_loss_masked_workspace(0, 3, 5, 7) == -1
    P = ctypes.c_void_p(16)
    ok = dict(n=2, k=3, m=4, kind=_lib.HKP_LOSS_BCE, absent=0, norm=0, beta=2.0, topk=0, heat=P, pts=P, mask=P, loss=P,
              ws=P)

    def masked(**kw):
        a = dict(ok, **kw)
        _lib.call("hkp_heat_loss_masked", a["n"], a["k"], a["m"], 5, 7, a["kind"], a["absent"], a["norm"], a["beta"],
                  a["topk"], a["heat"], a["pts"], None, a["mask"], 8.0, a["loss"], None, None, None, None, a["ws"], None)

    with pytest.raises(_lib.HkpError, match="null mask"):
        masked(mask=None)
    for k in (9, 64):
        with pytest.raises(_lib.HkpError, match="a mask byte holds 8"):
            masked(n=1, k=k)
    for topk in (-1, 4):
        with pytest.raises(_lib.HkpError, match="topk"):
            masked(topk=topk)
    for name in ("heat", "pts", "loss", "ws"):
        with pytest.raises(_lib.HkpError, match="null tensor"):
            masked(**{name: None})
    with pytest.raises(_lib.HkpError, match=r"outside \[1, 8\]"):
        masked(kind=_lib.HKP_LOSS_QFL, beta=0.5)
    for kw, what in (({"kind": 3}, "bad loss kind"), ({"norm": 2}, "bad norm mode"), ({"absent": -1}, "bad absent mode"),
                     ({"m": 17}, "bad sizes"), ({"n": 0}, "bad sizes")):
        with pytest.raises(_lib.HkpError, match=what):
            masked(**kw)

    def regions(n=1, r=1, H=4, W=8, regs=P, out=P):
        _lib.call("hkp_mask_regions_u8", n, r, H, W, regs, out, None)

    for r in (0, 65):
        with pytest.raises(_lib.HkpError, match="outside 1..64"):
            regions(r=r)
    for kw in ({"H": 0}, {"W": 4097}, {"H": 4097}):
        with pytest.raises(_lib.HkpError, match="outside 1..4096"):
            regions(**kw)
    for kw, what in (({"n": 0}, "bad batch size"), ({"n": 65536}, "bad batch size"), ({"regs": None}, "null pointer"),
                     ({"out": None}, "null pointer"), ({"regs": ctypes.c_void_p(18)}, "4-byte aligned")):
        with pytest.raises(_lib.HkpError, match=what):
            regions(**kw)

    xf = (_lib.WarpXform * 2)()

    def warp(n=2, hs=5, ws=7, src=P, h=4, w=8, dst=ctypes.c_void_p(4096), host=xf, dev=P, border=0, fill=0):
        _lib.call("hkp_warp_mask_u8", n, hs, ws, src, h, w, dst, host, dev, border, fill, None, None)

    for border in (-1, 3):
        with pytest.raises(_lib.HkpError, match="unknown border mode"):
            warp(border=border)
    for kw in ({"hs": 0}, {"ws": 16385}, {"h": 16385}, {"w": 0}):
        with pytest.raises(_lib.HkpError, match="outside 1..16384"):
            warp(**kw)
    for fill in (-1, 256):
        with pytest.raises(_lib.HkpError, match="fill"):
            warp(fill=fill)
    with pytest.raises(_lib.HkpError, match="REFLECT101 needs"):
        warp(hs=1, border=2)
    for kw in ({"src": None}, {"dst": None}, {"host": None}, {"dev": None}):
        with pytest.raises(_lib.HkpError, match="null pointer"):
            warp(**kw)
    with pytest.raises(_lib.HkpError, match="must not overlap"):
        warp(dst=ctypes.c_void_p(20))
    xf[1].reserved = 1
    with pytest.raises(_lib.HkpError, match="non-zero reserved"):
        warp()
