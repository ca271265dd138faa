"""Per-pixel ignore masks on the GPU: hkp_heat_loss_masked against hkp_heat_loss_planes bit
for bit where the two agree by definition (an all-zero mask; whole planes masked = weight 0)
and against the float64 reference of tests/_masks_ref.py; the rasteriser against its numpy
restatement; the mask warp against tests/_warp_ref.py and against the image warp itself;
and the layers above (ops, autograd, Trainer, WarpPlan, KeypointMetrics).

Loss shapes, labels and heat are those of tests/test_gpu_instances.py (imported): the scalar
and the 16-byte path, a misaligned base, fewer elements than a block, several trips.  The
dense target comes from the existing target kernel.  Each figure is printed before it is
asserted (pytest -s)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _masks_ref as mref
import _warp_ref as wref
from oracle import recipe
from test_gpu_focal import _differ, _labels, _loss_bound, _plus_zero, _r18, _within_one_ulp
from test_gpu_instances import SHAPES, _heat, _same_bits
from test_gpu_planes import _bits64, _target_of, _weights

pytestmark = pytest.mark.gpu

NAN = float("nan")
ABSENT = ["zero", "ignore"]
NORMS = ["elements", "instances"]
KINDS = [("bce", 2.0), ("mse", 2.0), ("qfl", 2.0), ("qfl", 1.5)]


def _close(what, got, want, total):
    err, bound = abs(got - want), _loss_bound(total, want)
    print("%s: loss %.17g ref %.17g err %.3e bound %.3e" % (what, got, want, err, bound))
    assert np.isfinite(got) and err <= bound, (what, err, bound)


def _planes_close(what, got, want, pixels):
    """plane_loss against the reference's: -1 in the same places, the others within the sum
    bound of the plane's kept pixels."""
    got, want = got.cpu(), want.cpu()
    print("%s: plane_loss worst error %.3e" % (what, (got - want).abs().max().item()))
    assert torch.equal(got == -1, want == -1)
    assert ((got - want).abs() <= (pixels.double() + 16) * 2.0 ** -53 * want.abs()).all()


def _ref(shape, mask, absent, norm, kind, beta, weights=None, topk=None, heat=None, sigma=8.0):
    return mref.masked_ref(_heat(shape) if heat is None else heat, _target_of(shape, absent, sigma),
                           _labels(shape, absent), mask, kind, absent, norm, beta, weights, topk)


def _all_equal(what, a, b, outputs=4):
    """loss, dheat, plane_loss, plane_used (and plane_pixels with outputs=5), bit for bit."""
    assert np.array_equal(_bits64(a[0]), _bits64(b[0])), what + ": loss"
    _same_bits(what, a[1], b[1])
    assert np.array_equal(_bits64(a[2]), _bits64(b[2])), what + ": plane_loss"
    assert torch.equal(a[3], b[3]), what + ": plane_used"
    if outputs == 5:
        assert torch.equal(a[4], b[4]), what + ": plane_pixels"


def _off_by(t, nbytes, align):
    """A contiguous copy of t that starts nbytes past an `align`-byte boundary."""
    es = t.element_size()
    assert nbytes % es == 0
    buf = torch.empty(t.numel() + align // es, device=t.device, dtype=t.dtype)
    start = ((-buf.data_ptr()) % align + nbytes) // es
    v = buf[start:start + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % align == nbytes
    return v


# ------------------------------------------------------------------ 1. the all-zero mask ----

@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("absent", ABSENT)
@pytest.mark.parametrize("shape", SHAPES)
def test_all_zero_mask_gives_the_bits_of_the_planes_entry(cuda_device, shape, absent, norm):
    from hkp import ops
    n, k, m, H, W = shape
    pd, ptsd = _heat(shape).to(cuda_device), _labels(shape, absent).to(cuda_device)
    zero = torch.zeros(n, H, W, dtype=torch.uint8, device=cuda_device)
    wd = _weights(shape).to(cuda_device)
    for kind, beta in KINDS:
        for w in (None, wd):
            what = "zero mask %s %g %s %s %s weights %s" % (kind, beta, absent, norm, shape, w is not None)
            a = ops.heat_loss_planes(pd, ptsd, 8.0, kind, absent, beta=beta, norm=norm, weights=w)
            b = ops.heat_loss_masked(pd, ptsd, zero, 8.0, kind, absent, beta=beta, norm=norm, weights=w)
            _all_equal(what, b, a)
            assert b[4].dtype == torch.int32 and torch.equal(b[4], a[3] * (H * W))


@pytest.mark.parametrize("absent", ABSENT)
def test_all_zero_mask_from_a_base_off_a_16_byte_boundary(cuda_device, absent):
    """W % 4 == 0 but the heatmaps start 4 bytes off a 16-byte boundary: the scalar path."""
    from hkp import ops
    shape = SHAPES[4]
    n, k, m, H, W = shape
    off = _off_by(_heat(shape).to(cuda_device), 4, 16)
    ptsd = _labels(shape, absent).to(cuda_device)
    zero = torch.zeros(n, H, W, dtype=torch.uint8, device=cuda_device)
    seeded = mref.seeded_mask(shape).to(cuda_device)
    wd = _weights(shape).to(cuda_device)
    for kind, beta in KINDS:
        for norm in NORMS:
            a = ops.heat_loss_planes(off, ptsd, 8.0, kind, absent, beta=beta, norm=norm, weights=wd)
            b = ops.heat_loss_masked(off, ptsd, zero, 8.0, kind, absent, beta=beta, norm=norm, weights=wd)
            _all_equal("unaligned base %s %s" % (kind, norm), b, a)
            # ... and with a real mask the two paths agree in everything but the order of the sums
            c = ops.heat_loss_masked(off, ptsd, seeded, 8.0, kind, absent, beta=beta, norm=norm, weights=wd)
            d = ops.heat_loss_masked(_heat(shape).to(cuda_device), ptsd, seeded, 8.0, kind, absent, beta=beta,
                                     norm=norm, weights=wd)
            assert torch.equal(c[3], d[3]) and torch.equal(c[4], d[4])
            _close("unaligned vs aligned", c[0].item(), d[0].item(), n * k * H * W)


# -------------------------------------------------------------------- 2. seeded masks ----

@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("absent", ABSENT)
@pytest.mark.parametrize("shape", SHAPES)
def test_seeded_masks_against_the_reference(cuda_device, shape, absent, norm):
    from hkp import ops
    n, k, m, H, W = shape
    mask = mref.seeded_mask(shape)
    keep = mref.keep_of(mask, k)
    p = _heat(shape)
    dirty = torch.where(keep, p, torch.full_like(p, NAN))         # NaN under every masked pixel
    pd, dd, ptsd, md = p.to(cuda_device), dirty.to(cuda_device), _labels(shape, absent).to(cuda_device), \
        mask.to(cuda_device)
    w = _weights(shape)
    for kind, beta in KINDS:
        for weights in (None, w):
            ref = _ref(shape, mask, absent, norm, kind, beta, weights)
            what = "seeded %s %g %s %s %s weights %s" % (kind, beta, absent, norm, shape, weights is not None)
            wd = None if weights is None else weights.to(cuda_device)
            got = ops.heat_loss_masked(pd, ptsd, md, 8.0, kind, absent, beta=beta, norm=norm, weights=wd)
            loss, dheat, plane_loss, plane_used, plane_pixels = got
            _within_one_ulp(what, dheat, ref["dheat"])
            g = dheat.cpu()
            assert _plus_zero(g[~keep]) and _plus_zero(g[~ref["used"]])
            assert torch.equal(plane_used.cpu().bool(), ref["used"])
            assert torch.equal(plane_pixels.cpu().long(), ref["plane_pixels"])
            _planes_close(what, plane_loss, ref["plane_loss"], ref["plane_pixels"])
            _close(what, loss.item(), ref["loss"], ref["elements"])
            if n > 1:
                assert not ref["used"][n - 1].any()                 # the image at 0xFF
            # NaN heat under the masked pixels: not one output bit moves
            _all_equal(what + " with NaN under the mask", ops.heat_loss_masked(
                dd, ptsd, md, 8.0, kind, absent, beta=beta, norm=norm, weights=wd), got, 5)
            # the same call through heat_loss_multi
            l2, g2 = ops.heat_loss_multi(pd, ptsd, 8.0, kind, absent, beta=beta, norm=norm, weights=wd, mask=md)
            assert np.array_equal(_bits64(l2), _bits64(loss))
            _same_bits(what + " via heat_loss_multi", g2, dheat)


@pytest.mark.parametrize("absent", ABSENT)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4], SHAPES[5]])
def test_whole_planes_masked_equal_weights_of_zero(cuda_device, shape, absent):
    from hkp import ops
    n, k, m, H, W = shape
    off = torch.zeros(n * k, dtype=torch.bool)
    off[1] = off[n * k - 1] = True
    off = off.view(n, k)
    md = mref.plane_mask(shape, off).to(cuda_device)
    pd, ptsd = _heat(shape).to(cuda_device), _labels(shape, absent).to(cuda_device)
    zero = torch.zeros_like(md)
    for kind, beta in KINDS:
        for norm in NORMS:
            for w in (None, _weights(shape)):
                w0 = torch.where(off, torch.zeros(()), torch.ones(n, k) if w is None else w).to(cuda_device)
                wd = None if w is None else w.to(cuda_device)
                for topk in (None, 1):
                    a = ops.heat_loss_masked(pd, ptsd, md, 8.0, kind, absent, beta=beta, norm=norm, weights=wd,
                                             topk=topk)
                    b = ops.heat_loss_masked(pd, ptsd, zero, 8.0, kind, absent, beta=beta, norm=norm, weights=w0,
                                             topk=topk)
                    _all_equal("planes masked %s %s %s topk %s" % (kind, norm, shape, topk), a, b, 5)
                    c = ops.heat_loss_planes(pd, ptsd, 8.0, kind, absent, beta=beta, norm=norm, weights=w0, topk=topk)
                    _all_equal("planes masked vs the planes entry", a, c)
                    assert (a[2].cpu()[off] == -1).all() and (a[4].cpu()[off] == 0).all()


def test_everything_masked(cuda_device):
    from hkp import ops
    shape = SHAPES[0]
    n, k, m, H, W = shape
    p = _heat(shape)
    p[0, 0, 0, 0] = NAN
    full = torch.full((n, H, W), 0xFF, dtype=torch.uint8, device=cuda_device)
    for kind, beta in KINDS:
        for norm in NORMS:
            for topk in (None, 2):
                loss, dheat, pl, pu, px = ops.heat_loss_masked(p.to(cuda_device), _labels(shape, "zero").to(cuda_device),
                                                               full, 8.0, kind, beta=beta, norm=norm, topk=topk)
                assert loss.item() == 0.0 and _plus_zero(dheat) and (pl == -1).all() and not pu.any() and not px.any()


@pytest.mark.parametrize("topk", [None, 2])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3], SHAPES[5]])
def test_second_run_and_missing_outputs_give_the_same_bits(cuda_device, shape, topk):
    from hkp import _lib, ops
    n, k, m, H, W = shape
    pd, ptsd = _heat(shape).to(cuda_device), _labels(shape, "ignore").to(cuda_device)
    wd, md = _weights(shape).to(cuda_device), mref.seeded_mask(shape).to(cuda_device)
    P = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    for kind, beta in KINDS:
        a = ops.heat_loss_masked(pd, ptsd, md, 8.0, kind, "ignore", beta=beta, weights=wd, topk=topk)
        b = ops.heat_loss_masked(pd, ptsd, md, 8.0, kind, "ignore", beta=beta, weights=wd, topk=topk)
        _all_equal("second run", b, a, 5)
        c = ops.heat_loss_masked(pd, ptsd, md, 8.0, kind, "ignore", want_grad=False, beta=beta, weights=wd, topk=topk)
        assert c[1] is None and np.array_equal(_bits64(a[0]), _bits64(c[0])) and torch.equal(a[3], c[3])
        ws = torch.empty(_lib.lib().hkp_heat_loss_masked_workspace(n, k, H, W) // 8, device=cuda_device,
                         dtype=torch.float64)
        loss = torch.full((), NAN, device=cuda_device, dtype=torch.float64)
        _lib.call("hkp_heat_loss_masked", n, k, m, H, W, {"bce": 0, "mse": 1, "qfl": 2}[kind], 1, 0, beta, topk or 0,
                  P(pd), P(ptsd), P(wd), P(md), 8.0, P(loss), None, None, None, None, P(ws), ops._stream())
        assert np.array_equal(_bits64(a[0]), _bits64(loss))


# ------------------------------------------------------------------ 3. mask alignment ----

@pytest.mark.parametrize("shape", [SHAPES[4], SHAPES[5]])
def test_mask_one_byte_off_a_4_byte_boundary(cuda_device, shape):
    """The 16-byte path with the mask bytes read singly equals the path with 32-bit loads."""
    from hkp import ops
    assert shape in ((2, 2, 3, 12, 40), (1, 2, 3, 260, 256))
    pd, ptsd = _heat(shape).to(cuda_device), _labels(shape, "ignore").to(cuda_device)
    md = mref.seeded_mask(shape).to(cuda_device)
    assert md.data_ptr() % 4 == 0 and pd.data_ptr() % 16 == 0
    off = _off_by(md, 1, 4)
    wd = _weights(shape).to(cuda_device)
    for kind, beta in KINDS:
        for norm in NORMS:
            for topk in (None, 1):
                a = ops.heat_loss_masked(pd, ptsd, md, 8.0, kind, "ignore", beta=beta, norm=norm, weights=wd, topk=topk)
                b = ops.heat_loss_masked(pd, ptsd, off, 8.0, kind, "ignore", beta=beta, norm=norm, weights=wd, topk=topk)
                _all_equal("mask off by one byte %s %s %s topk %s" % (kind, norm, shape, topk), b, a, 5)


# ----------------------------------------------------------------------------- 4. top-k ----

@pytest.mark.parametrize("kind", ["bce", "mse"])
@pytest.mark.parametrize("shape", mref.TOPK_SHAPES)
def test_topk_with_masks_against_the_reference(cuda_device, shape, kind):
    from hkp import ops
    n, k, m, H, W = shape
    for absent in ABSENT:
        p, pts, mask = mref.topk_inputs(shape, absent)
        pd, ptsd, md = p.to(cuda_device), pts.to(cuda_device), mask.to(cuda_device)
        for w in (None, mref.topk_weights(shape)):
            wd = None if w is None else w.to(cuda_device)
            base = _ref(shape, mask, absent, "elements", kind, 2.0, w, heat=p)
            gap = mref.rank_gap(base["S"], base["plane_pixels"], w, base["eligible"])
            print("top-k %s %s %s weights %s: smallest relative rank gap %.3e" % (shape, kind, absent, w is not None,
                                                                                 gap))
            assert gap >= mref.TOPK_MIN_GAP                      # the precondition (test_masks_cpu.py pins it too)
            for norm in NORMS:
                plain = ops.heat_loss_masked(pd, ptsd, md, 8.0, kind, absent, norm=norm, weights=wd)
                for T in (1, 2, k):
                    ref = _ref(shape, mask, absent, norm, kind, 2.0, w, T, heat=p)
                    what = "top-%d %s %s %s %s weights %s" % (T, shape, kind, absent, norm, w is not None)
                    loss, dheat, plane_loss, plane_used, plane_pixels = ops.heat_loss_masked(
                        pd, ptsd, md, 8.0, kind, absent, norm=norm, weights=wd, topk=T)
                    used = ref["used"]
                    assert torch.equal(plane_used.cpu().bool(), used), what
                    assert (used.sum(1) == torch.minimum(ref["eligible"].sum(1), torch.tensor(T))).all()
                    _close(what, loss.item(), ref["loss"], ref["elements"])
                    _within_one_ulp(what, dheat, ref["dheat"])
                    assert torch.equal(plane_pixels, plain[4])
                    assert np.array_equal(_bits64(plane_loss), _bits64(plain[2]))     # not counted: the value stays
                    # the same gradient as the selection written into the weights
                    sel = used.float() * (1.0 if w is None else w)
                    as_w = ops.heat_loss_masked(pd, ptsd, md, 8.0, kind, absent, norm=norm, weights=sel.to(cuda_device))
                    _same_bits(what + " vs the selection as weights", dheat, as_w[1])
                    if T == k:
                        _all_equal(what + " vs topk=None", (loss, dheat, plane_loss, plane_used, plane_pixels), plain, 5)


# --------------------------------------------------------------------------- 5. routing ----

def test_routing(cuda_device, monkeypatch):
    """Without a mask every layer makes the library calls it makes on the unmasked paths, in
    order, none of them hkp_heat_loss_masked; with one, exactly one such call.  (The calls are
    seen where tests/test_gpu_planes.py sees them, at ops.call: ops.set_observer is only told
    of the convolutions.)"""
    from hkp import _lib, ops, train
    from hkp import autograd as hkp_autograd
    B, K, H, W = 2, 3, 64, 96
    x = recipe.to_tensor_nchw(recipe.seeded_images_u8(B, H, W, 21)).to(cuda_device)
    uv = torch.from_numpy(recipe.seeded_keypoints(B, K, H, W, 22)).to(cuda_device)
    pts = torch.cat([uv, torch.ones(B, K, 1, device=cuda_device)], -1).reshape(B, K, 1, 3).contiguous()
    mask = mref.seeded_mask((B, K, 1, H, W)).to(cuda_device)
    names = []
    real = ops.call
    spy = lambda name, *a: (names.append(name), real(name, *a))[1]      # noqa: E731
    monkeypatch.setattr(ops, "call", spy)
    monkeypatch.setattr(_lib, "call", spy)
    seen = []
    ops.set_observer(lambda name, flops, nbytes, launch: (seen.append(name), launch()))

    def calls(fn):
        del names[:]
        fn()
        return [v for v in names if not v.endswith("_workspace") and not v.endswith("_bytes")]

    MASKED = "hkp_heat_loss_masked"
    try:
        model = _r18(cuda_device, K)
        for kw, entry in (({}, "hkp_heat_loss_multi"), ({"loss_params": {"topk": 2}}, "hkp_heat_loss_planes")):
            tr = train.Trainer(model, **kw)
            tr.forward_backward(x, pts=pts)                       # (the first step also packs the weights)
            plain = calls(lambda: tr.forward_backward(x, pts=pts))
            again = calls(lambda: tr.forward_backward(x, pts=pts, mask=None))
            assert plain == again and MASKED not in plain and plain.count(entry) == 1
            with_mask = calls(lambda: tr.forward_backward(x, pts=pts, mask=mask))
            assert with_mask.count(MASKED) == 1 and entry not in with_mask
            assert [MASKED if v == entry else v for v in plain] == with_mask       # nothing else moved
            assert tr.plane_pixels is not None and tr.plane_pixels.shape == (B, K)
            calls(lambda: tr.forward_backward(x, pts=pts))
            assert tr.plane_pixels is None
        tr = train.Trainer(model)
        assert MASKED not in calls(lambda: tr.forward_backward(x, uv=uv))
        assert calls(lambda: tr.forward_backward(x, uv=uv, mask=mask)).count(MASKED) == 1
        assert seen                                                # the observer saw the convolutions
        hm = model(x).detach()
        loss_calls = lambda fn: [v for v in calls(fn) if v.startswith("hkp_heat_loss")]     # noqa: E731
        assert loss_calls(lambda: ops.heat_loss_multi(hm, pts)) == ["hkp_heat_loss_multi"]
        assert loss_calls(lambda: ops.heat_loss_multi(hm, pts, mask=None, topk=1)) == ["hkp_heat_loss_planes"]
        assert loss_calls(lambda: ops.heat_loss_planes(hm, pts)) == ["hkp_heat_loss_planes"]
        assert loss_calls(lambda: ops.heat_loss(hm, uv=uv)) == ["hkp_heat_loss"]
        assert loss_calls(lambda: hkp_autograd.heatmap_loss(hm, pts=pts, return_planes=True)) == ["hkp_heat_loss_planes"]
        for fn in (lambda: ops.heat_loss_multi(hm, pts, mask=mask), lambda: ops.heat_loss(hm, uv=uv, mask=mask),
                   lambda: ops.heat_loss_masked(hm, pts, mask, topk=2),
                   lambda: hkp_autograd.heatmap_loss(hm, pts=pts, mask=mask),
                   lambda: hkp_autograd.heatmap_loss(hm, uv=uv, mask=mask, weights=torch.ones(B, K, device=cuda_device))):
            assert loss_calls(fn) == [MASKED]
    finally:
        ops.set_observer(None)


# ---------------------------------------------------------------------------- 6. layers ----

def test_training_step(cuda_device):
    from hkp import autograd as hkp_autograd
    from hkp import net, ops, train
    B, K, H, W = 2, 3, 96, 128
    x = recipe.to_tensor_nchw(recipe.seeded_images_u8(B, H, W, 21)).to(cuda_device)
    uv = torch.from_numpy(recipe.seeded_keypoints(B, K, H, W, 22)).to(cuda_device)
    pts = torch.cat([uv, torch.ones(B, K, 1, device=cuda_device)], -1).reshape(B, K, 1, 3).contiguous()
    g = torch.Generator().manual_seed(31)
    mask = torch.zeros(B, H, W, dtype=torch.int64)
    for c in range(K):
        mask |= (torch.rand(B, H, W, generator=g) < 0.3).long() << c
    k0 = 1
    mask |= 1 << k0                                                 # class 1 is masked everywhere
    mask = mask.to(torch.uint8).to(cuda_device)
    m_tr, m_man, m_auto, m_zero, m_plain = (_r18(cuda_device, K) for _ in range(5))
    # the manual chain
    trace = net.Trace(m_man.policy)
    hm, _, _ = net.keypoints_forward(m_man.resnet.net, x, K, heat=True, trace=trace)
    l_man, dheat, pl_man, pu_man, px_man = ops.heat_loss_masked(hm, pts, mask, 8.0, "bce", "zero", True)
    grads = net.Grads()
    net.keypoints_backward(m_man.resnet.net, trace, dheat, grads)
    for p in m_man.parameters():
        p.grad = grads[p]
    assert pu_man.sum(0).tolist() == [B, 0, B] and (px_man[:, k0] == 0).all() and (px_man[:, 0] > 0).all()
    tr = train.Trainer(m_tr)
    l_tr = tr.step(x, pts=pts, mask=mask)
    print("Trainer masked loss %.17g, manual %.17g" % (l_tr.item(), l_man.item()))
    assert l_tr.item() == l_man.item() and np.isfinite(l_tr.item()) and l_tr.item() > 0
    differ = _differ(m_tr, m_man)
    print("parameter gradients that differ between Trainer.step and the manual chain:", differ)
    assert not differ
    assert torch.equal(tr.plane_loss, pl_man) and torch.equal(tr.plane_used, pu_man)
    assert torch.equal(tr.plane_pixels, px_man) and tr.plane_pixels.is_cuda
    # the class masked everywhere: its row of the scoring conv gets exactly nothing
    fc = m_tr.resnet.net.fc
    assert (fc.weight.grad[k0] == 0).all() and fc.bias.grad[k0].item() == 0
    for kk in (0, 2):
        assert fc.weight.grad[kk].abs().max().item() > 0 and fc.bias.grad[kk].item() != 0
    # the autograd path
    l_auto, pl_auto, pu_auto, px_auto = hkp_autograd.heatmap_loss(m_auto(x), pts=pts, mask=mask, return_planes=True)
    assert l_auto.requires_grad and not pl_auto.requires_grad and not px_auto.requires_grad
    l_auto.backward()
    assert l_auto.item() == l_man.item() and torch.equal(pl_auto, pl_man) and torch.equal(px_auto, px_man)
    differ = _differ(m_auto, m_man)
    print("parameter gradients that differ between autograd and the manual chain:", differ)
    assert not differ
    # an all-zero mask: every gradient of the step without a mask
    l_zero = train.Trainer(m_zero).forward_backward(x, pts=pts, mask=torch.zeros_like(mask))
    l_plain = train.Trainer(m_plain).forward_backward(x, pts=pts)
    _close("all-zero mask vs no mask", l_zero.item(), l_plain.item(), B * K * H * W)      # (the sums' orders differ)
    assert not _differ(m_zero, m_plain)


# ------------------------------------------------------------------------ 7. rasteriser ----

RASTER_SIZES = [(1, 1, 1, 1), (2, 4, 17, 23), (2, 3, 12, 40), (1, 64, 33, 131)]


@functools.lru_cache(maxsize=None)
def _regions(size):
    """Seeded records float32 [n,r,6] (numpy, read-only use): boxes and discs with integer and
    fractional bounds, partly outside the frame, an empty slot of unknown kind full of NaN,
    a NaN bound, a radius of 0, bits of every value."""
    n, r, H, W = size
    rng = np.random.default_rng(n * 1000 + r * 10 + W)
    regs = np.zeros((n, r, 6), dtype=np.float32)
    for b in range(n):
        for j in range(r):
            kind = (1, 2, 1, 2, 7)[(b + j) % 5]
            if r == 1:
                kind = 1
            frac = rng.random() < 0.5
            a, bb = rng.uniform(-3, W), rng.uniform(-3, H)
            if kind == 1:
                c, d = a + rng.uniform(0, W / 2 + 1), bb + rng.uniform(0, H / 2 + 1)
            else:
                c, d = rng.uniform(0, max(H, W) / 3 + 1), NAN
            rec = [kind, a, bb, c, d]
            if not frac:
                rec = [kind] + [np.round(v) for v in rec[1:]]
            regs[b, j, :5] = rec
            regs[b, j, 5] = rng.integers(0, 256)
            if kind == 7:
                regs[b, j, 1:] = NAN
    if r >= 4:
        regs[0, 1] = (2.0, 5.0, 6.0, 5.0, 0.0, 64.0)              # (3, 4) away is exactly r^2
        regs[0, 2] = (1.0, NAN, 0.0, 9.0, 9.0, 255.0)              # a NaN bound: never inside
        regs[n - 1, 3] = (2.0, 4.0, 3.0, 0.0, 0.0, 16.0)           # r = 0: its centre alone
    if size == (1, 1, 1, 1):
        regs[0, 0] = (1.0, 0.0, 0.0, 0.0, 0.0, 37.0)
    return regs


@pytest.mark.parametrize("size", RASTER_SIZES)
def test_rasteriser_against_the_restatement(cuda_device, size):
    from hkp import ops
    n, r, H, W = size
    regs = _regions(size)
    want = torch.from_numpy(mref.regions_ref(regs, H, W))
    print("%s: %d of %d pixels set, values %s" % (size, int((want != 0).sum()), want.numel(), want.unique().numel()))
    assert (want != 0).any()
    rd = torch.from_numpy(regs).to(cuda_device)
    got = ops.mask_regions_u8(rd, H, W)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, H, W) and torch.equal(got.cpu(), want)
    if r >= 4:
        assert want[0, 6 + 4, 5 + 3] & 64 and want[0, 6 - 3, 5 - 4] & 64 and want[n - 1, 3, 4] & 16
    # a second run, and into a preallocated out that held 0xAA
    assert torch.equal(ops.mask_regions_u8(rd, H, W), got)
    out = torch.full((n, H, W), 0xAA, dtype=torch.uint8, device=cuda_device)
    assert ops.mask_regions_u8(rd, H, W, out=out) is out and torch.equal(out, got)
    # into a view one byte off alignment (the byte path also where W % 4 == 0), guards untouched
    buf = torch.full((n * H * W + 16,), 0x5C, dtype=torch.uint8, device=cuda_device)
    start = (-buf.data_ptr()) % 4 + 5
    view = buf[start:start + n * H * W].view(n, H, W)
    assert view.data_ptr() % 4 == 1
    ops.mask_regions_u8(rd, H, W, out=view)
    assert torch.equal(view, got) and (buf[:start] == 0x5C).all() and (buf[start + n * H * W:] == 0x5C).all()


def test_rasteriser_through_the_builders(cuda_device):
    from hkp import masks, ops
    recs = [[masks.box(2, 3, 5, 4, (0, 2)), masks.disc(10, 6, 5, 3)], [masks.disc(4, 7, 0, None)]]
    regs = masks.pack(recs, R=3)
    got = ops.mask_regions_u8(regs.to(cuda_device), 12, 20).cpu()
    assert torch.equal(got, torch.from_numpy(mref.regions_ref(regs.numpy(), 12, 20)))
    assert got[0, 3, 2] == 5 and got[0, 6 + 4, 10 + 3] == 8 and got[1].sum() == 255 and got[1, 7, 4] == 255


# ------------------------------------------------------------------------- 8. mask warp ----

def _warp_mats(hs, ws, h, w):
    from hkp import geometry as G
    base = G.resize_matrix(hs, ws, h, w)

    def after(M):                                            # the resize first, then M in the output frame
        A = np.vstack([M, [0, 0, 1]]) @ np.vstack([base, [0, 0, 1]])
        return A[:2]
    return [after(G.affine_matrix(h, w, rotate_deg=30, scale=0.9)), after(G.affine_matrix(h, w, hflip=True)),
            after(G.affine_matrix(h, w, translate_xy_px=(w / 2.0, 0.0)))]


@pytest.mark.parametrize("fill", [0, 255])
@pytest.mark.parametrize("border", ["constant", "replicate", "reflect101"])
@pytest.mark.parametrize("hw", [(12, 40), (13, 21)])
def test_mask_warp(cuda_device, hw, border, fill):
    from hkp import geometry as G
    from hkp import masks, ops
    hs, ws, (h, w) = 17, 23, hw
    g = torch.Generator().manual_seed(7)
    src = torch.randint(0, 256, (3, hs, ws), generator=g, dtype=torch.uint8)
    mats = _warp_mats(hs, ws, h, w)
    flipped = [False, True, False]
    plan = G.WarpPlan(mats, (h, w), flipped=flipped, fill=(fill, fill, fill), interp="bilinear", border=border)
    sd = src.to(cuda_device)
    got = ops.warp_mask_u8(sd, plan, fill=fill)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, h, w)
    # the restatement on the mask replicated to three channels
    rep = src[..., None].expand(3, hs, ws, 3).contiguous()
    want = wref.warp_batch(rep.numpy(), plan.coefficients(), h, w, wref.NEAREST, G.BORDER[border],
                           [(fill, fill, fill)] * 3)
    assert np.array_equal(got.cpu().numpy(), want[..., 0])
    outside = int((want[2, ..., 0] == fill).sum())
    print("%s %s fill %d: %d of %d pixels of the pushed image hold the fill value" % (hw, border, fill, outside, h * w))
    if border == "constant":
        assert outside >= h * w // 3
    # the existing kernel as the oracle: channel 0 of the nearest image warp of the replica
    near = G.WarpPlan(mats, (h, w), flipped=flipped, fill=(fill, fill, fill), interp="nearest", border=border)
    assert torch.equal(got, ops.warp_affine_u8(rep.to(cuda_device), near)[..., 0])
    # flip pairs: bits 0 and 1 of the flipped image change places, nothing else does
    pairs = G.WarpPlan(mats, (h, w), flipped=flipped, flip_pairs=((0, 1),), border=border)
    sw = pairs.apply_mask(sd, fill=fill)
    lut = torch.from_numpy(mref.flip_lut(((0, 1),)))
    want_sw = torch.from_numpy(want[..., 0].copy())
    moved = lut[want_sw[1].long()]
    if border == "constant":                                  # the fill byte is written as given
        ins = torch.from_numpy(wref.warp_batch(np.zeros_like(rep.numpy()), plan.coefficients(), h, w, wref.NEAREST,
                                               wref.CONSTANT, [(1, 1, 1)] * 3)[1, ..., 0] == 0)
        moved = torch.where(ins, moved, torch.full_like(moved, fill))
    want_sw[1] = moved
    assert torch.equal(sw.cpu(), want_sw)
    assert torch.equal(sw[0], got[0]) and torch.equal(sw[2], got[2])
    assert torch.equal(sw[1] & 0xFC, got[1] & 0xFC) and not torch.equal(sw[1], got[1])
    # apply_mask is warp_mask_u8 with the table built by hand; without pairs there is no table
    hand = torch.stack([torch.arange(256, dtype=torch.uint8), lut, torch.arange(256, dtype=torch.uint8)])
    assert torch.equal(sw, ops.warp_mask_u8(sd, pairs, fill=fill, lut=hand.to(cuda_device)))
    assert torch.equal(pairs.mask_lut(cuda_device).cpu(), hand) and plan.mask_lut(cuda_device) is None
    assert pairs.mask_lut(cuda_device) is pairs.mask_lut(cuda_device)            # cached on the plan
    assert torch.equal(plan.apply_mask(sd, fill=fill), got)
    assert torch.equal(masks.flip_lut(((0, 1),)), lut)


@pytest.mark.parametrize("hw", [(12, 40), (13, 21)])
def test_mask_warp_into_an_unaligned_view(cuda_device, hw):
    """The byte path from an output one byte off a 4-byte boundary: the same bytes, and the
    guard bytes around the view untouched."""
    from hkp import geometry as G
    from hkp import ops
    hs, ws, (h, w) = 17, 23, hw
    src = torch.randint(0, 256, (3, hs, ws), generator=torch.Generator().manual_seed(7), dtype=torch.uint8)
    plan = G.WarpPlan(_warp_mats(hs, ws, h, w), (h, w), border="constant")
    sd = src.to(cuda_device)
    want = ops.warp_mask_u8(sd, plan, fill=255)
    buf = torch.full((3 * h * w + 16,), 0x5C, dtype=torch.uint8, device=cuda_device)
    start = (-buf.data_ptr()) % 4 + 5
    view = buf[start:start + 3 * h * w].view(3, h, w)
    assert view.data_ptr() % 4 == 1
    assert ops.warp_mask_u8(sd, plan, fill=255, out=view) is view and torch.equal(view, want)
    assert (buf[:start] == 0x5C).all() and (buf[start + 3 * h * w:] == 0x5C).all()


# ------------------------------------------------------------------------ 9. end to end ----

def test_frame_end_to_end(cuda_device):
    """A disc rasterised on a keypoint, the mask and the points moved by one plan: the moved
    point lies on a set pixel of the moved mask; the GPU drops the peaks the CPU loops drop;
    and the metrics of update(mask=) are those of an update fed the filtered peaks."""
    from hkp import geometry as G
    from hkp import masks, metrics, ops
    B, K, H, W = 3, 3, 48, 64
    pts = torch.zeros(B, K, 1, 3)
    pts[..., 2] = 1.0
    pts[:, :, 0, 0] = torch.tensor([[20.0, 40.0, 31.0], [12.0, 50.0, 33.0], [25.0, 36.0, 44.0]])
    pts[:, :, 0, 1] = torch.tensor([[15.0, 30.0, 22.0], [35.0, 12.0, 24.0], [20.0, 28.0, 16.0]])
    # class 1's keypoint of every image lies under a disc that ignores class 1 (and, image 0, class 2)
    recs = [[masks.disc(float(pts[b, 1, 0, 0]), float(pts[b, 1, 0, 1]), 4, (1, 2) if b == 0 else 1)] for b in range(B)]
    src = ops.mask_regions_u8(masks.pack(recs).to(cuda_device), H, W)
    mats = [G.affine_matrix(H, W, rotate_deg=15, scale=0.95), G.affine_matrix(H, W, hflip=True),
            G.affine_matrix(H, W, translate_xy_px=(5.0, -3.0))]
    plan = G.WarpPlan(mats, (H, W), flipped=[False, True, False], flip_pairs=((1, 2),), border="constant")
    moved_mask = plan.apply_mask(src).cpu()
    moved_pts = plan.apply_points(pts)
    for b in range(B):
        c = 2 if b == 1 else 1                                  # the flipped image: class 1's row and bit are class 2's
        u, v, flag = moved_pts[b, c, 0].tolist()
        assert flag > 0
        byte = int(moved_mask[b, int(np.floor(v + 0.5)), int(np.floor(u + 0.5))])
        print("image %d: the moved point (%.2f, %.2f) of class %d lies on mask byte %#x" % (b, u, v, c, byte))
        assert (byte >> c) & 1
        assert not torch.equal(moved_mask[b], src[b].cpu())
    # peaks on and off the moved mask
    g = torch.Generator().manual_seed(13)
    P = 4
    peaks = torch.rand(B, K, P, 3, generator=g) * torch.tensor([W - 1.0, H - 1.0, 1.0])
    peaks[:, :, 0, :2] = moved_pts[:, :, 0, :2]                 # one peak per plane on its label
    peaks[0, 0, 1, 0] = NAN
    counts = torch.tensor([[4, 3, 2], [4, 4, 2], [1, 6, -2]], dtype=torch.int32)
    want_p, want_c = mref.peaks_drop_masked(peaks, counts, moved_mask)
    got_p, got_c = masks.peaks_drop_masked(peaks.to(cuda_device), counts.to(cuda_device), moved_mask.to(cuda_device))
    assert torch.equal(got_c.cpu(), want_c) and int((counts.clamp(0, P) - want_c).sum()) >= B
    assert np.array_equal(got_p.cpu().numpy().view(np.int32), want_p.numpy().view(np.int32))
    labels = moved_pts.to(cuda_device)
    a, b = metrics.KeypointMetrics(K, (2, 4), bins=64), metrics.KeypointMetrics(K, (2, 4), bins=64)
    a.update(peaks.to(cuda_device), counts.to(cuda_device), labels, mask=moved_mask.to(cuda_device))
    b.update(want_p.to(cuda_device), want_c.to(cuda_device), labels)
    assert torch.equal(a.hist, b.hist) and torch.equal(a.totals, b.totals) and int(a.totals.sum()) > 0
    c = metrics.KeypointMetrics(K, (2, 4), bins=64)
    c.update(peaks.to(cuda_device), counts.to(cuda_device), labels)
    assert not torch.equal(c.totals, a.totals)                  # the mask took detections out
