"""Multi-instance and absent keypoints on the GPU: hkp_gauss_target_multi and
hkp_heat_loss_multi against the existing single-instance kernels (bit for bit) and
the float64 references of tests/_tail_ref.py, the training step, the round trip with
the multi-peak decode and the device data path.

Shapes (N, K, M, H, W): odd widths (the scalar path), widths divisible by 4 (the
16-byte path, also from a base that is not 16-byte aligned), fewer elements than a
block, several blocks per plane and more than one trip of the block's stride in
either path (a plane gets at most 64 blocks of 256 items).  Each figure is printed
before it is asserted (pytest -s shows them)."""
import numpy as np
import pytest
import torch

import _instances_ref as iref
import _tail_ref as tref
from oracle import recipe

pytestmark = pytest.mark.gpu

NAN = float("nan")
SHAPES = [
    (2, 3, 4, 17, 23),       # odd W, total not a multiple of 4; 0, 1, 2, 4 present, 0,1,0,1, NaN in empty slots
    (1, 2, 16, 75, 101),     # M at its limit, 30 blocks per plane
    (1, 1, 1, 5, 7),         # fewer elements than a block
    (1, 3, 2, 300, 293),     # 87,900 pixels a plane: 6 trips of 58 blocks (scalar path)
    (2, 2, 3, 12, 40),       # W % 4 == 0: the 16-byte path, half a block per plane
    (1, 2, 3, 260, 256),     # 16,640 items of 4 pixels a plane: 2 trips of 33 blocks (16-byte path)
]


def _points(shape):
    """pts float32 [N,K,M,3] for a shape: on a pixel, between pixels, outside the image;
    present slots not packed; NaN / inf in empty slots."""
    n, k, m, H, W = shape
    if shape == SHAPES[0]:
        e = [0.0, 0.0, 0.0]
        return torch.tensor([[[e, e, e, e],                                                    # absent
                              [[10.0, 8.0, 1.0], e, e, e],                                      # on a pixel
                              [[5.5, 3.25, 1.0], [18.75, 12.5, 2.0], e, e]],                   # between pixels
                             [[[-5.5, 20.25, 1.0], [30.0, -3.5, 1.0], [0.0, 0.0, 1.0], [22.0, 16.0, 1.0]],   # outside
                              [e, [3.0, 4.0, 1.0], [7.0, 7.0, 0.0], [15.5, 9.5, 1.0]],          # 0,1,0,1
                              [[NAN, NAN, 0.0], [float("inf"), 2.0, 0.0], [11.25, 6.0, 1.0], [NAN, 5.0, -1.0]]]])
    g = torch.Generator().manual_seed(n * 1000 + k * 100 + m + H)
    pts = torch.empty(n, k, m, 3)
    pts[..., 0] = torch.rand(n, k, m, generator=g) * (W + 10) - 5
    pts[..., 1] = torch.rand(n, k, m, generator=g) * (H + 10) - 5
    pts[..., 2] = 1.0
    pts[0, 0, 0, :2] = torch.tensor([float(W // 2), float(H // 3)])                             # on a pixel
    if k > 1:
        pts[:, 1, 1::2, 2] = 0.0                                                               # every other slot empty
        pts[:, 1, 1::2, :2] = NAN
        if m == 1:
            pts[:, 1, :, 2] = 0.0
    if k > 2:
        pts[:, 1, :, 2] = 0.0                                                                  # an absent plane
    return pts


def _dense_from_single(pts, H, W, sigma):
    """The definition through the existing kernel: the elementwise maximum of
    ops.gauss_target's planes of the present slots, zero for absent planes."""
    from hkp import ops
    on = pts[..., 2] > 0
    out = torch.zeros(pts.shape[0], pts.shape[1], H, W, dtype=torch.float64, device=pts.device)
    for j in range(pts.shape[2]):
        uv = torch.where(on[:, :, j, None], pts[:, :, j, :2], torch.zeros_like(pts[:, :, j, :2])).contiguous()
        g = ops.gauss_target(uv, H, W, sigma)
        out = torch.maximum(out, torch.where(on[:, :, j, None, None], g, torch.zeros_like(g)))
    return out


def _heat(shape, seed=4):
    n, k, m, H, W = shape
    p = torch.rand(n, k, H, W, generator=torch.Generator().manual_seed(seed))
    assert (p > 0).all() and (p < 1).all()
    return p


def _loss_bound(total, want):
    # every term of either loss is >= 0, so any summation order stays within (n-1) u of
    # the exact sum; a few more ulp for the logs (tests/test_gpu_tail.py::_loss_bound)
    return (total + 8) * 2.0 ** -53 * abs(want)


def _close(what, got, want, total):
    err, bound = abs(got - want), _loss_bound(total, want)
    print("%s: loss %.17g ref %.17g err %.3e bound %.3e" % (what, got, want, err, bound))
    assert np.isfinite(got) and err <= bound, (what, err, bound)


def _same_bits(what, got, want):
    bad = int((got.cpu().numpy().view(np.int32) != want.cpu().numpy().view(np.int32)).sum())
    print("%s: %d of %d gradient elements differ" % (what, bad, got.numel()))
    assert got.shape == want.shape and bad == 0, (what, bad)


# ------------------------------------------------------------- 1. target ----

@pytest.mark.parametrize("sigma", [8.0, 0.75])
@pytest.mark.parametrize("shape", SHAPES)
def test_target_is_the_maximum_of_the_single_targets(cuda_device, shape, sigma):
    from hkp import ops
    n, k, m, H, W = shape
    pts = _points(shape).to(cuda_device)
    got = ops.gauss_target_multi(pts, H, W, sigma)
    want = _dense_from_single(pts, H, W, sigma)
    assert got.dtype == torch.float64 and got.shape == (n, k, H, W)
    assert torch.equal(got, want)
    absent = ~(pts[..., 2] > 0).any(-1)
    assert (got[absent] == 0).all()
    if sigma < 1 and H * W > 35:
        # expf(-d^2 / 1.125) is an exact 0 from d = 10.8 px on (-d^2 / 1.125 < -103.97): such pixels
        # exist in every shape but the 5 x 7 one, also in planes that hold instances
        zero = got == 0
        print("sigma %g %s: %.3f of the target is exactly 0" % (sigma, shape, zero.double().mean().item()))
        assert zero[~absent].any() and not zero[~absent].all()
    if shape == SHAPES[0]:
        assert absent.sum().item() == 1 and got[0, 1, 8, 10].item() == 1.0 and got.max().item() == 1.0
    # the restatement agrees to the last places of expf
    ref = iref.gauss_target_multi(pts.cpu().numpy(), H, W, sigma)
    assert np.abs(got.cpu().numpy() - ref).max() <= 4 * 2.0 ** -24


@pytest.mark.parametrize("shape", SHAPES)
def test_target_single_instance_is_gauss_target(cuda_device, shape):
    from hkp import ops
    n, k, m, H, W = shape
    pts = _points(shape)[:, :, :1].clone()
    pts[..., 2] = 1.0
    pts[..., :2] = torch.nan_to_num(pts[..., :2], nan=3.5, posinf=1.0)
    pts = pts.contiguous().to(cuda_device)
    for sigma in (8.0, 0.75):
        assert torch.equal(ops.gauss_target_multi(pts, H, W, sigma),
                           ops.gauss_target(pts[:, :, 0, :2].contiguous(), H, W, sigma))


# ------------------------------------------------------- 2. loss, "zero" ----

@pytest.mark.parametrize("sigma", [8.0, 0.75])
@pytest.mark.parametrize("kind", ["bce", "mse"])
@pytest.mark.parametrize("shape", SHAPES)
def test_loss_zero_mode(cuda_device, shape, kind, sigma):
    from hkp import ops
    n, k, m, H, W = shape
    pts = _points(shape).to(cuda_device)
    p = _heat(shape)
    pd = p.to(cuda_device)
    dense = ops.gauss_target_multi(pts, H, W, sigma)
    assert torch.equal(dense, _dense_from_single(pts, H, W, sigma))
    loss, dheat = ops.heat_loss_multi(pd, pts, sigma=sigma, kind=kind)           # absent="zero" is the default
    l_old, g_old = ops.heat_loss(pd, target=dense, kind=kind)
    _close("multi vs heat_loss(dense) %s %s" % (kind, shape), loss.item(), l_old.item(), p.numel())
    _same_bits("multi vs heat_loss(dense)", dheat, g_old)
    want_l, want_g = tref.loss_ref(p, dense.cpu(), kind)
    _close("multi vs loss_ref %s %s" % (kind, shape), loss.item(), want_l.item(), p.numel())
    assert np.array_equal(dheat.cpu().numpy(), want_g.numpy())
    l2, g2 = ops.heat_loss_multi(pd, pts, sigma=sigma, kind=kind, absent="zero", want_grad=False)
    assert g2 is None and l2.item() == loss.item()                                # the same loss bits without dheat
    l3, g3 = ops.heat_loss_multi(pd, pts, sigma=sigma, kind=kind)
    assert l3.item() == loss.item() and torch.equal(g3, dheat)                    # and on a second run


@pytest.mark.parametrize("kind", ["bce", "mse"])
def test_loss_unaligned_base_takes_the_scalar_path(cuda_device, kind):
    """W % 4 == 0 but the heatmaps start 4 bytes off a 16-byte boundary: the same bits
    (per element; the loss within the reassociation bound, its partials being other sums)."""
    from hkp import ops
    shape = SHAPES[4]
    n, k, m, H, W = shape
    pts = _points(shape).to(cuda_device)
    p = _heat(shape).to(cuda_device)
    buf = torch.empty(p.numel() + 1, device=cuda_device)
    off = buf[1:].view(p.shape)
    off.copy_(p)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4 and p.data_ptr() % 16 == 0
    l1, g1 = ops.heat_loss_multi(p, pts, kind=kind)
    l2, g2 = ops.heat_loss_multi(off, pts, kind=kind)
    _close("unaligned %s" % kind, l2.item(), l1.item(), p.numel())
    _same_bits("unaligned", g2, g1)


@pytest.mark.parametrize("kind", ["bce", "mse"])
def test_loss_saturated(cuda_device, kind):
    """_tail_ref.saturated_block()'s heat (exactly 0, exactly 1, below 1e-13, within 2e-7
    of 1) as four 100 x 100 planes; instances sit on pixels of each kind at sigma 0.75,
    so targets of exactly 1 and exactly 0 meet heat of exactly 0 and 1: BCE's -100 log
    clamp and the float 1e-12 denominator clamp both act."""
    from hkp import ops
    p = tref.saturated_block()[0].reshape(1, 4, 100, 100).contiguous()
    pts = torch.zeros(1, 4, 16, 3)
    for kk in (1, 2, 3):                                 # plane 0 stays absent: the all-zero target
        plane = p[0, kk]
        slot = 0
        for sel in (plane == 0, plane == 1, (plane > 0) & (plane < 1e-12), (plane < 1) & (plane > 0.5)):
            ys, xs = torch.nonzero(sel, as_tuple=True)
            for i in range(0, 4 * 97, 97):               # 4 pixels of each kind, spread over the plane
                pts[0, kk, slot] = torch.tensor([float(xs[i % len(xs)]), float(ys[i % len(ys)]), 1.0])
                slot += 1
    pd, ptsd = p.to(cuda_device), pts.to(cuda_device)
    dense = ops.gauss_target_multi(ptsd, 100, 100, 0.75)
    y = dense.cpu()
    for pv in (0.0, 1.0):
        for yv in (0.0, 1.0):
            assert ((p == pv) & (y == yv)).any(), (pv, yv)
    loss, dheat = ops.heat_loss_multi(pd, ptsd, sigma=0.75, kind=kind)
    l_old, g_old = ops.heat_loss(pd, target=dense, kind=kind)
    _close("saturated vs heat_loss(dense) %s" % kind, loss.item(), l_old.item(), p.numel())
    _same_bits("saturated vs heat_loss(dense)", dheat, g_old)
    want_l, want_g = tref.loss_ref(p, y, kind)
    _close("saturated vs loss_ref %s" % kind, loss.item(), want_l.item(), p.numel())
    assert np.array_equal(dheat.cpu().numpy(), want_g.numpy())
    if kind == "bce":
        assert want_l.item() > 1.0                       # terms of 100 are in the mean


# ----------------------------------------------------- 3. loss, "ignore" ----

@pytest.mark.parametrize("sigma", [8.0, 0.75])
@pytest.mark.parametrize("kind", ["bce", "mse"])
@pytest.mark.parametrize("shape", SHAPES)
def test_loss_ignore_mode(cuda_device, shape, kind, sigma):
    from hkp import ops
    n, k, m, H, W = shape
    pts = _points(shape)
    if n * k > 1:
        pts[-1, -1, :, 2] = 0.0                          # one more absent plane (a single plane stays active: A = 1)
    act = (pts[..., 2] > 0).any(-1)
    A = int(act.sum())
    assert A >= 1 and (A < n * k or n * k == 1)
    p = _heat(shape)
    ptsd, pd = pts.to(cuda_device), p.to(cuda_device)
    dense = ops.gauss_target_multi(ptsd, H, W, sigma).cpu()
    loss, dheat = ops.heat_loss_multi(pd, ptsd, sigma=sigma, kind=kind, absent="ignore")
    # the mean over exactly the active planes' elements
    want_l, want_g = tref.loss_ref(p[act].reshape(1, A, H, W).contiguous(), dense[act].reshape(1, A, H, W).contiguous(),
                                   kind)
    _close("ignore %s %s (A = %d of %d)" % (kind, shape, A, n * k), loss.item(), want_l.item(), A * H * W)
    g = dheat.cpu()
    assert np.array_equal(g[act].numpy(), want_g.reshape(A, H, W).numpy())
    off = g[~act].numpy()
    assert (off == 0).all() and not np.signbit(off).any()                         # +0.0, written
    l2, g2 = ops.heat_loss_multi(pd, ptsd, sigma=sigma, kind=kind, absent="ignore", want_grad=False)
    assert g2 is None and l2.item() == loss.item()
    l3, g3 = ops.heat_loss_multi(pd, ptsd, sigma=sigma, kind=kind, absent="ignore")
    assert l3.item() == loss.item() and torch.equal(g3, dheat)


@pytest.mark.parametrize("kind", ["bce", "mse"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4]])
def test_loss_ignore_mode_all_absent(cuda_device, shape, kind):
    from hkp import ops
    n, k, m, H, W = shape
    pts = torch.full((n, k, m, 3), NAN)
    pts[..., 2] = 0.0
    pd = _heat(shape).to(cuda_device)
    loss, dheat = ops.heat_loss_multi(pd, pts.to(cuda_device), kind=kind, absent="ignore")
    g = dheat.cpu().numpy()
    assert loss.item() == 0.0 and (g == 0).all() and not np.signbit(g).any()
    loss, dheat = ops.heat_loss_multi(pd, pts.to(cuda_device), kind=kind, absent="zero")        # negatives: they count
    zeros = torch.zeros(n, k, H, W, dtype=torch.float64)
    want_l, want_g = tref.loss_ref(pd.cpu(), zeros, kind)
    _close("all absent, zero mode %s" % kind, loss.item(), want_l.item(), pd.numel())
    assert np.array_equal(dheat.cpu().numpy(), want_g.numpy())


# --------------------------------------------------------- 4. rejections ----

def test_rejections(cuda_device):
    from hkp import ops
    from hkp._lib import HkpError
    p = torch.rand(2, 3, 5, 7).to(cuda_device)
    ok = torch.zeros(2, 3, 4, 3).to(cuda_device)
    ops.heat_loss_multi(p, ok)
    # M = 17, last axis 2, float64, M = 0, not 4-dimensional
    for bad in (torch.zeros(2, 3, 17, 3), torch.zeros(2, 3, 4, 2), torch.zeros(2, 3, 4, 3, dtype=torch.float64),
                torch.zeros(2, 3, 0, 3), torch.zeros(2, 3, 3)):
        with pytest.raises(HkpError):
            ops.heat_loss_multi(p, bad.to(cuda_device))
        with pytest.raises(HkpError):
            ops.gauss_target_multi(bad.to(cuda_device), 5, 7, 8.0)
    with pytest.raises(HkpError):
        ops.heat_loss_multi(p, torch.zeros(2, 4, 4, 3).to(cuda_device))        # another K than the heatmaps'
    with pytest.raises(HkpError):
        ops.gauss_target_multi(ok, 0, 7, 8.0)
    with pytest.raises(HkpError):
        ops.heat_loss_multi(p, ok, absent="skip")
    with pytest.raises(HkpError):
        ops.heat_loss_multi(p, ok, kind="l1")
    with pytest.raises(HkpError):
        ops.heat_loss_multi(p, ok.cpu())
    # the C ABI keeps its own checks
    import ctypes
    from hkp._lib import call
    loss = torch.zeros((), dtype=torch.float64, device=cuda_device)
    ws = torch.zeros(1 + 6 * 64, dtype=torch.float64, device=cuda_device)
    P = lambda t: ctypes.c_void_p(t.data_ptr())                                # noqa: E731
    for m, kind, mode in ((17, 0, 0), (0, 0, 0), (4, 2, 0), (4, 0, 2)):
        with pytest.raises(HkpError):
            call("hkp_heat_loss_multi", 2, 3, m, 5, 7, kind, mode, P(p), P(ok), 8.0, P(loss), None, P(ws),
                 ops._stream())
    with pytest.raises(HkpError):
        call("hkp_heat_loss_multi", 2, 3, 4, 5, 7, 0, 0, P(p), None, 8.0, P(loss), None, P(ws), ops._stream())
    torch.cuda.synchronize()


# ------------------------------------------------------ 5. training step ----

def _r18(cuda_device, K):
    from src.model import KeypointsGauss
    m = KeypointsGauss(K, backbone="resnet18", pretrained=False)
    m.load_state_dict(recipe.seeded_state_dict("resnet18", 23))
    return m.to(cuda_device)


def test_training_step(cuda_device):
    from hkp import autograd as hkp_autograd
    from hkp import train
    B, K, H, W = 2, 3, 64, 96
    x = recipe.to_tensor_nchw(recipe.seeded_images_u8(B, H, W, 21)).to(cuda_device)
    uv = torch.from_numpy(recipe.seeded_keypoints(B, K, H, W, 22)).to(cuda_device)
    pts = torch.cat([uv, torch.ones(B, K, 1, device=cuda_device)], -1).reshape(B, K, 1, 3).contiguous()
    m_uv, m_pts, m_auto, m_ign = (_r18(cuda_device, K) for _ in range(4))
    l_uv = train.Trainer(m_uv).forward_backward(x, uv=uv)
    l_pts = train.Trainer(m_pts).forward_backward(x, pts=pts)
    _close("Trainer pts vs uv", l_pts.item(), l_uv.item(), B * K * H * W)
    # the same dheat bits go through the same deterministic backward
    differ = [n for (n, a), b in zip(m_uv.named_parameters(), m_pts.parameters()) if not torch.equal(a.grad, b.grad)]
    print("parameter gradients that differ between uv and pts labels:", differ)
    assert not differ
    # the autograd path
    l_auto = hkp_autograd.heatmap_loss(m_auto(x), pts=pts)
    l_auto.backward()
    assert l_auto.item() == l_pts.item()
    differ = [n for (n, a), b in zip(m_auto.named_parameters(), m_pts.parameters()) if not torch.equal(a.grad, b.grad)]
    print("parameter gradients that differ between autograd and Trainer:", differ)
    assert not differ
    # keypoint class k0 absent in every image, ignored: its row of the scoring conv gets no gradient
    k0 = 1
    gone = pts.clone()
    gone[:, k0, :, 2] = 0.0
    gone[:, k0, :, :2] = NAN
    tr = train.Trainer(m_ign, absent="ignore")
    l_ign = tr.forward_backward(x, pts=gone)
    fc = m_ign.resnet.net.fc
    assert np.isfinite(l_ign.item()) and l_ign.item() > 0
    assert fc.weight.grad.shape[0] >= K and fc.bias.grad.shape[0] >= K
    assert (fc.weight.grad[k0] == 0).all() and fc.bias.grad[k0].item() == 0
    for kk in (0, 2):
        assert fc.weight.grad[kk].abs().max().item() > 0 and fc.bias.grad[kk].item() != 0
    assert all(torch.isfinite(q.grad).all() for q in m_ign.parameters())
    with pytest.raises(ValueError):
        train.Trainer(m_ign, absent="skip")


# ---------------------------------------------- 6. round trip with the decode ----

def test_round_trip_with_heat_peaks(cuda_device):
    """Setup: tests/_instances_ref.py (RT_*), where the one departure from the planned
    layout is explained (the 3-instance plane keeps 2 cells from the border, not 3)."""
    import _peaks_ref as pref
    from hkp import ops
    (H, W), pts = iref.RT_IMAGE, torch.from_numpy(iref.roundtrip_pts())
    target = ops.gauss_target_multi(pts.to(cuda_device), H, W, iref.RT_SIGMA).cpu().numpy()
    low = iref.lowres_logits(target)
    assert low.shape == (1, 4) + iref.RT_LATTICE and np.isfinite(low).all()
    # first the restatement alone
    peaks, counts = pref.heat_peaks(low, H, W, max_peaks=4, radius=1, threshold=0.5)
    for k, (c, want, err) in enumerate(iref.roundtrip_errors(peaks, counts)):
        print("restatement, plane %d: %d peaks for %d instances, worst %.3g px" % (k, c, want, err))
        assert c == want and err <= 1e-4
    gp, gc = ops.heat_peaks(torch.from_numpy(low).to(cuda_device), H, W, max_peaks=4, radius=1, threshold=0.5)
    for k, (c, want, err) in enumerate(iref.roundtrip_errors(gp.cpu().numpy(), gc.cpu().numpy())):
        print("kernel, plane %d: %d peaks for %d instances, worst %.3g px" % (k, c, want, err))
        assert c == want and err <= 1e-4


# ------------------------------------------------------------ 7. data path ----

def test_device_batches_carry_instances(cuda_device, tmp_path):
    from test_gpu_augment import _jpeg_folder
    from hkp import geometry as G, ops
    from src.dataset import DeviceBatches, KeypointsDataset, transform
    K, H, W, n = 2, 48, 64, 4
    _jpeg_folder(tmp_path, n, H, W)
    (tmp_path / "instances").mkdir()
    rng = np.random.default_rng(3)
    for i in range(n):
        lab = np.zeros((K, 2, 3))
        lab[:, :, 0], lab[:, :, 1], lab[:, :, 2] = rng.uniform(0, W - 1, (K, 2)), rng.uniform(0, H - 1, (K, 2)), 1.0
        lab[i % K, 1] = (NAN, NAN, 0.0)                      # an empty slot
        if i == 0:
            lab[1, 0] = (W + 5.0, 3.0, 1.0)                  # a present point outside the picture
        np.save(tmp_path / "instances" / ("%05d.npy" % i), lab)
    ds = KeypointsDataset(str(tmp_path / "images"), str(tmp_path / "instances"), K, H, W, transform, instances=2)
    old = KeypointsDataset(str(tmp_path / "images"), str(tmp_path / "labels"), K, H, W, transform)
    stored = np.stack(ds.labels_np)
    assert stored.shape == (n, K, 2, 3)
    make = lambda: G.GeometricAugmentation(seed=6, keep_inside=False, translate=(0.4, 0.4), rotate=(0, 0),   # noqa: E731
                                           scale=(1, 1))
    ga = make()
    plain = list(DeviceBatches(ds, 2))
    got = list(DeviceBatches(ds, 2, geometric=make()))
    today = list(DeviceBatches(old, 2, geometric=make()))
    cleared = 0
    for bi, ((img, pts), (pimg, ppts), (timg, _)) in enumerate(zip(got, plain, today)):
        idx = np.arange(2 * bi, 2 * bi + 2)
        assert np.array_equal(ppts.cpu().numpy(), stored[idx], equal_nan=True)      # carried unchanged
        plan = ga.plan(idx, 0, pts=stored[idx], hw=(H, W))
        want = plan.apply_points(stored[idx])
        assert pts.dtype == torch.float32 and pts.shape == (2, K, 2, 3)
        assert np.array_equal(pts.cpu().numpy(), want, equal_nan=True)
        cleared += int(((stored[idx][..., 2] > 0) & ~(want[..., 2] > 0)).sum())
        assert torch.equal(img, ops.warp_affine_u8(pimg, plan)) and torch.equal(img, timg)   # the images of today's path
    print("flags cleared by the translation:", cleared)
    assert cleared >= 1
    # the items of the dataset itself
    img, lab = KeypointsDataset(str(tmp_path / "images"), str(tmp_path / "instances"), K, H, W, transform,
                                instances=2, return_uv=True)[1]
    assert lab.shape == (K, 2, 3) and lab.dtype == torch.float32 and lab.is_cuda
    img, gauss = ds[1]
    assert gauss.shape == (K, H, W) and gauss.dtype == torch.float64
    assert torch.equal(gauss, ops.gauss_target_multi(lab[None].contiguous(), H, W, 8)[0])
    raw_img, raw_pts = ds.raw(1)
    assert raw_img.dtype == np.uint8 and np.array_equal(raw_pts.cpu().numpy(), stored[1], equal_nan=True)
    assert stored[0, 1, 0].tolist() == [W + 5.0, 3.0, 0.0]      # marked absent at load, not clipped
    # the sampler's call surface and the dataset's own `geometric`, image and instance labels together
    out_img, out_pts = make()(raw_img, pts=stored[1], index=1, epoch=0)
    p1 = ga.plan([1], 0, pts=stored[1:2], hw=(H, W))
    assert out_img.shape == raw_img.shape and out_pts.dtype == np.float32
    assert np.array_equal(out_pts, p1.apply_points(stored[1:2])[0], equal_nan=True)
    dsg = KeypointsDataset(str(tmp_path / "images"), str(tmp_path / "instances"), K, H, W, transform, instances=2,
                           return_uv=True, geometric=make())
    assert np.array_equal(dsg[1][1].cpu().numpy(), out_pts, equal_nan=True)
    # with a resize the labels stay as stored until the resize has mapped them
    from hkp.resample import Resize
    rs = Resize()
    h2, w2 = 24, 32
    dsr = KeypointsDataset(str(tmp_path / "images"), str(tmp_path / "instances"), K, h2, w2, transform, instances=2,
                           resize=rs)
    kept = np.stack(dsr.labels_np)
    assert kept[0, 1, 0].tolist() == [W + 5.0, 3.0, 1.0]
    rplan = rs.plan([(H, W)] * 2, (h2, w2))
    for bi, (img, pts) in enumerate(DeviceBatches(dsr, 2, resize=rs)):
        want = rplan.apply_points(kept[2 * bi:2 * bi + 2])
        assert img.shape == (2, h2, w2, 3) and np.array_equal(pts.cpu().numpy(), want, equal_nan=True)
        if bi == 0:
            assert want[0, 1, 0, 2] == 0.0 and want[0, 1, 0, 0] > w2 - 1 and (want[..., 2] > 0).sum() >= 4
    _, lab0 = dsr.raw(0)
    assert np.array_equal(lab0.cpu().numpy(), rplan.apply_points(kept[:2])[0], equal_nan=True)
