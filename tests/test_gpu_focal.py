"""The quality focal heatmap loss on the GPU: hkp_heat_loss_multi_ex (HKP_LOSS_QFL, both
divisors) against the float64 reference of tests/_focal_ref.py, the minimum at
heat == target, the BCE / MSE kinds against hkp_heat_loss_multi bit for bit, and the layers
above it (ops, autograd, Trainer, train.fit).

Shapes and labels are those of tests/test_gpu_instances.py (copied, not imported): the
scalar path and the 16-byte path, a misaligned base, fewer elements than a block, several
blocks per plane and more than one trip of the block's stride, M = 16, absent planes and
NaN in empty slots.  Each figure is printed before it is asserted (pytest -s)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _focal_ref as fref
import _tail_ref as tref
from oracle import recipe

pytestmark = pytest.mark.gpu

NAN = float("nan")
BETAS = [2.0, 1.0, 1.5]              # its own instantiation; 0^0 at d == 0; the pow path
ABSENT = ["zero", "ignore"]
NORMS = ["elements", "instances"]
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


def _heat(shape, seed=4):
    n, k, m, H, W = shape
    p = torch.rand(n, k, H, W, generator=torch.Generator().manual_seed(seed))
    assert (p > 0).all() and (p < 1).all()
    return p


def _labels(shape, absent):
    """The shape's labels; under "ignore" one more absent plane, as test_gpu_instances.py
    has it (a single plane stays active)."""
    n, k = shape[:2]
    pts = _points(shape)
    if absent == "ignore" and n * k > 1:
        pts[-1, -1, :, 2] = 0.0
    return pts


@functools.lru_cache(maxsize=None)
def _target(shape, absent, sigma):
    """The dense fp64 target of a shape's labels, from the existing target kernel
    (pinned by test_gpu_instances.py), on the CPU; computed once per case."""
    from hkp import ops
    pts = _labels(shape, absent)
    H, W = shape[3:]
    return ops.gauss_target_multi(pts.cuda(), H, W, sigma).cpu()


@functools.lru_cache(maxsize=None)
def _reference(shape, absent, norm, beta, sigma=8.0):
    """(loss, dheat over all planes with the ignored ones +0, counted elements, divisor)."""
    n, k, m, H, W = shape
    pts, p, y = _labels(shape, absent), _heat(shape), _target(shape, absent, sigma)
    return _ref_of(p, y, pts, absent, norm, beta)


def _ref_of(p, y, pts, absent, norm, beta):
    H, W = p.shape[2:]
    div = fref.divisor(pts, H, W, absent, norm)
    act = fref.active_planes(pts) if absent == "ignore" else torch.ones(pts.shape[:2], dtype=torch.bool)
    A = int(act.sum())
    grad = torch.zeros_like(p)
    if A == 0:
        return 0.0, grad, 0, div
    loss, g = fref.qfl_ref(p[act].reshape(1, A, H, W).contiguous(), y[act].reshape(1, A, H, W).contiguous(), beta, div)
    grad[act] = g.reshape(A, H, W)
    return loss.item(), grad, A * H * W, div


def _loss_bound(total, want):
    # every term is >= 0, so any summation order stays within (n - 1) u of the exact sum
    # (the project's reassociation bound); a few more ulp for the logs and pow
    return (total + 16) * 2.0 ** -53 * abs(want)


def _close(what, got, want, total):
    err, bound = abs(got - want), _loss_bound(total, want)
    print("%s: loss %.17g ref %.17g err %.3e bound %.3e" % (what, got, want, err, bound))
    assert np.isfinite(got) and err <= bound, (what, err, bound)


def _within_one_ulp(what, got, want):
    """Every element of the fp32 gradient within one fp32 ulp of the reference's."""
    g, w = got.cpu().numpy(), want.cpu().numpy()
    assert g.shape == w.shape and g.dtype == np.float32 and w.dtype == np.float32
    differ = int((g.view(np.int32) != w.view(np.int32)).sum())
    ulp = np.spacing(np.abs(w)).astype(np.float64)
    off = np.abs(g.astype(np.float64) - w.astype(np.float64)) / ulp
    print("%s: %d of %d gradient elements differ, worst %.2f ulp" % (what, differ, g.size, off.max()))
    assert np.isfinite(g).all() and off.max() <= 1.0, (what, differ, off.max())


def _plus_zero(t):
    return bool((t.cpu().numpy().view(np.int32) == 0).all())


# ------------------------------------------------- 1, 2, 6. dheat, loss, second run ----

@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("absent", ABSENT)
@pytest.mark.parametrize("shape", SHAPES)
def test_qfl_against_the_reference(cuda_device, shape, absent, norm):
    from hkp import ops
    pts = _labels(shape, absent)
    act = fref.active_planes(pts)
    pd, ptsd = _heat(shape).to(cuda_device), pts.to(cuda_device)
    for beta in BETAS:
        want_l, want_g, total, div = _reference(shape, absent, norm, beta)
        what = "qfl beta %g %s %s %s" % (beta, absent, norm, shape)
        loss, dheat = ops.heat_loss_multi(pd, ptsd, kind="qfl", absent=absent, beta=beta, norm=norm)
        assert loss.dtype == torch.float64 and dheat.dtype == torch.float32 and dheat.shape == pd.shape
        _within_one_ulp(what, dheat, want_g)
        _close(what, loss.item(), want_l, total)
        if absent == "ignore":
            assert _plus_zero(dheat.cpu()[~act])                                  # +0.0, written
            assert (~act).any() or shape[0] * shape[1] == 1
        l2, g2 = ops.heat_loss_multi(pd, ptsd, kind="qfl", absent=absent, want_grad=False, beta=beta, norm=norm)
        assert g2 is None and l2.item() == loss.item()                            # the same loss bits without dheat
        l3, g3 = ops.heat_loss_multi(pd, ptsd, kind="qfl", absent=absent, beta=beta, norm=norm)
        assert l3.item() == loss.item() and torch.equal(g3, dheat)                # and on a second run
        assert np.array_equal(g3.cpu().numpy().view(np.int32), dheat.cpu().numpy().view(np.int32))


@pytest.mark.parametrize("beta", BETAS)
def test_qfl_unaligned_base_takes_the_scalar_path(cuda_device, beta):
    """W % 4 == 0 but the heatmaps start 4 bytes off a 16-byte boundary: per element the
    same bits (the loss within the reassociation bound, its partials being other sums)."""
    from hkp import ops
    shape = SHAPES[4]
    pts = _points(shape).to(cuda_device)
    p = _heat(shape).to(cuda_device)
    buf = torch.empty(p.numel() + 1, device=cuda_device)
    off = buf[1:].view(p.shape)
    off.copy_(p)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4 and p.data_ptr() % 16 == 0
    l1, g1 = ops.heat_loss_multi(p, pts, kind="qfl", beta=beta)
    l2, g2 = ops.heat_loss_multi(off, pts, kind="qfl", beta=beta)
    _close("unaligned beta %g" % beta, l2.item(), l1.item(), p.numel())
    assert np.array_equal(g1.cpu().numpy().view(np.int32), g2.cpu().numpy().view(np.int32))
    want_l, want_g, total, _ = _reference(shape, "zero", "elements", beta)
    _within_one_ulp("unaligned beta %g" % beta, g2, want_g)
    _close("unaligned beta %g vs reference" % beta, l2.item(), want_l, total)


# ------------------------------------------------------------------ 3. saturation ----

def _saturated():
    """test_gpu_instances.py's saturated case: _tail_ref.saturated_block()'s heat (exactly
    0, exactly 1, below 1e-13, within 2e-7 of 1) as four 100 x 100 planes; instances sit on
    pixels of each kind at sigma 0.75, so targets of exactly 1, exactly 0 and in between
    meet heat of exactly 0 and 1.  Plane 0 stays absent."""
    p = tref.saturated_block()[0].reshape(1, 4, 100, 100).contiguous()
    pts = torch.zeros(1, 4, 16, 3)
    for kk in (1, 2, 3):
        plane = p[0, kk]
        slot = 0
        for sel in (plane == 0, plane == 1, (plane > 0) & (plane < 1e-12), (plane < 1) & (plane > 0.5)):
            ys, xs = torch.nonzero(sel, as_tuple=True)
            for i in range(0, 4 * 97, 97):
                pts[0, kk, slot] = torch.tensor([float(xs[i % len(xs)]), float(ys[i % len(ys)]), 1.0])
                slot += 1
    return p, pts


def test_qfl_saturated(cuda_device):
    from hkp import ops
    p, pts = _saturated()
    pd, ptsd = p.to(cuda_device), pts.to(cuda_device)
    y = ops.gauss_target_multi(ptsd, 100, 100, 0.75).cpu()
    for pv in (0.0, 1.0):
        for yv in (0.0, 1.0):
            assert ((p == pv) & (y == yv)).any(), (pv, yv)
        assert ((p == pv) & (y > 0) & (y < 1)).any(), pv
    for beta in BETAS:
        for absent in ABSENT:
            for norm in NORMS:
                want_l, want_g, total, _ = _ref_of(p, y, pts, absent, norm, beta)
                what = "saturated beta %g %s %s" % (beta, absent, norm)
                loss, dheat = ops.heat_loss_multi(pd, ptsd, sigma=0.75, kind="qfl", absent=absent, beta=beta,
                                                  norm=norm)
                assert np.isfinite(loss.item()) and torch.isfinite(dheat).all() and torch.isfinite(want_g).all()
                _within_one_ulp(what, dheat, want_g)
                _close(what, loss.item(), want_l, total)
                assert want_l > 0
                if absent == "ignore":
                    assert _plus_zero(dheat[0, 0])


# --------------------------------------------------------------------- 4. minimum ----

@pytest.mark.parametrize("sigma", [8.0, 0.75])
@pytest.mark.parametrize("shape", SHAPES)
def test_qfl_minimum_is_the_target(cuda_device, shape, sigma):
    """heat == target in every pixel: loss 0.0 and an all-zero-bits gradient, for every
    beta, absent mode and divisor (at sigma 0.75 most of the target is an exact 0, and the
    on-pixel instance an exact 1: the clamped logs)."""
    from hkp import ops
    n, k, m, H, W = shape
    pts = _points(shape).to(cuda_device)
    heat = ops.gauss_target_multi(pts, H, W, sigma).float().contiguous()
    assert heat.max().item() == 1.0 and (sigma > 1 or H * W <= 35 or (heat == 0).any())
    for beta in BETAS:
        for absent in ABSENT:
            for norm in NORMS:
                loss, dheat = ops.heat_loss_multi(heat, pts, sigma=sigma, kind="qfl", absent=absent, beta=beta,
                                                  norm=norm)
                bits = int((dheat.cpu().numpy().view(np.int32) != 0).sum())
                print("minimum sigma %g beta %g %s %s %s: loss %r, %d nonzero gradient words"
                      % (sigma, beta, absent, norm, shape, loss.item(), bits))
                assert loss.item() == 0.0 and not np.signbit(loss.item()) and bits == 0


# ------------------------------------------------------------------ 5. normaliser ----

@pytest.mark.parametrize("absent", ABSENT)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[5]])
def test_instances_norm_rescales_the_elements_norm(cuda_device, shape, absent):
    from hkp import ops
    n, k, m, H, W = shape
    pts = _labels(shape, absent)
    d_el, d_in = fref.divisor(pts, H, W, absent, "elements"), fref.divisor(pts, H, W, absent, "instances")
    assert d_in == float((pts[..., 2] > 0).sum()) and d_in >= 2
    pd, ptsd = _heat(shape).to(cuda_device), pts.to(cuda_device)
    for kind, beta in (("qfl", 2.0), ("qfl", 1.5), ("bce", 2.0), ("mse", 2.0)):
        l_el, g_el = ops.heat_loss_multi(pd, ptsd, kind=kind, absent=absent, beta=beta)
        l_in, g_in = ops.heat_loss_multi(pd, ptsd, kind=kind, absent=absent, beta=beta, norm="instances")
        _close("instances vs elements %s %g %s %s" % (kind, beta, absent, shape), l_in.item(),
               l_el.item() * (d_el / d_in), int(d_el))
        assert torch.isfinite(g_in).all() and g_in.shape == g_el.shape


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4]])
def test_instances_norm_without_an_instance(cuda_device, shape):
    from hkp import ops
    n, k, m, H, W = shape
    pts = torch.full((n, k, m, 3), NAN)
    pts[..., 2] = 0.0
    p = _heat(shape)
    pd, ptsd = p.to(cuda_device), pts.to(cuda_device)
    zeros = torch.zeros(n, k, H, W, dtype=torch.float64)
    for beta in BETAS:
        loss, dheat = ops.heat_loss_multi(pd, ptsd, kind="qfl", absent="zero", beta=beta, norm="instances")
        want_l, want_g = fref.qfl_ref(p, zeros, beta, 1.0)                         # divisor max(0, 1)
        assert np.isfinite(loss.item()) and torch.isfinite(dheat).all() and loss.item() > 0
        _close("no instance, zero mode, beta %g" % beta, loss.item(), want_l.item(), p.numel())
        _within_one_ulp("no instance, zero mode", dheat, want_g)
        for norm in NORMS:
            loss, dheat = ops.heat_loss_multi(pd, ptsd, kind="qfl", absent="ignore", beta=beta, norm=norm)
            assert loss.item() == 0.0 and _plus_zero(dheat)


# ------------------------------------------------- 7. the existing kernels unchanged ----

@pytest.mark.parametrize("absent", ABSENT)
@pytest.mark.parametrize("kind", ["bce", "mse"])
@pytest.mark.parametrize("shape", SHAPES)
def test_ex_with_elements_norm_gives_the_bits_of_heat_loss_multi(cuda_device, shape, kind, absent, monkeypatch):
    from hkp import _lib, ops
    n, k, m, H, W = shape
    pd, ptsd = _heat(shape).to(cuda_device), _labels(shape, absent).to(cuda_device)
    names = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    loss, dheat = ops.heat_loss_multi(pd, ptsd, kind=kind, absent=absent)
    assert names == ["hkp_heat_loss_multi"], names                                # the default call's only launch
    l_kw, g_kw = ops.heat_loss_multi(pd, ptsd, 8.0, kind, absent, True, beta=2.0, norm="elements")
    assert names == ["hkp_heat_loss_multi"] * 2 and torch.equal(l_kw, loss) and torch.equal(g_kw, dheat)
    ops.heat_loss_multi(pd, ptsd, kind="qfl", absent=absent)
    ops.heat_loss_multi(pd, ptsd, kind=kind, absent=absent, norm="instances")
    assert names[2:] == ["hkp_heat_loss_multi_ex"] * 2, names
    monkeypatch.setattr(ops, "call", real)
    P = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    ws = torch.empty(_lib.lib().hkp_heat_loss_multi_workspace(n, k, H, W) // 8, device=cuda_device,
                     dtype=torch.float64)
    l_ex = torch.full((), NAN, device=cuda_device, dtype=torch.float64)
    g_ex = torch.full_like(pd, NAN)
    # beta is not read for these kinds
    _lib.call("hkp_heat_loss_multi_ex", n, k, m, H, W, _lib.HKP_LOSS_BCE if kind == "bce" else _lib.HKP_LOSS_MSE,
              _lib.HKP_ABSENT_ZERO if absent == "zero" else _lib.HKP_ABSENT_IGNORE, _lib.HKP_NORM_ELEMENTS, NAN,
              P(pd), P(ptsd), 8.0, P(l_ex), P(g_ex), P(ws), ops._stream())
    assert torch.equal(l_ex, loss) and torch.equal(g_ex, dheat)
    assert np.array_equal(g_ex.cpu().numpy().view(np.int32), dheat.cpu().numpy().view(np.int32))


def test_ex_rejects_without_writing(cuda_device):
    from hkp import _lib, ops
    shape = SHAPES[2]
    n, k, m, H, W = shape
    pd, ptsd = _heat(shape).to(cuda_device), _points(shape).to(cuda_device)
    P = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    ws = torch.full((1 + n * k * 64,), 7.0, device=cuda_device, dtype=torch.float64)
    loss = torch.full((), 7.0, device=cuda_device, dtype=torch.float64)
    g = torch.full_like(pd, 7.0)
    for kind, norm, beta in ((2, 0, 0.5), (2, 0, 8.5), (2, 0, NAN), (2, 1, float("inf")), (3, 0, 2.0), (2, 2, 2.0)):
        with pytest.raises(_lib.HkpError):
            _lib.call("hkp_heat_loss_multi_ex", n, k, m, H, W, kind, 0, norm, beta, P(pd), P(ptsd), 8.0, P(loss), P(g),
                      P(ws), ops._stream())
    torch.cuda.synchronize()
    assert loss.item() == 7.0 and (g == 7.0).all() and (ws == 7.0).all()


# ------------------------------------------------------------------- 8. uv labels ----

@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4]])
def test_uv_labels_are_one_present_instance(cuda_device, shape):
    from hkp import autograd as hkp_autograd
    from hkp import ops
    n, k, m, H, W = shape
    uv = torch.from_numpy(recipe.seeded_keypoints(n, k, H, W, 9)).to(cuda_device)
    pts = torch.cat([uv, torch.ones(n, k, 1, device=cuda_device)], -1).reshape(n, k, 1, 3).contiguous()
    pd = _heat(shape).to(cuda_device)
    for beta, norm in ((2.0, "elements"), (1.5, "instances")):
        l_uv, g_uv = ops.heat_loss(pd, uv=uv, kind="qfl", beta=beta, norm=norm)
        l_pts, g_pts = ops.heat_loss_multi(pd, pts, kind="qfl", beta=beta, norm=norm)
        assert torch.equal(l_uv, l_pts) and torch.equal(g_uv, g_pts) and l_uv.item() > 0
        hp = pd.clone().requires_grad_(True)
        l_auto = hkp_autograd.heatmap_loss(hp, uv=uv, kind="qfl", beta=beta, norm=norm)
        l_auto.backward()
        assert torch.equal(l_auto.detach(), l_pts) and torch.equal(hp.grad, g_pts)
    with pytest.raises(ops.HkpError, match="dense target is not supported"):
        ops.heat_loss(pd, target=pd.double(), kind="qfl")


# ---------------------------------------------------------------------- 9. layers ----

def _r18(cuda_device, K):
    from src.model import KeypointsGauss
    m = KeypointsGauss(K, backbone="resnet18", pretrained=False)
    m.load_state_dict(recipe.seeded_state_dict("resnet18", 23))
    return m.to(cuda_device)


def _differ(a, b):
    return [n for (n, p), q in zip(a.named_parameters(), b.parameters()) if not torch.equal(p.grad, q.grad)]


def test_training_step(cuda_device):
    from hkp import autograd as hkp_autograd
    from hkp import net, ops, train
    B, K, H, W = 2, 3, 64, 96
    params = {"beta": 1.5, "norm": "instances"}
    x = recipe.to_tensor_nchw(recipe.seeded_images_u8(B, H, W, 21)).to(cuda_device)
    uv = torch.from_numpy(recipe.seeded_keypoints(B, K, H, W, 22)).to(cuda_device)
    pts = torch.cat([uv, torch.ones(B, K, 1, device=cuda_device)], -1).reshape(B, K, 1, 3).contiguous()
    pts = torch.cat([pts, torch.full_like(pts, NAN)], 2).contiguous()            # M = 2, the second slot empty
    pts[:, :, 1, 2] = 0.0
    pts[0, 1, 1] = torch.tensor([20.5, 30.25, 1.0])                               # but for one second instance
    m_tr, m_man, m_auto, m_uv, m_def = (_r18(cuda_device, K) for _ in range(5))
    # the manual chain
    trace = net.Trace(m_man.policy)
    hm, _, _ = net.keypoints_forward(m_man.resnet.net, x, K, heat=True, trace=trace)
    l_man, dheat = ops.heat_loss_multi(hm, pts, 8.0, "qfl", "zero", True, **params)
    grads = net.Grads()
    net.keypoints_backward(m_man.resnet.net, trace, dheat, grads)
    for p in m_man.parameters():
        p.grad = grads[p]
    l_tr = train.Trainer(m_tr, loss="qfl", loss_params=params).forward_backward(x, pts=pts)
    print("Trainer qfl loss %.17g, manual %.17g" % (l_tr.item(), l_man.item()))
    assert l_tr.item() == l_man.item() and np.isfinite(l_tr.item()) and l_tr.item() > 0
    differ = _differ(m_tr, m_man)
    print("parameter gradients that differ between Trainer and the manual chain:", differ)
    assert not differ
    assert all(torch.isfinite(q.grad).all() for q in m_tr.parameters())
    assert m_tr.resnet.net.fc.weight.grad.abs().max().item() > 0
    # the autograd path
    l_auto = hkp_autograd.heatmap_loss(m_auto(x), pts=pts, kind="qfl", **params)
    l_auto.backward()
    assert l_auto.item() == l_tr.item()
    differ = _differ(m_auto, m_tr)
    print("parameter gradients that differ between autograd and Trainer:", differ)
    assert not differ
    # uv labels through the Trainer: the M = 1 form
    one = pts[:, :, :1].contiguous()
    l_uv = train.Trainer(m_uv, loss="qfl").forward_backward(x, uv=uv)
    l_one = train.Trainer(m_def, loss="qfl", loss_params={"beta": 2.0}).forward_backward(x, pts=one)
    assert l_uv.item() == l_one.item() and not _differ(m_uv, m_def)
    with pytest.raises(ValueError):
        train.Trainer(m_def, loss="qfl", loss_params={"gamma": 2.0})
    with pytest.raises(ops.HkpError, match="dense target"):
        train.Trainer(m_def, loss="qfl").forward_backward(x, target=torch.zeros(B, K, H, W, dtype=torch.float64,
                                                                                   device=cuda_device))


def _write_split(root, split, n, seed, K, H, W):
    """Lossless image files under the reference's names and (u, v) label files."""
    from PIL import Image
    img_dir, kp_dir = root / split / "images", root / split / "keypoints"
    img_dir.mkdir(parents=True)
    kp_dir.mkdir(parents=True)
    bgr = recipe.seeded_images_u8(n, H, W, seed)
    uv = recipe.seeded_keypoints(n, K, H, W, seed + 1)
    for i in range(n):
        Image.fromarray(np.ascontiguousarray(bgr[i][:, :, ::-1])).save(img_dir / ("%05d.jpg" % i), format="PNG")
        np.save(kp_dir / ("%05d.npy" % i), uv[i].reshape(K, 2).astype(np.float64))


@pytest.mark.parametrize("instances", [None, 2])
def test_fit_with_config_loss_qfl(cuda_device, tmp_path, monkeypatch, capsys, instances):
    import train as train_mod
    from torch.utils.data import DataLoader
    from src.dataset import KeypointsDataset, transform
    K, H, W = 3, 64, 96
    assert train_mod.LOSS == "bce" and train_mod.LOSS_PARAMS == {}
    _write_split(tmp_path, "train", 2, 71, K, H, W)
    _write_split(tmp_path, "test", 4, 81, K, H, W)
    sets = [KeypointsDataset(str(tmp_path / s / "images"), str(tmp_path / s / "keypoints"), K, H, W, transform,
                             return_uv=True, instances=instances) for s in ("train", "test")]
    train_data, test_data = (DataLoader(s, batch_size=2, shuffle=False) for s in sets)
    model = _r18(cuda_device, K)
    monkeypatch.setattr(train_mod, "LOSS", "qfl")
    monkeypatch.setattr(train_mod, "LOSS_PARAMS", {"beta": 2.0, "norm": "instances"})
    monkeypatch.setattr(train_mod, "_bucketer", None)
    monkeypatch.setattr(train_mod, "optimizer", torch.optim.Adam(model.parameters(), lr=1.0e-4, weight_decay=1.0e-4))
    calls = []
    from hkp import ops
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    capsys.readouterr()
    train_mod.fit(train_data, test_data, model, epochs=1, checkpoint_path=str(tmp_path))
    out = capsys.readouterr().out
    monkeypatch.setattr(ops, "call", real)
    lines = [ln.split("\r")[-1] for ln in out.strip().split("\n")]
    print(lines)
    assert [ln.split(":")[0] for ln in lines] == ["train loss", "test loss"], lines     # the reference's lines only
    for ln in lines:
        v = float(ln.split(":")[1])
        assert np.isfinite(v) and v > 0, ln
    assert calls.count("hkp_heat_loss_multi_ex") == 3 and "hkp_heat_loss" not in calls \
        and "hkp_heat_loss_multi" not in calls
    assert (tmp_path / "model_2_1_0.pth").exists()
