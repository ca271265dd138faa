"""The references of tests/_tail_ref.py checked against torch on the CPU, so the
GPU tests that lean on them (test_gpu_tail.py) compare the kernels with
something that is itself pinned."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _tail_ref as ref
from _tail_ref import rand


@pytest.mark.parametrize("shape", ref.UPSAMPLE_SHAPES)
def test_upsample_emulated_matches_aten(shape):
    """in == 1, out == 1 and in == out included: the emulation stays within 1e-6
    of this host's ATen build (whose fma contraction depends on the ISA)."""
    n, k, h, w, H, W = shape
    low = rand(n, k, h, w, seed=16)
    up = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=True)
    emu = ref.upsample_emulated(low, H, W)
    assert emu.shape == up.shape and emu.dtype == torch.float32
    assert torch.isfinite(emu).all()
    assert (emu - up).abs().max().item() <= 1e-6


@pytest.mark.parametrize("shape", [ref.UPSAMPLE_SHAPES[0], ref.UPSAMPLE_SHAPES[4]])
@pytest.mark.parametrize("sig", [True, False])
def test_head_bwd_ref_matches_fp32_autograd(shape, sig):
    n, k, h, w, H, W = shape
    low = rand(n, k, h, w, seed=14).requires_grad_(True)
    up = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=True)
    heat = torch.sigmoid(up) if sig else up
    g = rand(n, k, H, W, seed=15)
    heat.backward(g)
    got = ref.head_bwd_ref(g, heat.detach() if sig else None, h, w)
    assert got.dtype == torch.float64 and got.shape == low.shape
    assert (got - low.grad.double()).abs().max().item() <= 2e-5 * max(1.0, got.abs().max().item())


@pytest.mark.parametrize("shape", [(2, 9, 15, 512, 4), (1, 6, 7, 96, 9)])
def test_head_fc_bwd_ref_matches_fp32_autograd(shape):
    n, h, w, c, k = shape
    feat = rand(n, c, h, w, seed=16).requires_grad_(True)
    wt = (rand(k, c, 1, 1, seed=17) * 0.05).requires_grad_(True)
    b = rand(k, seed=18).requires_grad_(True)
    low = F.conv2d(feat, wt, b)
    g = rand(*low.shape, seed=19)
    low.backward(g)
    dfeat, dw, db = ref.head_fc_bwd_ref(g, feat.detach().permute(0, 2, 3, 1), wt.detach().reshape(k, c))
    for got, want in ((dfeat.permute(0, 3, 1, 2), feat.grad), (dw, wt.grad.reshape(k, c)), (db, b.grad)):
        assert got.dtype == torch.float64
        assert (got - want.double()).abs().max().item() <= 2e-5 * max(1.0, got.abs().max().item())


def test_bce_gradient_clamp_is_the_float_constant():
    """Where hkp_heat_loss's denominator clamp comes from: ATen's
    binary_cross_entropy_backward clamps (1-x)*x at `constexpr float EPSILON =
    1e-12`, i.e. 9.99999996e-13 as a double.  On the saturated block torch's own
    fp32-cast gradient equals the formula with that constant on every element —
    and not with the double 1e-12 — so the reference alone meets the bit
    equality test_gpu_tail.py asks of the kernel."""
    p, y = ref.saturated_block()
    loss, grad = ref.loss_ref(p, y, "bce")
    assert torch.isfinite(loss) and torch.isfinite(grad).all()
    x, t = p.double().numpy(), y.numpy()
    n = x.size

    def formula(eps):
        return ((x - t) / np.maximum((1.0 - x) * x, eps) / n).astype(np.float32)

    eps_f = np.float64(np.float32(1e-12))
    assert eps_f != 1e-12 and abs(eps_f - 9.99999996e-13) < 1e-21
    assert np.array_equal(grad.numpy(), formula(eps_f))
    assert (grad.numpy() != formula(np.float64(1e-12))).sum() > 0
    # the clamp acts on three quarters of the block (p of 0, 1 and below 1e-13)
    assert ((1.0 - x) * x < eps_f).mean() > 0.7
