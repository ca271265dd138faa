"""Float64 torch reference of the quality focal heatmap loss (hkp_heat_loss_multi_ex,
HKP_LOSS_QFL), shared by test_focal_cpu.py and test_gpu_focal.py.  Nothing here touches
a GPU.

* qfl_terms   the per-element loss F.binary_cross_entropy(x, y, "none") * |x - y|^beta
              in float64 (ATen's clamps: the logs at -100, and in its backward the
              denominator (1 - x) x at the float 1e-12).
* qfl_formula the loss and the gradient of one element as include/hulkkp.h writes them,
              in numpy float64 (what the kernel evaluates).
* qfl_ref     sum(qfl_terms) / divisor on p.double(), the gradient by autograd, cast to
              fp32 by the .double() cast's own backward (the pattern of
              _tail_ref.loss_ref).
* divisor     the divisor of each (absent, norm) pair from the labels.
"""
import numpy as np
import torch
import torch.nn.functional as F


def qfl_terms(x, y, beta):
    """x, y float64 tensors of one shape -> the per-element loss, float64."""
    assert x.dtype == torch.float64 and y.dtype == torch.float64
    return F.binary_cross_entropy(x, y, reduction="none") * (x - y).abs().pow(beta)


def qfl_formula(x, y, beta):
    """(l, g) per element, numpy float64, divisor 1: the header's formulas as written."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        bce = (y - 1.0) * np.maximum(np.log1p(-x), -100.0) - y * np.maximum(np.log(x), -100.0)
        d = x - y
        ad = np.abs(d)
        den = np.maximum((1.0 - x) * x, np.float64(np.float32(1e-12)))
        pm1 = np.power(ad, beta - 1.0)
        l = pm1 * ad * bce
        g = beta * pm1 * np.sign(d) * bce + pm1 * ad * d / den
    zero = d == 0
    return np.where(zero, 0.0, l), np.where(zero, 0.0, g)


def qfl_ref(p_f32, target_f64, beta, divisor):
    """(loss float64 0-dim, dL/dp float32) of sum(qfl_terms(p.double(), target)) / divisor."""
    assert p_f32.dtype == torch.float32 and target_f64.dtype == torch.float64
    p = p_f32.detach().clone().requires_grad_(True)
    loss = qfl_terms(p.double(), target_f64, beta).sum() / divisor
    loss.backward()
    return loss.detach(), p.grad


def active_planes(pts):
    """bool [N,K]: the planes with a present slot (flag > 0)."""
    return (pts[..., 2] > 0).any(-1)


def divisor(pts, H, W, absent, norm):
    """What the sum over the counted planes' elements is divided by.  pts [N,K,M,3] on
    the CPU.  "elements": N*K*H*W, or H*W*A under "ignore" (A = active planes; A = 0:
    inf, which makes loss and gradient 0 as the kernel does); "instances": max(P, 1),
    P = the present slots of the whole batch."""
    n, k = pts.shape[:2]
    if norm == "instances":
        return float(max(int((pts[..., 2] > 0).sum()), 1))
    assert norm == "elements"
    if absent == "ignore":
        a = int(active_planes(pts).sum())
        return float(H * W * a) if a else float("inf")
    assert absent == "zero"
    return float(n * k * H * W)
