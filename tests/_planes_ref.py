"""Float64 torch reference of hkp_heat_loss_planes (plane weights, per-plane values, hard
keypoint mining), shared by test_planes_cpu.py and test_gpu_planes.py.  Nothing here
touches a GPU.

* terms      the per-element loss of a kind in float64: F.binary_cross_entropy(x, y, "none"),
             the square, or _focal_ref.qfl_terms.
* eligible   bool [N,K]: the planes that can be counted (include/hulkkp.h: not absent under
             "ignore", and weight > 0 when weights are given).
* select     the counted planes from the per-plane sums: per image the T eligible planes with
             the largest w * S, equal values to the lower class, NaN above everything.
* divisor    H*W*C or max(P, 1) from the counted planes.
* planes_ref everything at once; the gradient by autograd through the .double() cast.  The
             heat of a plane that is not eligible is never indexed.
* rank_gap   the smallest relative gap between neighbouring ranks, the top-k tests'
             precondition.
"""
import math

import torch
import torch.nn.functional as F

import _focal_ref as fref


def terms(x, y, kind, beta=2.0):
    assert x.dtype == torch.float64 and y.dtype == torch.float64
    if kind == "bce":
        return F.binary_cross_entropy(x, y, reduction="none")
    if kind == "mse":
        return (x - y) * (x - y)
    assert kind == "qfl"
    return fref.qfl_terms(x, y, beta)


def eligible(pts, absent, weights=None):
    el = torch.ones(pts.shape[:2], dtype=torch.bool)
    if absent == "ignore":
        el &= fref.active_planes(pts)
    else:
        assert absent == "zero"
    if weights is not None:
        el &= weights > 0                              # False for 0, negatives and NaN
    return el


def select(S, w, el, topk):
    """S float64 [N,K], w float32 [N,K] or None, el bool [N,K], topk None or T -> bool [N,K]."""
    if topk is None:
        return el.clone()
    used = torch.zeros_like(el)
    for b in range(S.shape[0]):
        r = [(1.0 if w is None else float(w[b, c])) * float(S[b, c]) for c in range(S.shape[1])]
        cls = [c for c in range(S.shape[1]) if el[b, c]]
        cls.sort(key=lambda c: (0, 0.0, c) if math.isnan(r[c]) else (1, -r[c], c))
        for c in cls[:topk]:
            used[b, c] = True
    return used


def divisor(pts, H, W, used, norm):
    """inf for no counted plane under "elements": loss and gradient 0, as the kernel."""
    if norm == "instances":
        return float(max(int(((pts[..., 2] > 0).sum(-1) * used).sum()), 1))
    assert norm == "elements"
    c = int(used.sum())
    return float(H * W * c) if c else float("inf")


def rank_gap(S, w, el):
    """The smallest (r_i - r_j) / r_i over neighbouring ranks i, j of one image (inf
    without a pair)."""
    gap = float("inf")
    for b in range(S.shape[0]):
        r = sorted(((1.0 if w is None else float(w[b, c])) * float(S[b, c]) for c in range(S.shape[1]) if el[b, c]),
                   reverse=True)
        for hi, lo in zip(r, r[1:]):
            gap = min(gap, (hi - lo) / hi)
    return gap


def planes_ref(p_f32, y_f64, pts, kind="bce", absent="zero", norm="elements", beta=2.0, weights=None, topk=None):
    """-> dict: loss (float), dheat (float32, +0 on the planes that are not counted), S,
    plane_loss (float64 [N,K], -1 where not eligible), used (bool [N,K]), eligible, D, and
    elements (the summed elements, for the loss bound)."""
    assert p_f32.dtype == torch.float32 and y_f64.dtype == torch.float64
    n, k, H, W = p_f32.shape
    el = eligible(pts, absent, weights)
    p = p_f32.detach().clone().requires_grad_(True)
    sums = {}
    S = torch.zeros(n, k, dtype=torch.float64)
    for b in range(n):
        for c in range(k):
            if el[b, c]:
                sums[b, c] = terms(p[b, c].double(), y_f64[b, c], kind, beta).sum()
                S[b, c] = sums[b, c].detach()
    used = select(S, weights, el, topk)
    D = divisor(pts, H, W, used, norm)
    total = None
    for b in range(n):
        for c in range(k):
            if used[b, c]:
                t = sums[b, c] if weights is None else weights[b, c].double() * sums[b, c]
                total = t if total is None else total + t
    if total is None:
        loss, grad = 0.0, torch.zeros_like(p_f32)
    else:
        out = total / D
        out.backward()
        loss, grad = out.item(), p.grad
    plane_loss = torch.where(el, S / float(H * W), torch.full_like(S, -1.0))
    return {"loss": loss, "dheat": grad, "S": S, "plane_loss": plane_loss, "used": used, "eligible": el, "D": D,
            "elements": int(used.sum()) * H * W}
