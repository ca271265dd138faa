"""Float64 torch reference of hkp_heat_loss_lines (the plane loss against line labels, with
weights, masks and top-k), shared by test_line_loss_cpu.py and test_gpu_line_loss.py.  The
target is tests/_lines_ref.py's restatement; the per-element terms and their gradient are
float64 autograd as in tests/_planes_ref.py / tests/_masks_ref.py (imported, not edited); the
rules around them are restated here, so that the three references can be held against each
other.  Nothing here touches a GPU or reads the package.

* present     int [N,K]: a plane's slots with flag > 0, points and pieces alike (its P).
* target      float64 [N,K,H,W]: the fp32 value exp(-d2 / den) of the restated d2, as float64
              (the float64 exp rounded to fp32: the kernel's expf is within one fp32 ulp).
* eligible    not (no present slot under "ignore"), weight > 0 when weights are given, and a
              kept pixel when a mask is given.
* select      per image the T eligible planes with the largest r = w * S (w * S / n_bc with a
              mask); equal r to the lower class, a NaN r above everything.
* line_loss_ref  everything at once.  The heat of a masked pixel or of a plane that is not
              eligible is never indexed.
* seeded inputs of the GPU tests (the CPU tests check their preconditions on the same tensors).
"""
import math

import numpy as np
import torch

import _lines_ref as lref
import _planes_ref as pref

terms = pref.terms


def present(lines):
    lines = torch.as_tensor(np.asarray(lines))
    return (lines[..., 4] > 0).sum(-1)


def target(lines, H, W, sigma):
    """float64 [N,K,H,W] holding fp32 values; +0 for a plane without a present slot."""
    t = lref.target64(lref.d2(np.asarray(lines), H, W), sigma)
    return torch.from_numpy(t.astype(np.float32).astype(np.float64))


def keep_of(mask, n, k, H, W):
    if mask is None:
        return torch.ones(n, k, H, W, dtype=torch.bool)
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (n, H, W)
    m = mask.long()
    return torch.stack([((m >> c) & 1) == 0 for c in range(k)], 1)


def eligible(pres, absent, weights, npix):
    el = torch.ones(pres.shape, dtype=torch.bool)
    if absent == "ignore":
        el &= pres > 0
    else:
        assert absent == "zero"
    if weights is not None:
        el &= weights > 0                              # False for 0, negatives and NaN
    return el & (npix > 0)


def ranks(S, npix, w, masked):
    """r float64 [N,K] as Python floats: w * S, or w * (S / n_bc) with a mask."""
    n, k = S.shape
    out = [[0.0] * k for _ in range(n)]
    for b in range(n):
        for c in range(k):
            v = float(S[b, c]) / float(max(int(npix[b, c]), 1)) if masked else float(S[b, c])
            out[b][c] = (1.0 if w is None else float(w[b, c])) * v
    return out


def select(S, npix, w, el, topk, masked):
    if topk is None:
        return el.clone()
    used = torch.zeros_like(el)
    r = ranks(S, npix, w, masked)
    for b in range(S.shape[0]):
        cls = [c for c in range(S.shape[1]) if el[b, c]]
        cls.sort(key=lambda c: (0, 0.0, c) if math.isnan(r[b][c]) else (1, -r[b][c], c))
        for c in cls[:topk]:
            used[b, c] = True
    return used


def rank_gap(S, npix, w, el, masked):
    """The smallest (r_i - r_j) / r_i over neighbouring ranks of one image (inf without a pair)."""
    gap = float("inf")
    r = ranks(S, npix, w, masked)
    for b in range(S.shape[0]):
        v = sorted((r[b][c] for c in range(S.shape[1]) if el[b, c]), reverse=True)
        for hi, lo in zip(v, v[1:]):
            gap = min(gap, (hi - lo) / hi)
    return gap


def divisor(pres, npix, used, norm):
    """inf for nothing counted under "elements": loss and gradient 0, as the kernel."""
    if norm == "instances":
        return float(max(int((pres * used).sum()), 1))
    assert norm == "elements"
    c = int((npix * used).sum())
    return float(c) if c else float("inf")


def line_loss_ref(p_f32, y_f64, lines, mask=None, kind="bce", absent="zero", norm="elements", beta=2.0, weights=None,
                  topk=None):
    """-> dict: loss (float), dheat (float32, +0 on masked pixels and on the planes that are
    not counted), S, plane_loss (float64 [N,K], -1 where not eligible), plane_pixels (int64
    [N,K], 0 where not eligible), used, eligible, D, keep, and elements (the kept elements of
    the counted planes, for the loss bound).  y_f64 is the target the terms are taken against
    (target(), or the kernel's own)."""
    assert p_f32.dtype == torch.float32 and y_f64.dtype == torch.float64
    n, k, H, W = p_f32.shape
    pres = present(lines)
    keep = keep_of(mask, n, k, H, W)
    npix = keep.sum((2, 3))
    el = eligible(pres, absent, weights, npix)
    p = p_f32.detach().clone().requires_grad_(True)
    sums = {}
    S = torch.zeros(n, k, dtype=torch.float64)
    for b in range(n):
        for c in range(k):
            if el[b, c]:
                kp = keep[b, c]
                sums[b, c] = terms(p[b, c][kp].double(), y_f64[b, c][kp], kind, beta).sum()
                S[b, c] = sums[b, c].detach()
    used = select(S, npix, weights, el, topk, mask is not None)
    D = divisor(pres, npix, used, norm)
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
    plane_loss = torch.where(el, S / npix.clamp(min=1).double(), torch.full_like(S, -1.0))
    return {"loss": loss, "dheat": grad, "S": S, "plane_loss": plane_loss, "plane_pixels": npix * el, "used": used,
            "eligible": el, "D": D, "keep": keep, "elements": int((npix * used).sum())}


# ------------------------------------------------------------------ seeded inputs ----

# (n, k, s, H, W): the smallest case; the scalar path in one tile; all 128 slots, 2 x 5 tiles and
# an odd W; 3 x 4 tiles on the 16-byte path; W % 4 == 2; 72 tiles, more than a plane has blocks
SHAPES = [(1, 1, 1, 1, 1), (2, 3, 4, 17, 23), (1, 2, 128, 33, 131), (1, 2, 8, 70, 100), (1, 3, 5, 35, 66),
          (1, 1, 4, 260, 256)]
VEC_SHAPES = [SHAPES[3], SHAPES[5]]                     # W % 4 == 0
TOPK_SHAPES = [(2, 5, 2, 17, 23), (2, 6, 3, 12, 40), (1, 4, 1, 75, 101)]
TOPK_MIN_GAP = 8e-4          # the planes tests' precondition on neighbouring ranks


def heat(shape, seed=4):
    n, k, s, H, W = shape
    p = torch.rand(n, k, H, W, generator=torch.Generator().manual_seed(seed))
    assert (p > 0).all() and (p < 1).all()
    return p


def weights(shape):
    n, k = shape[:2]
    return torch.rand(n, k, generator=torch.Generator().manual_seed(9)) * 1.5 + 0.25


def seeded_mask(shape, seed=11):
    """uint8 [N,H,W]: about 30 % of the pixels per class bit, one full row, class 0's whole
    plane in image 0 (K > 1), and (N > 1) the last image at 0xFF."""
    n, k, s, H, W = shape
    g = torch.Generator().manual_seed(seed + n * 1000 + k * 100 + H)
    mask = torch.zeros(n, H, W, dtype=torch.int64)
    for c in range(8):
        mask |= (torch.rand(n, H, W, generator=g) < 0.3).long() << c
    mask[:, H // 2, :] = 0xFF
    if k > 1:
        mask[0] |= 1
    if n > 1:
        mask[n - 1] = 0xFF
    if H * W == 1:
        mask[:] = 0xFE                                  # the one pixel stays for class 0
    return mask.to(torch.uint8)


def topk_lines(shape):
    """Line labels float32 [N,K,S,5] of a top-k shape (N, K, M, H, W), S = M + 2: the points of
    the planes tests' labels as zero-length segments, and in every image class 1 a true line
    plane (a diagonal and a horizontal piece) in place of its points."""
    from test_gpu_focal import _labels
    n, k, m, H, W = shape
    pts = _labels(shape, "zero")
    lines = torch.zeros(n, k, m + 2, 5)
    lines[:, :, :m] = torch.cat([pts[..., 0:2], pts[..., 0:2], pts[..., 2:3]], -1)
    lines[:, :, :m, :4] = torch.nan_to_num(lines[:, :, :m, :4], nan=0.0, posinf=0.0, neginf=0.0)
    w, h = float(W - 1), float(H - 1)
    lines[:, 1, :m, 4] = 0.0
    lines[:, 1, m] = torch.tensor([0.1 * w, 0.2 * h, 0.8 * w, 0.9 * h, 1.0])
    lines[:, 1, m + 1] = torch.tensor([0.3 * w, 0.5 * h, 0.9 * w, 0.5 * h, 1.0])
    return lines


def topk_case(shape, absent):
    """(heat, lines, mask) of a top-k case; under "ignore" the last plane is absent.  Class c's
    heat is the seeded heat to the power 1 + c / 4, so that planes with like labels still rank
    apart.  The same tensors on every call."""
    from _masks_ref import topk_mask
    lines = topk_lines(shape)
    if absent == "ignore":
        lines[-1, -1, :, 4] = 0.0
    p = heat(shape) ** (1.0 + 0.25 * torch.arange(shape[1]).view(1, -1, 1, 1))
    assert (p > 0).all() and (p < 1).all()
    return p, lines, topk_mask(shape)
