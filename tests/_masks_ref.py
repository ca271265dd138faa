"""Float64 torch reference of hkp_heat_loss_masked (per-pixel ignore masks in the heatmap
loss) and plain restatements of what goes with it, shared by test_masks_cpu.py and
test_gpu_masks.py.  Built on _planes_ref.py (imported, not edited).  Nothing here touches a
GPU or reads the package.

* keep        bool [N,K,H,W] from the mask bytes: !((mask[b][y][x] >> c) & 1).
* eligible    _planes_ref.eligible and n_bc > 0.
* select      the counted planes: per image the T eligible planes with the largest w * S / n.
* masked_ref  everything at once; S over the kept pixels, D = the kept pixels of the counted
              planes (or max(P, 1)), the gradient by autograd through the .double() cast.  The
              heat of a masked pixel or of a plane that is not eligible is never indexed.
* rank_gap    _planes_ref.rank_gap on the means S / n: the top-k tests' precondition.
* seeded_mask / topk_case   the seeded inputs the GPU tests use (the CPU tests check their
              preconditions on the very same tensors).
* regions_ref a numpy float32 restatement of hkp_mask_regions_u8.
* flip_lut    the 256-entry table that exchanges the class bits of the flip pairs.
* peaks_drop_masked  masks.peaks_drop_masked as plain loops.
"""
import math

import numpy as np
import torch

import _planes_ref as pref

terms = pref.terms


def keep_of(mask, k):
    """mask uint8 [N,H,W] -> bool [N,K,H,W]."""
    assert mask.dtype == torch.uint8 and mask.dim() == 3
    m = mask.long()
    return torch.stack([((m >> c) & 1) == 0 for c in range(k)], 1)


def eligible(pts, absent, weights, npix):
    return pref.eligible(pts, absent, weights) & (npix > 0)


def select(S, npix, w, el, topk):
    mean = torch.where(el, S / npix.clamp(min=1).double(), torch.zeros_like(S))
    return pref.select(mean, w, el, topk)


def rank_gap(S, npix, w, el):
    mean = torch.where(el, S / npix.clamp(min=1).double(), torch.zeros_like(S))
    return pref.rank_gap(mean, w, el)


def divisor(pts, npix, used, norm):
    """inf for no kept pixel in a counted plane under "elements": loss and gradient 0."""
    if norm == "instances":
        return float(max(int(((pts[..., 2] > 0).sum(-1) * used).sum()), 1))
    assert norm == "elements"
    c = int((npix * used).sum())
    return float(c) if c else float("inf")


def masked_ref(p_f32, y_f64, pts, mask, kind="bce", absent="zero", norm="elements", beta=2.0, weights=None,
               topk=None):
    """-> dict: loss (float), dheat (float32, +0 on masked pixels and on the planes that are
    not counted), S, plane_loss (float64 [N,K], -1 where not eligible), plane_pixels (int64
    [N,K], 0 where not eligible), used, eligible, D, keep, and elements (the kept elements of
    the counted planes, for the loss bound)."""
    assert p_f32.dtype == torch.float32 and y_f64.dtype == torch.float64
    n, k, H, W = p_f32.shape
    keep = keep_of(mask, k)
    npix = keep.sum((2, 3))
    el = eligible(pts, absent, weights, npix)
    p = p_f32.detach().clone().requires_grad_(True)
    sums = {}
    S = torch.zeros(n, k, dtype=torch.float64)
    for b in range(n):
        for c in range(k):
            if el[b, c]:
                kp = keep[b, c]
                sums[b, c] = terms(p[b, c][kp].double(), y_f64[b, c][kp], kind, beta).sum()
                S[b, c] = sums[b, c].detach()
    used = select(S, npix, weights, el, topk)
    D = divisor(pts, npix, used, norm)
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

def seeded_mask(shape, seed=11):
    """uint8 [N,H,W] for a loss shape (N, K, M, H, W): about 30 % of the pixels per class
    bit, one full row, class 0's whole plane in image 0, and (N > 1) the last image at 0xFF."""
    n, k, m, H, W = shape
    g = torch.Generator().manual_seed(seed + n * 1000 + k * 100 + H)
    mask = torch.zeros(n, H, W, dtype=torch.int64)
    for c in range(8):
        mask |= (torch.rand(n, H, W, generator=g) < 0.3).long() << c
    mask[:, H // 2, :] = 0xFF
    if k > 1:
        mask[0] |= 1
    if n > 1:
        mask[n - 1] = 0xFF
    return mask.to(torch.uint8)


def plane_mask(shape, off):
    """uint8 [N,H,W] that masks exactly the whole planes off (bool [N,K])."""
    n, k, m, H, W = shape
    bits = (off.long() << torch.arange(k)).sum(1)
    return bits.view(n, 1, 1).expand(n, H, W).contiguous().to(torch.uint8)


def topk_mask(shape, seed=5):
    """uint8 [N,H,W] for the top-k shapes: every class loses a different share of its
    pixels (class c about 10 % + 8 % * c), so that sums and means rank differently."""
    n, k, m, H, W = shape
    g = torch.Generator().manual_seed(seed + k * 10 + H)
    mask = torch.zeros(n, H, W, dtype=torch.int64)
    for c in range(k):
        mask |= (torch.rand(n, H, W, generator=g) < 0.10 + 0.08 * c).long() << c
    return mask.to(torch.uint8)


TOPK_SHAPES = [(2, 5, 2, 17, 23), (2, 6, 3, 12, 40), (1, 4, 1, 75, 101)]
TOPK_MIN_GAP = 8e-4          # the planes tests' precondition on neighbouring ranks


def topk_weights(shape):
    n, k = shape[:2]
    return torch.rand(n, k, generator=torch.Generator().manual_seed(9)) * 1.5 + 0.25


def topk_inputs(shape, absent):
    """(heat float32 [N,K,H,W], pts [N,K,M,3], mask uint8 [N,H,W]) of a top-k case: the heat
    and labels of the planes tests (tests/test_gpu_instances.py, tests/test_gpu_focal.py) and
    topk_mask.  The same tensors on every call."""
    from test_gpu_focal import _labels
    from test_gpu_instances import _heat
    return _heat(shape, seed=4), _labels(shape, absent), topk_mask(shape)


# --------------------------------------------------------------------- rasteriser ----

def regions_ref(regions, H, W):
    """regions float32 [N,R,6] (numpy) -> uint8 [N,H,W]: the definition of
    hkp_mask_regions_u8 (include/hulkkp.h) in numpy float32, every operation rounded on its
    own.  The fields of a slot of unknown kind are not read."""
    regions = np.asarray(regions)
    assert regions.dtype == np.float32 and regions.ndim == 3 and regions.shape[2] == 6
    n, r = regions.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    x, y = xx.astype(np.float32), yy.astype(np.float32)
    out = np.zeros((n, H, W), dtype=np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(n):
            for j in range(r):
                kind = regions[b, j, 0]
                if not (kind == np.float32(1) or kind == np.float32(2)):
                    continue
                a, bb, c, d, bf = (np.float32(v) for v in regions[b, j, 1:])
                bits = int(bf) if (bf >= 0 and bf <= 255) else 0
                if kind == np.float32(1):
                    inside = (a <= x) & (x <= c) & (bb <= y) & (y <= d)
                else:
                    dx, dy = x - a, y - bb
                    inside = (dx * dx + dy * dy) <= np.float32(c * c)
                out[b][inside] |= np.uint8(bits)
    return out


def flip_lut(flip_pairs=()):
    """uint8 [256] (numpy): byte v with bits a and b exchanged for every pair, in order."""
    out = np.zeros(256, dtype=np.uint8)
    for v in range(256):
        t = v
        for a, b in flip_pairs:
            ba, bb = (t >> a) & 1, (t >> b) & 1
            t = (t & ~((1 << a) | (1 << b))) | (bb << a) | (ba << b)
        out[v] = t
    return out


# --------------------------------------------------------------------- evaluation ----

def peaks_drop_masked(peaks, counts, mask):
    """peaks float32 [N,K,P,3], counts int32 [N,K], mask uint8 [N,H,W] (CPU tensors) ->
    (peaks, counts): the definition as loops."""
    n, k, p, _ = peaks.shape
    H, W = mask.shape[1:]
    out = torch.empty_like(peaks)
    out[..., 0] = -1.0
    out[..., 1] = -1.0
    out[..., 2] = 0.0
    cnt = torch.zeros_like(counts)
    for b in range(n):
        for c in range(k):
            j = 0
            for s in range(min(max(int(counts[b, c]), 0), p)):
                x, y = float(peaks[b, c, s, 0]), float(peaks[b, c, s, 1])
                drop = False
                if math.isfinite(x) and math.isfinite(y):
                    fx = float(np.float32(np.float32(x) + np.float32(0.5)))      # the fp32 sum, as the tensors do
                    fy = float(np.float32(np.float32(y) + np.float32(0.5)))
                    ix = min(max(int(math.floor(fx)), 0), W - 1)
                    iy = min(max(int(math.floor(fy)), 0), H - 1)
                    drop = bool((int(mask[b, iy, ix]) >> c) & 1)
                if not drop:
                    out[b, c, j] = peaks[b, c, s]
                    j += 1
            cnt[b, c] = j
    return out, cnt
