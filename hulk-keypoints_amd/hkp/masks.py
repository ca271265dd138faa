"""Per-pixel ignore masks for the heatmap loss and the evaluation (not in the reference).

A mask is a uint8 [N,H,W] tensor in the frame of the heatmaps and labels, one byte per
pixel holding class bits: bit c set means "this pixel is ignored for class c", 0xFF for
every class (so at most 8 classes).  ops.heat_loss_masked, heatmap_loss(mask=) and
Trainer.step(mask=) leave the masked pixels out of the loss; peaks_drop_masked drops the
decoded peaks that fall on them before they are matched (COCO's rule for ignore regions:
neither a true nor a false positive).

Masks are made from region records and travel with the images:
  * box / disc / pack build the float32 [N,R,6] records (kind, a, b, c, d, bits) that
    ops.mask_regions_u8 rasterises on the GPU;
  * ops.warp_mask_u8 / WarpPlan.apply_mask move a mask through the images' transforms,
    nearest-neighbour, and flip_lut is the byte table that exchanges the class bits of the
    flip pairs in a flipped image.
Regions are not transformed analytically: rasterise in the source frame, warp the mask.
"""
import numpy as np
import torch

from ._lib import HKP_MASK_BOX, HKP_MASK_DISC, HKP_MASK_MAX_REGIONS, MASK_MAX_K, HkpError

ALL_CLASSES = 0xFF


def class_bits(classes):
    """The mask byte of a set of classes: None or "all" -> 0xFF; an int c or a sequence of
    ints in 0..7 -> the OR of 1 << c."""
    if classes is None or (isinstance(classes, str) and classes == "all"):
        return ALL_CLASSES
    if np.ndim(classes) == 0:
        classes = (classes,)
    bits = 0
    for c in classes:
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= c < MASK_MAX_K:
            raise HkpError("class_bits: classes are integers in 0..%d, got %r" % (MASK_MAX_K - 1, c))
        bits |= 1 << int(c)
    return bits


def box(x0, y0, x1, y1, classes=None):
    """The record of the box x0 <= x <= x1, y0 <= y <= y1 (pixel centres, both ends
    included) ignored for `classes` (class_bits)."""
    return (float(HKP_MASK_BOX), float(x0), float(y0), float(x1), float(y1), float(class_bits(classes)))


def disc(cx, cy, r, classes=None):
    """The record of the disc (x-cx)^2 + (y-cy)^2 <= r^2 ignored for `classes`."""
    return (float(HKP_MASK_DISC), float(cx), float(cy), float(r), 0.0, float(class_bits(classes)))


def pack(per_image_lists, R=None, device=None):
    """per_image_lists: for every image a list of box / disc records -> float32 [N,R,6],
    the unused slots empty (kind 0).  R: the slots per image, default the longest list (at
    least 1), at most 64.  device: where the tensor goes (default: the CPU)."""
    lists = [list(l) for l in per_image_lists]
    if not lists:
        raise HkpError("masks.pack: need at least one image")
    longest = max(len(l) for l in lists)
    R = max(longest, 1) if R is None else int(R)
    if not 1 <= R <= HKP_MASK_MAX_REGIONS or longest > R:
        raise HkpError("masks.pack: R = %d outside 1..%d, or below the longest list (%d regions)"
                       % (R, HKP_MASK_MAX_REGIONS, longest))
    a = np.zeros((len(lists), R, 6), dtype=np.float32)
    for b, l in enumerate(lists):
        for j, rec in enumerate(l):
            if len(rec) != 6:
                raise HkpError("masks.pack: a region is (kind, a, b, c, d, bits), got %r" % (rec,))
            a[b, j] = rec
    t = torch.from_numpy(a)
    return t if device is None else t.to(device)


def flip_lut(flip_pairs=()):
    """uint8 [256] (CPU): the byte v with bits a and b exchanged for every (a, b) of
    flip_pairs, the other bits kept.  The identity without pairs; its own inverse."""
    v = np.arange(256, dtype=np.int64)
    out = v.copy()
    for a, b in flip_pairs:
        a, b = int(a), int(b)
        if not (0 <= a < MASK_MAX_K and 0 <= b < MASK_MAX_K):
            raise HkpError("flip_lut: a pair names classes in 0..%d, got %r" % (MASK_MAX_K - 1, (a, b)))
        ba, bb = (out >> a) & 1, (out >> b) & 1
        out = (out & ~((1 << a) | (1 << b))) | (bb << a) | (ba << b)
    return torch.from_numpy(out.astype(np.uint8))


def peaks_drop_masked(peaks, counts, mask):
    """Decoded peaks without those on ignored pixels: peaks float32 [N,K,P,3] (x, y, score)
    and counts int32 [N,K] as ops.heat_peaks returns them, mask uint8 [N,H,W] in the peaks'
    frame -> (peaks, counts), new tensors.  A peak of class c in the first clamp(counts, 0,
    P) slots is dropped iff x and y are finite and bit c of mask[b, clamp(floor(y + 0.5)),
    clamp(floor(x + 0.5))] is set; the kept peaks move to the front in their order, the
    freed slots get (-1, -1, 0), counts shrink.  Plain torch operations on the tensors'
    device (CPU or GPU), no host synchronisation."""
    if not (isinstance(peaks, torch.Tensor) and isinstance(counts, torch.Tensor) and isinstance(mask, torch.Tensor)):
        raise HkpError("peaks_drop_masked: expected tensors")
    if peaks.dim() != 4 or peaks.shape[3] != 3 or peaks.dtype != torch.float32:
        raise HkpError("peaks_drop_masked: peaks must be float32 [N,K,P,3], got %s %s"
                       % (peaks.dtype, tuple(peaks.shape)))
    n, k, p, _ = peaks.shape
    if counts.dtype != torch.int32 or tuple(counts.shape) != (n, k):
        raise HkpError("peaks_drop_masked: counts must be int32 [%d,%d], got %s %s"
                       % (n, k, counts.dtype, tuple(counts.shape)))
    if mask.dtype != torch.uint8 or mask.dim() != 3 or mask.shape[0] != n or mask.shape[1] < 1 or mask.shape[2] < 1:
        raise HkpError("peaks_drop_masked: mask must be uint8 [%d,H,W], got %s %s"
                       % (n, mask.dtype, tuple(mask.shape)))
    if k > MASK_MAX_K:
        raise HkpError("peaks_drop_masked: a mask holds %d class bits, the peaks have K = %d classes"
                       % (MASK_MAX_K, k))
    if counts.device != peaks.device or mask.device != peaks.device:
        raise HkpError("peaks_drop_masked: peaks on %s, counts on %s, mask on %s"
                       % (peaks.device, counts.device, mask.device))
    dev = peaks.device
    H, W = mask.shape[1], mask.shape[2]
    x, y = peaks[..., 0], peaks[..., 1]
    finite = torch.isfinite(x) & torch.isfinite(y)
    zero = torch.zeros((), dtype=x.dtype, device=dev)
    # (floor of a non-finite value is replaced before the integer cast)
    ix = torch.floor(torch.where(finite, x, zero) + 0.5).clamp(0, W - 1).long()
    iy = torch.floor(torch.where(finite, y, zero) + 0.5).clamp(0, H - 1).long()
    b = torch.arange(n, device=dev).view(n, 1, 1).expand(n, k, p)
    cls = torch.arange(k, device=dev).view(1, k, 1)
    hit = ((mask[b, iy, ix].long() >> cls) & 1) == 1
    slot = torch.arange(p, device=dev).view(1, 1, p)
    valid = slot < counts.clamp(0, p).view(n, k, 1).long()
    keep = valid & ~(hit & finite)
    # stable: the kept slots first, each group in slot order
    order = torch.argsort((~keep).long() * p + slot, dim=2)
    new_counts = keep.sum(2).to(torch.int32)
    moved = torch.gather(peaks, 2, order.unsqueeze(-1).expand(n, k, p, 3))
    empty = torch.cat([torch.full((2,), -1.0, dtype=peaks.dtype, device=dev),
                       torch.zeros(1, dtype=peaks.dtype, device=dev)]).expand(n, k, p, 3)
    out = torch.where((slot < new_counts.view(n, k, 1).long()).unsqueeze(-1), moved, empty)
    return out, new_counts
