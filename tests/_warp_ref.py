"""numpy int64 restatement of the affine warp's arithmetic (include/hulkkp.h,
"affine warp"), every interpolation and border mode.  It reads nothing of the
package: the Q16 coefficients, the fill colour and the modes come in as plain
numbers.

    warp(src uint8 [hs, ws, 3], m int[6], h, w, interp, border, fill) -> uint8 [h, w, 3]
    interp  0 bilinear, 1 nearest
    border  0 constant (fill), 1 replicate, 2 reflect-101 (once, then clamped)
"""
import numpy as np

BILINEAR, NEAREST = 0, 1
CONSTANT, REPLICATE, REFLECT101 = 0, 1, 2


def _tap(i, n, border):
    """Tap indices i (int64, already within [-2, n + 2]) -> (index in [0, n), outside)."""
    outside = (i < 0) | (i >= n)
    if border == REFLECT101:
        i = np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))
    return np.clip(i, 0, n - 1), outside


def _gather(src, iy, ix, oy, ox, border, fill):
    v = src[iy, ix].astype(np.int64)                         # [h, w, 3]
    if border == CONSTANT:
        v = np.where((oy | ox)[..., None], np.asarray(fill, dtype=np.int64)[:3], v)
    return v


def warp(src, m, h, w, interp=BILINEAR, border=CONSTANT, fill=(0, 0, 0)):
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[2] == 3
    hs, ws = src.shape[:2]
    m = [int(v) for v in m]
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    sx = m[0] * x + m[1] * y + m[2]
    sy = m[3] * x + m[4] * y + m[5]
    if interp == NEAREST:
        ix = np.clip((sx + 32768) >> 16, -2, ws + 1)
        iy = np.clip((sy + 32768) >> 16, -2, hs + 1)
        tx, ox = _tap(ix, ws, border)
        ty, oy = _tap(iy, hs, border)
        return _gather(src, ty, tx, oy, ox, border, fill).astype(np.uint8)
    qx, qy = (sx + 128) >> 8, (sy + 128) >> 8
    fx, fy = (qx & 255)[..., None], (qy & 255)[..., None]
    ix = np.clip(qx >> 8, -2, ws + 1)
    iy = np.clip(qy >> 8, -2, hs + 1)
    x0, ox0 = _tap(ix, ws, border)
    x1, ox1 = _tap(ix + 1, ws, border)
    y0, oy0 = _tap(iy, hs, border)
    y1, oy1 = _tap(iy + 1, hs, border)
    p00 = _gather(src, y0, x0, oy0, ox0, border, fill)
    p01 = _gather(src, y0, x1, oy0, ox1, border, fill)
    p10 = _gather(src, y1, x0, oy1, ox0, border, fill)
    p11 = _gather(src, y1, x1, oy1, ox1, border, fill)
    top = p00 * (256 - fx) + p01 * fx
    bot = p10 * (256 - fx) + p11 * fx
    return ((top * (256 - fy) + bot * fy + 32768) >> 16).astype(np.uint8)


def warp_batch(srcs, ms, h, w, interp=BILINEAR, border=CONSTANT, fills=None):
    """srcs [n, hs, ws, 3], ms [n, 6] -> [n, h, w, 3]."""
    n = len(srcs)
    return np.stack([warp(srcs[b], ms[b], h, w, interp, border, (0, 0, 0) if fills is None else fills[b])
                     for b in range(n)])


def inside_mask(src_hw, m, h, w):
    """bool [h, w]: the bilinear taps (ix, ix+1, iy, iy+1) of an output pixel all lie
    inside the source."""
    hs, ws = src_hw
    m = [int(v) for v in m]
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    ix = ((m[0] * x + m[1] * y + m[2] + 128) >> 8) >> 8
    iy = ((m[3] * x + m[4] * y + m[5] + 128) >> 8) >> 8
    return (ix >= 0) & (ix + 1 < ws) & (iy >= 0) & (iy + 1 < hs)
