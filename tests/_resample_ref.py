"""numpy restatement of the antialiased resize (include/hulkkp.h "antialiased
resize", csrc/resample.hip): Pillow's separable fixed-point resampler for RGB
uint8 images, `Image.resize(size, filter, reducing_gap=None)`.

The axis tables are built in float64 (the transcendentals through `math`, the C
library's, one value at a time, as Pillow calls them); everything after the tables
is int64.  The horizontal pass runs first and its result is rounded to uint8; a
pass whose axis keeps its size is skipped.  Written independently of hkp.resample:
tests/test_resample_cpu.py compares the two, and this file with Pillow."""
import math

import numpy as np

PRECISION_BITS = 22


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (0.54 + 0.46 * math.cos(x))


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


FILTERS = {"box": (_box, 0.5), "bilinear": (_bilinear, 1.0), "hamming": (_hamming, 1.0), "bicubic": (_bicubic, 2.0),
           "lanczos": (_lanczos, 3.0)}


def axis_table(n_in, n_out, name):
    """(ksize, bounds int64 [n_out, 2] = (xmin, cnt), coefficients int64 [n_out, ksize])."""
    f, fsupport = FILTERS[name]
    scale = float(n_in) / float(n_out)
    fs = max(scale, 1.0)
    support = fsupport * fs
    ksize = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / fs
    bounds = np.zeros((n_out, 2), dtype=np.int64)
    kk = np.zeros((n_out, ksize), dtype=np.int64)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        cnt = min(int(center + support + 0.5), n_in) - xmin
        w = [f((x + xmin - center + 0.5) * inv) for x in range(cnt)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[xx, x] = int(0.5 + v * (1 << PRECISION_BITS)) if v >= 0 else int(-0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, cnt)
    return ksize, bounds, kk


def identity_table(n):
    """The table of an axis that keeps its size: one tap of weight 2^22."""
    bounds = np.stack([np.arange(n, dtype=np.int64), np.ones(n, dtype=np.int64)], 1)
    return 1, bounds, np.full((n, 1), 1 << PRECISION_BITS, dtype=np.int64)


def _pass(img, table, axis):
    """One pass along `axis` (0: rows, 1: columns) of an [H, W, C] image, int64."""
    ksize, bounds, kk = table
    a = np.moveaxis(np.asarray(img).astype(np.int64), axis, 0)
    out = np.empty((bounds.shape[0],) + a.shape[1:], dtype=np.int64)
    for i, (lo, cnt) in enumerate(bounds):
        k = kk[i, :cnt].reshape((cnt,) + (1,) * (a.ndim - 1))
        out[i] = ((1 << (PRECISION_BITS - 1)) + (a[lo:lo + cnt] * k).sum(0)) >> PRECISION_BITS
    return np.moveaxis(np.clip(out, 0, 255), 0, axis).astype(np.uint8)


def resize(img, h, w, name="bilinear"):
    """uint8 [hs, ws, 3] -> [h, w, 3]: horizontal pass, uint8, vertical pass."""
    img = np.asarray(img)
    hs, ws = img.shape[:2]
    if ws != w:
        img = _pass(img, axis_table(ws, w, name), 1)
    if hs != h:
        img = _pass(img, axis_table(hs, h, name), 0)
    return np.array(img, dtype=np.uint8)


def placement(hs, ws, h, w, mode="stretch"):
    """(x0, y0, wd, hd): where an hs x ws source lands in the h x w output."""
    if mode == "stretch":
        return 0, 0, w, h
    s = min(w / ws, h / hs)
    wd = min(w, max(1, int(math.floor(ws * s + 0.5))))
    hd = min(h, max(1, int(math.floor(hs * s + 0.5))))
    return (w - wd) // 2, (h - hd) // 2, wd, hd


def resample(img, h, w, name="bilinear", mode="stretch", fill=(0, 0, 0)):
    x0, y0, wd, hd = placement(img.shape[0], img.shape[1], h, w, mode)
    out = np.empty((h, w, 3), dtype=np.uint8)
    out[:] = np.asarray(fill, dtype=np.uint8)
    out[y0:y0 + hd, x0:x0 + wd] = resize(img, hd, wd, name)
    return out


def resample_ragged(flat, sizes, h, w, name="bilinear", mode="stretch", fill=(0, 0, 0)):
    """flat: the images of `sizes` [(hs, ws), ...] packed one after the other."""
    flat = np.asarray(flat, dtype=np.uint8).reshape(-1)
    out, off = [], 0
    for hs, ws in sizes:
        nb = int(hs) * int(ws) * 3
        out.append(resample(flat[off:off + nb].reshape(int(hs), int(ws), 3), h, w, name, mode, fill))
        off += nb
    return np.stack(out)


def apply_uv(uv, hs, ws, h, w, mode="stretch"):
    """Forward label map (half-pixel centres), clipped to the output image."""
    x0, y0, wd, hd = placement(hs, ws, h, w, mode)
    p = np.asarray(uv, dtype=np.float64)
    out = np.empty(p.shape, dtype=np.float64)
    out[..., 0] = np.clip((p[..., 0] + 0.5) * wd / ws - 0.5 + x0, 0, w - 1)
    out[..., 1] = np.clip((p[..., 1] + 0.5) * hd / hs - 0.5 + y0, 0, h - 1)
    return out.astype(np.float32)


def images(hs, ws, seed):
    """A random image with saturated stripes (0 and 255 side by side: overshoot of the
    negative lobes has to clip)."""
    rng = np.random.default_rng([seed, hs, ws])
    a = rng.integers(0, 256, (hs, ws, 3), dtype=np.uint8)
    a[:, ws // 3:ws // 3 + max(1, ws // 8)] = 255
    a[hs // 2:hs // 2 + max(1, hs // 8)] = 0
    a[:max(1, hs // 10), :, 1] = 255
    return a
