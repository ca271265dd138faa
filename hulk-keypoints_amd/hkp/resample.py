"""Antialiased resize on the GPU for uint8 images of any size: the first stage of
the data path, decoded frame -> network-size frame, with the labels (and, back
again, the predictions) mapped by the same transform.  One kernel,
hkp_resample_u8 (csrc/resample.hip), one launch per batch; every image of a batch
has its own source size.

Contract: the pixels equal Pillow's `Image.resize((w, h), filter,
reducing_gap=None)` of the RGB image bit for bit (include/hulkkp.h spells the
arithmetic out; tests/_resample_ref.py restates it; the tests pin the kernel
against both).  The filter lives in the axis tables built here in float64, as
Pillow builds its coefficients; the device arithmetic is integer only.

  stretch  the whole source goes onto the whole output.
  fit      the aspect ratio is kept: s = min(w/ws, h/hs), wd = min(w, max(1,
           floor(ws*s + 0.5))), hd likewise, centred (x0 = (w - wd)//2); the
           rest of the output takes the fill colour.

Labels use half-pixel centres (as geometry.resize_matrix):
  forward  u' = (u + 0.5)*wd/ws - 0.5 + x0, then clipped to the output image
           (the reference's label rule, dataset.py:65-66)
  inverse  u  = (u' - x0 + 0.5)*ws/wd - 0.5
Not pinned: cv2.resize (not installed), Pillow's reducing_gap prefilter, other
pixel formats.  There is no CPU path.
"""
import ctypes
import functools
import math

import numpy as np
import torch

from ._lib import HKP_WARP_MAX_DIM, HkpError, ResampleImage

PRECISION_BITS = 22
MODES = ("stretch", "fit")


def _box(x):
    return np.where((x > -0.5) & (x <= 0.5), 1.0, 0.0)


def _bilinear(x):
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


def _bicubic(x):                     # Keys, a = -0.5, in Pillow's order of operations
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def _each(f):
    """A scalar filter over an array, one value at a time through `math` (the C
    library's sin / cos, as Pillow calls them: numpy's vector forms may round
    differently in the last place)."""
    def g(x):
        return np.array([f(float(v)) for v in x.reshape(-1)], dtype=np.float64).reshape(x.shape)
    return g


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _hamming1(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (0.54 + 0.46 * math.cos(x))


def _lanczos1(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


# name -> (filter over a float64 array, support)
FILTERS = {"box": (_box, 0.5), "bilinear": (_bilinear, 1.0), "hamming": (_each(_hamming1), 1.0),
           "bicubic": (_bicubic, 2.0), "lanczos": (_each(_lanczos1), 3.0)}


def _check_filter(name, who):
    if name not in FILTERS:
        raise HkpError("%s: unknown filter %r (known: %s)" % (who, name, ", ".join(FILTERS)))


def _check_dim(v, who):
    if int(v) != v or not 1 <= int(v) <= HKP_WARP_MAX_DIM:
        raise HkpError("%s: a dimension of %r is outside 1..%d" % (who, v, HKP_WARP_MAX_DIM))
    return int(v)


@functools.lru_cache(maxsize=256)
def axis_table(n_in, n_out, filter="bilinear"):
    """The axis table n_in -> n_out as read-only int32 words: ksize, n_out, then
    n_out x (xmin, cnt), then n_out x ksize coefficients (Q22, rows summing to
    about 2^22).  Cached per (n_in, n_out, filter)."""
    _check_filter(filter, "axis_table")
    n_in, n_out = _check_dim(n_in, "axis_table"), _check_dim(n_out, "axis_table")
    f, fsupport = FILTERS[filter]
    scale = float(n_in) / float(n_out)
    fs = max(scale, 1.0)
    support = fsupport * fs
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5), 0.0)
    cnt = np.minimum(np.trunc(center + support + 0.5), float(n_in)) - xmin
    t = np.arange(ksize, dtype=np.float64)[None, :]
    live = t < cnt[:, None]
    w = np.where(live, f((t + xmin[:, None] - center[:, None] + 0.5) * (1.0 / fs)), 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                       # summed in index order, as Pillow sums
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    one = float(1 << PRECISION_BITS)
    k = np.where(w < 0, np.trunc(-0.5 + w * one), np.trunc(0.5 + w * one))
    k = np.where(live, k, 0.0)
    words = np.empty(2 + 2 * n_out + n_out * ksize, dtype=np.int32)
    words[0], words[1] = ksize, n_out
    words[2:2 + 2 * n_out:2] = xmin.astype(np.int32)
    words[3:3 + 2 * n_out:2] = cnt.astype(np.int32)
    words[2 + 2 * n_out:] = k.astype(np.int32).reshape(-1)
    words.setflags(write=False)
    return words


@functools.lru_cache(maxsize=64)
def identity_table(n):
    """The table of an axis that keeps its size: one tap of weight 2^22 per output,
    which returns the pixel exactly (Pillow skips such a pass)."""
    n = _check_dim(n, "identity_table")
    words = np.empty(2 + 3 * n, dtype=np.int32)
    words[0], words[1] = 1, n
    words[2:2 + 2 * n:2] = np.arange(n, dtype=np.int32)
    words[3:3 + 2 * n:2] = 1
    words[2 + 2 * n:] = 1 << PRECISION_BITS
    words.setflags(write=False)
    return words


def table_parts(words):
    """(ksize, bounds [out, 2] = (xmin, cnt), coefficients [out, ksize]) views of a table."""
    ksize, out = int(words[0]), int(words[1])
    return ksize, words[2:2 + 2 * out].reshape(out, 2), words[2 + 2 * out:2 + 2 * out + out * ksize].reshape(out, ksize)


def placement(hs, ws, h, w, mode="stretch"):
    """(x0, y0, wd, hd): the destination rectangle of an hs x ws source in the h x w output."""
    if mode not in MODES:
        raise HkpError("resample: unknown mode %r (known: %s)" % (mode, ", ".join(MODES)))
    if mode == "stretch":
        return 0, 0, int(w), int(h)
    s = min(float(w) / float(ws), float(h) / float(hs))
    wd = min(int(w), max(1, int(math.floor(ws * s + 0.5))))
    hd = min(int(h), max(1, int(math.floor(hs * s + 0.5))))
    return (int(w) - wd) // 2, (int(h) - hd) // 2, wd, hd


def _host_uv(uv, n, who):
    is_t = isinstance(uv, torch.Tensor)
    a = uv.detach().cpu().numpy() if is_t else np.asarray(uv)
    if a.ndim != 3 or a.shape[0] != n or a.shape[2] != 2:
        raise HkpError("%s: expected [%d, K, 2], got %s" % (who, n, a.shape))
    return is_t, a


class ResamplePlan:
    """One batch of resizes: image b of size sizes[b] = (hs, ws), packed one after
    the other in a flat uint8 buffer, onto the output hw = (h, w).

    records   ctypes ResampleImage * n (hkp_resample_image)
    tables    int32 words: the axis tables, one per distinct (in, out) pair
    rects     int [n, 4]: (x0, y0, wd, hd) per image
    in_bytes  the size of the flat input
    device_arrays() uploads records and tables from pinned memory on the current
    stream; the plan keeps the pinned and the device copies alive, so keep the plan
    until the batch has been consumed."""

    def __init__(self, sizes, hw, filter="bilinear", mode="stretch", fill=(0, 0, 0)):
        _check_filter(filter, "ResamplePlan")
        sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
        if sizes.shape[0] < 1:
            raise HkpError("ResamplePlan: no images")
        if len(fill) != 3 or any(int(f) != f or not 0 <= f <= 255 for f in fill):
            raise HkpError("ResamplePlan: fill is three integers in 0..255 (B, G, R), got %r" % (fill,))
        h, w = _check_dim(hw[0], "ResamplePlan"), _check_dim(hw[1], "ResamplePlan")
        self.n = sizes.shape[0]
        self.sizes = sizes
        self.hw = (h, w)
        self.filter, self.mode, self.fill = filter, mode, tuple(int(f) for f in fill)
        self.records = (ResampleImage * self.n)()
        self.rects = np.empty((self.n, 4), dtype=np.int64)
        chunks, where, words, off = [], {}, 0, 0

        def table(n_in, n_out):
            nonlocal words
            key = (n_in, n_out)
            if key not in where:
                t = identity_table(n_in) if n_in == n_out else axis_table(n_in, n_out, filter)
                where[key] = words
                chunks.append(t)
                words += t.size
            return where[key]

        for b in range(self.n):
            hs, ws = _check_dim(sizes[b, 0], "ResamplePlan"), _check_dim(sizes[b, 1], "ResamplePlan")
            x0, y0, wd, hd = placement(hs, ws, h, w, mode)
            self.rects[b] = (x0, y0, wd, hd)
            r = self.records[b]
            r.offset, r.hs, r.ws = off, hs, ws
            r.xtab, r.ytab = table(ws, wd), table(hs, hd)
            r.x0, r.y0, r.wd, r.hd = x0, y0, wd, hd
            for i in range(3):
                r.fill[i] = self.fill[i]
            off += hs * ws * 3
        self.in_bytes = off
        self.tables = np.concatenate(chunks).astype(np.int32)
        self._dev = {}

    def record_bytes(self):
        """The records as a numpy uint8 view [n, 64] (shares memory)."""
        return np.frombuffer(self.records, dtype=np.uint8).reshape(self.n, ctypes.sizeof(ResampleImage))

    def offsets(self):
        """int64 [n]: byte offset of each image in the flat input."""
        return np.array([r.offset for r in self.records], dtype=np.int64)

    def device_arrays(self, device):
        """(records, tables) on `device`, uploaded once from pinned memory."""
        device = torch.device(device)
        key = device.index if device.index is not None else torch.cuda.current_device()
        got = self._dev.get(key)
        if got is None:
            dev = torch.device("cuda", key)
            pin_r = torch.from_numpy(self.record_bytes().copy()).pin_memory()
            pin_t = torch.from_numpy(self.tables).pin_memory()
            got = (pin_r.to(dev, non_blocking=True), pin_t.to(dev, non_blocking=True), pin_r, pin_t)
            self._dev[key] = got
        return got[0], got[1]

    def _maps(self):
        s = self.sizes.astype(np.float64)
        r = self.rects.astype(np.float64)
        gain = np.stack([r[:, 2] / s[:, 1], r[:, 3] / s[:, 0]], 1)[:, None, :]          # (wd/ws, hd/hs)
        return gain, r[:, None, 0:2]

    def apply_uv(self, uv):
        """Labels uv [n, K, 2] in source pixels (numpy or a CPU tensor; the same kind
        comes back, float32) -> output pixels, clipped to [0, w-1] x [0, h-1]."""
        is_t, a = _host_uv(uv, self.n, "apply_uv")
        gain, org = self._maps()
        out = (a.astype(np.float64) + 0.5) * gain - 0.5 + org
        h, w = self.hw
        out[..., 0] = np.clip(out[..., 0], 0, w - 1)
        out[..., 1] = np.clip(out[..., 1], 0, h - 1)
        out = out.astype(np.float32)
        return torch.from_numpy(out) if is_t else out

    def apply_points(self, pts):
        """Instance labels pts [n, K, M, 3] (u, v, flag) in source pixels (numpy or a CPU
        tensor; the same kind comes back, float32) -> output pixels, in `stretch` and
        `fit` modes alike: (u, v) of the present slots (flag > 0) through apply_uv's
        map; a present point that leaves [0, w-1] x [0, h-1] gets flag 0 and is not
        clipped; empty slots pass through as they are."""
        from .geometry import host_points
        is_t, a = host_points(pts, self.n, "apply_points")
        out = np.array(a, dtype=np.float32, copy=True)
        gain, org = self._maps()
        on = out[..., 2] > 0
        src = np.where(on[..., None], out[..., :2], 0.0).astype(np.float64)
        q = ((src + 0.5) * gain[:, None] - 0.5 + org[:, None]).astype(np.float32)
        h, w = self.hw
        inside = (q[..., 0] >= 0) & (q[..., 0] <= w - 1) & (q[..., 1] >= 0) & (q[..., 1] <= h - 1)
        out[..., :2] = np.where(on[..., None], q, out[..., :2])
        out[..., 2] = np.where(on & ~inside, 0.0, out[..., 2])
        return torch.from_numpy(out) if is_t else out

    def apply_lines(self, lines):
        """Line labels lines [n, K, S, 5] (x0, y0, x1, y1, flag) in source pixels (numpy or a
        CPU tensor; the same kind comes back, float32) -> output pixels: both ends of the
        present slots (flag > 0) through apply_points' map.  Nothing is clipped or dropped;
        empty slots pass through as they are."""
        from .geometry import host_lines
        is_t, a = host_lines(lines, self.n, "apply_lines")
        out = np.array(a, dtype=np.float32, copy=True)
        gain, org = self._maps()
        on = (out[..., 4] > 0)[..., None]
        for e in (0, 2):
            src = np.where(on, out[..., e:e + 2], 0.0).astype(np.float64)
            q = ((src + 0.5) * gain[:, None] - 0.5 + org[:, None]).astype(np.float32)
            out[..., e:e + 2] = np.where(on, q, out[..., e:e + 2])
        return torch.from_numpy(out) if is_t else out

    def invert_uv(self, uv):
        """Predictions uv [n, K, 2] in output pixels -> the source image's pixels (not clipped)."""
        is_t, a = _host_uv(uv, self.n, "invert_uv")
        gain, org = self._maps()
        out = ((a.astype(np.float64) - org + 0.5) / gain - 0.5).astype(np.float32)
        return torch.from_numpy(out) if is_t else out

    def invert_peaks(self, peaks, counts):
        """The multi-peak decode (ops.heat_peaks: peaks [n, K, P, 3] (x, y, score),
        counts [n, K]; numpy or CPU tensors, the same kind comes back) mapped into
        the source images' pixels: invert_uv on (x, y) of the first counts[b, k]
        slots of every plane; the unused slots and the scores are left as they are."""
        is_t = isinstance(peaks, torch.Tensor)
        p = np.array(peaks.detach().cpu().numpy() if is_t else peaks, dtype=np.float32)      # a copy
        c = counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
        if p.ndim != 4 or p.shape[0] != self.n or p.shape[3] != 3 or c.shape != p.shape[:2]:
            raise HkpError("invert_peaks: expected peaks [%d, K, P, 3] and counts [%d, K], got %s and %s"
                           % (self.n, self.n, p.shape, c.shape))
        n, k, pk, _ = p.shape
        used = np.arange(pk)[None, None, :] < c[:, :, None]
        xy = self.invert_uv(np.ascontiguousarray(p[..., :2]).reshape(n, k * pk, 2)).reshape(n, k, pk, 2)
        p[..., :2] = np.where(used[..., None], xy, p[..., :2])
        return torch.from_numpy(p) if is_t else p


class Resize:
    """What the data path takes (DeviceBatches(resize=...), KeypointsDataset(resize=...)):
    filter ("box", "bilinear", "hamming", "bicubic", "lanczos"), mode ("stretch",
    "fit") and the fill colour (B, G, R) of "fit"."""

    def __init__(self, filter="bilinear", mode="stretch", fill=(0, 0, 0)):
        if filter not in FILTERS:
            raise ValueError("unknown filter %r (known: %s)" % (filter, ", ".join(FILTERS)))
        if mode not in MODES:
            raise ValueError("unknown mode %r (known: %s)" % (mode, ", ".join(MODES)))
        if len(fill) != 3 or any(int(f) != f or not 0 <= f <= 255 for f in fill):
            raise ValueError("fill is three integers in 0..255 (B, G, R), got %r" % (fill,))
        self.filter, self.mode, self.fill = filter, mode, tuple(int(f) for f in fill)

    def plan(self, sizes, hw):
        """The ResamplePlan of a batch of images of `sizes` [(hs, ws), ...] onto hw = (h, w)."""
        return ResamplePlan(sizes, hw, filter=self.filter, mode=self.mode, fill=self.fill)

    def __repr__(self):
        return "Resize(filter=%r, mode=%r, fill=%r)" % (self.filter, self.mode, self.fill)
