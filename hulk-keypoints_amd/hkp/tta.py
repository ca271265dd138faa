"""Test-time augmentation on the stride-8 lattice (not in the reference).

TestTimeAugmentation describes a set of views of one input batch — the batch as
it is, mirrored, rescaled — and merges the low-res logits of one forward per view
into logits on the base view's lattice with one launch (hkp_logits_merge,
include/hulkkp.h).  What comes out is read by ops.heat_peaks exactly as one
forward's `low` is: no full-resolution heatmap is formed.

Frames.  Base node j of a lattice of w nodes stands at base pixel
X = j (W - 1) / (w - 1) (0 when w == 1): the align_corners frame of hkp_heat_peaks
and the labels.  A view of another size sees that pixel at
X_v = (X + 0.5) W_v / W - 0.5, the half-pixel rule of ops.resample_u8 and
ResamplePlan.apply_uv in "stretch" mode; a flip gives X_v <- W_v - 1 - X_v; the
view's lattice coordinate is X_v (w_v - 1) / (W_v - 1) (0 when w_v == 1).  The
composition is one (a, b) per axis, formed in float64 on the host; a view with the
base's image size and lattice gets exactly (1, 0), or (-1, w - 1) when flipped.
"""
import ctypes

import numpy as np
import torch

from ._lib import HKP_MERGE_LOGIT, HKP_MERGE_MAX_VIEWS, HKP_MERGE_PROB, HkpError, MergeView

MODES = {"logit": HKP_MERGE_LOGIT, "prob": HKP_MERGE_PROB}
TTA_KEYS = ("hflip", "vflip", "scales", "flip_pairs", "mode", "filter", "weights", "hvflip")
MIN_VIEW_SIDE = 32                 # a scaled view is never smaller than this (pixels)


def lattice_size(n):
    """Nodes of the stride-8 lattice along an axis of n pixels: three halvings, each
    rounding up (the stem conv, the max-pool and layer2's stride)."""
    n = int(n)
    for _ in range(3):
        n = (n + 1) // 2
    return n


def view_size(n, scale):
    """The side of a view of scale `scale` of an axis of n pixels: a multiple of 8,
    at least MIN_VIEW_SIDE; scale 1 is n itself."""
    if float(scale) == 1.0:
        return int(n)
    return max(MIN_VIEW_SIDE, 8 * int(round(float(scale) * int(n) / 8.0)))


def pixel_map(N, N_v, flip):
    """(g, c): base pixel X -> the view's pixel g X + c (float64)."""
    if int(N) == int(N_v):
        g, c = 1.0, 0.0
    else:
        g = float(N_v) / float(N)
        c = 0.5 * g - 0.5
    if flip:
        g, c = -g, float(N_v - 1) - c
    return g, c


def axis_map(N, n, N_v, n_v, flip):
    """(a, b): base lattice node j -> the view's lattice coordinate a j + b along one
    axis (float64); N, n the base's pixels and nodes, N_v, n_v the view's."""
    N, n, N_v, n_v = int(N), int(n), int(N_v), int(n_v)
    if N == N_v and n == n_v:                      # exact: a flip must stay a copy
        return (-1.0, float(n - 1)) if flip else (1.0, 0.0)
    step = float(N - 1) / float(n - 1) if n > 1 else 0.0          # pixels per base node
    back = float(n_v - 1) / float(N_v - 1) if n_v > 1 and N_v > 1 else 0.0
    g, c = pixel_map(N, N_v, flip)
    return step * g * back, c * back


class View:
    """One view: its scale, its flips and its image size."""
    __slots__ = ("scale", "hflip", "vflip", "hw")

    def __init__(self, scale, hflip, vflip, hw):
        self.scale, self.hflip, self.vflip, self.hw = float(scale), bool(hflip), bool(vflip), (int(hw[0]), int(hw[1]))

    @property
    def odd(self):
        """An odd number of flips: left / right landmarks change places."""
        return self.hflip != self.vflip

    def __repr__(self):
        return "View(scale=%g, hflip=%s, vflip=%s, hw=%s)" % (self.scale, self.hflip, self.vflip, self.hw)


class MergePlan:
    """The records of one hkp_logits_merge launch: n images, k channels, base lattice
    hw = (h, w) and per view (h_v, w_v, ay, by, ax, bx, weight); perm int [views, k].
    The views are packed in order, view v at element offset sum_{u<v} n k h_u w_u.
    Everything is validated here, on the host; device_arrays() uploads the table and
    perm once per device from pinned memory."""

    def __init__(self, n, k, hw, views, perm):
        n, k, h, w = int(n), int(k), int(hw[0]), int(hw[1])
        views = [tuple(v) for v in views]
        if min(n, k, h, w) < 1:
            raise HkpError("MergePlan: need n, k, h, w >= 1, got %s" % ((n, k, h, w),))
        if not 1 <= len(views) <= HKP_MERGE_MAX_VIEWS:
            raise HkpError("MergePlan: %d views outside 1..%d" % (len(views), HKP_MERGE_MAX_VIEWS))
        p = np.asarray(perm)
        if p.shape != (len(views), k) or not np.issubdtype(p.dtype, np.integer) or p.min() < 0 or p.max() >= k:
            raise HkpError("MergePlan: perm must be integers in 0..%d of shape %s" % (k - 1, (len(views), k)))
        self.n, self.k, self.hw, self.n_views = n, k, (h, w), len(views)
        self.perm = np.ascontiguousarray(p, dtype=np.int32)
        self.records = (MergeView * self.n_views)()
        self.lattices = []
        off = 0
        for r, v in zip(self.records, views):
            if len(v) != 7:
                raise HkpError("MergePlan: a view is (h_v, w_v, ay, by, ax, bx, weight), got %r" % (v,))
            hv, wv = int(v[0]), int(v[1])
            co = [float(c) for c in v[2:]]
            if hv < 1 or wv < 1 or not all(np.isfinite(co)):
                raise HkpError("MergePlan: need h_v, w_v >= 1 and finite coefficients, got %r" % (v,))
            r.off, r.h, r.w = off, hv, wv
            r.ay, r.by, r.ax, r.bx, r.weight = co
            self.lattices.append((hv, wv))
            off += n * k * hv * wv
        self.total = off
        self._dev = {}

    def record_bytes(self):
        """The records as a numpy uint8 view [views, 64] (shares memory)."""
        return np.frombuffer(self.records, dtype=np.uint8).reshape(self.n_views, ctypes.sizeof(MergeView))

    def coefficients(self):
        """float64 [views, 5]: (ay, by, ax, bx, weight) per view (a copy)."""
        return np.array([[r.ay, r.by, r.ax, r.bx, r.weight] for r in self.records], dtype=np.float64)

    def device_arrays(self, device):
        """(table, perm) on `device`, uploaded once from pinned memory."""
        device = torch.device(device)
        key = device.index if device.index is not None else torch.cuda.current_device()
        got = self._dev.get(key)
        if got is None:
            dev = torch.device("cuda", key)
            pin_t = torch.from_numpy(self.record_bytes().copy()).pin_memory()
            pin_p = torch.from_numpy(self.perm).pin_memory()
            got = (pin_t.to(dev, non_blocking=True), pin_p.to(dev, non_blocking=True), pin_t, pin_p)
            self._dev[key] = got
        return got[0], got[1]


class TestTimeAugmentation:
    """A set of views and how their logits are merged.

    hflip, vflip  add the mirrored views (left-right, up-down).  With both on, the
                  view mirrored both ways (a rotation by 180 degrees) is added only
                  with hvflip=True.
    scales        must hold 1.0.  A view of scale s has H_v = max(32, 8 round(s H / 8))
                  rows, W_v likewise; it is made with ops.resample_u8(filter=...), so
                  scales other than 1 need a uint8 NHWC batch.
    flip_pairs    keypoint classes that change places in a view with an odd number
                  of flips (left / right landmarks): WarpPlan's rule.
    mode          "prob": the logit of the weighted mean probability; "logit": the
                  weighted mean logit.
    weights       one per view in the order below, any positive scale; default
                  equal.  Normalised to sum 1 in float64.

    Order of the views: scale 1.0 first, then the other scales as given; within a
    scale: plain, hflip, vflip, hvflip (those that are on).  View 0 is always the
    input itself.  More than 8 views raises."""
    __test__ = False               # (not a test class, whatever the name says)

    def __init__(self, hflip=True, vflip=False, scales=(1.0,), flip_pairs=(), mode="prob", filter="bilinear",
                 weights=None, hvflip=False):
        from .resample import FILTERS
        if mode not in MODES:
            raise ValueError("TestTimeAugmentation: unknown mode %r (known: %s)" % (mode, ", ".join(MODES)))
        if filter not in FILTERS:
            raise ValueError("TestTimeAugmentation: unknown filter %r (known: %s)" % (filter, ", ".join(FILTERS)))
        scales = tuple(float(s) for s in scales)
        if 1.0 not in scales or len(set(scales)) != len(scales) or not all(np.isfinite(s) and s > 0 for s in scales):
            raise ValueError("TestTimeAugmentation: scales must be distinct, positive and hold 1.0 (view 0 is the "
                             "input itself), got %r" % (scales,))
        if hvflip and not (hflip and vflip):
            raise ValueError("TestTimeAugmentation: hvflip needs hflip and vflip")
        self.hflip, self.vflip, self.hvflip = bool(hflip), bool(vflip), bool(hvflip)
        self.scales = (1.0,) + tuple(s for s in scales if s != 1.0)
        self.flip_pairs = tuple((int(a), int(b)) for a, b in flip_pairs)
        self.mode, self.filter = mode, filter
        flips = [(False, False)] + [(True, False)] * self.hflip + [(False, True)] * self.vflip \
            + [(True, True)] * self.hvflip
        self._kinds = [(s, fh, fv) for s in self.scales for fh, fv in flips]
        if len(self._kinds) > HKP_MERGE_MAX_VIEWS:
            raise ValueError("TestTimeAugmentation: %d views, at most %d" % (len(self._kinds), HKP_MERGE_MAX_VIEWS))
        if weights is None:
            wts = np.ones(len(self._kinds), dtype=np.float64)
        else:
            wts = np.asarray(weights, dtype=np.float64).reshape(-1)
            if wts.size != len(self._kinds) or not np.all(np.isfinite(wts)) or np.any(wts < 0) or wts.sum() <= 0:
                raise ValueError("TestTimeAugmentation: weights: %d non-negative numbers with a positive sum, one "
                                 "per view, got %r" % (len(self._kinds), weights))
        self.weights = wts / wts.sum()
        self._plans = {}

    @property
    def n_views(self):
        return len(self._kinds)

    def views(self, H, W):
        """The views of an H x W input, in order."""
        return [View(s, fh, fv, (view_size(H, s), view_size(W, s))) for s, fh, fv in self._kinds]

    def perm(self, k):
        """int32 [views, k]: the channel of view v that feeds output channel c."""
        k = int(k)
        out = np.tile(np.arange(k, dtype=np.int32), (self.n_views, 1))
        for a, b in self.flip_pairs:
            if not (0 <= a < k and 0 <= b < k):
                raise ValueError("TestTimeAugmentation: flip pair (%d, %d) outside 0..%d" % (a, b, k - 1))
        for v, (_, fh, fv) in enumerate(self._kinds):
            if fh != fv:
                for a, b in self.flip_pairs:
                    out[v, [a, b]] = out[v, [b, a]]
        return out

    def plan(self, n, k, H, W, lattices=None, base=None):
        """The MergePlan of n images of k channels of an H x W input.  lattices: the
        (h_v, w_v) the network gave per view, default lattice_size of each view's
        size; base: the output lattice, default view 0's.  Cached."""
        views = self.views(H, W)
        lat = tuple((lattice_size(v.hw[0]), lattice_size(v.hw[1])) for v in views) if lattices is None \
            else tuple((int(a), int(b)) for a, b in lattices)
        if len(lat) != len(views):
            raise HkpError("TestTimeAugmentation: %d lattices for %d views" % (len(lat), len(views)))
        h, w = lat[0] if base is None else (int(base[0]), int(base[1]))
        key = (int(n), int(k), int(H), int(W), lat, (h, w))
        got = self._plans.get(key)
        if got is None:
            recs = []
            for v, (hv, wv), wt in zip(views, lat, self.weights):
                ay, by = axis_map(H, h, v.hw[0], hv, v.vflip)
                ax, bx = axis_map(W, w, v.hw[1], wv, v.hflip)
                recs.append((hv, wv, ay, by, ax, bx, float(wt)))
            got = self._plans[key] = MergePlan(n, k, (h, w), recs, self.perm(k))
        return got

    def check_input(self, x):
        """Raises, before anything is launched, for an input the views cannot be made of."""
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise ValueError("expected a [B,3,H,W] fp32 or [B,H,W,3] uint8 batch")
        if x.dtype != torch.uint8 and self.scales != (1.0,):
            raise HkpError("TestTimeAugmentation: scales %r need a uint8 NHWC batch (a scaled view goes through "
                           "ops.resample_u8); an fp32 batch takes scales=(1.0,) only" % (self.scales,))

    def view_inputs(self, x):
        """The input of every view, in order: x itself first.  A scaled view is
        resampled first (ops.resample_u8, once per scale) and mirrored after."""
        from . import ops
        self.check_input(x)
        u8 = x.dtype == torch.uint8
        H, W = (x.shape[1], x.shape[2]) if u8 else (x.shape[2], x.shape[3])
        ydim, xdim = (1, 2) if u8 else (2, 3)
        out, scaled = [], {}
        for v in self.views(H, W):
            if v.scale not in scaled:
                scaled[v.scale] = x if v.hw == (H, W) else ops.resample_u8(x, v.hw[0], v.hw[1], filter=self.filter)
            xv = scaled[v.scale]
            dims = [d for d, on in ((ydim, v.vflip), (xdim, v.hflip)) if on]
            out.append(torch.flip(xv, dims) if dims else xv)
        return out

    def merge(self, lows, H, W, out=None):
        """The views' logits (one [B,K,h_v,w_v] fp32 tensor per view, in order) merged
        on view 0's lattice: one launch, [B,K,h,w] fp32."""
        from . import ops
        if len(lows) != self.n_views:
            raise HkpError("TestTimeAugmentation.merge: %d tensors for %d views" % (len(lows), self.n_views))
        for t in lows:
            if not isinstance(t, torch.Tensor) or t.dim() != 4:
                raise HkpError("TestTimeAugmentation.merge: expected [B,K,h,w] tensors")
        n, k = lows[0].shape[:2]
        plan = self.plan(n, k, H, W, lattices=[tuple(t.shape[2:]) for t in lows])
        return ops.logits_merge(lows, plan, mode=self.mode, out=out)

    def run(self, x, forward, low0=None):
        """forward(x_v) -> low-res logits, once per view in order (view 0 is skipped
        when its logits are given as low0), then the merge."""
        xs = self.view_inputs(x)
        lows = [forward(xv) if (i or low0 is None) else low0 for i, xv in enumerate(xs)]
        u8 = x.dtype == torch.uint8
        H, W = (x.shape[1], x.shape[2]) if u8 else (x.shape[2], x.shape[3])
        return self.merge(lows, H, W)

    def __repr__(self):
        return "TestTimeAugmentation(%d views: hflip=%s vflip=%s hvflip=%s scales=%s mode=%s)" % (
            self.n_views, self.hflip, self.vflip, self.hvflip, self.scales, self.mode)


def from_config(cfg):
    """The "tta" entry of config.PEAKS / config.EVAL (None, a TestTimeAugmentation, or a
    dict of its keyword arguments) -> None or the object."""
    if cfg is None or isinstance(cfg, TestTimeAugmentation):
        return cfg
    if not isinstance(cfg, dict):
        raise ValueError("tta: expected a dict of TestTimeAugmentation's keyword arguments, got %r" % (cfg,))
    unknown = sorted(set(cfg) - set(TTA_KEYS))
    if unknown:
        raise ValueError("tta: unknown keys %s (known: %s)" % (unknown, ", ".join(TTA_KEYS)))
    return TestTimeAugmentation(**cfg)


def split_config(cfg):
    """config.PEAKS (None or a dict) -> (the dict without "tta", the
    TestTimeAugmentation its "tta" entry describes or None)."""
    if cfg is None:
        return None, None
    rest = dict(cfg)
    return rest, from_config(rest.pop("tta", None))
