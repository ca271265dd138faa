"""Line labels: a heatmap class trained against a polyline (a cable's centreline).

Labels are lines float32 [N,K,S,5], last axis (x0, y0, x1, y1, flag), 1 <= S <= 128, in
the frame of pts (x the column, y the row, integers pixel centres).  flag > 0 marks a
present segment; anything else is an empty slot whose coordinates are never read.  A point
is a zero-length segment, so a plane may mix both.  ops.line_target (hkp_line_target,
csrc/lines.hip; include/hulkkp.h is the definition) turns them into the dense target and
the squared distance to the nearest segment.
"""

import numpy as np
import torch

from ._lib import HKP_LINE_MAX_S, HkpError


def from_points(pts):
    """Instance labels pts [N,K,M,3] (u, v, flag) as zero-length segments [N,K,M,5] =
    (u, v, u, v, flag), on the device of pts, without a synchronisation."""
    if not isinstance(pts, torch.Tensor) or pts.dim() != 4 or pts.shape[3] != 3:
        raise HkpError("from_points: expected a tensor [N,K,M,3], got %s"
                       % (tuple(pts.shape) if isinstance(pts, torch.Tensor) else type(pts).__name__,))
    return torch.cat([pts[..., 0:2], pts[..., 0:2], pts[..., 2:3]], -1).contiguous()


def from_polylines(polys, S):
    """One image's line labels float32 [K,S,5] (numpy) from a list per class of float [n,2]
    vertex arrays (a class may hold several polylines, or none): the pieces of each
    polyline, vertex pair by vertex pair, in list order; a polyline of one vertex is a
    point.  Raises when a class has more than S pieces."""
    S = int(S)
    if not 1 <= S <= HKP_LINE_MAX_S:
        raise HkpError("from_polylines: S = %d outside 1..%d" % (S, HKP_LINE_MAX_S))
    out = np.zeros((len(polys), S, 5), dtype=np.float32)
    for k, cls in enumerate(polys):
        at = 0
        for poly in cls:
            v = np.asarray(poly, dtype=np.float64)
            if v.ndim != 2 or v.shape[1] != 2 or v.shape[0] < 1:
                raise HkpError("from_polylines: a polyline is float [n,2] with n >= 1, got %s" % (v.shape,))
            a, b = (v, v) if len(v) == 1 else (v[:-1], v[1:])
            if at + len(a) > S:
                raise HkpError("from_polylines: class %d has more than S = %d pieces" % (k, S))
            out[k, at:at + len(a), 0:2], out[k, at:at + len(a), 2:4], out[k, at:at + len(a), 4] = a, b, 1.0
            at += len(a)
    return out


def concat(a, b):
    """Two sets of line labels [N,K,Sa,5] and [N,K,Sb,5] as one, [N,K,Sa+Sb,5]."""
    for t in (a, b):
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[3] != 5:
            raise HkpError("concat: expected tensors [N,K,S,5]")
    if a.shape[:2] != b.shape[:2] or a.device != b.device or a.dtype != b.dtype:
        raise HkpError("concat: %s (%s, %s) does not go with %s (%s, %s)"
                       % (tuple(a.shape), a.dtype, a.device, tuple(b.shape), b.dtype, b.device))
    if a.shape[2] + b.shape[2] > HKP_LINE_MAX_S:
        raise HkpError("concat: %d + %d slots exceed %d" % (a.shape[2], b.shape[2], HKP_LINE_MAX_S))
    return torch.cat([a, b], 2).contiguous()


class LineMetrics:
    """How well a heatmap covers a centreline, per class, over the pixels of a batch:
    with P = (heat >= threshold) and G = (distance to the nearest segment <= radius),
        completeness = |P and G| / |G|     correctness = |P and G| / |P|
        iou          = |P and G| / |P or G|
    The counts are int64 on the device; update() makes no host read, compute() one."""

    def __init__(self, num_keypoints, radius=4.0, threshold=0.5):
        if int(num_keypoints) < 1 or not float(radius) >= 0 or not 0 < float(threshold) <= 1:
            raise HkpError("LineMetrics: bad num_keypoints %r, radius %r or threshold %r"
                           % (num_keypoints, radius, threshold))
        self.k, self.radius, self.threshold = int(num_keypoints), float(radius), float(threshold)
        self.counts = None

    def reset(self):
        self.counts = None

    def update(self, heat, lines):
        """heat float [N,K,H,W] and lines float32 [N,K,S,5], on the GPU."""
        from . import ops
        if not isinstance(heat, torch.Tensor) or heat.dim() != 4 or heat.shape[1] != self.k:
            raise HkpError("LineMetrics.update: expected heat [N,%d,H,W]" % self.k)
        _, d2 = ops.line_target(lines, heat.shape[2], heat.shape[3], want_target=False, want_d2=True)
        if d2.shape != heat.shape:
            raise HkpError("LineMetrics.update: lines %s do not go with heat %s" % (tuple(lines.shape), tuple(heat.shape)))
        p = heat >= self.threshold
        g = d2 <= float(np.float32(self.radius) * np.float32(self.radius))
        c = torch.stack([(p & g).sum((0, 2, 3)), p.sum((0, 2, 3)), g.sum((0, 2, 3))], 1)
        self.counts = c if self.counts is None else self.counts + c

    def compute(self):
        """A list of dicts, one per class: completeness, correctness, iou (nan over 0) and the
        counts hit (P and G), pred (P), line (G)."""
        c = np.zeros((self.k, 3), dtype=np.int64) if self.counts is None else self.counts.cpu().numpy()
        nan = float("nan")
        out = []
        for hit, pred, line in c.tolist():
            union = pred + line - hit
            out.append({"completeness": hit / line if line else nan, "correctness": hit / pred if pred else nan,
                        "iou": hit / union if union else nan, "hit": hit, "pred": pred, "line": line})
        return out
