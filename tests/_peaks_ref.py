"""numpy restatement of hkp_heat_peaks (include/hulkkp.h): the multi-peak decode
of the low-res logits, by its definition.

Per plane z[h][w] (fp32), output size H x W, radius r, max_peaks P, threshold t:
  order       NaN counts as -inf, -0 as +0; node a beats node b if z[a] > z[b], or
              z[a] == z[b] and a has the smaller linear index i*w + j.
  candidates  z > -inf, score = sigmoid(z) (fp32) >= t, and the node beats every
              other node of its (2r+1)^2 window clipped to the plane.
  selection   the P best candidates in that order; counts = how many were written;
              unused slots hold (-1, -1, 0).
  refinement  per axis in fp64 from the fp32 logits, g(z) = min(z,0) - log1p(exp(-|z|)):
              both neighbours inside the plane, all three g finite and
              den = 2 g0 - g- - g+ > 1e-6 -> d = clamp(0.5 (g+ - g-)/den, -0.5, 0.5),
              else 0; x = (j + dx)(W-1)/(w-1) (0 when w == 1), y likewise; rounded
              once to fp32.
  output      peaks [n][k][P][3] = (x, y, score) fp32, counts [n][k] int32.
"""
import numpy as np

DEN_MIN = 1e-6


def sigmoid_f32(z):
    """1 / (1 + exp(-z)) in fp32 (the kernel's sigmoid_f up to the last bit of expf)."""
    z = np.asarray(z, dtype=np.float32)
    with np.errstate(over="ignore"):
        return (np.float32(1) / (np.float32(1) + np.exp(-z, dtype=np.float32))).astype(np.float32)


def canonical(z):
    z = np.array(z, dtype=np.float32)
    z[np.isnan(z)] = -np.inf
    z[z == 0] = 0.0
    return z


def log_sigmoid(z):
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.minimum(z, 0.0) - np.log1p(np.exp(-np.abs(z)))


def window_maxima(z, r):
    """bool [h][w]: the node beats every other node of its clipped window (z canonical)."""
    h, w = z.shape
    pad = np.full((h + 2 * r, w + 2 * r), -np.inf, dtype=np.float32)
    pad[r:r + h, r:r + w] = z
    ok = z > -np.inf
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dy == 0 and dx == 0:
                continue
            zb = pad[r + dy:r + dy + h, r + dx:r + dx + w]
            first = dy < 0 or (dy == 0 and dx < 0)           # the neighbour has the smaller linear index
            ok &= ~((zb > z) | ((zb == z) & first))
    return ok


def axis_offset(gm, g0, gp, dens=None):
    if not (np.isfinite(gm) and np.isfinite(g0) and np.isfinite(gp)):
        return 0.0
    den = 2.0 * g0 - gm - gp
    if dens is not None:
        dens.append(float(den))
    if not den > DEN_MIN:
        return 0.0
    return float(min(max(0.5 * (gp - gm) / den, -0.5), 0.5))


def plane_peaks(z, H, W, max_peaks=4, radius=1, threshold=0.0, scores=None, dens=None, picked=None):
    """One plane -> (peaks float32 [P][3], count).  scores: the fp32 sigmoid of every
    node (default: sigmoid_f32 here); dens: a list that receives every den computed;
    picked: a list that receives the node (i, j) of every peak written."""
    z = canonical(z)
    h, w = z.shape
    scores = sigmoid_f32(z) if scores is None else np.asarray(scores, dtype=np.float32)
    cand = window_maxima(z, radius) & (scores >= np.float32(threshold))
    idx = np.flatnonzero(cand.ravel())
    zz = z.ravel()[idx]
    order = idx[np.lexsort((idx, -zz.astype(np.float64)))]     # by value descending, then index ascending
    out = np.zeros((max_peaks, 3), dtype=np.float32)
    out[:, :2] = -1
    g = log_sigmoid(z)
    count = min(len(order), max_peaks)
    for p in range(count):
        i, j = divmod(int(order[p]), w)
        if picked is not None:
            picked.append((i, j))
        dx = axis_offset(g[i, j - 1], g[i, j], g[i, j + 1], dens) if 0 < j < w - 1 else 0.0
        dy = axis_offset(g[i - 1, j], g[i, j], g[i + 1, j], dens) if 0 < i < h - 1 else 0.0
        x = (j + dx) * (W - 1) / (w - 1) if w > 1 else 0.0
        y = (i + dy) * (H - 1) / (h - 1) if h > 1 else 0.0
        out[p] = (np.float32(x), np.float32(y), scores[i, j])
    return out, count


def heat_peaks(low, H, W, max_peaks=4, radius=1, threshold=0.0, scores=None, dens=None, picked=None):
    """low [n][k][h][w] fp32 -> (peaks float32 [n][k][P][3], counts int32 [n][k]).
    picked: a dict that receives {(n, k): [(i, j), ...]}, the nodes of the peaks."""
    low = np.asarray(low, dtype=np.float32)
    n, k = low.shape[:2]
    peaks = np.zeros((n, k, max_peaks, 3), dtype=np.float32)
    counts = np.zeros((n, k), dtype=np.int32)
    for a in range(n):
        for b in range(k):
            got = [] if picked is not None else None
            peaks[a, b], counts[a, b] = plane_peaks(low[a, b], H, W, max_peaks, radius, threshold,
                                                    None if scores is None else scores[a, b], dens, got)
            if picked is not None:
                picked[(a, b)] = got
    return peaks, counts
