"""numpy float64 restatement of the associative-embedding tags (include/hulkkp.h,
hkp_tag_loss and hkp_peaks_group): the lattice frame and the bilinear sample, the
pull / push loss, its closed-form gradient on the lattice, and the greedy grouping
of decoded peaks by tag — plain loops, by the definitions.

Conventions restated:
  * the tag map of class c is channel K + c of low_all [B,2K,h,w];
  * frame: x = u (w-1)/(W-1) (0 when W == 1 or w == 1), clamped to [0, w-1] (NaN -> 0),
    x0 = min(floor(x), w-2) (0 when w == 1), fx = x - x0, x1 = min(x0+1, w-1); y likewise;
  * sample: top = (1-fx) t[y0,x0] + fx t[y0,x1], bot likewise on y1, (1-fy) top + fy bot;
  * a slot takes part when flag > 0 and 0 <= gid < 32; other slots are never read.
"""
import math

import numpy as np

MAX_GROUPS = 32


def tap(u, w, W):
    """(x0, fx) of pixel coordinate u on a w-node lattice under a W-pixel picture."""
    x = float(np.float64(np.float32(u)) * np.float64(w - 1) / np.float64(W - 1)) if (W > 1 and w > 1) else 0.0
    x = x if x > 0.0 else 0.0
    hi = float(w - 1)
    x = x if x < hi else hi
    x0 = min(int(math.floor(x)), w - 2) if w > 1 else 0
    return x0, x - x0


def sample(plane, u, v, H, W):
    """fp64 bilinear value of the fp32 [h,w] plane at pixel (u, v), and its taps
    [(y, x, weight)] in the order 00, 01, 10, 11."""
    h, w = plane.shape
    x0, fx = tap(u, w, W)
    y0, fy = tap(v, h, H)
    x1, y1 = min(x0 + 1, w - 1), min(y0 + 1, h - 1)
    p = plane.astype(np.float64)
    top = (1.0 - fx) * p[y0, x0] + fx * p[y0, x1]
    bot = (1.0 - fx) * p[y1, x0] + fx * p[y1, x1]
    val = (1.0 - fy) * top + fy * bot
    taps = [(y0, x0, (1.0 - fy) * (1.0 - fx)), (y0, x1, (1.0 - fy) * fx), (y1, x0, fy * (1.0 - fx)), (y1, x1, fy * fx)]
    return val, taps


def image_loss(t, g):
    """(pull, push, dpull/dt, dpush/dt) of one image from the participating points'
    tags t (float64 [P]) and group ids g (int [P]), by the closed form."""
    t = np.asarray(t, np.float64)
    g = np.asarray(g)
    ids = sorted(set(int(v) for v in g))
    G = len(ids)
    dpull, dpush = np.zeros_like(t), np.zeros_like(t)
    if G == 0:
        return 0.0, 0.0, dpull, dpush
    mu = {q: t[g == q].sum() / (g == q).sum() for q in ids}
    n = {q: int((g == q).sum()) for q in ids}
    pull = 0.0
    for q in ids:
        pull += ((t[g == q] - mu[q]) ** 2).sum() / n[q]
    pull /= G
    push = 0.0
    dmu = {q: 0.0 for q in ids}
    if G >= 2:
        for a in ids:
            for b in ids:
                if a != b:
                    d = mu[a] - mu[b]
                    e = math.exp(-(d * d) * 0.5)
                    push += e
                    dmu[a] += d * e
        push /= G * (G - 1)
        for q in ids:
            dmu[q] *= -2.0 / (G * (G - 1))
    for i in range(len(t)):
        q = int(g[i])
        dpull[i] = 2.0 * (t[i] - mu[q]) / (G * n[q])
        dpush[i] = dmu[q] / n[q]
    return float(pull), float(push), dpull, dpush


def tag_loss(tags, pts, gid, H, W, scale=1.0, pull=1.0, push=1.0):
    """tags float32 [B,K,h,w] (the tag planes), pts [B,K,M,3], gid [B,K,M] ->
    (out float64 [3] = (total, mean pull, mean push), dtag float64 [B,K,h,w] =
    scale * d total / d tags).  scale, pull and push as their float32 values."""
    tags = np.asarray(tags, np.float32)
    B, K, h, w = tags.shape
    M = pts.shape[2]
    scale, pull, push = (float(np.float32(v)) for v in (scale, pull, push))
    out = np.zeros(3)
    dtag = np.zeros((B, K, h, w))
    for b in range(B):
        ts, gs, taps = [], [], []
        for c in range(K):
            for m in range(M):
                q = int(gid[b, c, m])
                if pts[b, c, m, 2] > 0 and 0 <= q < MAX_GROUPS:
                    val, tp = sample(tags[b, c], pts[b, c, m, 0], pts[b, c, m, 1], H, W)
                    ts.append(val), gs.append(q), taps.append((c, tp))
        pl, ps, dpl, dps = image_loss(ts, gs)
        out += (pull * pl + push * ps, pl, ps)
        for i, (c, tp) in enumerate(taps):
            cf = (scale / B) * (pull * dpl[i] + push * dps[i])
            for (y, x, wt) in tp:
                dtag[b, c, y, x] += cf * wt
    return out / B, dtag


def peaks_group(peaks, counts, tags, H, W, order, max_dist=1.0):
    """peaks float32 [B,K,P,3], counts [B,K], tags float32 [B,K,h,w] ->
    (group int32 [B,K,P], tag float32 [B,K,P], ngroups int32 [B])."""
    tags = np.asarray(tags, np.float32)
    B, K, P = peaks.shape[:3]
    group = np.full((B, K, P), -1, np.int32)
    tag = np.zeros((B, K, P), np.float32)
    ngroups = np.zeros(B, np.int32)
    md = float(np.float32(max_dist))
    for b in range(B):
        cnt = [min(max(int(counts[b, c]), 0), P) for c in range(K)]
        for c in range(K):
            for j in range(cnt[c]):
                tag[b, c, j] = np.float32(sample(tags[b, c], peaks[b, c, j, 0], peaks[b, c, j, 1], H, W)[0])
        sums, ns, has = [], [], []            # per group: fp64 sum, count, classes held
        for c in order:
            for j in range(cnt[c]):
                t = float(tag[b, c, j])
                best, best_d = -1, math.inf
                for q in range(len(sums)):
                    if c in has[q]:
                        continue
                    d = abs(t - sums[q] / ns[q])
                    if d < best_d:            # a NaN never is; equal goes to the lower id
                        best, best_d = q, d
                if best >= 0 and best_d <= md:
                    sums[best] += t
                    ns[best] += 1
                    has[best].add(c)
                else:
                    best = len(sums)
                    sums.append(t), ns.append(1), has.append({c})
                group[b, c, j] = best
        ngroups[b] = len(sums)
    return group, tag, ngroups


# ---- hand cases of the grouping, shared by the CPU test (the restatement against the written-out
# answers) and the GPU test (the kernel against both): peaks on the nodes of a lattice with
# H = 8(h-1)+1, W = 8(w-1)+1, tags multiples of 2^-4, so every sample and every mean is exact

def node_case(K, P, h, w, B=1):
    H, W = 8 * (h - 1) + 1, 8 * (w - 1) + 1
    tags = np.zeros((B, K, h, w), np.float32)
    peaks = np.full((B, K, P, 3), -1, np.float32)
    peaks[..., 2] = 0
    counts = np.zeros((B, K), np.int32)
    return tags, peaks, counts, H, W


def put(tags, peaks, counts, b, c, node, t):
    """The next peak of plane (b, c) on lattice node (i, j) with tag t."""
    i, j = node
    s = counts[b, c]
    tags[b, c, i, j] = t
    peaks[b, c, s] = (8 * j, 8 * i, 0.9 - 0.1 * s)
    counts[b, c] = s + 1


def hand_cases():
    """name -> (tags, peaks, counts, H, W, order, max_dist, expected group, expected ngroups)."""
    out = {}
    # two cables whose slot order disagrees with their tags
    a = node_case(2, 2, 3, 4)
    put(*a[:3], 0, 0, (0, 0), 1.0), put(*a[:3], 0, 0, (1, 1), 3.0)
    put(*a[:3], 0, 1, (2, 2), 3.0625), put(*a[:3], 0, 1, (0, 3), 0.9375)
    out["crossed"] = a + ((0, 1), 1.0, [[[0, 1], [1, 0]]], [2])
    # a distance exactly max_dist joins, one step of 2^-4 above does not
    a = node_case(2, 2, 3, 4)
    put(*a[:3], 0, 0, (0, 0), 1.0), put(*a[:3], 0, 1, (1, 1), 1.5)
    out["at_max_dist"] = a + ((0, 1), 0.5, [[[0, -1], [0, -1]]], [1])
    a = node_case(2, 2, 3, 4)
    put(*a[:3], 0, 0, (0, 0), 1.0), put(*a[:3], 0, 1, (1, 1), 1.5625)
    out["above_max_dist"] = a + ((0, 1), 0.5, [[[0, -1], [1, -1]]], [2])
    # a tie goes to the lower group
    a = node_case(2, 2, 3, 4)
    put(*a[:3], 0, 0, (0, 0), 1.0), put(*a[:3], 0, 0, (2, 2), 2.0), put(*a[:3], 0, 1, (1, 1), 1.5)
    out["tie"] = a + ((0, 1), 1.0, [[[0, 1], [0, -1]]], [2])
    # two tails near one cap: the second opens a group
    a = node_case(2, 2, 3, 4)
    put(*a[:3], 0, 0, (0, 0), 1.0), put(*a[:3], 0, 1, (1, 1), 1.0625), put(*a[:3], 0, 1, (2, 3), 0.9375)
    out["two_tails"] = a + ((0, 1), 1.0, [[[0, -1], [0, 1]]], [2])
    # Q = 3: the running mean decides the third member (group 0's mean moves from 0 to 0.5)
    a = node_case(3, 2, 3, 4)
    put(*a[:3], 0, 0, (0, 0), 0.0), put(*a[:3], 0, 0, (0, 2), 2.0)
    put(*a[:3], 0, 1, (1, 0), 1.0), put(*a[:3], 0, 2, (2, 0), 1.125)
    # class 1: |1-0| = |1-2| -> group 0 (mean 0.5); class 2: |1.125-0.5| = 0.625 < |1.125-2| = 0.875 -> group 0
    # (against group 0's first member alone it would be 1.125 > 0.875: group 1)
    out["running_mean"] = a + ((0, 1, 2), 1.0, [[[0, 1], [0, -1], [0, -1]]], [2])
    # counts of -1 and P + 3; a class outside order
    a = node_case(3, 2, 3, 4)
    put(*a[:3], 0, 0, (0, 0), 1.0), put(*a[:3], 0, 0, (1, 1), 5.0)
    put(*a[:3], 0, 1, (2, 2), 1.0), put(*a[:3], 0, 2, (0, 3), 5.0)
    a[2][0, 0], a[2][0, 1] = 5, -1
    out["counts_clamped"] = a + ((0, 1), 1.0, [[[0, 1], [-1, -1], [-1, -1]]], [2])
    # a NaN tag opens a group nobody joins
    a = node_case(2, 2, 3, 4)
    put(*a[:3], 0, 0, (0, 0), np.nan), put(*a[:3], 0, 0, (1, 1), 1.0)
    put(*a[:3], 0, 1, (2, 2), 1.0), put(*a[:3], 0, 1, (0, 3), np.nan)
    out["nan"] = a + ((0, 1), 1.0, [[[0, 1], [1, 2]]], [3])
    return out
