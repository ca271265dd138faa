"""Numpy restatement of hkp_synth_cables_u8 (include/hulkkp.h is the definition): a
SynthPlan's records -> uint8 [B,H,W,3], in int64, over whole images (no tiles, no
cull: every piece is evaluated on every pixel).  Also the float64 helpers of the CPU
tests: distance to a polyline and segment intersection, written independently of
hkp/synth.py (plain loops)."""
import math

import numpy as np

M32 = 0xFFFFFFFF


def philox_x0(c0, c1, c2, k0, k1):
    """First word of Philox4x32-10 at counter (c0, c1, c2, 0); uint64 arrays / ints."""
    c0 = np.asarray(c0, dtype=np.uint64)
    c1 = np.asarray(c1, dtype=np.uint64) + np.zeros_like(c0)
    c2 = np.asarray(c2, dtype=np.uint64) + np.zeros_like(c0)
    c3 = np.zeros_like(c0)
    k0, k1 = int(k0), int(k1)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(M32)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(M32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0


def noise_octave(h, w, sh, octave, key):
    """n_o [h, w] int64 of one octave: bilinear Q8 between the hashed lattice values."""
    x, y = np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64)
    m = (1 << sh) - 1
    ix, iy = x >> sh, y >> sh
    fx, fy = ((x & m) << 8) >> sh, (((y & m) << 8) >> sh)[:, None]
    gx, gy = np.arange(ix.max() + 2), np.arange(iy.max() + 2)
    cx, cy = np.meshgrid(gx, gy)                           # [len(gy), len(gx)]: v[j, i] = v(i, j)
    v = (philox_x0(cx, cy, octave, key[0], key[1]) & np.uint64(255)).astype(np.int64)
    v00, v01 = v[iy][:, ix], v[iy][:, ix + 1]
    v10, v11 = v[iy + 1][:, ix], v[iy + 1][:, ix + 1]
    top = v00 * (256 - fx) + v01 * fx
    bot = v10 * (256 - fx) + v11 * fx
    return (top * (256 - fy) + bot * fy + 32768) >> 16


def background(h, w, sc):
    n0 = noise_octave(h, w, sc.cell_log2, 0, sc.key)
    n1 = noise_octave(h, w, sc.cell_log2 - 1, 1, sc.key)
    n = (3 * n0 + n1 + 2) >> 2
    out = np.empty((h, w, 3), dtype=np.int64)
    for c in range(3):
        out[:, :, c] = int(sc.bg0[c]) + (((int(sc.bg1[c]) - int(sc.bg0[c])) * n + 128) >> 8)
    return out


def piece_alpha_d2(s, h, w):
    """(alpha, d2) int64 [h, w] of piece record s on every pixel."""
    ax = (np.arange(w, dtype=np.int64) * 16 - s.x0)[None, :] + np.zeros((h, 1), dtype=np.int64)
    ay = (np.arange(h, dtype=np.int64) * 16 - s.y0)[:, None] + np.zeros((1, w), dtype=np.int64)
    t = np.clip((ax * s.ux + ay * s.uy) >> 14, 0, s.len)
    cx, cy = ax - ((t * s.ux) >> 14), ay - ((t * s.uy) >> 14)
    d2 = cx * cx + cy * cy
    alpha = np.where(d2 <= s.r_in2, 256, np.where(d2 >= s.r_out2, 0, ((s.r_out2 - d2) * int(s.inv)) >> 24))
    return alpha, d2


def alpha_of_d2(s, d2):
    """The blended alpha of piece record s at squared distances d2 (Q8)."""
    d2 = np.asarray(d2, dtype=np.int64)
    return np.where(d2 <= s.r_in2, 256, np.where(d2 >= s.r_out2, 0, ((s.r_out2 - d2) * int(s.inv)) >> 24))


def render(plan):
    """uint8 [B,H,W,3] of a SynthPlan."""
    h, w = plan.hw
    out = np.empty((plan.n, h, w, 3), dtype=np.uint8)
    for b in range(plan.n):
        sc = plan.scenes[b]
        o = background(h, w, sc)
        run_arc = np.full((h, w), -1, dtype=np.int64)
        run_last = np.full((h, w), -2, dtype=np.int64)
        run_a = np.zeros((h, w), dtype=np.int64)
        run_d2 = np.zeros((h, w), dtype=np.int64)
        run_c = np.zeros((h, w, 3), dtype=np.int64)
        for i in range(sc.seg_cnt):
            s = plan.segs[sc.seg_off + i]
            alpha, d2 = piece_alpha_d2(s, h, w)
            cov = alpha > 0
            if not cov.any():
                continue
            lum = 256 - ((s.shade * ((np.minimum(d2, s.r2) * int(s.inv_r2)) >> 24)) >> 8)
            ends = cov & ~((run_arc == s.arc) & (run_last == i - 1))
            for c in range(3):
                o[:, :, c] = np.where(ends, (run_c[:, :, c] * run_a + o[:, :, c] * (256 - run_a) + 128) >> 8, o[:, :, c])
            run_a = np.where(ends, 0, run_a)
            run_arc = np.where(ends, s.arc, run_arc)
            run_last = np.where(cov, i, run_last)
            take = cov & ((alpha > run_a) | ((alpha == run_a) & (d2 <= run_d2)))
            run_a = np.where(take, alpha, run_a)
            run_d2 = np.where(take, d2, run_d2)
            for c in range(3):
                run_c[:, :, c] = np.where(take, (int(s.bgr[c]) * lum + 128) >> 8, run_c[:, :, c])
        for c in range(3):
            o[:, :, c] = (run_c[:, :, c] * run_a + o[:, :, c] * (256 - run_a) + 128) >> 8
        assert o.min() >= 0 and o.max() <= 255
        out[b] = o.astype(np.uint8)
    return out


# ------------------------------------------------------ float64 helpers ----
def dist_point_segment(p, a, b):
    dx, dy = b[0] - a[0], b[1] - a[1]
    l2 = dx * dx + dy * dy
    t = 0.0 if l2 == 0 else min(1.0, max(0.0, ((p[0] - a[0]) * dx + (p[1] - a[1]) * dy) / l2))
    return math.hypot(a[0] + t * dx - p[0], a[1] + t * dy - p[1])


def dist_to_polyline(p, poly, first=0, last=None):
    """Distance of p to pieces first .. last - 1 of polyline poly [n, 2] (inf: no piece)."""
    n = len(poly) - 1
    last = n if last is None else last
    return min([dist_point_segment(p, poly[i], poly[i + 1]) for i in range(first, last)], default=math.inf)


def segment_intersection(a0, a1, b0, b1):
    """The intersection of the half-open pieces [a0, a1) and [b0, b1), or None."""
    rx, ry, sx, sy = a1[0] - a0[0], a1[1] - a0[1], b1[0] - b0[0], b1[1] - b0[1]
    den = rx * sy - ry * sx
    if den == 0:
        return None
    wx, wy = b0[0] - a0[0], b0[1] - a0[1]
    t, u = (wx * sy - wy * sx) / den, (wx * ry - wy * rx) / den
    if 0 <= t < 1 and 0 <= u < 1:
        return (a0[0] + t * rx, a0[1] + t * ry)
    return None


def brute_crossings(polys):
    """Every intersection of the centrelines, pieces next to each other on one polyline
    (and a piece with itself) excluded: list of ((x, y), angle in degrees 0..90)."""
    segs = [(k, i, p[i], p[i + 1]) for k, p in enumerate(polys) for i in range(len(p) - 1)]
    out = []
    for m in range(len(segs)):
        for n in range(m + 1, len(segs)):
            ka, ia, a0, a1 = segs[m]
            kb, ib, b0, b1 = segs[n]
            if ka == kb and abs(ia - ib) <= 1:
                continue
            x = segment_intersection(a0, a1, b0, b1)
            if x is not None:
                da, db = (a1[0] - a0[0], a1[1] - a0[1]), (b1[0] - b0[0], b1[1] - b0[1])
                cos = abs(da[0] * db[0] + da[1] * db[1]) / (math.hypot(*da) * math.hypot(*db))
                out.append((x, math.degrees(math.acos(min(1.0, cos)))))
    return out
