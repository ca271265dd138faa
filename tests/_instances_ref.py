"""numpy restatement of the multi-instance target and loss (include/hulkkp.h:
hkp_gauss_target_multi, hkp_heat_loss_multi), by their definition.

  labels   pts [n][k][m][3] fp32 = (u, v, flag); flag > 0: the slot holds an instance,
           anything else: the slot is empty and its (u, v) are never read.
  target   t[n][k][y][x] = max over the present slots of
           (double) exp_f32( -((x-u)^2 + (y-v)^2) / den ), den = (float)(2 sigma^2),
           every step rounded to fp32 in that order; 0 for a plane without a slot.
           (numpy's fp32 exp may differ from the device's expf in the last place, so
           this pins the rule, not the kernel's bits: the GPU tests hold the kernel to
           the existing hkp_gauss_target for those.)
  loss     BCE  l = (y-1) max(log1p(-p), -100) - y max(log p, -100)
           MSE  l = (p-y)^2
           "zero":   every plane counts, the divisor is n*k*H*W
           "ignore": planes without a present slot contribute nothing, the divisor is
                     H*W*A (A = planes with a slot); A = 0 gives 0
  gradient BCE  g = (p-y) / max((1-p) p, (double)1e-12f) / N,  MSE  g = 2 (p-y) / N,
           rounded to fp32; +0 on ignored planes.
"""
import numpy as np

EPS = float(np.float32(1e-12))


def present(pts):
    """bool [n][k][m]: the slot holds an instance (a NaN flag does not)."""
    with np.errstate(invalid="ignore"):
        return np.asarray(pts)[..., 2] > 0


def active_planes(pts):
    """bool [n][k]: the plane has a present slot."""
    return present(pts).any(-1)


def gauss_target_multi(pts, H, W, sigma):
    pts = np.asarray(pts, dtype=np.float32)
    n, k, m, _ = pts.shape
    f = np.float32
    den = f(2.0 * float(sigma) * float(sigma))
    xs, ys = np.arange(W, dtype=f)[None, :], np.arange(H, dtype=f)[:, None]
    on = present(pts)
    out = np.zeros((n, k, H, W), dtype=np.float64)
    for a in range(n):
        for b in range(k):
            t = np.zeros((H, W), dtype=f)
            for j in range(m):
                if not on[a, b, j]:
                    continue                                  # selected on the flag: (u, v) are not touched
                dx, dy = (xs - pts[a, b, j, 0]).astype(f), (ys - pts[a, b, j, 1]).astype(f)
                d2 = ((dx * dx).astype(f) + (dy * dy).astype(f)).astype(f)
                with np.errstate(under="ignore"):
                    t = np.maximum(t, np.exp((-d2 / den).astype(f), dtype=f))
            out[a, b] = t.astype(np.float64)
    return out


# ---- the round trip with the multi-peak decode: a 9 x 11 lattice under a 65 x 81 image,
# so lattice node j sits on pixel 8 j.  Planes with 0, 1, 2 and 3 instances, every one off
# the nodes, at least 3 cells (24 px) from the others, and at least 3 cells from the border
# — except in the 3-instance plane, where 2 cells (16 px) have to do: the nodes 3 cells
# inside a 9 x 11 lattice span 2 x 4 cells, which cannot hold three points 3 cells apart.
# (The parabola fit reads one neighbour node on each side, so 2 cells leave a node to spare.)
RT_LATTICE, RT_IMAGE, RT_SIGMA = (9, 11), (65, 81), 8.0
RT_POINTS = [[],
             [(43.3, 29.6)],
             [(25.7, 37.2), (54.9, 27.4)],
             [(17.3, 18.6), (62.4, 19.7), (41.9, 46.3)]]


def roundtrip_pts():
    """pts float32 [1][4][4][3] of RT_POINTS, the present slots not packed; empty ones hold NaN."""
    pts = np.full((1, 4, 4, 3), np.nan, dtype=np.float32)
    pts[..., 2] = 0.0
    slots = [[], [2], [0, 3], [1, 2, 3]]
    for k, (inst, where) in enumerate(zip(RT_POINTS, slots)):
        for (u, v), j in zip(inst, where):
            pts[0, k, j] = (u, v, 1.0)
    return pts


def lowres_logits(target):
    """fp32 logits of the target at the lattice nodes (every 8th pixel), clamped to
    finite as tests/test_peaks_cpu.py's ideal_logits clamps."""
    t = np.clip(np.asarray(target, dtype=np.float64)[..., ::8, ::8], 1e-30, 1.0 - 2.0 ** -24)
    return (np.log(t) - np.log1p(-t)).astype(np.float32)


def roundtrip_errors(peaks, counts):
    """Per plane: (count returned, count wanted, the largest distance in pixels from an
    instance to its nearest returned peak; 0 without instances)."""
    out = []
    for k, inst in enumerate(RT_POINTS):
        c = int(counts[0, k])
        got = np.asarray(peaks[0, k, :c, :2], dtype=np.float64)
        worst = 0.0
        for u, v in inst:
            u, v = float(np.float32(u)), float(np.float32(v))       # the labels are fp32
            d = np.hypot(got[:, 0] - u, got[:, 1] - v) if c else np.array([np.inf])
            worst = max(worst, float(d.min()))
        out.append((c, len(inst), worst))
    return out


def heat_loss_multi(p, pts, sigma, kind="bce", absent="zero"):
    """(loss float64, dheat float32 [n][k][H][W])."""
    assert kind in ("bce", "mse") and absent in ("zero", "ignore")
    p32 = np.asarray(p, dtype=np.float32)
    n, k, H, W = p32.shape
    y = gauss_target_multi(pts, H, W, sigma)
    x = p32.astype(np.float64)
    act = active_planes(pts) if absent == "ignore" else np.ones((n, k), dtype=bool)
    A = int(act.sum())
    if A == 0:
        return 0.0, np.zeros(p32.shape, dtype=np.float32)
    inv_n = 1.0 / float(H * W * A)
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == "bce":
            l = (y - 1.0) * np.maximum(np.log1p(-x), -100.0) - y * np.maximum(np.log(x), -100.0)
            g = (x - y) / np.maximum((1.0 - x) * x, EPS) * inv_n
        else:
            l = (x - y) ** 2
            g = 2.0 * inv_n * (x - y)
    mask = act[:, :, None, None]
    loss = float(np.where(mask, l, 0.0).sum() * inv_n)
    return loss, np.where(mask, g, 0.0).astype(np.float32)
