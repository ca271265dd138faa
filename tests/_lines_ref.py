"""hkp_line_target restated in numpy (include/hulkkp.h is the definition): the fp32
operation order without fused multiply-add and WITHOUT the kernel's culling, and a float64
geometry function to hold the restatement itself against.  Test infrastructure.

lines [n,k,s,5] = (x0, y0, x1, y1, flag); flag > 0 is a present slot, anything else (NaN
included) an empty one whose coordinates are never read."""
import numpy as np

F = np.float32


def d2_plane(rec, H, W):
    """float32 [H,W]: the definition's minimum over the present slots of rec [s,5], in slot
    order; +inf without one."""
    rec = np.asarray(rec, dtype=F)
    x = np.arange(W, dtype=F)[None, :]
    y = np.arange(H, dtype=F)[:, None]
    d2 = np.full((H, W), np.inf, dtype=F)
    with np.errstate(all="ignore"):
        for x0, y0, x1, y1, flag in rec:
            if not flag > 0:
                continue
            dx, dy = F(x1 - x0), F(y1 - y0)
            l2 = F(F(dx * dx) + F(dy * dy))
            px, py = x - x0, y - y0                               # [1,W], [H,1], float32
            if l2 > 0:
                inv = F(F(1.0) / l2)
                prod = (px * dx + py * dy) * inv                  # float32 throughout: numpy does not fuse
                t = np.fmin(np.fmax(prod, F(0.0)), F(1.0))        # fmax / fmin: a NaN product gives 0
            else:
                t = np.zeros((H, W), dtype=F)
            cx, cy = px - t * dx, py - t * dy
            d2 = np.fmin(d2, cx * cx + cy * cy)
    assert d2.dtype == F
    return d2


def d2(lines, H, W):
    """float32 [n,k,H,W]."""
    lines = np.asarray(lines, dtype=F)
    n, k = lines.shape[:2]
    return np.stack([np.stack([d2_plane(lines[b, c], H, W) for c in range(k)]) for b in range(n)])


def den(sigma):
    return F(2.0 * float(sigma) * float(sigma))


def target64(d2_f32, sigma):
    """float64 exp of the fp32 quotient -d2 / den: what the kernel's expf is within one fp32
    ulp of (ocml's stated accuracy); 0 where d2 is +inf."""
    with np.errstate(all="ignore"):
        q = (-np.asarray(d2_f32, dtype=F)) / den(sigma)
    assert q.dtype == F
    return np.exp(q.astype(np.float64))


def dist64(rec, H, W):
    """float64 [H,W]: the distance to the nearest present segment of rec [s,5], computed
    in float64 from the float32 coordinates (np.hypot; t clipped in float64)."""
    rec = np.asarray(rec, dtype=F).astype(np.float64)
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    d = np.full((H, W), np.inf)
    for x0, y0, x1, y1, flag in rec:
        if not flag > 0:
            continue
        dx, dy = x1 - x0, y1 - y0
        l2 = dx * dx + dy * dy
        px, py = x - x0, y - y0
        t = np.clip((px * dx + py * dy) / l2, 0.0, 1.0) if l2 > 0 else 0.0
        d = np.minimum(d, np.hypot(px - t * dx, py - t * dy))
    return d


def point_d2(u, v, H, W):
    """hkp_gauss_target's (x-u)^2 + (y-v)^2 in its fp32 operation order, [H,W]."""
    x = np.arange(W, dtype=F)[None, :]
    y = np.arange(H, dtype=F)[:, None]
    dx, dy = x - F(u), y - F(v)
    return dx * dx + dy * dy


def seg(x0, y0, x1, y1, flag=1.0):
    return [x0, y0, x1, y1, flag]


def fill(rows, s, junk=(0.0, 0.0, 0.0, 0.0, 0.0)):
    """rows padded with `junk` slots to s, float32 [s,5]."""
    rows = [list(r) for r in rows]
    assert len(rows) <= s
    return np.array(rows + [list(junk)] * (s - len(rows)), dtype=F).reshape(s, 5)
