"""numpy float64 restatement of hkp_logits_merge (include/hulkkp.h) and of the
host's coordinate map (hkp/tta.py), written from their definitions, not from
their code (test infrastructure).

merge(lows, views, perm, hw, mode): lows one float32 [n,k,h_v,w_v] array per
view, views (ay, by, ax, bx, weight) per view, perm int [views,k] -> float32
[n,k,h,w].  Every product and sum is its own float64 operation, in view order.
"""
import numpy as np

LOGIT, PROB = 0, 1


def lattice(n):
    """Nodes of the network's stride-8 lattice along n pixels."""
    for _ in range(3):
        n = (n + 1) // 2
    return n


def view_side(n, s):
    return n if s == 1 else max(32, 8 * int(round(s * n / 8.0)))


def axis_coeffs(N, n, N_v, n_v, flip):
    """(a, b) of base node j -> view lattice coordinate a*j + b, by the definition:
    node -> base pixel (align_corners) -> view pixel (half-pixel rule) -> flip ->
    view node (align_corners).  Exact for a view of the base's own size."""
    if N == N_v and n == n_v:
        return (-1.0, float(n - 1)) if flip else (1.0, 0.0)
    # two points of the affine map, evaluated step by step in float64
    def f(j):
        X = j * (N - 1) / (n - 1) if n > 1 else 0.0
        Xv = (X + 0.5) * N_v / N - 0.5
        if flip:
            Xv = N_v - 1 - Xv
        return Xv * (n_v - 1) / (N_v - 1) if n_v > 1 else 0.0
    b = f(0.0)
    a = (f(float(max(n - 1, 1))) - b) / float(max(n - 1, 1))
    return a, b


def node_positions(N, n, N_v, n_v, flip):
    """Base-pixel coordinate that node t of a view's axis stands for (float64 [n_v]):
    the inverse of the chain above."""
    t = np.arange(n_v, dtype=np.float64)
    Xv = t * (N_v - 1) / (n_v - 1) if n_v > 1 else np.zeros(1)
    if flip:
        Xv = N_v - 1 - Xv
    return (Xv + 0.5) * N / N_v - 0.5


def _axis(a, b, count, n_v):
    c = np.float64(a) * np.arange(count, dtype=np.float64) + np.float64(b)
    clamped = (c < 0) | (c > n_v - 1)
    c = np.clip(c, 0.0, float(n_v - 1))
    i0 = np.floor(c).astype(np.int64)
    f = c - i0
    i1 = np.minimum(i0 + 1, n_v - 1)
    return i0, i1, f, clamped


def sample(z, ay, by, ax, bx, hw):
    """One view's z_v on the base lattice: z float32 [..., h_v, w_v] -> float64
    [..., h, w].  A tap of weight exactly 0 is not read."""
    h, w = hw
    y0, y1, fy, _ = _axis(ay, by, h, z.shape[-2])
    x0, x1, fx, _ = _axis(ax, bx, w, z.shape[-1])
    z = z.astype(np.float64)
    fxb = fx[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        def row(r):
            z0 = z[..., r, :][..., x0]
            z1 = z[..., r, :][..., x1]
            return np.where(fxb == 0, z0, z0 + fxb * (z1 - z0))
        top, bot = row(y0), row(y1)
        fyb = fy[:, None]
        return np.where(fyb == 0, top, top + fyb * (bot - top))


def merge(lows, views, perm, hw, mode):
    perm = np.asarray(perm)
    n, k = lows[0].shape[:2]
    acc = np.zeros((n, k) + tuple(hw), dtype=np.float64)
    neg = np.zeros_like(acc)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for v, (z, (ay, by, ax, bx, wt)) in enumerate(zip(lows, views)):
            zv = sample(np.asarray(z)[:, perm[v]], ay, by, ax, bx, hw)
            wt = np.float64(wt)
            if mode == LOGIT:
                acc = wt * zv if v == 0 else acc + wt * zv         # starts with view 0's term: -0 stays -0
            else:
                zc = np.where(zv < -700.0, -700.0, np.where(zv > 700.0, 700.0, zv))
                acc = acc + wt / (1.0 + np.exp(-zc))
                neg = neg + wt / (1.0 + np.exp(zc))
        if mode == LOGIT:
            return acc.astype(np.float32)
        return (np.log(acc) - np.log(neg)).astype(np.float32)


def unclamped(views, lattices, hw):
    """bool [h, w]: nodes whose coordinates no view clamped."""
    ok = np.ones(hw, dtype=bool)
    for (ay, by, ax, bx, _), (hv, wv) in zip(views, lattices):
        cy = _axis(ay, by, hw[0], hv)[3]
        cx = _axis(ax, bx, hw[1], wv)[3]
        ok &= ~cy[:, None] & ~cx[None, :]
    return ok


# ---- ideal targets: the planes of tests/_instances_ref.py's round trip (a 65 x 81 image
# over a 9 x 11 lattice, 0..3 instances per plane, sigma 8), seen by several views
IDEAL_SCALES = (1.0, 0.75, 1.25)


def ideal_views(scales, flips):
    """[(H_v, W_v, h_v, w_v, hflip, vflip)] for the round trip's image."""
    import _instances_ref as iref
    H, W = iref.RT_IMAGE
    out = []
    for s in scales:
        Hv, Wv = view_side(H, s), view_side(W, s)
        hv, wv = (iref.RT_LATTICE if s == 1 else (lattice(Hv), lattice(Wv)))
        out += [(Hv, Wv, hv, wv, fh, fv) for fh, fv in flips]
    return out


def ideal_logits(view):
    """fp32 logits [1,4,h_v,w_v] of the maximum of the instances' Gaussians at the base
    pixels the view's nodes stand for, clamped to finite as _instances_ref.lowres_logits."""
    import _instances_ref as iref
    H, W = iref.RT_IMAGE
    Hv, Wv, hv, wv, fh, fv = view
    Y = node_positions(H, iref.RT_LATTICE[0], Hv, hv, fv)[:, None]
    X = node_positions(W, iref.RT_LATTICE[1], Wv, wv, fh)[None, :]
    out = np.zeros((1, len(iref.RT_POINTS), hv, wv), dtype=np.float64)
    for k, inst in enumerate(iref.RT_POINTS):
        for u, v in inst:
            u, v = float(np.float32(u)), float(np.float32(v))
            out[0, k] = np.maximum(out[0, k], np.exp(-((X - u) ** 2 + (Y - v) ** 2) / (2.0 * iref.RT_SIGMA ** 2)))
    t = np.clip(out, 1e-30, 1.0 - 2.0 ** -24)
    return (np.log(t) - np.log1p(-t)).astype(np.float32)


def ideal_table(views):
    """(records (ay, by, ax, bx, weight), lattices) of equal weights for ideal_views."""
    import _instances_ref as iref
    (H, W), (h, w) = iref.RT_IMAGE, iref.RT_LATTICE
    recs = []
    for Hv, Wv, hv, wv, fh, fv in views:
        recs.append(axis_coeffs(H, h, Hv, hv, fv) + axis_coeffs(W, w, Wv, wv, fh) + (1.0 / len(views),))
    return recs, [(v[2], v[3]) for v in views]


def ulp32(x):
    """One fp32 unit in the last place at |x| (float32 array)."""
    x = np.abs(np.asarray(x, dtype=np.float32))
    return np.spacing(np.maximum(x, np.float32(np.finfo(np.float32).tiny)))


def within_ulps(got, want, ulps=1):
    """got, want float32: equal NaN pattern, equal infinities, and elsewhere
    |got - want| <= ulps * max(ulp(got), ulp(want))."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    fin = np.isfinite(got) & np.isfinite(want)
    rest = ~fin & ~np.isnan(want)
    if not np.array_equal(got[rest], want[rest]):
        return False
    d = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64))
    return bool(np.all(d <= ulps * np.maximum(ulp32(got[fin]), ulp32(want[fin])).astype(np.float64)))
