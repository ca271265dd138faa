"""numpy restatement of csrc/augment.hip (shared by test_augment_cpu.py and
test_gpu_augment.py): applies a hkp.augment.Plan stage by stage in np.float32
arithmetic, every operation rounded on its own, in the order the kernel's
comments fix.  Its own Philox4x32-10.  No tolerance anywhere: the kernel has to
give these bits."""
import numpy as np

F = np.float32
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints), key: two ints → four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def q8(v):
    """float32 → uint8: rint (half to even), clamp."""
    assert v.dtype == np.float32
    return np.minimum(np.maximum(np.rint(v), F(0)), F(255)).astype(np.uint8)


def stage_lut(img, lut):
    out = np.empty_like(img)
    for c in range(3):
        out[..., c] = lut[c][img[..., c]]
    return out


def stage_hsv(img, dh, add, mul):
    """The HSV stage, line for line as the comment above aug_hsv in csrc/augment.hip."""
    dh, add, mul = F(dh), F(add), F(mul)
    b, g, r = (img[..., c].astype(F) for c in range(3))
    mx = np.maximum(np.maximum(r, g), b)
    mn = np.minimum(np.minimum(r, g), b)
    d = mx - mn
    S = np.where(mx > 0, (F(255) * d) / np.where(mx > 0, mx, F(1)), F(0))
    dd = np.where(d == 0, F(1), d)
    h_r = (g - b) / dd
    h_r = np.where(h_r < 0, h_r + F(6), h_r)
    h_g = F(2) + (b - r) / dd
    h_b = F(4) + (r - g) / dd
    h = np.where(d == 0, F(0), np.where(mx == r, h_r, np.where(mx == g, h_g, h_b)))
    h = h + dh
    h = np.where(h < 0, h + F(6), h)
    h = np.where(h >= 6, h - F(6), h)
    S = np.minimum(np.maximum(S * mul + add, F(0)), F(255))
    c = (mx * S) / F(255)
    i = np.floor(h)
    f = h - i
    p = mx - c
    q = mx - c * f
    t = mx - c * (F(1) - f)
    for a in (S, h, c, f, p, q, t):
        assert a.dtype == np.float32
    ro = np.select([i == 0, i == 1, i == 2, i == 3, i == 4], [mx, q, p, p, t], mx)
    go = np.select([i == 0, i == 1, i == 2, i == 3, i == 4], [t, mx, mx, q, p], p)
    bo = np.select([i == 0, i == 1, i == 2, i == 3, i == 4], [p, p, t, mx, mx], q)
    return np.stack([q8(bo), q8(go), q8(ro)], -1)


def _taps(a, w0, w1, w2, axis):
    """((((w2 a[-2] + w1 a[-1]) + w0 a[0]) + w1 a[1]) + w2 a[2]) along `axis` of a
    float32 array padded by 2 on that axis."""
    n = a.shape[axis] - 4

    def s(k):
        idx = [slice(None)] * a.ndim
        idx[axis] = slice(2 + k, 2 + k + n)
        return a[tuple(idx)]
    v = w2 * s(-2) + w1 * s(-1)
    v = v + w0 * s(0)
    v = v + w1 * s(1)
    v = v + w2 * s(2)
    assert v.dtype == np.float32
    return v


def stage_blur(img, w0, w1, w2):
    w0, w1, w2 = F(w0), F(w1), F(w2)
    a = np.pad(img, ((2, 2), (2, 2), (0, 0)), mode="reflect").astype(F)    # reflect-101
    return q8(_taps(_taps(a, w0, w1, w2, 1), w0, w1, w2, 0))


def stage_noise(img, scale, key, table):
    h, w, _ = img.shape
    ctr = (np.arange(h, dtype=np.uint64)[:, None] * np.uint64(w) + np.arange(w, dtype=np.uint64)[None, :])
    x0 = philox4x32_10((ctr, 0, 0, 0), key)[0]
    nz = table[x0 >> np.uint32(20)] * F(scale)
    assert nz.dtype == np.float32
    return q8(img.astype(F) + nz[..., None])


def apply_plan(imgs, plan):
    """imgs uint8 [B,H,W,3] → what hkp_augment_u8 must produce for `plan`."""
    from hkp import _lib
    table = plan.table.host
    out = np.empty_like(imgs)
    for b in range(imgs.shape[0]):
        img = imgs[b].copy()
        prog = plan.programs[b]
        for i in range(prog.nstages):
            st = prog.stages[i]
            if st.kind == _lib.HKP_AUG_LUT:
                img = stage_lut(img, plan.luts[b, i])
            elif st.kind == _lib.HKP_AUG_HSV:
                img = stage_hsv(img, st.f[0], st.f[1], st.f[2])
            elif st.kind == _lib.HKP_AUG_BLUR:
                img = stage_blur(img, st.f[0], st.f[1], st.f[2])
            elif st.kind == _lib.HKP_AUG_NOISE:
                img = stage_noise(img, st.f[0], (st.key[0], st.key[1]), table)
            else:
                raise AssertionError("unknown stage kind %d" % st.kind)
        out[b] = img
    return out
