"""Host side of the affine warp (hkp/geometry.py, the hkp_warp_affine_u8 ABI): the
record layout, the matrix builders and their quantisation, the labels' path, the
sampler's contract, and the numpy restatement (tests/_warp_ref.py) against an
independent float64 implementation.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _warp_ref as ref
from conftest import REPO

HEADER = os.path.join(REPO, "include", "hulkkp.h")


def test_struct_layout_matches_header():
    from hkp import _lib
    X = _lib.WarpXform
    assert ctypes.sizeof(X) == 32
    assert (X.m.offset, X.m.size) == (0, 24)
    assert (X.fill.offset, X.fill.size) == (24, 4)
    assert (X.reserved.offset, X.reserved.size) == (28, 4)
    text = open(HEADER).read()
    body = re.search(r"typedef struct hkp_warp_xform \{(.*?)\} hkp_warp_xform;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [" ".join(f.split()) for f in body.split(";") if f.strip()]
    assert fields == ["int32_t m[6]", "uint8_t fill[4]", "int32_t reserved"]
    for name in ("HKP_WARP_BILINEAR", "HKP_WARP_NEAREST", "HKP_WARP_BORDER_CONSTANT", "HKP_WARP_BORDER_REPLICATE",
                 "HKP_WARP_BORDER_REFLECT101", "HKP_WARP_MAX_DIM"):
        value = int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
        assert getattr(_lib, name) == value, name
    assert (ref.BILINEAR, ref.NEAREST) == (_lib.HKP_WARP_BILINEAR, _lib.HKP_WARP_NEAREST)
    assert (ref.CONSTANT, ref.REPLICATE, ref.REFLECT101) == (
        _lib.HKP_WARP_BORDER_CONSTANT, _lib.HKP_WARP_BORDER_REPLICATE, _lib.HKP_WARP_BORDER_REFLECT101)


def test_known_matrices():
    from hkp import geometry as G
    h, w = 48, 64
    one = 65536
    assert np.array_equal(G.affine_matrix(h, w), [[1, 0, 0], [0, 1, 0]])
    assert G.quantize_inverse(G.affine_matrix(h, w)).tolist() == [one, 0, 0, 0, one, 0]
    q = G.quantize_inverse(G.affine_matrix(h, w, hflip=True))
    assert q.dtype == np.int32 and q.tolist() == [-one, 0, (w - 1) << 16, 0, one, 0]
    assert G.quantize_inverse(G.affine_matrix(h, w, vflip=True)).tolist() == [one, 0, 0, 0, -one, (h - 1) << 16]
    # +90 degrees about the centre of a square turns counter-clockwise on the screen:
    # dest (x, y) reads source (n-1-y, x)
    n = 24
    assert G.quantize_inverse(G.affine_matrix(n, n, rotate_deg=90)).tolist() == [0, -one, (n - 1) << 16, one, 0, 0]
    assert G.quantize_inverse(G.affine_matrix(n, n, rotate_deg=-90)).tolist() == [0, one, 0, -one, 0, (n - 1) << 16]
    # integer translation: dest = source + (5, -3)
    assert G.quantize_inverse(G.affine_matrix(h, w, translate_xy_px=(5, -3))).tolist() == [
        one, 0, -5 * one, 0, one, 3 * one]
    # resize, half-pixel centres: src = (dst + 0.5) * ws / w - 0.5
    assert G.quantize_inverse(G.resize_matrix(12, 20, 24, 40)).tolist() == [one // 2, 0, -one // 4, 0, one // 2, -one // 4]
    assert G.quantize_inverse(G.resize_matrix(12, 20, 6, 10)).tolist() == [2 * one, 0, one // 2, 0, 2 * one, one // 2]
    assert G.quantize_inverse(G.resize_matrix(12, 20, 12, 20)).tolist() == [one, 0, 0, 0, one, 0]
    # flips innermost, translation outermost: flip, then rotate, then shift
    M = G.affine_matrix(h, w, rotate_deg=90, translate_xy_px=(2, 0), hflip=True)
    c = np.array([(w - 1) / 2, (h - 1) / 2])
    p = np.array([w - 1.0, c[1]])                     # right-middle -(hflip)-> left-middle -(+90 ccw)-> bottom
    assert np.allclose(M[:, :2] @ p + M[:, 2], [c[0] + 2, c[1] + c[0]])


def test_quantised_inverse_composes_to_identity():
    from hkp import geometry as G
    from hkp._lib import HkpError
    h, w = 480, 640
    rng = np.random.default_rng(3)
    for _ in range(20):
        M = G.affine_matrix(h, w, rng.uniform(-180, 180), rng.uniform(0.5, 2), rng.uniform(-50, 50, 2),
                            rng.uniform(-20, 20), rng.random() < 0.5, rng.random() < 0.5)
        Qi = G.quantize_inverse(M).astype(np.float64).reshape(2, 3) / 65536.0
        corners = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], dtype=np.float64)
        dest = corners @ M[:, :2].T + M[:, 2]
        back = dest @ Qi[:, :2].T + Qi[:, 2]
        # each coefficient is off by <= 2^-17; dest coordinates stay below 2 (w + h) here
        assert np.abs(back - corners).max() <= 2.0 ** -16 * (w + h)
    with pytest.raises(HkpError, match="singular"):
        G.quantize_inverse([[1, 2, 0], [2, 4, 0]])
    with pytest.raises(HkpError, match="singular"):
        G.quantize_inverse(np.zeros((2, 3)))
    with pytest.raises(HkpError, match="int32"):
        G.quantize_inverse([[1e-5, 0, 0], [0, 1, 0]])              # inverse 1e5 * 65536 > 2^31
    with pytest.raises(HkpError, match="int32"):
        G.quantize_inverse([[1, 0, 40000], [0, 1, 0]])             # offset 40000 px in Q16
    with pytest.raises(HkpError, match="2x3"):
        G.quantize_inverse(np.eye(3))


def test_labels():
    from hkp import geometry as G
    h, w = 48, 64
    uv = np.array([[10.0, 5.0], [63.0, 47.0], [0.0, 0.0]])
    got = G.transform_uv(G.affine_matrix(h, w, hflip=True), uv)
    assert got.dtype == np.float32 and np.array_equal(got, [[53, 5], [0, 47], [63, 0]])
    assert np.array_equal(G.transform_uv(G.affine_matrix(h, w, vflip=True), uv), [[10, 42], [63, 0], [0, 47]])
    assert np.array_equal(G.transform_uv(G.affine_matrix(h, w, translate_xy_px=(5, -3)), uv), uv + [5, -3])
    sq = G.transform_uv(G.affine_matrix(24, 24, rotate_deg=90), [[23.0, 0.0], [0.0, 0.0]])
    assert np.allclose(sq, [[0, 0], [0, 23]], atol=1e-5)           # top-right -> top-left: counter-clockwise
    assert np.allclose(G.transform_uv(G.affine_matrix(h, w, scale=2), [[31.5, 23.5], [32.5, 23.5]]),
                       [[31.5, 23.5], [33.5, 23.5]])
    assert np.allclose(G.transform_uv(G.resize_matrix(12, 20, 24, 40), [[0.0, 0.0]]), [[0.5, 0.5]])
    assert np.array_equal(G.swap_pairs(uv, [(0, 2)]), uv[[2, 1, 0]])
    assert np.array_equal(G.swap_pairs(uv, []), uv)
    # flip pairs: exchanged on an odd number of flips only
    mats = [G.affine_matrix(h, w, hflip=hf, vflip=vf) for hf, vf in ((0, 0), (1, 0), (0, 1), (1, 1))]
    plan = G.WarpPlan(mats, (h, w), flipped=[False, True, True, False], flip_pairs=[(0, 1)])
    lab = np.tile(np.array([[10.0, 5.0], [20.0, 30.0]], dtype=np.float32), (4, 1, 1))
    out = plan.apply_uv(lab)
    assert out.dtype == np.float32
    assert np.array_equal(out[0], lab[0])
    assert np.array_equal(out[1], [[43, 30], [53, 5]])             # hflip, rows exchanged
    assert np.array_equal(out[2], [[20, 17], [10, 42]])            # vflip, rows exchanged
    assert np.array_equal(out[3], [[53, 42], [43, 17]])            # both: a half turn, no exchange
    t = plan.apply_uv(torch.from_numpy(lab))
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), out)
    # the clip is the reference's label rule
    far = G.WarpPlan([G.affine_matrix(h, w, translate_xy_px=(100, -100))], (h, w))
    assert np.array_equal(far.apply_uv(lab[:1])[0], [[63, 0], [63, 0]])
    from hkp._lib import HkpError
    with pytest.raises(HkpError, match="labels"):
        plan.apply_uv(lab[:3])


def test_sampler_contract():
    from hkp import geometry as G
    from hkp.augment import DomainRandomization
    hw = (48, 64)
    ga = G.GeometricAugmentation(seed=7, hflip=0.5, vflip=0.5, shear=(-5, 5))
    a = ga.plan([3, 9, 4], epoch=2, hw=hw)
    b = ga.plan([9], epoch=2, hw=hw)
    c = ga.plan([0, 1, 2, 3, 4, 5, 6, 7, 8, 9], epoch=2, hw=hw)
    assert np.array_equal(a.coefficients()[1], b.coefficients()[0])
    assert np.array_equal(a.coefficients()[[0, 2, 1]], c.coefficients()[[3, 4, 9]])
    assert a.params[1] == ga.sample(9, 2) == G.GeometricAugmentation(seed=7, hflip=0.5, vflip=0.5,
                                                                      shear=(-5, 5)).sample(9, 2)
    # epochs, indices and seeds differ
    base = ga.sample(9, 2)
    for other in (ga.sample(9, 3), ga.sample(8, 2), G.GeometricAugmentation(seed=8, hflip=0.5, vflip=0.5,
                                                                            shear=(-5, 5)).sample(9, 2)):
        assert other["rotate"] != base["rotate"] and other["scale"] != base["scale"]
    # the documented draw order, and independence of DomainRandomization under the same seed
    rng = np.random.default_rng([7, 2, 9, 1])
    assert base["rotate"] == float(rng.uniform(-30, 30))
    assert base["scale"] == float(rng.uniform(0.9, 1.1))
    t = rng.uniform(-0.1, 0.1, 2)
    assert base["translate"] == (float(t[0]), float(t[1]))
    assert base["shear"] == float(rng.uniform(-5, 5))
    f = rng.random(2)
    assert (base["hflip"], base["vflip"]) == (bool(f[0] < 0.5), bool(f[1] < 0.5))
    dr_first = np.random.default_rng([7, 2, 9]).random(4)          # DomainRandomization's stream
    ga_first = np.random.default_rng([7, 2, 9, 1]).random(4)
    assert not np.any(dr_first == ga_first)
    assert DomainRandomization(seed=7).sample(9, 2) == DomainRandomization(seed=7).sample(9, 2)
    # ranges are honoured; degenerate ranges give constants
    wide = G.GeometricAugmentation(seed=1, rotate=(10, 20), scale=(1.2, 1.3), translate=(0.02, 0.05), shear=(-3, -1),
                                   hflip=1.0, vflip=0.0)
    for i in range(64):
        p = wide.sample(i, 0)
        assert 10 <= p["rotate"] <= 20 and 1.2 <= p["scale"] <= 1.3 and -3 <= p["shear"] <= -1
        assert all(0.02 <= v <= 0.05 for v in p["translate"])
        assert p["hflip"] is True and p["vflip"] is False           # hflip=1.0 always flips
    fixed = G.GeometricAugmentation(rotate=(0, 0), scale=(1, 1), translate=(0, 0)).plan(range(5), 0, hw=hw)
    assert np.array_equal(fixed.coefficients(), np.tile([65536, 0, 0, 0, 65536, 0], (5, 1)))
    assert wide.plan(range(4), 0, hw=hw).flipped.tolist() == [True] * 4
    with pytest.raises(ValueError):
        G.GeometricAugmentation(rotate=(5, 1))
    with pytest.raises(ValueError):
        G.GeometricAugmentation(border="wrap")


def test_keep_inside():
    from hkp import geometry as G
    h, w = 48, 64
    uv = np.array([[1.0, 1.0], [40.0, 20.0]])                      # one keypoint next to a corner
    ga = G.GeometricAugmentation(seed=5)
    taken, identity = 0, 0
    for i in range(40):
        p = ga.sample(i, 0, uv=uv, hw=(h, w))
        q = G.transform_uv(ga.matrix(p, (h, w)), uv)
        assert np.all(q >= 0) and np.all(q[:, 0] <= w - 1) and np.all(q[:, 1] <= h - 1), (i, p)
        if p["try"] < 0:
            identity += 1
            assert np.array_equal(G.quantize_inverse(ga.matrix(p, (h, w))), [65536, 0, 0, 0, 65536, 0])
        else:
            taken += 1
            # try t is the (t+1)-th draw of the one generator
            rng = np.random.default_rng([5, 0, i, 1])
            for _ in range(p["try"] + 1):
                d = ga._draw(rng)
            assert {k: p[k] for k in d} == d
    assert taken > 0
    # nothing fits: the identity; without labels or with keep_inside off: the first draw
    out = G.GeometricAugmentation(seed=5, translate=(2.0, 3.0), tries=3)
    assert out.sample(0, 0, uv=uv, hw=(h, w))["try"] == -1
    assert out.sample(0, 0)["try"] == 0
    off = G.GeometricAugmentation(seed=5, translate=(2.0, 3.0), keep_inside=False)
    assert off.sample(0, 0, uv=uv, hw=(h, w)) == off.sample(0, 0)
    # the label-dependent choice does not depend on the batch either
    p1 = ga.plan([4, 11], 0, uvs=np.stack([uv, uv]), hw=(h, w))
    p2 = ga.plan([11], 0, uvs=uv[None], hw=(h, w))
    assert np.array_equal(p1.coefficients()[1], p2.coefficients()[0])


def _bilinear_f64(src, inv, h, w):
    """A plain float64 bilinear sampler (no border handling: callers mask)."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    sx = inv[0, 0] * x + inv[0, 1] * y + inv[0, 2]
    sy = inv[1, 0] * x + inv[1, 1] * y + inv[1, 2]
    ix, iy = np.floor(sx).astype(int), np.floor(sy).astype(int)
    fx, fy = (sx - ix)[..., None], (sy - iy)[..., None]
    ix0, ix1 = np.clip(ix, 0, src.shape[1] - 1), np.clip(ix + 1, 0, src.shape[1] - 1)
    iy0, iy1 = np.clip(iy, 0, src.shape[0] - 1), np.clip(iy + 1, 0, src.shape[0] - 1)
    s = src.astype(np.float64)
    return (s[iy0, ix0] * (1 - fx) + s[iy0, ix1] * fx) * (1 - fy) + (s[iy1, ix0] * (1 - fx) + s[iy1, ix1] * fx) * fy


def test_reference_against_independent_float64():
    """_warp_ref (bilinear, CONSTANT) against scipy.ndimage.affine_transform(order=1)
    in float64, on the output pixels whose four taps lie inside the source.

    The bound is derived, not measured: the coordinate is quantised to 1/256 px with
    rounding, so it is off by <= 2^-9 px per axis, and a bilinear surface over uint8
    data has a slope of at most 255 per px along each axis: <= 2 * 255 * 2^-9 ~ 1.0.
    The Q16 rounding of the six coefficients moves the coordinate by
    <= 2^-17 * (w + h) px per axis: < 0.5 grey levels for w + h <= 128.  The final
    rounding to uint8 adds 0.5.  Together < 2 grey levels."""
    from scipy import ndimage
    from hkp import geometry as G
    h, w = 40, 56
    src = np.random.default_rng(11).integers(0, 256, (h, w, 3), dtype=np.uint8)
    M = G.affine_matrix(h, w, rotate_deg=17, scale=1.1)
    q = G.quantize_inverse(M)
    got = ref.warp(src, q, h, w, ref.BILINEAR, ref.CONSTANT, (0, 0, 0)).astype(np.float64)
    full = np.vstack([M, [0, 0, 1]])
    inv = np.linalg.inv(full)[:2]
    # scipy maps output (row, col) to input (row, col): swap the axes of the x/y matrix
    mat_rc = np.array([[inv[1, 1], inv[1, 0]], [inv[0, 1], inv[0, 0]]])
    off_rc = np.array([inv[1, 2], inv[0, 2]])
    want = np.stack([ndimage.affine_transform(src[..., c].astype(np.float64), mat_rc, offset=off_rc,
                                              output_shape=(h, w), order=1, mode="constant", cval=0.0)
                     for c in range(3)], -1)
    mask = ref.inside_mask((h, w), q, h, w)
    assert mask.sum() >= h * w // 2
    assert np.abs(got - want)[mask].max() <= 2.0
    # and the ten-line float64 bilinear agrees with scipy there (the two independent ones)
    mine = _bilinear_f64(src, inv, h, w)
    assert np.abs(mine - want)[mask].max() < 1e-9
    assert np.abs(got - mine)[mask].max() <= 2.0
    # the picture really turned: not the input
    assert np.abs(got - src)[mask].mean() > 20


def test_reference_identities():
    """The restatement's exact cases (what the GPU tests then ask of the kernel)."""
    from hkp import geometry as G
    h, w = 9, 13
    src = np.random.default_rng(2).integers(0, 256, (h, w, 3), dtype=np.uint8)
    ident = [65536, 0, 0, 0, 65536, 0]
    for interp in (ref.BILINEAR, ref.NEAREST):
        for border in (ref.CONSTANT, ref.REPLICATE, ref.REFLECT101):
            assert np.array_equal(ref.warp(src, ident, h, w, interp, border, (1, 2, 3)), src)
            hf = ref.warp(src, G.quantize_inverse(G.affine_matrix(h, w, hflip=True)), h, w, interp, border)
            assert np.array_equal(hf, src[:, ::-1])
    # borders, nearest, shifted two pixels to the right: columns -2, -1 of the source
    sh = G.quantize_inverse(G.affine_matrix(h, w, translate_xy_px=(2, 0)))
    c = ref.warp(src, sh, h, w, ref.NEAREST, ref.CONSTANT, (7, 200, 31))
    assert np.array_equal(c[:, 2:], src[:, :-2]) and np.all(c[:, :2] == [7, 200, 31])
    assert np.array_equal(ref.warp(src, sh, h, w, ref.NEAREST, ref.REPLICATE)[:, :2], src[:, [0, 0]])
    assert np.array_equal(ref.warp(src, sh, h, w, ref.NEAREST, ref.REFLECT101)[:, :2], src[:, [2, 1]])
    # a half-pixel shift averages neighbours, rounding half up
    half = [65536, 0, 32768, 0, 65536, 0]
    avg = ref.warp(src, half, h, w - 1, ref.BILINEAR, ref.REPLICATE)
    assert np.array_equal(avg, (src[:, :-1].astype(int) + src[:, 1:] + 1) // 2)


def test_argument_checks_without_a_device(monkeypatch):
    from hkp import geometry as G, ops
    from hkp._lib import HkpError
    plan = G.WarpPlan([G.affine_matrix(8, 8)], (8, 8))
    with pytest.raises(HkpError, match="expected a tensor"):
        ops.warp_affine_u8(np.zeros((1, 8, 8, 3), np.uint8), plan)
    with pytest.raises(HkpError, match="must be on the GPU"):
        ops.warp_affine_u8(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), plan)
    with pytest.raises(HkpError, match="must be on the GPU"):
        ops.resize_u8(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), 4, 4)
    with pytest.raises(HkpError, match="unknown interp"):
        ops.resize_u8(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), 4, 4, interp="cubic")
    with pytest.raises(HkpError, match="unknown border"):
        G.WarpPlan([G.affine_matrix(8, 8)], (8, 8), border="wrap")
    with pytest.raises(HkpError, match="unknown interp"):
        G.WarpPlan([G.affine_matrix(8, 8)], (8, 8), interp="cubic")
    with pytest.raises(HkpError, match="fill"):
        G.WarpPlan([G.affine_matrix(8, 8)], (8, 8), fill=(0, 0, 256))
    with pytest.raises(HkpError, match=r"\[n, 2, 3\]"):
        G.WarpPlan(np.zeros((2, 3)), (8, 8))
    with pytest.raises(HkpError, match="singular"):
        G.WarpPlan(np.zeros((1, 2, 3)), (8, 8))
    ga = G.GeometricAugmentation()
    with pytest.raises(HkpError, match="hw"):
        ga.plan([0, 1])
    with pytest.raises(HkpError, match="labels"):
        ga.plan([0, 1], 0, uvs=np.zeros((3, 2, 2)), hw=(8, 8))
    with pytest.raises(HkpError, match="numpy image or a device tensor"):
        ga([[1, 2, 3]])
    with pytest.raises(HkpError, match=r"uint8 \[H,W,3\]"):
        ga(np.zeros((8, 8, 3), np.float32))
    # the C entry point validates before any launch (no device is touched)
    from hkp import _lib
    xf = (_lib.WarpXform * 1)()
    P = ctypes.c_void_p
    bad = [((0, 8, 8, 16, 8, 8, 4096, 0, 0), "batch size"), ((1, 0, 8, 16, 8, 8, 4096, 0, 0), "source"),
           ((1, 8, 8, 16, 8, _lib.HKP_WARP_MAX_DIM + 1, 4096, 0, 0), "output"),
           ((1, 8, 8, 16, 8, 8, 4096, 2, 0), "interpolation"), ((1, 8, 8, 16, 8, 8, 4096, 0, 3), "border"),
           ((1, 1, 8, 16, 8, 8, 4096, 0, 2), "REFLECT101"), ((1, 8, 8, 0, 8, 8, 4096, 0, 0), "null"),
           ((1, 8, 8, 16, 8, 8, 100, 0, 0), "overlap")]
    for (n, hs, ws, pin, h, w, pout, interp, border), what in bad:
        with pytest.raises(HkpError, match=what):
            _lib.call("hkp_warp_affine_u8", n, hs, ws, P(pin), h, w, P(pout), xf, P(64), interp, border, None)
    xf[0].reserved = 1
    with pytest.raises(HkpError, match="reserved"):
        _lib.call("hkp_warp_affine_u8", 1, 8, 8, P(16), 8, 8, P(4096), xf, P(64), 0, 0, None)
    # the DataLoader-worker guard
    monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: object())
    with pytest.raises(HkpError, match="num_workers=0"):
        ga(np.zeros((8, 8, 3), np.uint8))
