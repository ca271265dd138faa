"""Test-time augmentation without a GPU: the numpy restatement of hkp_logits_merge
(tests/_tta_ref.py) against the property that defines the coordinate map (a field
linear in base pixels comes back exactly), the host's map against
ResamplePlan.apply_uv, the view table / perm / weights of hkp.tta, the config
keys, and the C ABI's argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import _tta_ref as ref

SIZES = [(96, 128), (75, 100)]
SCALES = [1.0, 0.75, 1.25, 0.5]
FLIPS = [(False, False), (True, False), (False, True), (True, True)]


def _host_view(H, W, s, fh, fv):
    """(record (h_v, w_v, ay, by, ax, bx), (H_v, W_v)) of one view as hkp.tta composes it."""
    from hkp import tta
    Hv, Wv = tta.view_size(H, s), tta.view_size(W, s)
    h, w, hv, wv = (tta.lattice_size(v) for v in (H, W, Hv, Wv))
    ay, by = tta.axis_map(H, h, Hv, hv, fv)
    ax, bx = tta.axis_map(W, w, Wv, wv, fh)
    return (hv, wv, ay, by, ax, bx), (Hv, Wv)


def _ramp_view(H, W, Hv, Wv, hv, wv, fh, fv, al, be, ga):
    """The ramp al*X + be*Y + ga (base pixels) at the positions the view's nodes stand for, fp32."""
    Y = ref.node_positions(H, ref.lattice(H), Hv, hv, fv)
    X = ref.node_positions(W, ref.lattice(W), Wv, wv, fh)
    return (al * X[None, :] + be * Y[:, None] + ga).astype(np.float32)[None, None]


@pytest.mark.parametrize("H,W", SIZES)
def test_ramp_comes_back(H, W):
    """Bilinear interpolation reproduces a linear field, so any slip in the half-pixel
    rule, the flip or the align_corners frame shows as an error of whole fractions of
    a pixel.  The ramp stays inside one binade ([1024, 2048)), where fp32 values are
    a uniform grid of step u: every tap is within u/2 of the field, so is their convex
    combination, and rounding a value within u/2 of x lands within one step of
    round(x) — the one-ulp bound, with nothing to spare for an error of the map."""
    al, be, ga = 0.9, 1.3, 1100.0
    h, w = ref.lattice(H), ref.lattice(W)
    assert (h, w) == {(96, 128): (12, 16), (75, 100): (10, 13)}[(H, W)]
    Yb = np.arange(h) * (H - 1) / (h - 1)
    Xb = np.arange(w) * (W - 1) / (w - 1)
    want = (al * Xb[None, :] + be * Yb[:, None] + ga).astype(np.float32)
    assert want.min() >= 1024 and want.max() < 2048
    recs, lows = [], []
    for s in SCALES:
        for fh, fv in FLIPS:
            (hv, wv, ay, by, ax, bx), (Hv, Wv) = _host_view(H, W, s, fh, fv)
            assert (hv, wv) == (ref.lattice(Hv), ref.lattice(Wv)) and (Hv, Wv) == (ref.view_side(H, s), ref.view_side(W, s))
            low = _ramp_view(H, W, Hv, Wv, hv, wv, fh, fv, al, be, ga)
            # each view on its own ...
            got = ref.merge([low], [(ay, by, ax, bx, 1.0)], [[0]], (h, w), ref.LOGIT)[0, 0]
            ok = ref.unclamped([(ay, by, ax, bx, 1.0)], [(hv, wv)], (h, w))
            assert ok.sum() >= (h - 2) * (w - 2) * (0.2 if s < 1 else 0.9), (s, fh, fv, int(ok.sum()))
            assert ref.within_ulps(got[ok], want[ok]), (H, W, s, fh, fv, np.abs(got[ok] - want[ok]).max())
            if s == 1.0:
                assert ok.all() and np.array_equal(got, want)
            recs.append((hv, wv, ay, by, ax, bx))
            lows.append(low)
    # ... and eight of them together, unequal weights
    pick = [0, 1, 2, 5, 6, 9, 12, 15]
    wts = np.arange(1, 9, dtype=np.float64)
    wts /= wts.sum()
    views = [recs[i][2:] + (wts[j],) for j, i in enumerate(pick)]
    got = ref.merge([lows[i] for i in pick], views, [[0]] * 8, (h, w), ref.LOGIT)[0, 0]
    ok = ref.unclamped(views, [recs[i][:2] for i in pick], (h, w))
    assert ok.sum() > 0 and ref.within_ulps(got[ok], want[ok])


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("s", [0.75, 1.25, 0.5])
def test_pixel_map_is_the_resample_plans(H, W, s):
    from hkp import tta
    from hkp.resample import ResamplePlan
    Hv, Wv = tta.view_size(H, s), tta.view_size(W, s)
    rng = np.random.default_rng(int(H * 10 + s * 100))
    uv = np.stack([rng.uniform(2, W - 3, 64), rng.uniform(2, H - 3, 64)], 1)[None].astype(np.float32)
    want = ResamplePlan([(H, W)], (Hv, Wv)).apply_uv(uv)
    gx, cx = tta.pixel_map(W, Wv, False)
    gy, cy = tta.pixel_map(H, Hv, False)
    got = np.stack([gx * uv[0, :, 0].astype(np.float64) + cx, gy * uv[0, :, 1].astype(np.float64) + cy], 1)
    assert got[:, 0].min() > 0 and got[:, 0].max() < Wv - 1 and got[:, 1].min() > 0 and got[:, 1].max() < Hv - 1
    assert np.array_equal(got.astype(np.float32), want[0])
    # the flip mirrors the view's pixels
    gf, cf = tta.pixel_map(W, Wv, True)
    assert np.allclose(gf * uv[0, :, 0].astype(np.float64) + cf, Wv - 1 - got[:, 0], rtol=0, atol=1e-9)


def test_host_map_is_the_restatements():
    from hkp import tta
    for H, W in SIZES:
        for s in SCALES:
            for flip in (False, True):
                for N in (H, W):
                    Nv = tta.view_size(N, s)
                    n, nv = tta.lattice_size(N), tta.lattice_size(Nv)
                    a, b = tta.axis_map(N, n, Nv, nv, flip)
                    ra, rb = ref.axis_coeffs(N, n, Nv, nv, flip)
                    assert abs(a - ra) <= 1e-13 * max(1, abs(ra)) and abs(b - rb) <= 1e-12 * max(1, abs(rb))
    assert tta.axis_map(40, 1, 40, 1, True) == (-1.0, 0.0)
    a, b = tta.axis_map(40, 5, 32, 1, False)                 # a view of one node: always node 0
    assert (a, b) == (0.0, 0.0)


def test_views_table_perm_and_weights():
    from hkp import tta
    from hkp._lib import HkpError
    T = tta.TestTimeAugmentation
    t = T()                                                   # the default: the flip test
    assert [(v.scale, v.hflip, v.vflip, v.hw) for v in t.views(96, 128)] == [(1.0, False, False, (96, 128)),
                                                                             (1.0, True, False, (96, 128))]
    assert t.mode == "prob" and np.array_equal(t.weights, [0.5, 0.5])
    p = t.plan(2, 4, 96, 128)
    co = p.coefficients()
    assert p.hw == (12, 16) and p.lattices == [(12, 16)] * 2 and p.total == 2 * 2 * 4 * 12 * 16
    assert co[0].tolist() == [1.0, 0.0, 1.0, 0.0, 0.5] and co[1].tolist() == [1.0, 0.0, -1.0, 15.0, 0.5]
    assert [r.off for r in p.records] == [0, 2 * 4 * 12 * 16] and t.plan(2, 4, 96, 128) is p      # cached
    assert np.array_equal(p.perm, [[0, 1, 2, 3]] * 2)
    # both flips: no rot-180 view unless asked for; order plain, h, v, (hv); then the other scales
    t = T(hflip=True, vflip=True, flip_pairs=((0, 1), (2, 3)))
    assert [(v.hflip, v.vflip) for v in t.views(75, 100)] == [(False, False), (True, False), (False, True)]
    co = t.plan(1, 5, 75, 100).coefficients()
    assert co[2].tolist()[:4] == [-1.0, 9.0, 1.0, 0.0] and np.array_equal(co[:, 4], [1 / 3] * 3)
    t4 = T(hflip=True, vflip=True, hvflip=True, flip_pairs=((0, 1), (2, 3)))
    assert [(v.hflip, v.vflip) for v in t4.views(75, 100)][3] == (True, True) and t4.n_views == 4
    # an odd number of flips exchanges the pairs, two flips do not (WarpPlan's rule)
    assert np.array_equal(t4.perm(5), [[0, 1, 2, 3, 4], [1, 0, 3, 2, 4], [1, 0, 3, 2, 4], [0, 1, 2, 3, 4]])
    with pytest.raises(ValueError):
        T(flip_pairs=((0, 7),)).perm(4)
    t = T(scales=(0.75, 1.0, 1.25))
    vs = t.views(96, 128)
    assert [(v.scale, v.hflip) for v in vs] == [(1.0, False), (1.0, True), (0.75, False), (0.75, True),
                                                (1.25, False), (1.25, True)]
    assert vs[0].hw == (96, 128) and vs[2].hw == (72, 96) and vs[4].hw == (120, 160)
    assert T(scales=(1.0, 0.1)).views(96, 128)[2].hw == (32, 32)                # never below 32
    assert t.plan(1, 2, 96, 128).lattices == [(12, 16)] * 2 + [(9, 12)] * 2 + [(15, 20)] * 2
    # weights: any scale, normalised in float64, one per view
    t = T(weights=(2, 1, 1, 0), vflip=True, hvflip=True)
    assert np.array_equal(t.weights, [0.5, 0.25, 0.25, 0.0]) and t.weights.dtype == np.float64
    w3 = T(vflip=True).weights
    assert w3.sum() == pytest.approx(1.0, abs=1e-15) and np.all(w3 == w3[0])
    for bad in (dict(weights=(1, 1, 1)), dict(weights=(1, -1)), dict(weights=(0, 0)), dict(mode="mean"),
                dict(filter="nearest"), dict(scales=(0.5, 2.0)), dict(scales=(1.0, 1.0)), dict(hvflip=True),
                dict(scales=(1.0, 0.0))):
        with pytest.raises(ValueError):
            T(**bad)
    # more than 8 views
    assert T(vflip=True, hvflip=True, scales=(1.0, 0.5)).n_views == 8
    with pytest.raises(ValueError, match="at most 8"):
        T(vflip=True, scales=(1.0, 0.75, 1.25))
    with pytest.raises(ValueError, match="at most 8"):
        T(hflip=False, scales=tuple(1.0 + 0.1 * i for i in range(9)))
    # scaled views of fp32 input: refused, and said so
    with pytest.raises(HkpError, match="uint8"):
        T(scales=(1.0, 0.75)).view_inputs(torch.zeros(1, 3, 96, 128))
    with pytest.raises(HkpError, match="uint8"):
        T(scales=(1.0, 0.75)).check_input(torch.zeros(1, 3, 96, 128))
    # flips of both layouts are plumbing and run anywhere
    x = torch.arange(2 * 3 * 4 * 5, dtype=torch.float32).reshape(2, 3, 4, 5)
    xs = T(vflip=True, hvflip=True).view_inputs(x)
    assert xs[0] is x and torch.equal(xs[1], x.flip(3)) and torch.equal(xs[2], x.flip(2))
    assert torch.equal(xs[3], x.flip(2).flip(3))
    u = torch.arange(2 * 4 * 5 * 3, dtype=torch.uint8).reshape(2, 4, 5, 3)
    us = T(vflip=True).view_inputs(u)
    assert us[0] is u and torch.equal(us[1], u.flip(2)) and torch.equal(us[2], u.flip(1))
    # MergePlan validates on the host
    for bad in (dict(views=[]), dict(views=[(1, 1, 1, 0, 1, 0, 1)] * 9), dict(views=[(0, 1, 1, 0, 1, 0, 1)]),
                dict(views=[(1, 1, float("nan"), 0, 1, 0, 1)]), dict(perm=[[2, 0]]), dict(perm=[[0]]), dict(n=0)):
        kw = dict(n=1, k=2, hw=(1, 1), views=[(1, 1, 1, 0, 1, 0, 1)], perm=[[0, 1]])
        kw.update(bad)
        if "views" in bad and "perm" not in bad:
            kw["perm"] = [[0, 1]] * len(bad["views"])
        with pytest.raises(HkpError):
            tta.MergePlan(**kw)


def test_config_keys():
    from hkp import tta
    from hkp.metrics import from_config
    mt, kw = from_config({"thresholds": (2, 4), "max_peaks": 3}, 4)
    assert "tta" not in kw                                                      # as before
    mt, kw = from_config({"thresholds": (2, 4), "tta": {"hflip": True, "flip_pairs": ((0, 1),), "mode": "logit"}}, 4)
    assert isinstance(kw["tta"], tta.TestTimeAugmentation) and kw["tta"].mode == "logit" and kw["max_peaks"] == 4
    assert kw["tta"].flip_pairs == ((0, 1),)
    with pytest.raises(ValueError, match="rotate"):
        from_config({"tta": {"rotate": 90}}, 4)                                 # EVAL
    with pytest.raises(ValueError, match="unknown keys"):
        from_config({"ttaa": {}}, 4)
    rest, t = tta.split_config({"max_peaks": 3, "tta": {"vflip": True}})        # PEAKS
    assert rest == {"max_peaks": 3} and t.n_views == 3
    assert tta.split_config(None) == (None, None) and tta.split_config({"radius": 2}) == ({"radius": 2}, None)
    with pytest.raises(ValueError, match="rotate"):
        tta.split_config({"max_peaks": 3, "tta": {"rotate": 90}})
    with pytest.raises(ValueError):
        tta.split_config({"tta": True})
    import config
    assert "tta" in config.__doc__ and config.PEAKS is None and config.EVAL is None


def test_bad_arguments_leave_out_untouched():
    """Every limit of hkp_logits_merge is checked on the host arguments alone: the
    call returns HKP_ERR_BAD_ARG before a device is touched (this runs without one),
    so `out` — host memory here — keeps its bytes."""
    from hkp import _lib
    L = _lib.lib()
    out = np.full(64, 7.25, dtype=np.float32)
    packed = np.zeros(64, dtype=np.float32)
    table = (_lib.MergeView * 8)()
    perm = np.zeros(64, dtype=np.int32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    good = dict(n=1, k=1, h=2, w=2, views=1, mode=0, packed=P(packed), table=ctypes.c_void_p(ctypes.addressof(table)),
                perm=P(perm), out=P(out))
    order = ("n", "k", "h", "w", "views", "mode", "packed", "table", "perm", "out")
    bad = [dict(n=0), dict(k=0), dict(h=0), dict(w=-1), dict(views=0), dict(views=9), dict(views=-1), dict(mode=2),
           dict(mode=-1), dict(packed=None), dict(table=None), dict(perm=None), dict(out=None),
           dict(out=ctypes.c_void_p(out.ctypes.data + 2)), dict(packed=ctypes.c_void_p(packed.ctypes.data + 1)),
           dict(table=ctypes.c_void_p(ctypes.addressof(table) + 4)), dict(n=1 << 20, k=1 << 20, h=1 << 10, w=1 << 10)]
    for b in bad:
        a = dict(good)
        a.update(b)
        rc = L.hkp_logits_merge(*[a[k] for k in order], None)
        assert rc == -1, (b, rc)                              # HKP_ERR_BAD_ARG
        assert L.hkp_last_error().decode().startswith("hkp_logits_merge"), b
        with pytest.raises(_lib.HkpError, match="hkp_logits_merge"):
            _lib.call("hkp_logits_merge", *[a[k] for k in order], None)
    assert (out == 7.25).all()
    assert _lib.HKP_MERGE_MAX_VIEWS == 8 and (_lib.HKP_MERGE_LOGIT, _lib.HKP_MERGE_PROB) == (0, 1)
    assert ctypes.sizeof(_lib.MergeView) == 64 and _lib.MergeView.weight.offset == 48
