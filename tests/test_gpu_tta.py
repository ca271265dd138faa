"""hkp_logits_merge on the GPU: the kernel against its numpy restatement
(tests/_tta_ref.py, pinned in tests/test_tta_cpu.py), its exact cases, special
values and determinism, the round trip with hkp_heat_peaks on ideal targets, and
test-time augmentation through the model, the DP wrappers, train.fit and
analysis.main."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import _instances_ref as iref
import _peaks_ref as pref
import _tta_ref as ref
from conftest import PKG, REPO
from oracle import recipe

pytestmark = pytest.mark.gpu

MODES = (("logit", ref.LOGIT), ("prob", ref.PROB))
INF, NAN = float("inf"), float("nan")


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a, np.float32).view(np.uint32),
                                                 np.asarray(b, np.float32).view(np.uint32))


def _same_values(a, b):
    """Equal fp32 values, NaN where NaN (a NaN's payload is not part of the contract)."""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _views(kind, k, h, w):
    """[(h_v, w_v, ay, by, ax, bx, weight)], perm for one of the four view sets."""
    ident = list(range(k))
    swapped = [1, 0] + ident[2:] if k >= 2 else ident
    if kind == "identity":
        return [(h, w, 1.0, 0.0, 1.0, 0.0, 1.0)], [ident]
    if kind == "hflip":
        return [(h, w, 1.0, 0.0, 1.0, 0.0, 0.5), (h, w, 1.0, 0.0, -1.0, float(w - 1), 0.5)], [ident, swapped]
    if kind == "hvflip":
        third = 1.0 / 3.0
        return [(h, w, 1.0, 0.0, 1.0, 0.0, third), (h, w, 1.0, 0.0, -1.0, float(w - 1), third),
                (h, w, -1.0, float(h - 1), 1.0, 0.0, third)], [ident, swapped, swapped]
    assert kind == "lattices"
    out = []
    for (hv, wv), wt, (sy, oy, sx, ox) in zip(((4, 6), (5, 7), (9, 11)), (0.5, 0.3, 0.2),
                                              ((1.0, 0.0, 1.0, 0.0), (1.1, -0.3, -1.05, 0.2), (0.9, 0.4, 1.2, -0.7))):
        ay = sy * (hv - 1) / (h - 1) if h > 1 else 0.37
        ax = abs(sx) * (wv - 1) / (w - 1) if w > 1 else 0.37
        bx = ox if sx > 0 else (wv - 1) - ox                  # the second lattice is seen mirrored
        out.append((hv, wv, ay, oy, ax if sx > 0 else -ax, bx, wt))
    return out, [ident, swapped, ident]


def _lows(views, n, k, seed):
    rng = np.random.default_rng(seed)
    return [(4.0 * rng.standard_normal((n, k, v[0], v[1]))).astype(np.float32) for v in views]


def _plan(lows, views, perm, hw):
    from hkp.tta import MergePlan
    return MergePlan(lows[0].shape[0], lows[0].shape[1], hw, views, perm)


def _gpu_merge(lows, views, perm, hw, mode, dev, out=None):
    from hkp import ops
    ts = [torch.from_numpy(a).to(dev) for a in lows]
    got = ops.logits_merge(ts, _plan(lows, views, perm, hw), mode=mode, out=out)
    assert out is None or got is out
    assert tuple(got.shape) == tuple(lows[0].shape[:2]) + tuple(hw) and got.dtype == torch.float32
    return got.cpu().numpy()


def _check(lows, views, perm, hw, dev, out_of=None):
    for name, code in MODES:
        want = ref.merge(lows, [v[2:] for v in views], perm, hw, code)
        got = _gpu_merge(lows, views, perm, hw, name, dev, None if out_of is None else out_of())
        if code == ref.LOGIT:
            assert _same_values(got, want), (name, np.nanmax(np.abs(got - want)))
        else:
            assert ref.within_ulps(got, want, 1), (name, np.nanmax(np.abs(got - want)))


# -------------------------------------------- 1. kernel against restatement ----

@pytest.mark.parametrize("kind", ["identity", "hflip", "hvflip", "lattices"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 5, 7), (1, 2, 12, 16), (2, 4, 60, 80)])
def test_kernel_against_restatement(cuda_device, shape, kind):
    """LOGIT: only IEEE fp64 multiplies and adds and one rounding to fp32: equal values.
    PROB: the device's fp64 exp / log and numpy's differ by a few fp64 ulps, which moves
    the final fp32 rounding by at most one step.  (2,3,5,7): w % 4 != 0, the scalar path;
    (1,2,12,16) and (2,4,60,80): 16-byte stores."""
    n, k, h, w = shape
    views, perm = _views(kind, k, h, w)
    _check(_lows(views, n, k, 10 * sum(shape) + len(kind)), views, perm, (h, w), cuda_device)


@pytest.mark.parametrize("shape", [(2, 3, 211, 211), (4, 4, 256, 260)])
def test_more_than_one_grid_trip(cuda_device, shape):
    """The grid is capped at 1024 blocks of 256 threads: 267,126 scalar items and
    266,240 vector items (of 4) both take a second trip."""
    n, k, h, w = shape
    assert n * k * h * (w // 4 if w % 4 == 0 else w) > 1024 * 256
    views, perm = _views("hflip", k, h, w)
    _check(_lows(views, n, k, 7), views, perm, (h, w), cuda_device)


def test_out_one_element_off_alignment(cuda_device):
    """w % 4 == 0 but out starts 4 bytes past a 16-byte boundary: the scalar path, and
    nothing outside out is written."""
    n, k, h, w = 1, 2, 12, 16
    views, perm = _views("lattices", k, h, w)
    holder = []

    def out_of():
        big = torch.full((n * k * h * w + 8,), 123.0, device=cuda_device)
        assert big.data_ptr() % 16 == 0
        holder.append(big)
        return big[1:1 + n * k * h * w].view(n, k, h, w)
    _check(_lows(views, n, k, 11), views, perm, (h, w), cuda_device, out_of)
    for big in holder:
        assert big[0].item() == 123.0 and (big[1 + n * k * h * w:] == 123.0).all()


# ------------------------------------------------------------- 2. exact cases ----

def test_exact_cases(cuda_device):
    n, k, h, w = 2, 3, 5, 7
    views, perm = _views("identity", k, h, w)
    z = _lows(views, n, k, 21)[0]
    # PROB inverts the sigmoid in fp64: exact to fp32 rounding for ordinary logits (these are
    # N(0, 16) draws, 1e-3 < |z| < 20), not for a subnormal or beyond the +-700 clamp
    assert 1e-3 < np.abs(z).min() and np.abs(z).max() < 20
    assert ref.within_ulps(_gpu_merge([z], views, perm, (h, w), "prob", cuda_device), z, 1)
    z[0, 0, 0, :4] = (0.0, -0.0, 1e-40, -3e38)                # a signed zero, a subnormal, a large value
    assert _bits_equal(_gpu_merge([z], views, perm, (h, w), "logit", cuda_device), z)
    # a plane and its mirrored copy: (float)(0.5 (a + b)) formed by torch in fp64
    views, perm = _views("hflip", 1, h, w)
    a, b = (torch.from_numpy(x).to(cuda_device) for x in _lows(views, n, 1, 22))
    from hkp import ops
    got = ops.logits_merge([a, b], views, [[0], [0]], mode="logit")          # (the table form: views and perm)
    want = (0.5 * (a.double() + b.flip(3).double())).float()
    assert torch.equal(got, want)


# ---------------------------------------------------------- 3. special values ----

SPECIALS = (700.0, -700.0, 1e30, -1e30, INF, -INF, NAN)


def test_special_values(cuda_device):
    """One special logit per row, in column 3 of a 7 x 8 view read at half steps
    (ax = 0.5): node 6 reads it alone (weight 1), node 7 as the base tap of a lerp of
    weight 0.5, node 5 as the far tap, every other node not at all — for node 4
    (x0 = 2, fx = 0, x1 = 3) it is the far tap whose weight is exactly 0, and for all of
    them the taps of the next row (fy = 0).  The results are the restatement's.  PROB is finite
    wherever no NaN is read, with the one exception the definition itself makes: an
    infinity in the BASE tap of a fractional lerp gives z00 + fx (z01 - z00) =
    inf - inf = NaN (row +-inf, node 7); the restatement pins that too."""
    hv, wv, w = len(SPECIALS), 8, 12
    views, perm = [(hv, wv, 1.0, 0.0, 0.5, 0.0, 1.0)], [[0]]
    z = _lows(views, 1, 1, 31)[0]
    z[0, 0, :, 3] = SPECIALS
    got = {}
    for name, code in MODES:
        want = ref.merge([z], [v[2:] for v in views], perm, (hv, w), code)
        got[name] = _gpu_merge([z], views, perm, (hv, w), name, cuda_device)
        assert _same_values(got[name], want) if code == ref.LOGIT else ref.within_ulps(got[name], want, 1)
    bad = np.zeros((hv, w), dtype=bool)
    bad[6, 5:8] = True                                        # the NaN row: the three nodes that read it
    bad[4:6, 7] = True                                        # +-inf as the base tap of a fractional lerp
    assert np.array_equal(~np.isfinite(got["prob"][0, 0]), bad)
    assert np.array_equal(np.isnan(got["logit"][0, 0]), bad)
    assert got["logit"][0, 0, 4, 5] == INF and got["logit"][0, 0, 5, 6] == -INF
    # |z| >= 700 saturates: sigmoid(700) is 1 to within 1e-304, the merged logit is finite
    assert np.all(np.abs(got["prob"][0, 0, :6, 6]) > 600)
    # beside an exact copy and an exact flip nothing leaks: only the node itself and its mirror image
    views, perm = _views("hflip", 1, hv, wv)
    for name, code in MODES:
        want = ref.merge([z, z], [v[2:] for v in views], perm, (hv, wv), code)
        g = _gpu_merge([z, z], views, perm, (hv, wv), name, cuda_device)
        assert _same_values(g, want) if code == ref.LOGIT else ref.within_ulps(g, want, 1)
        hit = np.zeros((hv, wv), dtype=bool)
        hit[6, [3, 4]] = True
        assert np.array_equal(np.isnan(g[0, 0]), hit)
        if code == ref.PROB:
            assert np.isfinite(g[0, 0][~hit]).all()


# -------------------------------------------------------------- 4. determinism ----

def test_determinism(cuda_device):
    from hkp import ops
    n, k, h, w = 2, 4, 60, 80
    views, perm = _views("lattices", k, h, w)
    lows = _lows(views, n, k, 41)
    ts = [torch.from_numpy(a).to(cuda_device) for a in lows]
    plan = _plan(lows, views, perm, (h, w))
    for name, _ in MODES:
        a = ops.logits_merge(ts, plan, mode=name)
        b = ops.logits_merge(ts, plan, mode=name)
        buf = torch.full((n, k, h, w), NAN, device=cuda_device)
        c = ops.logits_merge(ts, plan, mode=name, out=buf)
        assert c is buf and a.data_ptr() != b.data_ptr()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32),
                                                                                     c.view(torch.int32))


def test_wrapper_rejects_before_a_launch(cuda_device, monkeypatch):
    from hkp import ops
    from hkp._lib import HkpError
    calls = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    views, perm = _views("hflip", 2, 5, 7)
    good = [torch.zeros((1, 2, 5, 7), device=cuda_device) for _ in range(2)]
    for lows, kw in (([good[0]], {}), ([good[0], good[1].double()], {}), ([good[0], good[1].cpu()], {}),
                     ([good[0], good[1][:, :, :, :6]], {}), ([good[0], torch.zeros((1, 2, 5, 6), device=cuda_device)], {}),
                     ([good[0], torch.zeros((2, 2, 5, 7), device=cuda_device)], {}), (good, dict(mode="mean")),
                     (good, dict(out=torch.zeros((2, 2, 5, 7), device=cuda_device))),
                     (good, dict(out=torch.zeros((1, 2, 5, 7), device=cuda_device, dtype=torch.float64)))):
        with pytest.raises(HkpError):
            ops.logits_merge(lows, views, perm, **kw)
    with pytest.raises(HkpError):
        ops.logits_merge(good, views, [[0, 1], [0, 2]])
    with pytest.raises(HkpError):
        ops.logits_merge(good, views, None)
    with pytest.raises(HkpError):
        ops.logits_merge([good[0]] * 9, [views[0]] * 9, [[0, 1]] * 9)
    assert calls == []
    ops.logits_merge(good, views, perm)
    assert calls == ["hkp_logits_merge"]


# ------------------------------------------------------------ 5. ideal targets ----

# The largest distance from an instance to its peak that the restatement (numpy, CPU)
# gives on the round trip's planes with the views 1.0, 0.75 and 1.25 x {plain, hflip},
# equal weights: 0.458204 px in LOGIT mode and 0.691050 px in PROB mode (the interpolated
# views flatten the Gaussian's log-parabola between their nodes; sigma = 8 px, nodes 8 px
# apart).  With flip views alone the restatement's error is 0 to the last fp32 place.
SCALED_ERR = {"logit": 0.458204, "prob": 0.691050}


def _ideal(scales, flips):
    views = ref.ideal_views(scales, flips)
    recs, lats = ref.ideal_table(views)
    return [ref.ideal_logits(v) for v in views], [lat + rec for lat, rec in zip(lats, recs)]


def test_ideal_targets_flip_views(cuda_device):
    """Flip views only: every instance comes back as in tests/test_gpu_instances.py.
    View 0 is the target kernel's own plane at the nodes; the mirrored views hold the
    same numbers mirrored (node j of a mirrored 81-px view stands on pixel 80 - 8 j)."""
    from hkp import ops
    (H, W), pts = iref.RT_IMAGE, torch.from_numpy(iref.roundtrip_pts())
    target = ops.gauss_target_multi(pts.to(cuda_device), H, W, iref.RT_SIGMA).cpu().numpy()
    low = iref.lowres_logits(target)
    h, w = iref.RT_LATTICE
    views, perm = _views("hvflip", 4, h, w)
    perm = [list(range(4))] * 3
    lows = [torch.from_numpy(np.ascontiguousarray(a)).to(cuda_device) for a in (low, low[..., ::-1], low[..., ::-1, :])]
    for name, _ in MODES:
        m = ops.logits_merge(lows, views, perm, mode=name)               # (all views on the base lattice)
        gp, gc = ops.heat_peaks(m, H, W, max_peaks=4, radius=1, threshold=0.5)
        for kk, (c, want, err) in enumerate(iref.roundtrip_errors(gp.cpu().numpy(), gc.cpu().numpy())):
            print("%s, plane %d: %d peaks for %d instances, worst %.3g px" % (name, kk, c, want, err))
            assert c == want and err <= 1e-4


@pytest.mark.parametrize("name,code", MODES)
def test_ideal_targets_scaled_views(cuda_device, name, code):
    from hkp import ops
    H, W = iref.RT_IMAGE
    lows, views = _ideal(ref.IDEAL_SCALES, [(False, False), (True, False)])
    perm = [list(range(4))] * len(views)
    # the condition, on the CPU: the restatement alone finds every instance, at the recorded error
    rm = ref.merge(lows, [v[2:] for v in views], perm, iref.RT_LATTICE, code)
    rp, rc = pref.heat_peaks(rm, H, W, max_peaks=4, radius=1, threshold=0.5)
    worst = 0.0
    for c, want, err in iref.roundtrip_errors(rp, rc):
        assert c == want
        worst = max(worst, err)
    print("restatement, %s: worst %.6f px" % (name, worst))
    assert abs(worst - SCALED_ERR[name]) <= 1e-5
    m = ops.logits_merge([torch.from_numpy(a).to(cuda_device) for a in lows],
                         _plan(lows, views, perm, iref.RT_LATTICE), mode=name)
    gp, gc = ops.heat_peaks(m, H, W, max_peaks=4, radius=1, threshold=0.5)
    gp, gc = gp.cpu().numpy(), gc.cpu().numpy()
    for kk, (c, want, err) in enumerate(iref.roundtrip_errors(gp, gc)):
        print("kernel, %s, plane %d: %d peaks for %d instances, worst %.6f px" % (name, kk, c, want, err))
        assert c == want and err <= 1.1 * SCALED_ERR[name]
    # and the kernel's peaks are the restatement's, to one fp32 ulp of position
    assert np.array_equal(gc, rc)
    for kk in range(4):
        a, b = gp[0, kk, :gc[0, kk], :2], rp[0, kk, :rc[0, kk], :2].astype(np.float32)
        assert np.all(np.abs(a - b) <= np.maximum(ref.ulp32(a), ref.ulp32(b))), (kk, a, b)


# --------------------------------------------------------------- 6. model layer ----

K_, H_, W_, B_ = 4, 96, 128, 2
PEAK_KW = dict(max_peaks=5, radius=2, threshold=0.05)
EVAL_TH = (2.0, 4.0, 8.0, 16.0)
PAIRS = ((0, 1),)
_cache = {}


def _model(dev, seed=61):
    from src.model import KeypointsGauss
    m = KeypointsGauss(K_, H_, W_, backbone="resnet18", pretrained=False)
    m.load_state_dict(recipe.seeded_state_dict("resnet18", seed))
    return m.to(dev)


def _shared(dev):
    if not _cache:
        _cache["m"] = _model(dev)
        _cache["u8"] = torch.from_numpy(recipe.seeded_images_u8(B_, H_, W_, 62)).to(dev)
        _cache["x"] = recipe.to_tensor_nchw(recipe.seeded_images_u8(B_, H_, W_, 62)).to(dev)
    return _cache["m"], _cache["x"], _cache["u8"]


def _labels(n, seed, dev=None):
    import _metrics_ref as mref
    _, _, lab = mref.random_batch(seed, n, K_, 4, 3, size=float(H_))
    t = torch.from_numpy(lab)
    return t if dev is None else t.to(dev)


def _tta(**kw):
    from hkp.tta import TestTimeAugmentation
    return TestTimeAugmentation(**kw)


def test_lowres_logits_flip(cuda_device):
    from hkp import net
    m, x, _ = _shared(cuda_device)
    t = _tta(hflip=True, mode="logit", flip_pairs=PAIRS)
    plain = lambda xx: net.keypoints_forward(m.resnet.net, xx, K_, heat=False, argmax=False, pol=m.policy,  # noqa: E731
                                             upsample=False)[2]
    a, b = plain(x), plain(x.flip(3))
    assert tuple(a.shape) == (B_, K_, 12, 16)
    assert torch.equal(m.lowres_logits(x), a)
    bb = b.flip(3)[:, [1, 0, 2, 3]]                            # mirrored back, the pair exchanged
    want = (0.5 * (a.double() + bb.double())).float()
    got = m.lowres_logits(x, tta=t)
    assert torch.equal(got, want)
    # the merge commutes with the flip
    again = m.lowres_logits(x.flip(3), tta=t).flip(3)[:, [1, 0, 2, 3]]
    assert torch.equal(got, again)
    # PROB: the logit of the mean probability, to fp32 rounding
    gp = m.lowres_logits(x, tta=_tta(hflip=True, flip_pairs=PAIRS))
    p = 0.5 * (torch.sigmoid(a.double()) + torch.sigmoid(bb.double()))
    assert torch.allclose(gp.double(), torch.log(p) - torch.log1p(-p), rtol=1e-6, atol=1e-6)


def test_predict_and_evaluate_with_tta(cuda_device):
    from hkp import ops, parallel
    from hkp.metrics import KeypointMetrics
    from src.prediction import Prediction
    m, x, _ = _shared(cuda_device)
    t = _tta(hflip=True, vflip=True, flip_pairs=PAIRS)
    low = m.lowres_logits(x, tta=t)
    wp, wc = ops.heat_peaks(low, H_, W_, **PEAK_KW)
    assert int(wc.sum()) > 0
    lab = _labels(B_, 63, cuda_device)
    hist = torch.zeros((K_, len(EVAL_TH), 2, 1024), dtype=torch.int64, device=cuda_device)
    totals = torch.zeros((K_, 8), dtype=torch.int64, device=cuda_device)
    ops.peaks_match(wp, wc, lab, EVAL_TH, hist, totals, bins=1024)
    for run in (lambda: m.predict_peaks(x, tta=t, **PEAK_KW),
                lambda: Prediction(m, K_, H_, W_, True).peaks(x, tta=t, **PEAK_KW),
                lambda: parallel.predict_peaks_dp(m, x, tta=t, **PEAK_KW)):
        gp, gc = run()
        assert torch.equal(gp, wp) and torch.equal(gc, wc)
    for run in (lambda mt: m.evaluate(x, lab, mt, tta=t, **PEAK_KW),
                lambda mt: Prediction(m, K_, H_, W_, True).evaluate(x, lab, mt, tta=t, **PEAK_KW),
                lambda mt: parallel.evaluate_dp(m, x, lab, mt, tta=t, **PEAK_KW)):
        mt = KeypointMetrics(K_, EVAL_TH)
        gp, gc = run(mt)
        assert torch.equal(gp, wp) and torch.equal(gc, wc)
        hh, tt = mt.state()
        assert torch.equal(hh, hist.cpu()) and torch.equal(tt, totals.cpu())


def test_tta_none_reaches_the_same_calls(cuda_device, monkeypatch):
    """tta=None: the library calls of predict_peaks are those of one forward and the
    decode, as before; with the flip test: two forwards, one merge, one decode."""
    from hkp import net, ops
    m, x, _ = _shared(cuda_device)
    m.predict_peaks(x, **PEAK_KW)                            # (the first forward packs the weights, once)
    names = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    low = net.keypoints_forward(m.resnet.net, x, K_, heat=False, argmax=False, pol=m.policy, upsample=False)[2]
    ops.heat_peaks(low, H_, W_, **PEAK_KW)
    before, names[:] = list(names), []
    m.predict_peaks(x, **PEAK_KW)
    none, names[:] = list(names), []
    assert none == before and before[-1] == "hkp_heat_peaks" and "hkp_logits_merge" not in none
    from hkp.metrics import KeypointMetrics
    m.evaluate(x, _labels(B_, 63, cuda_device), KeypointMetrics(K_, EVAL_TH), **PEAK_KW)
    ev, names[:] = list(names), []
    assert ev == before + ["hkp_peaks_match"]
    m.predict_peaks(x, tta=_tta(), **PEAK_KW)
    assert names == before[:-1] * 2 + ["hkp_logits_merge", "hkp_heat_peaks"]


def test_scaled_views_of_a_uint8_batch(cuda_device, monkeypatch):
    from hkp import ops
    from hkp._lib import HkpError
    m, x, u8 = _shared(cuda_device)
    t = _tta(hflip=False, scales=(0.75, 1.0))
    seen = []
    real = ops.logits_merge
    monkeypatch.setattr(ops, "logits_merge", lambda lows, plan, **kw: (seen.append((lows, plan)), real(lows, plan, **kw))[1])
    low = m.lowres_logits(u8, tta=t)
    (lows, plan), = seen
    assert [tuple(a.shape) for a in lows] == [(B_, K_, 12, 16), (B_, K_, 9, 12)]
    assert plan.lattices == t.plan(B_, K_, H_, W_).lattices == [(12, 16), (9, 12)] and plan.n_views == 2
    assert [v.hw for v in t.views(H_, W_)] == [(96, 128), (72, 96)]
    assert tuple(low.shape) == (B_, K_, 12, 16) and torch.isfinite(low).all()
    assert torch.equal(lows[0], m.lowres_logits(u8))
    # steady state: the second call uploads nothing new (the same device table)
    m.lowres_logits(u8, tta=t)
    assert seen[1][1] is plan
    pk, ct = m.predict_peaks(u8, tta=t, **PEAK_KW)
    assert tuple(pk.shape) == (B_, K_, 5, 3)
    # an fp32 batch with scales: refused before any launch
    names = []
    real_call = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real_call(name, *a))[1])
    with pytest.raises(HkpError, match="uint8"):
        m.lowres_logits(x, tta=t)
    with pytest.raises(HkpError, match="uint8"):
        m.predict_peaks(x, tta=t)
    assert names == []


# ---- data parallel: gloo world 2 on one GPU, as tests/test_gpu_metrics.py

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, q):
    import sys
    sys.path[:0] = [REPO, PKG, os.path.join(REPO, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from hkp import parallel
        from hkp.metrics import KeypointMetrics
        dev = torch.device("cuda:0")
        m = _model(dev)
        t = _tta(hflip=True, flip_pairs=PAIRS)
        lo, hi = parallel.shard_range(4, rank, world)
        x = recipe.to_tensor_nchw(recipe.seeded_images_u8(4, H_, W_, 64))[lo:hi].to(dev)
        lab = _labels(4, 65)[lo:hi].contiguous().to(dev)
        pk, ct = parallel.predict_peaks_dp(m, x, tta=t, **PEAK_KW)
        mt = KeypointMetrics(K_, EVAL_TH)
        parallel.evaluate_dp(m, x, lab, mt, tta=t, **PEAK_KW)
        mt.all_reduce()
        hh, tt = mt.state()
        # SyncBN: every rank makes the same forwards in the same order, view by view
        spk, sct = parallel.predict_peaks_dp(m, x, tta=t, sync=True, global_batch=4, **PEAK_KW)
        torch.cuda.synchronize()
        q.put(dict(rank=rank, peaks=pk.cpu().numpy(), counts=ct.cpu().numpy(), hist=hh.numpy(), totals=tt.numpy(),
                   sync_shape=tuple(spk.shape), sync_counts=sct.cpu().numpy()))
        dist.destroy_process_group()
    except Exception as e:            # report instead of hanging the parent on q.get
        q.put(dict(rank=rank, error=repr(e)))
        raise


def test_dp_gloo_world2(cuda_device):
    """Two ranks on one GPU, each its half of a batch of 4 (per-shard BN statistics):
    the gathered peaks and the summed integers are those of the two halves run here."""
    from hkp import ops
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(60)
    assert all("error" not in r for r in res), res
    assert all(p.exitcode == 0 for p in procs)
    m = _model(cuda_device)
    t = _tta(hflip=True, flip_pairs=PAIRS)
    x = recipe.to_tensor_nchw(recipe.seeded_images_u8(4, H_, W_, 64)).to(cuda_device)
    lab = _labels(4, 65, cuda_device)
    hist = torch.zeros((K_, len(EVAL_TH), 2, 1024), dtype=torch.int64, device=cuda_device)
    totals = torch.zeros((K_, 8), dtype=torch.int64, device=cuda_device)
    pks, cts = [], []
    for lo, hi in ((0, 2), (2, 4)):
        pk, ct = m.predict_peaks(x[lo:hi], tta=t, **PEAK_KW)
        ops.peaks_match(pk, ct, lab[lo:hi].contiguous(), EVAL_TH, hist, totals, bins=1024)
        pks.append(pk)
        cts.append(ct)
    wp, wc = torch.cat(pks).cpu().numpy(), torch.cat(cts).cpu().numpy()
    assert int(wc.sum()) > 0
    for r in res:
        assert np.array_equal(r["peaks"], wp) and np.array_equal(r["counts"], wc), r["rank"]
        assert np.array_equal(r["hist"], hist.cpu().numpy()) and np.array_equal(r["totals"], totals.cpu().numpy())
        assert r["sync_shape"] == (4, K_, 5, 3)
    assert np.array_equal(res[0]["sync_counts"], res[1]["sync_counts"])


# ---- train.fit and analysis.main

def test_fit_eval_with_tta(cuda_device, tmp_path, monkeypatch, capsys):
    """EVAL's "tta": the plain forward still gives `test loss:` and is view 0; the other
    view is one more forward under no_grad; the `test eval:` line is that of
    evaluate(tta=...)."""
    import train as train_mod
    from hkp import net
    from hkp.metrics import KeypointMetrics
    dev = cuda_device
    imgs = recipe.to_tensor_nchw(recipe.seeded_images_u8(4, H_, W_, 71))
    lab = _labels(4, 72)
    test_data = [(imgs[:2], lab[:2]), (imgs[2:], lab[2:])]
    monkeypatch.setattr(train_mod, "_bucketer", None)

    def run(cfg):
        monkeypatch.setattr(train_mod, "EVAL", cfg)
        m = _model(dev, 73)
        monkeypatch.setattr(train_mod, "optimizer", torch.optim.SGD(m.parameters(), lr=0.0))
        calls = []
        real = net.keypoints_forward
        monkeypatch.setattr(net, "keypoints_forward", lambda *a, **kw: (calls.append(
            (torch.is_grad_enabled(), kw.get("heat"), kw.get("upsample", True))), real(*a, **kw))[1])
        capsys.readouterr()
        train_mod.fit([], test_data, m, epochs=1, checkpoint_path=str(tmp_path))
        monkeypatch.setattr(net, "keypoints_forward", real)
        return capsys.readouterr().out.strip().split("\n"), calls

    base = dict(thresholds=EVAL_TH, **PEAK_KW)
    plain, calls0 = run(base)
    assert calls0 == [(False, True, True)] * 2
    lines, calls = run(dict(base, tta={"hflip": True, "flip_pairs": PAIRS}))
    assert calls == [(False, True, True), (False, False, False)] * 2
    assert [ln.split(":")[0] for ln in lines] == ["train loss", "test loss", "test eval"]
    assert lines[1] == plain[1]                               # the same forward, the same loss
    m = _model(dev, 73)
    mt = KeypointMetrics(K_, EVAL_TH)
    for x, lb in test_data:
        m.evaluate(x.to(dev), lb.to(dev), mt, tta=_tta(hflip=True, flip_pairs=PAIRS), **PEAK_KW)
    assert lines[2] == "test eval: " + mt.summary()
    with pytest.raises(ValueError, match="unknown keys"):
        run(dict(base, tta={"rotate": 90}))


def test_analysis_peaks_with_tta(tmp_path, monkeypatch, cuda_device):
    """analysis.main with PEAKS = {..., "tta": {...}}: peaks.npy is predict_peaks(tta=...)
    of each image; keypoints.npy is what it is without."""
    import analysis as analysis_mod
    from PIL import Image
    from src.dataset import transform
    from src.model import KeypointsGauss
    BB, K, H, W = "resnet34", 4, 64, 96
    kw = {"max_peaks": 3, "radius": 1, "threshold": 0.1}
    tcfg = {"hflip": True, "vflip": True, "flip_pairs": PAIRS, "mode": "logit"}
    for name, v in (("IMG_HEIGHT", H), ("IMG_WIDTH", W)):
        monkeypatch.setattr(analysis_mod, name, v)
    assert (analysis_mod.BACKBONE, analysis_mod.NUM_KEYPOINTS, analysis_mod.PEAKS) == (BB, K, None)
    sd = recipe.seeded_state_dict(BB, 91)
    (tmp_path / "ck").mkdir()
    torch.save(sd, tmp_path / "ck" / "m.pth")
    (tmp_path / "imgs").mkdir()
    srcs = [recipe.seeded_images_u8(1, H, W, 92 + i)[0] for i in range(2)]
    for i, bgr in enumerate(srcs):
        Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(tmp_path / "imgs" / ("f%d.png" % i))
    run = lambda out: analysis_mod.main("m.pth", str(tmp_path / "imgs"), out_dir=str(tmp_path / out),    # noqa: E731
                                        checkpoint_dir=str(tmp_path / "ck"))
    monkeypatch.setattr(analysis_mod, "PEAKS", dict(kw))
    kp_plain = run("plain")
    monkeypatch.setattr(analysis_mod, "PEAKS", dict(kw, tta=tcfg))
    kp = run("preds")
    assert np.array_equal(kp, kp_plain)
    assert np.array_equal(np.load(tmp_path / "preds" / "keypoints.npy"), np.load(tmp_path / "plain" / "keypoints.npy"))
    peaks, counts = np.load(tmp_path / "preds" / "peaks.npy"), np.load(tmp_path / "preds" / "peak_counts.npy")
    assert not np.array_equal(peaks, np.load(tmp_path / "plain" / "peaks.npy"))
    m = KeypointsGauss(K, H, W, backbone=BB, pretrained=False)
    m.load_state_dict(sd)
    m = m.to(cuda_device)
    for i, frame in enumerate(srcs):
        pk, ct = m.predict_peaks(transform(frame).to(cuda_device)[None], tta=_tta(**tcfg), **kw)
        assert np.array_equal(counts[i:i + 1], ct.cpu().numpy()) and np.array_equal(peaks[i:i + 1], pk.cpu().numpy()), i
    monkeypatch.setattr(analysis_mod, "PEAKS", dict(kw, tta={"rotate": 90}))
    with pytest.raises(ValueError, match="unknown keys"):
        run("bad")
