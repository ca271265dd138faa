"""Multi-instance and absent keypoints, the host side: the numpy restatement of the
target and the loss (tests/_instances_ref.py; the kernels are held to the existing
single-instance kernels and to it in tests/test_gpu_instances.py), the labels through
WarpPlan / ResamplePlan.apply_points and GeometricAugmentation, and the loader's
label files.  No GPU."""
import numpy as np
import pytest
import torch

import _instances_ref as iref
import _tail_ref as tref

NAN = float("nan")


def _pts(rows):
    return np.array(rows, dtype=np.float32)


# ------------------------------------------------------- the restatement ----

def test_target_is_the_maximum_not_the_sum():
    H, W, s = 21, 33, 3.0
    pts = _pts([[[[8.0, 10.0, 1.0], [12.5, 9.25, 1.0], [0.0, 0.0, 0.0]]]])
    t = iref.gauss_target_multi(pts, H, W, s)[0, 0]
    a = iref.gauss_target_multi(pts[:, :, :1], H, W, s)[0, 0]
    b = iref.gauss_target_multi(pts[:, :, 1:2], H, W, s)[0, 0]
    assert np.array_equal(t, np.maximum(a, b))
    assert t.max() == 1.0 and t[10, 8] == 1.0            # an instance on a pixel keeps a peak of exactly 1
    assert (a + b).max() > 1.0                           # which the sum would not
    # the single Gaussian, in the reference's fp32 order
    f = np.float32
    yy, xx = np.mgrid[0:H, 0:W].astype(f)
    d2 = ((xx - f(8)) * (xx - f(8)) + (yy - f(10)) * (yy - f(10))).astype(f)
    assert np.array_equal(a, np.exp(-d2 / f(2 * s * s), dtype=f).astype(np.float64))


def test_empty_slots_do_not_reach_the_result():
    H, W = 9, 11
    clean = _pts([[[[0.0, 0.0, 0.0], [4.0, 3.0, 1.0], [0.0, 0.0, 0.0], [7.5, 2.5, 2.0]],
                   [[0.0, 0.0, 0.0]] * 4]])
    dirty = clean.copy()
    dirty[0, 0, 0] = (NAN, NAN, 0.0)                     # the pattern 0,1,0,1, NaN in the empty slots
    dirty[0, 0, 2] = (np.inf, -5.0, 0.0)
    dirty[0, 1, :, :2] = NAN                             # an absent plane full of NaN
    dirty[0, 1, 3, 2] = NAN                              # a NaN flag is not a present slot
    assert iref.present(dirty).tolist() == [[[False, True, False, True], [False] * 4]]
    t = iref.gauss_target_multi(dirty, H, W, 2.0)
    assert np.isfinite(t).all() and np.array_equal(t, iref.gauss_target_multi(clean, H, W, 2.0))
    assert (t[0, 1] == 0).all() and t[0, 0].max() == 1.0
    p = tref.rand(1, 2, H, W, seed=3).sigmoid().numpy()
    for kind in ("bce", "mse"):
        for absent in ("zero", "ignore"):
            l, g = iref.heat_loss_multi(p, dirty, 2.0, kind, absent)
            l2, g2 = iref.heat_loss_multi(p, clean, 2.0, kind, absent)
            assert np.isfinite(l) and np.isfinite(g).all() and l == l2 and np.array_equal(g, g2)


@pytest.mark.parametrize("kind", ["bce", "mse"])
def test_absent_modes_against_torch(kind):
    """"zero": nn.BCELoss / nn.MSELoss over every plane against the dense target;
    "ignore": the same over the active planes alone, zero gradient elsewhere."""
    H, W = 13, 17
    pts = _pts([[[[5.0, 6.0, 1.0], [0.0, 0.0, 0.0]], [[NAN, NAN, 0.0], [0.0, 0.0, 0.0]],
                 [[20.0, 3.0, 1.0], [2.25, 9.5, 1.0]]]])
    p = tref.rand(1, 3, H, W, seed=5).sigmoid()
    y = torch.from_numpy(iref.gauss_target_multi(pts, H, W, 2.5))
    want_l, want_g = tref.loss_ref(p, y, kind)
    l, g = iref.heat_loss_multi(p.numpy(), pts, 2.5, kind, "zero")
    assert abs(l - want_l.item()) <= 1e-14 * abs(want_l.item())
    np.testing.assert_allclose(g, want_g.numpy(), rtol=2e-7, atol=0)
    act = [0, 2]
    want_l, want_g = tref.loss_ref(p[:, act].contiguous(), y[:, act].contiguous(), kind)
    l, g = iref.heat_loss_multi(p.numpy(), pts, 2.5, kind, "ignore")
    assert abs(l - want_l.item()) <= 1e-14 * abs(want_l.item())
    np.testing.assert_allclose(g[:, act], want_g.numpy(), rtol=2e-7, atol=0)
    assert (g[:, 1] == 0).all() and not np.signbit(g[:, 1]).any()


def test_no_active_plane_gives_zero():
    pts = np.zeros((2, 3, 4, 3), dtype=np.float32)
    pts[..., :2] = NAN
    p = tref.rand(2, 3, 5, 7, seed=1).sigmoid().numpy()
    for kind in ("bce", "mse"):
        l, g = iref.heat_loss_multi(p, pts, 8.0, kind, "ignore")
        assert l == 0.0 and (g == 0).all() and not np.signbit(g).any()
        l, g = iref.heat_loss_multi(p, pts, 8.0, kind, "zero")     # as negatives they do count
        assert l > 0 and np.isfinite(g).all() and (g > 0).all()


def test_round_trip_with_the_decode_restated():
    """The target's lattice samples through the multi-peak decode's restatement
    (tests/_peaks_ref.py) give every instance back: the counts, and each position to
    the 1e-4 px of test_peaks_cpu's ideal Gaussians.  The max rule is what keeps log t
    a parabola around each peak."""
    import _peaks_ref as pref
    (H, W), pts = iref.RT_IMAGE, iref.roundtrip_pts()
    for k, inst in enumerate(iref.RT_POINTS):              # the setup is what the comment in _instances_ref says
        border = 16 if len(inst) == 3 else 24
        for a, (u, v) in enumerate(inst):
            assert border <= u <= W - 1 - border and border <= v <= H - 1 - border
            assert min(abs(u / 8 - round(u / 8)), abs(v / 8 - round(v / 8))) > 0.05
            assert all(np.hypot(u - u2, v - v2) >= 24 for u2, v2 in inst[a + 1:])
    low = iref.lowres_logits(iref.gauss_target_multi(pts, H, W, iref.RT_SIGMA))
    assert low.shape == (1, 4) + iref.RT_LATTICE and np.isfinite(low).all()
    peaks, counts = pref.heat_peaks(low, H, W, max_peaks=4, radius=1, threshold=0.5)
    for k, (c, want, err) in enumerate(iref.roundtrip_errors(peaks, counts)):
        print("plane %d: %d peaks for %d instances, worst %.3g px" % (k, c, want, err))
        assert c == want and err <= 1e-4


# ---------------------------------------------------------- apply_points ----

def test_warp_plan_apply_points():
    from hkp import geometry as G
    h, w = 48, 64
    M = [G.affine_matrix(h, w, translate_xy_px=(10.0, 0.0)), G.affine_matrix(h, w, hflip=True)]
    plan = G.WarpPlan(M, (h, w), flipped=[False, True], flip_pairs=[(0, 1)])
    pts = _pts([[[[53.0, 20.0, 1.0], [53.5, 20.0, 1.0], [NAN, 7.0, 0.0]],       # lands on u = w-1 / just outside
                 [[5.0, 47.0, 1.0], [0.0, 0.0, 0.0], [10.0, 10.0, 3.0]]],
                [[[0.0, 0.0, 1.0], [NAN, NAN, 0.0], [63.0, 47.0, 1.0]],
                 [[20.0, 30.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]]])
    out = plan.apply_points(pts)
    assert out.dtype == np.float32 and out.shape == pts.shape
    assert out[0, 0, 0].tolist() == [63.0, 20.0, 1.0]                # on the edge: stays present
    assert out[0, 0, 1].tolist() == [63.5, 20.0, 0.0]                # just outside: absent, not clipped
    assert np.isnan(out[0, 0, 2, 0]) and out[0, 0, 2, 1:].tolist() == [7.0, 0.0]   # empty slots untouched
    assert out[0, 1].tolist() == [[15.0, 47.0, 1.0], [0.0, 0.0, 0.0], [20.0, 10.0, 3.0]]
    # image 1 was flipped: u -> w-1-u, and the keypoint rows 0 and 1 change places as whole [M,3] rows
    assert out[1, 0].tolist() == [[43.0, 30.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    assert out[1, 1, 0].tolist() == [63.0, 0.0, 1.0] and out[1, 1, 2].tolist() == [0.0, 47.0, 1.0]
    assert np.isnan(out[1, 1, 1, :2]).all() and out[1, 1, 1, 2] == 0
    t = plan.apply_points(torch.from_numpy(pts))                      # a CPU tensor comes back as one
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), out, equal_nan=True)
    assert np.array_equal(pts[0, 0, 0], _pts([53.0, 20.0, 1.0]))     # the input is not written
    # on in-frame points of [K,2] labels the result is apply_uv's
    rng = np.random.default_rng(0)
    uv = np.stack([rng.uniform(12, 50, (2, 5)), rng.uniform(3, 44, (2, 5))], -1).astype(np.float32)
    rot = G.WarpPlan([G.affine_matrix(h, w, rotate_deg=7, scale=1.05)] * 2, (h, w), flipped=[True, False],
                     flip_pairs=[(0, 4), (1, 2)])
    lifted = np.concatenate([uv, np.ones((2, 5, 1), np.float32)], -1)[:, :, None, :]
    got = rot.apply_points(lifted)
    assert (got[..., 2] == 1).all() and np.array_equal(got[:, :, 0, :2], rot.apply_uv(uv))
    with pytest.raises(G.HkpError):
        plan.apply_points(uv)


@pytest.mark.parametrize("mode", ["stretch", "fit"])
def test_resample_plan_apply_points(mode):
    from hkp.resample import ResamplePlan
    plan = ResamplePlan([(100, 200), (60, 40)], (48, 64), mode=mode)
    rng = np.random.default_rng(1)
    uv = np.stack([np.stack([rng.uniform(2, ws - 3, 4), rng.uniform(2, hs - 3, 4)], -1)
                   for hs, ws in ((100, 200), (60, 40))]).astype(np.float32)
    lifted = np.concatenate([uv, np.ones((2, 4, 1), np.float32)], -1)[:, :, None, :]
    got = plan.apply_points(lifted)
    assert (got[..., 2] == 1).all() and np.array_equal(got[:, :, 0, :2], plan.apply_uv(uv))
    # the rule itself, in both modes (half-pixel centres: (197 + 0.5) * 64 / 200 - 0.5 = 62.7 in stretch mode)
    pts = _pts([[[[197.0, 50.0, 1.0], [250.0, 50.0, 1.0], [NAN, NAN, 0.0]]],
                [[[20.0, 30.0, 1.0], [-30.0, 30.0, 1.0], [5.0, 5.0, 0.0]]]])
    out = plan.apply_points(pts)
    gain, org = plan._maps()
    for b in range(2):
        for j in range(2):
            q = ((pts[b, 0, j, :2].astype(np.float64) + 0.5) * gain[b, 0] - 0.5 + org[b, 0]).astype(np.float32)
            inside = 0 <= q[0] <= 63 and 0 <= q[1] <= 47
            assert np.array_equal(out[b, 0, j, :2], q) and out[b, 0, j, 2] == (1.0 if inside else 0.0)
    assert out[0, 0, 0, 2] == 1.0 and out[0, 0, 1, 2] == 0.0 and out[0, 0, 1, 0] > 63      # not clipped
    assert out[1, 0, 1, 2] == 0.0 and out[1, 0, 1, 0] < 0
    assert np.isnan(out[0, 0, 2, :2]).all() and out[1, 0, 2].tolist() == [5.0, 5.0, 0.0]


# -------------------------------------------------------------- sampling ----

def test_sample_with_points():
    from hkp import geometry as G
    hw = (48, 64)
    ga = G.GeometricAugmentation(seed=4, rotate=(-40, 40), translate=(-0.3, 0.3))
    rng = np.random.default_rng(2)
    later = 0
    for i in range(30):
        uv = np.stack([rng.uniform(0, 63, 3), rng.uniform(0, 47, 3)], -1).astype(np.float32)
        pts = np.concatenate([uv, np.ones((3, 1), np.float32)], -1)[:, None, :]
        want = ga.sample(i, 1, uv=uv, hw=hw)
        assert ga.sample(i, 1, pts=pts, hw=hw) == want          # all present: the same draws as with uv
        later += want["try"] != 0
        # empty slots, whatever they hold, are not tested: a far-away one would fail every draw
        padded = np.concatenate([pts, np.tile(_pts([1e6, NAN, 0.0]), (3, 1, 1))], 1)
        assert ga.sample(i, 1, pts=padded, hw=hw) == want
        # ... and a present one there does: the identity after `tries` draws
        padded[0, 1] = (1e6, 0.0, 1.0)
        assert ga.sample(i, 1, pts=padded, hw=hw)["try"] == -1
    assert later > 0                                            # keep_inside did reject draws
    none = np.zeros((3, 2, 3), np.float32)
    assert ga.sample(5, 0, pts=none, hw=hw) == ga.sample(5, 0)  # nothing present: the first draw
    free = G.GeometricAugmentation(seed=4, rotate=(-40, 40), translate=(-0.3, 0.3), keep_inside=False)
    assert free.sample(5, 0, pts=none, hw=hw) == ga.sample(5, 0)
    plan = ga.plan([0, 1], 1, pts=np.zeros((2, 3, 2, 3), np.float32), hw=hw)
    assert plan.n == 2 and np.array_equal(plan.matrices, ga.plan([0, 1], 1, hw=hw).matrices)
    with pytest.raises(G.HkpError):
        ga.sample(0, 0, uv=np.zeros((3, 2)), pts=none, hw=hw)


# --------------------------------------------------------------- dataset ----

def _label_folder(tmp_path, labels):
    (tmp_path / "images").mkdir()
    (tmp_path / "labels").mkdir()
    for i, a in enumerate(labels):
        np.save(tmp_path / "labels" / ("%05d.npy" % i), a)
    return str(tmp_path / "images"), str(tmp_path / "labels")


def test_dataset_pads_label_files_and_marks_outside_points(tmp_path):
    from src.dataset import KeypointsDataset, transform
    K, H, W = 2, 48, 64
    files = [np.array([[3.5, 40.0], [-2.0, 7.25]]),                                   # [K,2]
             np.array([[63.0, 47.0, 1.0], [10.0, 48.0, 1.0]]),                        # [K,3]
             np.array([[[5.0, 6.0, 1.0], [NAN, NAN, 0.0]], [[70.0, 1.0, 0.0], [7.0, 8.0, 2.0]]])]   # [K,2,3]
    imgs, labels = _label_folder(tmp_path, files)
    ds = KeypointsDataset(imgs, labels, K, H, W, transform, device="cpu", instances=3)
    assert len(ds) == 3 and all(a.shape == (K, 3, 3) and a.dtype == np.float32 for a in ds.labels_np)
    a, b, c = ds.labels_np
    assert a.tolist() == [[[3.5, 40.0, 1.0], [0, 0, 0], [0, 0, 0]],
                          [[-2.0, 7.25, 0.0], [0, 0, 0], [0, 0, 0]]]                 # outside: absent, not clipped
    assert b[:, 0].tolist() == [[63.0, 47.0, 1.0], [10.0, 48.0, 0.0]] and (b[:, 1:] == 0).all()
    assert c[0, 0].tolist() == [5.0, 6.0, 1.0] and np.isnan(c[0, 1, :2]).all() and c[0, 1, 2] == 0
    assert c[1].tolist() == [[70.0, 1.0, 0.0], [7.0, 8.0, 2.0], [0, 0, 0]]
    assert all(np.array_equal(t.numpy(), x, equal_nan=True) for t, x in zip(ds.labels, ds.labels_np))
    with pytest.raises(ValueError):
        KeypointsDataset(imgs, labels, K, H, W, transform, device="cpu", instances=1)   # the [K,2,3] file
    with pytest.raises(ValueError):
        KeypointsDataset(imgs, labels, K, H, W, transform, device="cpu", instances=17)


def test_dataset_without_instances_is_unchanged(tmp_path):
    from src.dataset import KeypointsDataset, transform
    K, H, W = 2, 48, 64
    files = [np.array([[3.5, 40.0], [-2.0, 7.25]]), np.array([[70.0, 50.0], [10.0, 20.0]])]
    imgs, labels = _label_folder(tmp_path, files)
    ds = KeypointsDataset(imgs, labels, K, H, W, transform, device="cpu")
    assert ds.instances is None
    assert [a.tolist() for a in ds.labels_np] == [[[3.5, 40.0], [0.0, 7.25]], [[63.0, 47.0], [10.0, 20.0]]]
    assert all(a.dtype == np.float32 and a.shape == (K, 2) for a in ds.labels_np)
    assert all(t.dtype == torch.float64 and t.shape == (K, 2) for t in ds.labels)


def test_config_defaults():
    import config
    assert config.INSTANCES is None and config.ABSENT == "zero"
