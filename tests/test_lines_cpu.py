"""Line labels without a GPU: the numpy restatement of hkp_line_target against float64
geometry, the label helpers of hkp.lines, apply_lines of both plans, the scenes' line class,
and every rejection from the C entry up to Trainer."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import _lines_ref as ref

F = np.float32


# ---- the restatement

def _seeded_planes(R, seed, cases=50):
    """(rec [s,5], H, W) cases with coordinates of magnitude up to R: long and short segments,
    points, near-zero pieces; the picture's pixels lie in 0..R too."""
    rng = np.random.default_rng([seed, int(R)])
    for c in range(cases):
        s = int(rng.integers(1, 7))
        a = rng.uniform(-R, R, (s, 2))
        kind = rng.integers(0, 4, s)
        length = np.where(kind == 0, rng.uniform(0, 2 * R, s), np.where(kind == 1, rng.uniform(0, 8, s),
                          np.where(kind == 2, 0.0, 10.0 ** rng.uniform(-12, -3, s) * R)))
        ang = rng.uniform(0, 2 * np.pi, s)
        b = a + length[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
        rec = np.concatenate([a, b, np.ones((s, 1))], 1).astype(F)
        rec[kind == 2, 2:4] = rec[kind == 2, 0:2]
        H, W = (9, 13) if c % 2 else (int(min(R, 8192)), 3)      # small, and a tall strip out to y = R
        yield rec, H, W


@pytest.mark.parametrize("R", [200, 2048, 8192])
def test_restatement_against_float64(R):
    """|sqrt(d2) - d64| <= 4 * R * 2^-23 px.  Measured worst over these seeded cases (50 per
    R, printed below): 0.75, 1.14 and 0.74 times R * 2^-23 at R = 200, 2048, 8192.  The factor
    4 is the margin for degenerate pieces the sample does not reach."""
    worst = 0.0
    for rec, H, W in _seeded_planes(R, 5):
        got = np.sqrt(ref.d2_plane(rec, H, W).astype(np.float64))
        want = ref.dist64(rec, H, W)
        worst = max(worst, float(np.abs(got - want).max()))
    print("R = %d: worst |sqrt(d2) - d64| = %.3g px = %.2f * R * 2^-23" % (R, worst, worst / (R * 2.0 ** -23)))
    assert worst <= 4 * R * 2.0 ** -23


def test_zero_length_segments_have_the_bits_of_the_point_formula():
    rng = np.random.default_rng(3)
    H, W = 17, 23
    for u, v in [(0.0, 0.0), (22.0, 16.0), (-3.25, 40.5)] + [tuple(rng.uniform(-30, 60, 2)) for _ in range(20)]:
        u, v = F(u), F(v)
        got = ref.d2_plane(ref.fill([ref.seg(u, v, u, v)], 3, junk=(np.nan,) * 5), H, W)
        assert np.array_equal(got.view(np.uint32), ref.point_d2(u, v, H, W).view(np.uint32))


def test_restatement_empty_slots_and_order():
    H, W = 6, 7
    nan = float("nan")
    a = ref.seg(1, 1, 5, 4)
    for flag in (0.0, -1.0, nan):
        rec = ref.fill([[nan, nan, nan, nan, flag], a, [1e30, nan, 0, 0, flag]], 4)
        assert np.array_equal(ref.d2_plane(rec, H, W), ref.d2_plane(ref.fill([a], 1), H, W))
    assert np.isposinf(ref.d2_plane(ref.fill([], 2), H, W)).all()
    assert (ref.target64(ref.d2_plane(ref.fill([], 2), H, W), 8.0) == 0).all()
    # a horizontal segment: distance 0 on it, |y - y0| beside it, Euclidean past its ends
    d2 = ref.d2_plane(ref.fill([ref.seg(2, 3, 4, 3)], 1), H, W)
    assert (d2[3, 2:5] == 0).all() and d2[0, 3] == 9 and d2[3, 6] == 4 and d2[0, 0] == 13


# ---- hkp.lines

def test_from_points_from_polylines_concat():
    from hkp import lines as L
    from hkp._lib import HKP_LINE_MAX_S, HkpError
    assert HKP_LINE_MAX_S == 128
    pts = torch.tensor([[[[1.5, 2.0, 1.0], [0.0, 0.0, 0.0], [7.0, 8.0, -1.0]]]])
    got = L.from_points(pts)
    assert got.shape == (1, 1, 3, 5) and got.dtype == torch.float32 and got.is_contiguous()
    assert got.tolist() == [[[[1.5, 2.0, 1.5, 2.0, 1.0], [0, 0, 0, 0, 0], [7.0, 8.0, 7.0, 8.0, -1.0]]]]
    for bad in (torch.zeros(1, 1, 3), torch.zeros(1, 1, 3, 2), None):
        with pytest.raises(HkpError, match="from_points"):
            L.from_points(bad)

    poly = np.array([[0, 0], [2, 0], [2, 3]], dtype=np.float64)
    out = L.from_polylines([[poly, [[9.0, 9.0]]], [], [poly[::-1]]], 4)
    assert out.shape == (3, 4, 5) and out.dtype == np.float32
    assert out[0].tolist() == [[0, 0, 2, 0, 1], [2, 0, 2, 3, 1], [9, 9, 9, 9, 1], [0, 0, 0, 0, 0]]
    assert (out[1] == 0).all()
    assert out[2, :2].tolist() == [[2, 3, 2, 0, 1], [2, 0, 0, 0, 1]]
    with pytest.raises(HkpError, match="more than S"):
        L.from_polylines([[poly, poly]], 3)
    with pytest.raises(HkpError, match="outside 1.."):
        L.from_polylines([[poly]], 129)
    with pytest.raises(HkpError, match="outside 1.."):
        L.from_polylines([[poly]], 0)
    with pytest.raises(HkpError, match=r"\[n,2\]"):
        L.from_polylines([[np.zeros((2, 3))]], 4)

    a, b = torch.zeros(2, 3, 4, 5), torch.ones(2, 3, 6, 5)
    c = L.concat(a, b)
    assert c.shape == (2, 3, 10, 5) and c.is_contiguous()
    assert torch.equal(c[:, :, :4], a) and torch.equal(c[:, :, 4:], b)
    for x, y in ((a, torch.ones(2, 2, 6, 5)), (a, torch.ones(2, 3, 6, 4)), (a, b.double()), (a, None),
                 (torch.zeros(1, 1, 100, 5), torch.zeros(1, 1, 29, 5))):
        with pytest.raises(HkpError, match="concat"):
            L.concat(x, y)
    assert L.concat(torch.zeros(1, 1, 100, 5), torch.zeros(1, 1, 28, 5)).shape[2] == 128


# ---- apply_lines

def _lines_batch():
    nan = float("nan")
    lines = np.zeros((2, 3, 3, 5), dtype=np.float32)
    rng = np.random.default_rng(11)
    lines[..., :4] = rng.uniform(5, 40, (2, 3, 3, 4))
    lines[..., 4] = 1.0
    lines[:, 0, 0] = (10.0, 12.0, 200.0, -80.0, 1.0)           # leaves the picture by far
    lines[:, 1, 2] = (nan, nan, nan, nan, 0.0)                 # empty slots, NaN inside
    lines[:, 2, 1] = (nan, 3.0, nan, 4.0, -1.0)
    lines[0, 2, 2] = (1.0, 2.0, 3.0, 4.0, nan)
    return lines


def _as_points(lines, e):
    """End e (0 or 2) of every slot as instance labels [n,K,S,3]."""
    return np.concatenate([lines[..., e:e + 2], lines[..., 4:5]], -1)


def test_warp_plan_apply_lines():
    from hkp.geometry import WarpPlan, affine_matrix
    hw = (48, 64)
    mats = [affine_matrix(48, 64, rotate_deg=20, scale=1.1, translate_xy_px=(3, -2), hflip=True),
            affine_matrix(48, 64, rotate_deg=-10, scale=0.9)]
    lines = _lines_batch()
    for pairs, flipped in (((), [True, False]), (((0, 2),), [True, False]), (((0, 2),), [False, False])):
        plan = WarpPlan(np.stack(mats), hw, flipped=flipped, flip_pairs=pairs)
        got = plan.apply_lines(lines)
        assert got.dtype == np.float32 and got.shape == lines.shape
        # the same points through apply_points, in a picture so large that none leaves it
        big = WarpPlan(np.stack(mats), (1 << 20, 1 << 20), flipped=flipped, flip_pairs=pairs)
        for b in range(2):
            swap = flipped[b] and pairs
            src = lines[b][[2, 1, 0]] if swap else lines[b]         # row k of the result came from here
            on = src[..., 4] > 0
            for e in (0, 2):
                want = plan.matrices[b] @ np.concatenate([src[..., e:e + 2].astype(np.float64),
                                                          np.ones(src.shape[:2] + (1,))], -1)[..., None]
                assert np.array_equal(got[b][on][:, e:e + 2], want[..., 0].astype(np.float32)[on])
            # empty slots: bit for bit what they held, NaN included
            assert np.array_equal(got[b][~on].view(np.uint32), src[~on].view(np.uint32))
            assert np.array_equal(got[b][..., 4].view(np.uint32), src[..., 4].view(np.uint32))
        # ... and apply_points gives the same coordinates for the same points (where it keeps them)
        for e in (0, 2):
            p = np.nan_to_num(_as_points(lines, e), nan=0.0)
            p[..., 2] = np.where(lines[..., 4] > 0, 1.0, 0.0)
            q = big.apply_points(p)
            keep = q[..., 2] > 0
            assert np.array_equal(got[..., e:e + 2][keep], q[..., :2][keep])
        # the segment that leaves the picture keeps its flag and is not clipped
        k = 2 if (flipped[0] and pairs) else 0
        assert got[0, k, 0, 4] == 1.0
        assert not (0 <= got[0, k, 0, 2] <= 63 and 0 <= got[0, k, 0, 3] <= 47)
    # tensors come back as tensors; shapes are checked
    t = plan.apply_lines(torch.from_numpy(lines))
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy().view(np.uint32), plan.apply_lines(lines).view(np.uint32))
    from hkp._lib import HkpError
    with pytest.raises(HkpError, match="apply_lines"):
        plan.apply_lines(lines[:1])
    with pytest.raises(HkpError, match="apply_lines"):
        plan.apply_lines(lines[..., :4])


def test_resample_plan_apply_lines():
    from hkp.resample import ResamplePlan
    lines = _lines_batch()
    for mode in ("stretch", "fit"):
        plan = ResamplePlan([(96, 100), (40, 200)], (48, 64), mode=mode)
        got = plan.apply_lines(lines)
        on = lines[..., 4] > 0
        assert np.array_equal(got[~on].view(np.uint32), lines[~on].view(np.uint32))
        assert np.array_equal(got[..., 4].view(np.uint32), lines[..., 4].view(np.uint32))
        for e in (0, 2):
            p = np.nan_to_num(_as_points(lines, e), nan=0.0)
            p[..., 2] = np.where(on, 1.0, 0.0)
            q = plan.apply_points(p)
            keep = q[..., 2] > 0
            assert keep.any()
            assert np.array_equal(got[..., e:e + 2][keep], q[..., :2][keep])
        assert got[0, 0, 0, 4] == 1.0 and got[0, 0, 0, 3] < 0          # outside, kept, not clipped


# ---- the scenes

def test_cable_scenes_line_class():
    from hkp import synth
    assert synth.CLASSES == ("cap", "tail", "crossing", "blob") and synth.LINE_CLASSES == ("cable",)
    assert inspect.signature(synth.CableScenes.__init__).parameters["classes"].default == synth.CLASSES
    hw = (96, 128)
    a = synth.CableScenes(seed=4, classes=("cap", "tail"))
    b = synth.CableScenes(seed=4, classes=("cap", "tail", "cable"))
    assert a.line_slots == 0 and b.line_slots == 96
    pa, pb = a.plan([0, 1, 5], 2, hw), b.plan([0, 1, 5], 2, hw)
    assert pa.lines is None and a.line_labels(pa.descs[0]) is None
    assert np.array_equal(pa.seg_bytes(), pb.seg_bytes()) and np.array_equal(pa.scene_bytes(), pb.scene_bytes())
    assert np.array_equal(pa.pts, pb.pts[:, :2])
    assert (pb.pts[:, 2] == 0).all()                                   # the line class's point row is empty
    assert pb.lines.shape == (3, 3, 96, 5) and pb.lines.dtype == np.float32
    assert (pb.lines[:, :2] == 0).all()
    for i, d in enumerate(pb.descs):
        want = np.concatenate([np.concatenate([c["poly"][:-1], c["poly"][1:]], 1) for c in d["cables"]], 0)
        n = len(want)
        assert n in (48, 96)
        assert np.array_equal(pb.lines[i, 2, :n, :4], want.astype(np.float32))
        assert (pb.lines[i, 2, :n, 4] == 1).all() and (pb.lines[i, 2, n:] == 0).all()
        assert np.array_equal(b.line_labels(d), pb.lines[i])
    # the same through hkp.lines.from_polylines
    from hkp import lines as L
    d = pb.descs[0]
    assert np.array_equal(L.from_polylines([[], [], [c["poly"] for c in d["cables"]]], 96), pb.lines[0])
    with pytest.raises(ValueError, match="segment slots"):
        synth.CableScenes(classes=("cap", "cable"), cables=(1, 3))      # 3 * 48 = 144 > 128
    synth.CableScenes(classes=("cap",), cables=(1, 3))                  # no line class: as before
    synth.CableScenes(classes=("cable",), cables=(1, 4), segments=32)   # 128 fits
    with pytest.raises(ValueError, match="distinct names"):
        synth.CableScenes(classes=("cap", "rope"))
    with pytest.raises(ValueError, match="distinct names"):
        synth.CableScenes(classes=("cable", "cable"))


# ---- rejections

def test_c_entry_rejects_without_a_gpu_and_leaves_outputs_alone():
    from hkp import _lib
    L = _lib.lib()
    n, k, s, H, W = 2, 2, 3, 5, 6
    lines = np.zeros((n, k, s, 5), np.float32)
    target = np.full((n, k, H, W), 7.0)
    d2 = np.full((n, k, H, W), 7.0, np.float32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    good = dict(n=n, k=k, s=s, H=H, W=W, sigma=8.0, lines=P(lines), target=P(target), d2=P(d2))
    bad = [dict(n=0), dict(n=-1), dict(k=0), dict(H=0), dict(W=0), dict(W=-3), dict(s=0), dict(s=129), dict(s=-1),
           dict(H=1 << 15, W=(1 << 15) + 1), dict(H=1 << 30, W=2), dict(sigma=0.0), dict(sigma=-1.0),
           dict(sigma=float("nan")), dict(sigma=float("inf")), dict(sigma=1e39), dict(target=None, d2=None),
           dict(target=None, d2=None, sigma=-1.0), dict(lines=None),
           dict(target=None, sigma=float("nan")), dict(target=None, sigma=0.0)]   # sigma is checked though not read
    for b in bad:
        a = dict(good, **b)
        rc = L.hkp_line_target(a["n"], a["k"], a["s"], a["H"], a["W"], a["sigma"], a["lines"], a["target"], a["d2"], None)
        assert rc == -1, b
        assert L.hkp_last_error().decode().startswith("hkp_line_target"), b
    assert (target == 7).all() and (d2 == 7).all()


def test_ops_line_target_rejects_before_a_tensor_is_touched():
    """Argument errors are raised on shapes and numbers alone; tensors that pass them (here
    on the CPU) are then refused for their device: nothing is launched."""
    from hkp import ops
    from hkp._lib import HkpError
    good = torch.zeros(2, 3, 4, 5)
    lt = lambda **kw: ops.line_target(kw.pop("lines", good), kw.pop("H", 9), kw.pop("W", 11), **kw)  # noqa: E731
    for kw, msg in ((dict(lines=None), "expected a tensor"), (dict(lines=torch.zeros(2, 3, 4)), r"\[N,K,S,5\]"),
                    (dict(lines=torch.zeros(2, 3, 4, 3)), r"\[N,K,S,5\]"), (dict(lines=torch.zeros(2, 3, 0, 5)), "1 <= S"),
                    (dict(lines=torch.zeros(2, 3, 129, 5)), "1 <= S"), (dict(lines=torch.zeros(0, 3, 4, 5)), r"\[N,K,S,5\]"),
                    (dict(H=0), "bad size"), (dict(W=-1), "bad size"), (dict(H=1 << 16, W=1 << 15), "bad size"),
                    (dict(sigma=0.0), "sigma"), (dict(sigma=-2.0), "sigma"), (dict(sigma=float("nan")), "sigma"),
                    (dict(sigma=float("inf")), "sigma"), (dict(want_target=False), "neither"),
                    (dict(lines=good.double()), "on the GPU"), (dict(), "on the GPU"),
                    (dict(want_d2=True), "on the GPU")):
        with pytest.raises(HkpError, match=msg):
            lt(**kw)


def test_trainer_and_heatmap_loss_reject_lines_before_the_forward():
    from hkp import ops, train
    from hkp.autograd import heatmap_loss
    from src.model import KeypointsGauss
    model = KeypointsGauss(3, backbone="resnet18", pretrained=False)
    x = torch.zeros(1, 3, 32, 32)
    lines = torch.zeros(1, 3, 4, 5)
    pts = torch.zeros(1, 3, 2, 3)
    E = ops.HkpError
    with pytest.raises(E, match="'bce' or 'mse'"):
        train.Trainer(model, loss="qfl").step(x, lines=lines)
    with pytest.raises(E, match="norm"):
        train.Trainer(model, loss_params={"norm": "instances"}).step(x, lines=lines)
    with pytest.raises(E, match="absent='zero'"):
        train.Trainer(model, absent="ignore").step(x, pts=pts, lines=lines)
    with pytest.raises(E, match="not supported with lines"):
        train.Trainer(model, loss_params={"class_weights": [1.0, 1.0, 1.0]}).step(x, pts=pts, lines=lines)
    with pytest.raises(E, match="not supported with lines"):
        train.Trainer(model, loss_params={"topk": 2}).step(x, pts=pts, lines=lines)
    tr = train.Trainer(model)
    with pytest.raises(E, match="not supported with lines"):
        tr.step(x, pts=pts, lines=lines, weights=torch.ones(1, 3))
    with pytest.raises(E, match="not supported with lines"):
        tr.step(x, pts=pts, lines=lines, mask=torch.zeros(1, 32, 32, dtype=torch.uint8))
    with pytest.raises(E):                                             # weights or a mask without pts: refused earlier still
        tr.step(x, lines=lines, weights=torch.ones(1, 3))
    with pytest.raises(E, match="not with uv or target"):
        tr.step(x, uv=torch.zeros(1, 3, 2), lines=lines)
    with pytest.raises(E, match="not with uv or target"):
        tr.forward_backward(x, target=torch.zeros(1, 3, 32, 32, dtype=torch.float64), lines=lines)
    with pytest.raises(E, match=r"\[N,K,S,5\]"):
        tr.step(x, lines=torch.zeros(1, 3, 4, 4))
    with pytest.raises(E, match="do not go with"):
        tr.step(x, lines=torch.zeros(1, 2, 4, 5))
    with pytest.raises(E, match="do not go with"):
        tr.step(x, lines=torch.zeros(2, 3, 4, 5))
    with pytest.raises(E, match="on the GPU"):                         # all of it passed: the device is next
        tr.step(x, lines=lines)
    with pytest.raises(E, match="tags need pts"):
        train.Trainer(model, tags={"classes": (0, 1)}).step(x, lines=lines)

    heat = torch.zeros(1, 3, 8, 8)
    hl = lambda **kw: heatmap_loss(heat, lines=kw.pop("lines", lines), **kw)  # noqa: E731
    for kw, msg in ((dict(kind="qfl"), "'bce' or 'mse'"), (dict(norm="instances"), "'bce' or 'mse'"),
                    (dict(absent="ignore", pts=pts), "'bce' or 'mse'"), (dict(weights=torch.ones(1, 3)), "not supported"),
                    (dict(topk=1), "not supported"), (dict(return_planes=True), "not supported"),
                    (dict(mask=torch.zeros(1, 8, 8, dtype=torch.uint8)), "not supported"),
                    (dict(uv=torch.zeros(1, 3, 2)), "not with uv or target"),
                    (dict(target=torch.zeros(1, 3, 8, 8, dtype=torch.float64)), "not with uv or target"),
                    (dict(lines=torch.zeros(1, 3, 4, 6)), r"\[N,K,S,5\]"), (dict(lines=torch.zeros(1, 2, 4, 5)), "do not go with"),
                    (dict(), "on the GPU")):
        with pytest.raises(E, match=msg):
            hl(**kw)


def test_line_metrics_arguments_and_empty_compute():
    from hkp import lines as L
    from hkp._lib import HkpError
    for kw in (dict(num_keypoints=0), dict(num_keypoints=2, radius=-1.0), dict(num_keypoints=2, threshold=0.0)):
        with pytest.raises(HkpError, match="LineMetrics"):
            L.LineMetrics(**kw)
    m = L.LineMetrics(2)
    assert m.radius == 4.0 and m.threshold == 0.5
    out = m.compute()
    assert len(out) == 2 and all(np.isnan(o["completeness"]) and np.isnan(o["correctness"]) and np.isnan(o["iou"])
                                 and o["hit"] == o["pred"] == o["line"] == 0 for o in out)
    with pytest.raises(HkpError, match="heat"):
        m.update(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 2, 5))


def test_new_keywords_default_to_none():
    from hkp import ops
    from hkp.autograd import heatmap_loss
    from hkp.train import Trainer
    for f in (Trainer.step, Trainer.forward_backward, heatmap_loss):
        params = inspect.signature(f).parameters
        assert list(params)[-1] == "lines" and params["lines"].default is None
    sig = inspect.signature(ops.line_target).parameters
    assert [(n, p.default) for n, p in sig.items()][3:] == [("sigma", 8.0), ("want_target", True), ("want_d2", False),
                                                           ("out", None), ("out_d2", None)]
