"""hkp_heat_peaks on the GPU: the kernel against its numpy restatement
(tests/_peaks_ref.py, pinned in tests/test_peaks_cpu.py), against the existing
argmax decode, through the model / Prediction / the DP wrapper, and through
analysis.main with config.PEAKS set."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _peaks_ref as ref
from oracle import recipe

pytestmark = pytest.mark.gpu

UNUSED = np.float32([-1, -1, 0])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _inputs(shape, variant, seed):
    """Logits round(N(0,3)*8)/8 clipped to +-10 (quantised: ties) with planted bumps;
    plane p is of kind (p + variant) % 4: 0 as is, 1 with NaN / +inf / -inf nodes,
    2 all -inf, 3 a constant."""
    n, k, h, w = shape
    rng = np.random.default_rng(seed)
    low = np.clip(np.round(rng.normal(0, 3, shape) * 8) / 8, -10, 10).astype(np.float32)
    for p in range(n * k):
        z = low[p // k, p % k]
        for _ in range(1 + h * w // 40):                   # bumps: a node and, half as high, its neighbours
            i, j, a = rng.integers(h), rng.integers(w), np.float32(rng.integers(8, 40)) / 4
            z[max(i - 1, 0):i + 2, max(j - 1, 0):j + 2] += a / 2
            z[i, j] += a / 2
        kind = (p + variant) % 4
        if kind == 1:
            for v in (np.nan, np.inf, -np.inf, -0.0):
                for _ in range(1 + h * w // 60):
                    z[rng.integers(h), rng.integers(w)] = v
        elif kind == 2:
            z[:] = -np.inf
        elif kind == 3:
            z[:] = np.float32(rng.integers(-16, 16)) / 4
    return low


def _node_scores(low_t):
    """sigmoid_f(z) of every node from the shipped heatmap kernel: the upsample at
    identity size (lerp_index returns the node itself when in == out).  Its
    interpolation forms z + z*0, which is NaN at an infinite node, so those take
    the IEEE values of 1 / (1 + expf(-z)): 1 at +inf, 0 at -inf."""
    from hkp import ops
    n, k, h, w = low_t.shape
    s = ops.upsample_sigmoid(low_t, h, w, heat=True, argmax=False)[0].cpu().numpy()
    z = low_t.cpu().numpy()
    s[np.isposinf(z)] = 1.0
    s[np.isneginf(z)] = 0.0
    return s


SHAPES = [((1, 1, 1, 1), (8, 8)), ((1, 2, 1, 13), (1, 104)), ((1, 2, 11, 1), (88, 1)), ((2, 3, 7, 9), (50, 75)),
          ((2, 4, 60, 80), (480, 640)), ((1, 1, 120, 160), (960, 1280))]
COMBOS = [(r, p, t) for r in (1, 2, 8) for p in (1, 4, 16) for t in (0.0, 0.5)]


@pytest.mark.parametrize("shape,HW", SHAPES, ids=["x".join(map(str, s)) for s, _ in SHAPES])
def test_kernel_equals_restatement(shape, HW, cuda_device):
    from hkp import ops
    H, W = HW
    ulp = np.spacing(np.float32(max(H, W)))
    variants = range(4) if shape[2] * shape[3] <= 4800 else range(1)   # the largest plane: one input
    lows = [_inputs(shape, v, 100 * v + shape[3]) for v in variants]
    # on the CPU, before the GPU is touched: no den near the guard (two libms could disagree there)
    dens = []
    for low in lows:
        ref.heat_peaks(low, H, W, max_peaks=16, radius=1, dens=dens)
        ref.heat_peaks(low, H, W, max_peaks=16, radius=8, dens=dens)
    assert not [d for d in dens if 0.5e-6 <= d <= 2e-6]
    if dens:
        print("smallest den %.3g of %d" % (min(dens), len(dens)))
    used_counts = set()
    for low in lows:
        low_t = torch.from_numpy(low).to(cuda_device)
        scores = _node_scores(low_t)
        assert not np.isnan(scores[~np.isnan(low)]).any()
        for r, P, t in COMBOS:
            want, want_c = ref.heat_peaks(low, H, W, max_peaks=P, radius=r, threshold=t, scores=scores)
            peaks_t, counts_t = ops.heat_peaks(low_t, H, W, max_peaks=P, radius=r, threshold=t)
            again_p, again_c = ops.heat_peaks(low_t, H, W, max_peaks=P, radius=r, threshold=t)
            assert peaks_t.dtype == torch.float32 and tuple(peaks_t.shape) == shape[:2] + (P, 3)
            assert counts_t.dtype == torch.int32 and tuple(counts_t.shape) == shape[:2]
            assert torch.equal(_bits(peaks_t), _bits(again_p)) and torch.equal(counts_t, again_c)
            got, got_c = peaks_t.cpu().numpy(), counts_t.cpu().numpy()
            assert np.array_equal(got_c, want_c), (r, P, t)
            assert np.array_equal(got[..., 2].view(np.int32), want[..., 2].view(np.int32)), (r, P, t)
            assert (np.abs(got[..., :2].astype(np.float64) - want[..., :2].astype(np.float64)) <= ulp).all(), (r, P, t)
            unused = np.arange(P)[None, None, :] >= want_c[:, :, None]
            assert np.array_equal(got[unused], np.tile(UNUSED, (int(unused.sum()), 1)))
            used_counts.update(int(c) for c in want_c.ravel())
    if len(lows) == 4 and shape[2] * shape[3] > 16:
        assert 0 in used_counts and max(used_counts) > 1     # the inputs reach empty and multi-peak planes


def test_bad_arguments_raise(cuda_device):
    from hkp import _lib, ops
    low = torch.zeros((1, 1, 8, 8), device=cuda_device)
    big = torch.zeros((1, 1, 129, 256), device=cuda_device)          # 33024 nodes > the cap of 32768
    assert big.shape[2] * big.shape[3] > ops.HEAT_PEAKS_MAX_NODES
    ok = torch.zeros((1, 1, 128, 256), device=cuda_device)           # exactly the cap
    peaks, counts = ops.heat_peaks(ok, 1024, 2048, max_peaks=2)
    assert counts.item() == 1 and tuple(peaks[0, 0, 0].tolist()) == (0.0, 0.0, 0.5)
    for kw in (dict(radius=0), dict(radius=9), dict(max_peaks=0), dict(max_peaks=17), dict(threshold=-0.1),
               dict(threshold=1.5), dict(threshold=float("nan"))):
        with pytest.raises(ops.HkpError):
            ops.heat_peaks(low, 64, 64, **kw)
    with pytest.raises(ops.HkpError):
        ops.heat_peaks(big, 64, 64)
    with pytest.raises(ops.HkpError):
        ops.heat_peaks(low, 0, 64)

    # the library's own checks, behind the wrapper's
    def raw(t, H=64, W=64, radius=1, max_peaks=4, threshold=0.0, null=False):
        n, k, h, w = t.shape
        pk = torch.empty((n, k, max(max_peaks, 1), 3), device=cuda_device)
        ct = torch.empty((n, k), device=cuda_device, dtype=torch.int32)
        _lib.call("hkp_heat_peaks", n, k, h, w, H, W, radius, max_peaks, threshold, ctypes.c_void_p(t.data_ptr()),
                  ctypes.c_void_p(0 if null else pk.data_ptr()), ctypes.c_void_p(ct.data_ptr()),
                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    raw(low)
    for kw, what in ((dict(radius=0), "radius"), (dict(radius=9), "radius"), (dict(max_peaks=0), "max_peaks"),
                     (dict(max_peaks=17), "max_peaks"), (dict(threshold=1.5), "threshold"), (dict(H=0), "bad sizes"),
                     (dict(null=True), "null")):
        with pytest.raises(_lib.HkpError, match=what):
            raw(low, **kw)
    with pytest.raises(_lib.HkpError, match="cap"):
        raw(big)
    torch.cuda.synchronize()


def _planted(seed):
    """K = 4 planes 8 x 12 of N(0,1) logits, each with one node (a corner, two border
    nodes, an interior one) exceeding every other node by 0.5 .. 4."""
    rng = np.random.default_rng(seed)
    low = rng.normal(0, 1, (1, 4, 8, 12)).astype(np.float32)
    nodes = [(0, 0), (7, 5), (3, 11), (int(rng.integers(1, 7)), int(rng.integers(1, 11)))]
    for k, (i, j) in enumerate(nodes):
        low[0, k, i, j] = -np.inf
        low[0, k, i, j] = low[0, k].max() + np.float32(rng.uniform(0.5, 4))
    return low, nodes


def test_first_peak_agrees_with_the_argmax_decode(cuda_device):
    from hkp import ops
    h, w, H, W = 8, 12, 64, 96
    for seed in range(3):
        low, nodes = _planted(seed)
        pos = [(i * (H - 1) / (h - 1), j * (W - 1) / (w - 1)) for i, j in nodes]          # (y, x) of the nodes
        # the condition, with the reference interpolation on the CPU
        heat = torch.sigmoid(F.interpolate(torch.from_numpy(low), size=(H, W), mode="bilinear", align_corners=True))
        for k in range(4):
            y, x = np.unravel_index(int(heat[0, k].argmax()), (H, W))
            assert max(abs(y - pos[k][0]), abs(x - pos[k][1])) <= 1.0
        low_t = torch.from_numpy(low).to(cuda_device)
        _, yx = ops.upsample_sigmoid(low_t, H, W, heat=False, argmax=True)
        peaks, counts = ops.heat_peaks(low_t, H, W, max_peaks=4, radius=1)
        picked = {}
        want, want_c = ref.heat_peaks(low, H, W, max_peaks=4, radius=1, scores=_node_scores(low_t), picked=picked)
        peaks, counts, yx = peaks.cpu().numpy(), counts.cpu().numpy(), yx.cpu().numpy()
        assert np.array_equal(counts, want_c) and np.abs(peaks - want).max() <= np.spacing(np.float32(W))
        for k in range(4):
            assert picked[(0, k)][0] == nodes[k]                     # peak 0 sits on the planted node
            assert abs(peaks[0, k, 0, 0] - pos[k][1]) <= 0.5 * (W - 1) / (w - 1)
            assert abs(peaks[0, k, 0, 1] - pos[k][0]) <= 0.5 * (H - 1) / (h - 1)
            assert max(abs(yx[0, k, 0] - pos[k][0]), abs(yx[0, k, 1] - pos[k][1])) <= 1.0, (seed, k)


def test_through_the_model(cuda_device):
    from hkp import net, ops, parallel
    from src.model import KeypointsGauss
    from src.prediction import Prediction
    K, H, W = 4, 64, 96
    m = KeypointsGauss(K, H, W, backbone="resnet18", pretrained=False)
    m.load_state_dict(recipe.seeded_state_dict("resnet18", 21))
    m = m.to(cuda_device)
    u8 = torch.from_numpy(recipe.seeded_images_u8(2, H, W, 22)).to(cuda_device)
    kw = dict(max_peaks=5, radius=2, threshold=0.05)
    for x in (recipe.to_tensor_nchw(recipe.seeded_images_u8(2, H, W, 22)).to(cuda_device), u8):
        with torch.no_grad():
            _, yx, low = net.keypoints_forward(m.resnet.net, x, K, heat=False, argmax=True, pol=m.policy)
        assert tuple(low.shape) == (2, K, H // 8, W // 8)
        want_p, want_c = ops.heat_peaks(low, H, W, **kw)
        assert int(want_c.sum()) > 0
        for got_p, got_c in (m.predict_peaks(x, **kw), Prediction(m, K, H, W, True).peaks(x, **kw),
                             parallel.predict_peaks_dp(m, x, **kw)):
            assert torch.equal(_bits(got_p), _bits(want_p)) and torch.equal(got_c, want_c)
        assert torch.equal(m.predict_keypoints(x), yx)               # the existing decode is what it was
        dflt_p, dflt_c = m.predict_peaks(x)
        assert tuple(dflt_p.shape) == (2, K, 4, 3) and tuple(dflt_c.shape) == (2, K)


def test_analysis_writes_peaks(tmp_path, monkeypatch, cuda_device):
    """analysis.main with config.PEAKS set: peaks.npy / peak_counts.npy beside an
    unchanged keypoints.npy; with RESIZE, an image of another size has its peaks
    mapped back into its own pixels (invert_uv of the used slots)."""
    import analysis as analysis_mod
    from PIL import Image
    from hkp import ops, resample
    from src.dataset import transform
    from src.model import KeypointsGauss
    BB, K, H, W = "resnet34", 4, 64, 96
    cfg = {"max_peaks": 3, "radius": 1, "threshold": 0.1}
    for name, v in (("IMG_HEIGHT", H), ("IMG_WIDTH", W), ("RESIZE", "hamming"), ("RESIZE_PARAMS", {"mode": "fit"})):
        monkeypatch.setattr(analysis_mod, name, v)
    assert (analysis_mod.BACKBONE, analysis_mod.NUM_KEYPOINTS, analysis_mod.PEAKS) == (BB, K, None)
    sd = recipe.seeded_state_dict(BB, 91)
    (tmp_path / "ck").mkdir()
    torch.save(sd, tmp_path / "ck" / "m.pth")
    (tmp_path / "imgs").mkdir()
    srcs = [recipe.seeded_images_u8(1, H, W, 92)[0], recipe.seeded_images_u8(1, 150, 330, 93)[0]]
    for i, bgr in enumerate(srcs):
        Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(tmp_path / "imgs" / ("f%d.png" % i))
    run = lambda out: analysis_mod.main("m.pth", str(tmp_path / "imgs"), out_dir=str(tmp_path / out),    # noqa: E731
                                        checkpoint_dir=str(tmp_path / "ck"))
    kp_plain = run("plain")
    assert not (tmp_path / "plain" / "peaks.npy").exists() and not (tmp_path / "plain" / "peak_counts.npy").exists()
    monkeypatch.setattr(analysis_mod, "PEAKS", cfg)
    kp = run("preds")
    assert np.array_equal(kp, kp_plain)
    assert np.array_equal(np.load(tmp_path / "preds" / "keypoints.npy"), np.load(tmp_path / "plain" / "keypoints.npy"))
    peaks, counts = np.load(tmp_path / "preds" / "peaks.npy"), np.load(tmp_path / "preds" / "peak_counts.npy")
    assert peaks.shape == (2, K, 3, 3) and peaks.dtype == np.float32
    assert counts.shape == (2, K) and counts.dtype == np.int32
    m = KeypointsGauss(K, H, W, backbone=BB, pretrained=False)
    m.load_state_dict(sd)
    m = m.to(cuda_device)
    plan = resample.Resize("hamming", mode="fit").plan([(150, 330)], (H, W))
    flat = torch.from_numpy(np.ascontiguousarray(srcs[1]).reshape(-1)).to(cuda_device)
    frames = [srcs[0], ops.resample_ragged_u8(flat, plan)[0].cpu().numpy()]
    for i, frame in enumerate(frames):
        pk, ct = m.predict_peaks(transform(frame).to(cuda_device)[None], **cfg)    # batch 1, train-mode BN
        pk, ct = pk.cpu().numpy(), ct.cpu().numpy()
        assert np.array_equal(counts[i:i + 1], ct)
        if i == 1:
            uv = plan.invert_uv(np.ascontiguousarray(pk[0, :, :, :2]).reshape(1, K * 3, 2)).reshape(K, 3, 2)
            for k in range(K):
                pk[0, k, :ct[0, k], :2] = uv[k, :ct[0, k]]
        assert np.array_equal(peaks[i:i + 1], pk), i
    assert int(counts.sum()) > 0
