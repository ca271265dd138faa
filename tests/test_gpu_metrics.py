"""hkp_peaks_match on the GPU: the kernel against its numpy restatement
(tests/_metrics_ref.py, pinned in tests/test_metrics_cpu.py), its accumulation
properties and limits, end to end with hkp_gauss_target_multi and hkp_heat_peaks,
and through the model / Prediction / the DP wrapper / train.fit / analysis.main."""
import ctypes
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import _instances_ref as iref
import _metrics_ref as ref
from conftest import PKG, REPO
from oracle import recipe

pytestmark = pytest.mark.gpu

SENTINEL = -(7 << 40) - 12345
THRESHOLDS = {1: (4.0,), 2: (2.0, 8.0), 4: (2.0, 4.0, 8.0, 16.0), 8: (1.0, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0)}
# (B, K, P, M, T), bins, seed
CASES = [((1, 1, 1, 1, 1), 1024, 101), ((2, 3, 4, 1, 2), 1024, 102), ((2, 4, 4, 3, 4), 1024, 103),
         ((5, 1, 16, 2, 1), 1024, 104), ((3, 2, 16, 16, 8), 1024, 105), ((2, 4, 4, 3, 4), 7, 106)]
CONDITION = {(2, 4, 4, 3, 4), (3, 2, 16, 16, 8)}
_cache = {}


def _case(shape, bins, seed):
    """(peaks, counts, pts, thresholds, the restatement's five results), computed once."""
    key = (shape, bins, seed)
    if key not in _cache:
        B, K, P, M, T = shape
        pk, ct, lab = ref.random_batch(seed, B, K, P, M)
        hp, hc, hl = ref.hand_batch(K, P, M)
        pk, ct, lab = np.concatenate([pk, hp]), np.concatenate([ct, hc]), np.concatenate([lab, hl])
        th = THRESHOLDS[T]
        want = ref.peaks_match(pk, ct, lab, th, bins=bins)
        for a in (pk, ct, lab) + tuple(want):
            a.setflags(write=False)
        _cache[key] = (pk, ct, lab, th, want)
    return _cache[key]


def _fresh(K, T, bins, dev):
    hist = torch.zeros((K, T, 2, bins), dtype=torch.int64, device=dev)
    totals = torch.zeros((K, 8), dtype=torch.int64, device=dev)
    totals[:, 7] = SENTINEL
    return hist, totals


def _run(pk, ct, lab, th, bins, dev, outputs=True, hist=None, totals=None):
    from hkp import ops
    K = pk.shape[1]
    if hist is None:
        hist, totals = _fresh(K, len(th), bins, dev)
    out = ops.peaks_match(torch.from_numpy(np.array(pk)).to(dev), torch.from_numpy(np.array(ct)).to(dev),
                          torch.from_numpy(np.array(lab)).to(dev), th, hist, totals, bins=bins, outputs=outputs)
    return hist, totals, out


@pytest.mark.parametrize("shape,bins,seed", CASES)
def test_kernel_against_restatement(cuda_device, shape, bins, seed):
    pk, ct, lab, th, (w_hist, w_tot, w_pm, w_gm, w_gd) = _case(shape, bins, seed)
    K, T = shape[1], shape[4]
    if shape in CONDITION:                    # the inputs reach what the comparison is about
        tp = w_hist[:, :, 0].sum(axis=2)
        fp = w_hist[:, :, 1].sum(axis=2)
        for c in range(K):
            assert tp[c, 0] >= 1 and fp[c, T - 1] >= 1 and (w_gm[:, c] == -1).any() and tp[c, 0] != tp[c, T - 1], c
    hist, totals, (pm, gm, gd) = _run(pk, ct, lab, th, bins, cuda_device)
    hist, totals, pm, gm, gd = (t.cpu().numpy() for t in (hist, totals, pm, gm, gd))
    assert np.array_equal(hist, w_hist)
    assert np.array_equal(totals[:, 0:5], w_tot[:, 0:5]) and np.array_equal(totals[:, 6], w_tot[:, 6])
    assert np.array_equal(pm, w_pm) and np.array_equal(gm, w_gm)
    on = w_gm >= 0
    assert np.array_equal(gd[~on], w_gd[~on])                          # -1 where nothing matched
    assert (np.abs(gd[on] - w_gd[on]) <= np.spacing(w_gd[on])).all()  # one fp32 ulp (the device's fp64 sqrt)
    for c in range(K):
        assert totals[c, 5] == sum(ref.dist_q16(d) for d in gd[:, c][on[:, c]])
    assert (totals[:, 7] == SENTINEL).all()


def test_accumulation(cuda_device):
    shape, bins, seed = CASES[4]
    pk, ct, lab, th, want = _case(shape, bins, seed)
    K, T = shape[1], shape[4]
    dev = cuda_device
    h1, t1, o1 = _run(pk, ct, lab, th, bins, dev)
    h2, t2, o2 = _run(pk, ct, lab, th, bins, dev)                     # a second run: the same bits everywhere
    assert torch.equal(h1, h2) and torch.equal(t1, t2)
    for a, b in zip(o1, o2):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # two updates into one accumulator = the sum of two fresh ones
    half = pk.shape[0] // 2
    ha, ta, _ = _run(pk[:half], ct[:half], lab[:half], th, bins, dev)
    hb, tb, _ = _run(pk[half:], ct[half:], lab[half:], th, bins, dev)
    hc, tc, _ = _run(pk[:half], ct[:half], lab[:half], th, bins, dev)
    _run(pk[half:], ct[half:], lab[half:], th, bins, dev, hist=hc, totals=tc)
    tsum = ta + tb
    tsum[:, 7] = SENTINEL
    assert torch.equal(hc, ha + hb) and torch.equal(tc, tsum)
    assert torch.equal(hc, h1) and torch.equal(tc, t1)
    # the batch rows permuted
    perm = np.random.default_rng(1).permutation(pk.shape[0])
    hp, tp, _ = _run(pk[perm], ct[perm], lab[perm], th, bins, dev)
    assert torch.equal(hp, h1) and torch.equal(tp, t1)
    # without the per-batch outputs
    hn, tn, none = _run(pk, ct, lab, th, bins, dev, outputs=False)
    assert none is None and torch.equal(hn, h1) and torch.equal(tn, t1)


def test_uv_labels_are_one_present_instance(cuda_device):
    rng = np.random.default_rng(9)
    B, K, P = 3, 2, 4
    pk, ct, _ = ref.random_batch(31, B, K, P, 1)
    uv = (np.round(rng.uniform(20, 180, (B, K, 2)) * 4) / 4).astype(np.float32)
    pk[:, :, 0, :2] = uv + np.float32([1.0, 0.0])
    ct = np.maximum(ct, 1)
    lab = np.concatenate([uv, np.ones((B, K, 1), np.float32)], axis=2)[:, :, None, :]
    th = (2.0, 4.0)
    a = _run(pk, ct, uv, th, 64, cuda_device)
    b = _run(pk, ct, lab, th, 64, cuda_device)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert int(a[1][:, 4].sum()) == B * K
    want = ref.peaks_match(pk, ct, uv, th, bins=64)
    assert np.array_equal(a[0].cpu().numpy(), want[0])


def test_limits_are_bad_arg_and_leave_the_accumulators(cuda_device):
    from hkp import _lib, ops
    dev = cuda_device
    hist, totals = _fresh(2, 8, 4096, dev)
    hist += 3
    totals[:, :7] = 5
    h0, t0 = hist.clone(), totals.clone()
    pk = torch.zeros((1, 2, 16, 3), device=dev)
    ct = torch.ones((1, 2), dtype=torch.int32, device=dev)
    lab = torch.ones((1, 2, 16, 3), device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())         # noqa: E731

    def raw(n=1, k=2, p=4, m=3, t=2, bins=1024, th=(2.0, 4.0), null=False):
        arr = (ctypes.c_float * 8)(*(list(th) + [0.0] * (8 - len(th)))[:8])
        return _lib.lib().hkp_peaks_match(n, k, p, m, t, bins, arr, P(pk), P(ct), ctypes.c_void_p(0) if null else P(lab),
                                          P(hist), P(totals), None, None, None, ops._stream())
    nan = float("nan")
    for kw in (dict(p=17), dict(p=0), dict(m=0), dict(m=17), dict(t=9), dict(t=0), dict(bins=4097), dict(bins=0),
               dict(th=(4.0, 2.0)), dict(th=(2.0, 2.0)), dict(th=(0.0, 2.0)), dict(th=(nan, 2.0)), dict(th=(1.0, nan)),
               dict(th=(1.0, float("inf"))), dict(n=0), dict(k=0), dict(null=True)):
        assert raw(**kw) == -1, kw                          # HKP_ERR_BAD_ARG
        assert _lib.lib().hkp_last_error().decode().startswith("hkp_peaks_match"), kw
    torch.cuda.synchronize()
    assert torch.equal(hist, h0) and torch.equal(totals, t0)
    assert raw() == 0
    torch.cuda.synchronize()
    assert int((hist - h0).sum()) == 2 * 2 and (totals[:, 7] == SENTINEL).all()
    # the wrapper's own checks
    ok = _fresh(2, 2, 8, dev)
    for bad in (lambda: ops.peaks_match(pk.cpu(), ct, lab, (2.0, 4.0), *ok, bins=8),
                lambda: ops.peaks_match(pk, ct.long(), lab, (2.0, 4.0), *ok, bins=8),
                lambda: ops.peaks_match(pk, ct, lab[:, :1], (2.0, 4.0), *ok, bins=8),
                lambda: ops.peaks_match(pk, ct, lab, (2.0, 4.0), ok[0][:, :1], ok[1], bins=8),
                lambda: ops.peaks_match(pk, ct, lab, (2.0, 4.0), ok[0], ok[1][:1], bins=8),
                lambda: ops.peaks_match(pk[..., :2], ct, lab, (2.0, 4.0), *ok, bins=8),
                lambda: ops.peaks_match(pk, ct, lab[..., :2].contiguous(), (2.0, 4.0), *ok, bins=8),
                lambda: ops.peaks_match(pk, ct, lab, (2.0, 4.0), ok[0].int(), ok[1], bins=8)):
        with pytest.raises(ops.HkpError):
            bad()
    with pytest.raises(ValueError):
        ops.peaks_match(pk, ct, lab, (4.0, 2.0), *ok, bins=8)
    assert int(ok[0].sum()) == 0


def test_end_to_end_with_target_and_decode(cuda_device):
    """gauss_target_multi -> its lattice samples as logits -> heat_peaks ->
    KeypointMetrics.update with the same pts (the inputs of test_gpu_instances.py's
    round trip, every instance decoded within 1e-4 px): perfect scores at thresholds
    of 1e-3 and 1 px; then one class's labels shifted by 3 px."""
    from hkp import ops
    from hkp.metrics import KeypointMetrics
    (H, W), pts = iref.RT_IMAGE, torch.from_numpy(iref.roundtrip_pts()).to(cuda_device)
    target = ops.gauss_target_multi(pts, H, W, iref.RT_SIGMA).cpu().numpy()
    low = torch.from_numpy(iref.lowres_logits(target)).to(cuda_device)
    peaks, counts = ops.heat_peaks(low, H, W, max_peaks=4, radius=1, threshold=0.5)
    th = (1e-3, 1.0)
    m = KeypointMetrics(4, th, device=cuda_device)
    assert m.hist.is_cuda and tuple(m.hist.shape) == (4, 2, 2, 1024)
    m.update(peaks, counts, pts)
    res = m.compute()
    ninst = [len(p) for p in iref.RT_POINTS]
    for c, r in enumerate(res["per_class"]):
        assert r["instances"] == ninst[c] and r["absent_false_alarms"] == 0
        assert r["absent_planes"] == (1 if ninst[c] == 0 else 0)
        if ninst[c]:
            assert r["recall"] == [1.0, 1.0] and r["precision"] == [1.0, 1.0] and r["ap"] == [1.0, 1.0], (c, r)
            assert r["mean_error_px"] < 1e-3
        else:
            assert r["peaks"] == 0 and np.isnan(r["ap"][0])
    assert res["overall"]["mAP"] == 1.0 and res["overall"]["recall"] == [1.0, 1.0]
    shifted = pts.clone()
    shifted[:, 2, :, 0] += 3.0
    m2 = KeypointMetrics(4, th, device=cuda_device)
    m2.update(peaks, counts, shifted)
    res2 = m2.compute()
    assert res2["per_class"][2]["recall"] == [0.0, 0.0] and res2["per_class"][2]["precision"] == [0.0, 0.0]
    for c in (0, 1, 3):
        assert res2["per_class"][c] == res["per_class"][c] or c == 0
    assert res2["per_class"][1]["recall"] == [1.0, 1.0] and res2["per_class"][3]["recall"] == [1.0, 1.0]
    m.merge(m2)
    assert m.compute()["per_class"][2]["recall"] == [0.5, 0.5]
    m.reset()
    assert int(m.state()[1].sum()) == 0


# ------------------------------------------------------------------ layers ----

K_, H_, W_ = 4, 64, 96
PEAK_KW = dict(max_peaks=5, radius=2, threshold=0.05)
EVAL_TH = (2.0, 4.0, 8.0, 16.0)


def _model(dev, seed=21):
    from src.model import KeypointsGauss
    m = KeypointsGauss(K_, H_, W_, backbone="resnet18", pretrained=False)
    m.load_state_dict(recipe.seeded_state_dict("resnet18", seed))
    return m.to(dev)


def _labels(n, seed, dev=None):
    pk, ct, lab = ref.random_batch(seed, n, K_, 4, 3, size=float(H_))
    t = torch.from_numpy(lab)
    return t if dev is None else t.to(dev)


def _direct(m, x, lab, th=EVAL_TH, bins=1024, kw=PEAK_KW):
    """The integers of ops.peaks_match on predict_peaks of the same input."""
    from hkp import ops
    pk, ct = m.predict_peaks(x, **kw)
    hist = torch.zeros((K_, len(th), 2, bins), dtype=torch.int64, device=x.device)
    totals = torch.zeros((K_, 8), dtype=torch.int64, device=x.device)
    ops.peaks_match(pk, ct, lab, th, hist, totals, bins=bins)
    return hist.cpu(), totals.cpu()


def test_model_and_prediction_evaluate(cuda_device):
    from hkp import parallel
    from hkp.metrics import KeypointMetrics
    from src.prediction import Prediction
    m = _model(cuda_device)
    x = recipe.to_tensor_nchw(recipe.seeded_images_u8(2, H_, W_, 22)).to(cuda_device)
    lab = _labels(2, 23, cuda_device)
    want_h, want_t = _direct(m, x, lab)
    assert int(want_t[:, 3].sum()) > 0 and int(want_t[:, 2].sum()) > 0
    for run in (lambda mt: m.evaluate(x, lab, mt, **PEAK_KW),
                lambda mt: Prediction(m, K_, H_, W_, True).evaluate(x, lab, mt, **PEAK_KW),
                lambda mt: parallel.evaluate_dp(m, x, lab, mt, **PEAK_KW)):
        mt = KeypointMetrics(K_, EVAL_TH)
        pk, ct = run(mt)
        assert mt.hist.is_cuda and tuple(pk.shape) == (2, K_, 5, 3) and tuple(ct.shape) == (2, K_)
        h, t = mt.state()
        assert torch.equal(h, want_h) and torch.equal(t, want_t)
        assert mt.all_reduce() is mt                         # no process group: nothing to do


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
        lo, hi = parallel.shard_range(4, rank, world)
        x = recipe.to_tensor_nchw(recipe.seeded_images_u8(4, H_, W_, 22))[lo:hi].to(dev)
        lab = _labels(4, 23)[lo:hi].contiguous().to(dev)
        mt = KeypointMetrics(K_, EVAL_TH)
        parallel.evaluate_dp(m, x, lab, mt, **PEAK_KW)
        mt.all_reduce()
        h, t = mt.state()
        torch.cuda.synchronize()
        q.put(dict(rank=rank, hist=h.numpy(), totals=t.numpy()))
        dist.destroy_process_group()
    except Exception as e:            # report instead of hanging the parent on q.get
        q.put(dict(rank=rank, error=repr(e)))
        raise


def test_evaluate_dp_gloo_world2(cuda_device):
    """Two ranks on one GPU, each its half of a batch of 4 (per-shard BN statistics),
    one all_reduce at the end: the integers of the two halves matched directly."""
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
    x = recipe.to_tensor_nchw(recipe.seeded_images_u8(4, H_, W_, 22)).to(cuda_device)
    lab = _labels(4, 23, cuda_device)
    parts = [_direct(m, x[lo:hi], lab[lo:hi].contiguous()) for lo, hi in ((0, 2), (2, 4))]
    want_h, want_t = parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]
    assert int(want_t[:, 0].sum()) == 4 * K_ and int(want_t[:, 3].sum()) > 0
    for r in res:
        assert np.array_equal(r["hist"], want_h.numpy()) and np.array_equal(r["totals"], want_t.numpy()), r["rank"]


def _parent_fit(train_mod, train_data, test_data, model, epochs, checkpoint_path=""):
    """fit() of the commit before config.EVAL, statement for statement."""
    for epoch in range(epochs):
        train_loss = 0.0
        i_batch = 0
        for i_batch, sample_batched in enumerate(train_data):
            train_mod.optimizer.zero_grad()
            loss = train_mod.forward(sample_batched, model)
            loss.backward()
            train_mod._reduce_grads(model)
            train_mod.optimizer.step()
            train_loss += loss.item()
            print("[%d, %5d] loss: %.3f" % (epoch + 1, i_batch + 1, loss.item()), end="")
            print("\r", end="")
        print("train loss:", train_loss / max(i_batch, 1))
        test_loss = 0.0
        i_batch = 0
        for i_batch, sample_batched in enumerate(test_data):
            loss = train_mod.forward(sample_batched, model)
            test_loss += loss.item()
        print("test loss:", test_loss / max(i_batch, 1))
        if epoch % 2 == 0:
            torch.save(model.state_dict(), checkpoint_path + "/model_2_1_" + str(epoch) + ".pth")


def test_fit_with_and_without_eval(cuda_device, tmp_path, monkeypatch, capsys):
    import _spy
    import train as train_mod
    from hkp import net
    from hkp.metrics import KeypointMetrics
    dev = cuda_device
    imgs = recipe.to_tensor_nchw(recipe.seeded_images_u8(6, H_, W_, 41))
    lab = _labels(6, 42)
    train_data = [(imgs[:2], lab[:2])]
    test_data = [(imgs[2:4], lab[2:4]), (imgs[4:6], lab[4:6])]
    assert train_mod.EVAL is None
    monkeypatch.setattr(train_mod, "_bucketer", None)

    def run(fit, model):
        monkeypatch.setattr(train_mod, "optimizer", torch.optim.SGD(model.parameters(), lr=0.0))
        capsys.readouterr()
        fit(train_data, test_data, model, epochs=2, checkpoint_path=str(tmp_path))
        return capsys.readouterr().out

    # EVAL = None: the output of the parent commit's fit, line for line
    out_parent = run(lambda *a, **kw: _parent_fit(train_mod, *a, **kw), _model(dev, 43))
    out_none = run(train_mod.fit, _model(dev, 43))
    assert out_none == out_parent and out_none.count("test loss:") == 2 and "test eval" not in out_none

    # EVAL set: one forward per test batch, one more line after `test loss:`
    cfg = dict(thresholds=EVAL_TH, **PEAK_KW)
    monkeypatch.setattr(train_mod, "EVAL", cfg)
    m = _model(dev, 43)
    calls, convs = [], []
    real = net.keypoints_forward

    def counting(*a, **kw):
        calls.append((torch.is_grad_enabled(), kw.get("heat"), kw.get("trace") is not None))
        return real(*a, **kw)
    monkeypatch.setattr(net, "keypoints_forward", counting)
    first = m.resnet.net.layer1[0].conv1
    with _spy.spy_calls(on_conv_fwd=lambda conv, *a: convs.append(conv is first)):
        monkeypatch.setattr(train_mod, "optimizer", torch.optim.SGD(m.parameters(), lr=0.0))
        capsys.readouterr()
        train_mod.fit([], test_data, m, epochs=1, checkpoint_path=str(tmp_path))
        out = capsys.readouterr().out
    monkeypatch.setattr(net, "keypoints_forward", real)
    assert calls == [(False, True, False)] * 2, calls           # under no_grad, heat=True, no trace
    assert sum(convs) == 2                                      # the backbone ran once per test batch
    lines = out.strip().split("\n")
    assert [ln.split(":")[0] for ln in lines] == ["train loss", "test loss", "test eval"], lines
    mt = KeypointMetrics(K_, EVAL_TH)
    for x, lb in test_data:
        m.evaluate(x.to(dev), lb.to(dev), mt, **PEAK_KW)
    assert lines[2] == "test eval: " + mt.summary()
    for t in EVAL_TH:
        assert "@%g " % t in lines[2]
    assert "mAP" in lines[2] and "mean error" in lines[2]
    # the loss of that forward is the test loss the plain loop reports
    l_eval = float(lines[1].split(":")[1])
    l_none = float(out_none.strip().split("\n")[-1].split(":")[1])
    assert abs(l_eval - l_none) <= 1e-4 * abs(l_none), (l_eval, l_none)    # two fp32-accurate forwards
    # dense targets cannot be evaluated
    from hkp import ops
    with pytest.raises(ops.HkpError, match="point labels"):
        train_mod.fit([], [(imgs[:1], torch.zeros((1, K_, H_, W_), dtype=torch.float64))], m, epochs=1,
                      checkpoint_path=str(tmp_path))


def test_analysis_writes_metrics(tmp_path, monkeypatch, cuda_device):
    """analysis.main(label_dir=...) with config.EVAL set: metrics.json holds the
    integers of a direct update over the same files ([K,2] and [K,m,3] label files; with
    RESIZE an image of another size is matched in its own pixels); nothing else changes,
    and without label_dir or EVAL there is no metrics.json."""
    import analysis as analysis_mod
    from PIL import Image
    from hkp import ops, resample
    from hkp.metrics import KeypointMetrics
    from src.dataset import transform
    from src.model import KeypointsGauss
    BB = "resnet34"
    cfg = {"thresholds": (4.0, 16.0, 64.0), "max_peaks": 3, "radius": 1, "threshold": 0.1, "bins": 32}
    for name, v in (("IMG_HEIGHT", H_), ("IMG_WIDTH", W_), ("RESIZE", "hamming"), ("RESIZE_PARAMS", {"mode": "fit"})):
        monkeypatch.setattr(analysis_mod, name, v)
    assert (analysis_mod.BACKBONE, analysis_mod.NUM_KEYPOINTS, analysis_mod.EVAL) == (BB, K_, None)
    sd = recipe.seeded_state_dict(BB, 91)
    (tmp_path / "ck").mkdir()
    torch.save(sd, tmp_path / "ck" / "m.pth")
    (tmp_path / "imgs").mkdir()
    (tmp_path / "labels").mkdir()
    srcs = [recipe.seeded_images_u8(1, H_, W_, 92)[0], recipe.seeded_images_u8(1, 150, 330, 93)[0]]
    rng = np.random.default_rng(94)
    labs = [rng.uniform(0, 60, (K_, 2)), np.concatenate([rng.uniform(0, 150, (K_, 2, 2)), np.ones((K_, 2, 1))], 2)]
    labs[1][1, :, 2] = 0                                           # an absent keypoint
    for i, bgr in enumerate(srcs):
        Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(tmp_path / "imgs" / ("f%d.png" % i))
        np.save(tmp_path / "labels" / ("f%d.npy" % i), labs[i])
    run = lambda out, **kw: analysis_mod.main("m.pth", str(tmp_path / "imgs"), out_dir=str(tmp_path / out),  # noqa: E731
                                              checkpoint_dir=str(tmp_path / "ck"), **kw)
    kp_plain = run("plain", label_dir=str(tmp_path / "labels"))     # EVAL is None
    assert not (tmp_path / "plain" / "metrics.json").exists()
    monkeypatch.setattr(analysis_mod, "EVAL", cfg)
    run("nolabels")
    assert not (tmp_path / "nolabels" / "metrics.json").exists()
    kp = run("preds", label_dir=str(tmp_path / "labels"))
    assert np.array_equal(kp, kp_plain) and not (tmp_path / "preds" / "peaks.npy").exists()
    got = json.load(open(tmp_path / "preds" / "metrics.json"))
    m = KeypointsGauss(K_, H_, W_, backbone=BB, pretrained=False)
    m.load_state_dict(sd)
    m = m.to(cuda_device)
    plan = resample.Resize("hamming", mode="fit").plan([(150, 330)], (H_, W_))
    flat = torch.from_numpy(np.ascontiguousarray(srcs[1]).reshape(-1)).to(cuda_device)
    frames = [srcs[0], ops.resample_ragged_u8(flat, plan)[0].cpu().numpy()]
    mt = KeypointMetrics(K_, cfg["thresholds"], bins=32)
    kw = {k: cfg[k] for k in ("max_peaks", "radius", "threshold")}
    for i, frame in enumerate(frames):
        pk, ct = m.predict_peaks(transform(frame).to(cuda_device)[None], **kw)
        if i == 1:
            pk = plan.invert_peaks(pk.cpu(), ct.cpu()).to(cuda_device)
        lab = labs[i].astype(np.float32)
        mt.update(pk, ct, torch.from_numpy(lab[None] if lab.ndim == 2 else lab[None]).to(cuda_device).contiguous())
    want = analysis_mod._json_safe(mt.compute())
    assert got == json.loads(json.dumps(want))
    assert got["overall"]["planes"] == 2 * K_ and got["overall"]["instances"] == K_ + 2 * (K_ - 1)
    assert got["overall"]["peaks"] > 0 and got["per_class"][1]["absent_planes"] == 1
    assert got["thresholds"] == [4.0, 16.0, 64.0] and got["bins"] == 32
