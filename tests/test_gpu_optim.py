"""Gradient clipping by the global L2 norm and the weight EMA of FusedAdam
(hkp_grad_norm, hkp_adam_step_ex; csrc/adam.hip), pinned as chains of torch ops.

Tensor set: the smallest shapes at which the 4096-element unit table can go wrong —
lengths 1, 37, 4096, 4097, 3*4096+5, an empty tensor, one of 300*4096+1 elements (the
finishing block loops over more than 256 partials), a misaligned view (store[1:], a
multiple of 4 long, so only the pointer sends it down the scalar path), 50 tensors in
all (the 48-tensor launches are crossed).

* norm: within one fp32 ulp of float32(sqrt(sum g.double()^2)) (the squares are exact
  in fp64 and the fp64 sum of N < 2^25 non-negative terms is off by < 2^-28 relative,
  below half an fp32 ulp); the coefficient bit-equal to the fp32 formula
  c = max_norm / (norm + 1e-6), min(c, 1) with NaN kept, on the kernel's own norm;
* clipped step == plain FusedAdam fed g * coef (torch's multiply), torch.equal;
* EMA == torch._foreach_lerp_(ema, params, 1 - decay) after each step, torch.equal.
"""
import copy
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import recipe

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "hulk-keypoints_amd")

BIG = 300 * 4096 + 1
LENGTHS = [1, 37, 4096, 4097, 3 * 4096 + 5, 0, BIG] + [5 + 3 * i for i in range(38)] + [8, 64, 1000, 2048]
MISALIGNED = 8192                     # the 50th tensor: store[1:] of 8193 elements
N_TENSORS = len(LENGTHS) + 1
CLIP = 50.0                           # the norms of the four steps are ~1.1, 11, 110, 1100


def _tensors(dev, seed, scale=1.0):
    """50 fresh tensors of the set (the last one a misaligned view), from a seed."""
    gen = torch.Generator().manual_seed(seed)
    ts = [(torch.randn(n, generator=gen) * scale).to(dev) for n in LENGTHS]
    store = (torch.randn(MISALIGNED + 1, generator=gen) * scale).to(dev)
    ts.append(store[1:])
    assert len(ts) == N_TENSORS == 50 and ts[-1].data_ptr() % 16 == 4 and ts[-1].numel() % 4 == 0
    return ts


def _params(dev, seed=5):
    return [torch.nn.Parameter(t) for t in _tensors(dev, seed)]


def _set_grads(ps, dev, step, seed=100):
    """The gradients of test_fused_adam_matches_torch_adam: randn * 10^(step-3)."""
    gs = _tensors(dev, seed + step, 10.0 ** (step - 3))
    for p, g in zip(ps, gs):
        p.grad = g
    return gs


def _kernel_norm(grads, max_norm):
    """hkp_grad_norm on a list of gradients: (norm, coef) as numpy float32."""
    from hkp import _lib
    arr = (_lib.AdamTensor * len(grads))()
    for a, g in zip(arr, grads):
        a.grad, a.n = g.data_ptr(), g.numel()
    need = _lib.lib().hkp_grad_norm_partials(len(grads), arr)
    assert need == sum((g.numel() + 4095) // 4096 for g in grads)
    ws = torch.full((need,), float("nan"), dtype=torch.float64, device=grads[0].device)
    out = torch.full((2,), float("nan"), device=grads[0].device)
    _lib.call("hkp_grad_norm", len(grads), arr, max_norm, ctypes.c_void_p(ws.data_ptr()), need,
              ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    o = out.cpu().numpy()
    return o[0], o[1]


def _coef_formula(norm, max_norm):
    """The issue's fp32 formula on a float32 norm."""
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
    return c if c < 1 else (c if c != c else np.float32(1))


def _bits(x):
    return np.float32(x).view(np.uint32)


def _ref_norm(grads):
    return np.float32(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)).item())


@pytest.fixture(scope="module")
def grads(cuda_device):
    return _tensors(cuda_device, 7)                  # norm ~ sqrt(1.3e6) ~ 1130; left unchanged


@pytest.mark.parametrize("case", ["clipped", "not_clipped", "zero", "nan", "inf"])
def test_grad_norm_and_coefficient(cuda_device, grads, case):
    max_norm = {"clipped": 1.0, "not_clipped": 1.0e6, "zero": 1.0, "nan": 1.0, "inf": float("inf")}[case]
    gs = grads
    if case == "zero":
        gs = [torch.zeros_like(g) for g in grads]
    elif case == "nan":
        gs = [g.clone() for g in grads]
        gs[6][200 * 4096 + 17] = float("nan")
    norm, coef = _kernel_norm(gs, max_norm)
    again = _kernel_norm(gs, max_norm)
    ref = _ref_norm(gs)
    print(case, "norm", norm, "ref", ref, "coef", coef)
    if case == "nan":
        assert np.isnan(norm) and np.isnan(coef) and np.isnan(again[0]) and np.isnan(again[1])
        return
    assert _bits(again[0]) == _bits(norm) and _bits(again[1]) == _bits(coef)        # the same bits on a second run
    assert abs(float(norm) - float(ref)) <= float(np.spacing(ref))                  # one fp32 ulp
    assert _bits(coef) == _bits(_coef_formula(norm, max_norm))
    if case == "clipped":
        assert 0 < coef < 1e-3
    else:
        assert coef == 1.0
    if case == "zero":
        assert norm == 0.0
    # the definition (not the arithmetic): clip_grad_norm_'s return
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in gs]
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    assert abs(float(total) - float(norm)) <= 1e-5 * float(norm)


def test_clipped_step_equals_adam_on_scaled_gradients(cuda_device):
    from hkp.optim import FusedAdam
    dev = cuda_device
    pc, pr = _params(dev), _params(dev)
    oc = FusedAdam(pc, lr=1e-3, weight_decay=1e-4, max_grad_norm=CLIP)
    orf = FusedAdam(pr, lr=1e-3, weight_decay=1e-4)
    coefs = []
    for step in range(4):
        gs = _set_grads(pc, dev, step)
        keep = [g.clone() for g in gs]
        oc.step()
        norm, coef = _kernel_norm(keep, CLIP)
        assert _bits(oc.grad_norm.item()) == _bits(norm) and _bits(oc.clip_coef.item()) == _bits(coef)
        assert oc.grad_norm.dim() == 0 and oc.grad_norm.is_cuda and oc.clip_coef.dim() == 0
        coefs.append(float(coef))
        for p, g, k in zip(pc, gs, keep):
            assert p.grad is g and torch.equal(g, k)                # the gradient is not written
        for p, k in zip(pr, keep):
            p.grad = k * oc.clip_coef                               # torch's multiply, the kernel's coefficient
        orf.step()
        for a, b in zip(pc, pr):
            assert torch.equal(a, b)
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(oc.state[a][key], orf.state[b][key])
            assert float(oc.state[a]["step"]) == step + 1
    print("coefs", coefs)
    assert coefs[0] == 1.0 and coefs[1] == 1.0 and coefs[2] < 1.0 and coefs[3] < 0.1    # engages on some steps only
    assert set(oc.state[pc[0]]) == {"step", "exp_avg", "exp_avg_sq"}


@pytest.mark.parametrize("decay", [0.999, 0.9])
@pytest.mark.parametrize("clip", [None, CLIP])
def test_ema_equals_foreach_lerp(cuda_device, decay, clip):
    from hkp.optim import FusedAdam
    dev = cuda_device
    ps = _params(dev)
    opt = FusedAdam(ps, lr=1e-3, weight_decay=1e-4, ema_decay=decay, max_grad_norm=clip)
    ref = [p.detach().clone() for p in ps]                      # ema_0 = p_0
    fast = []
    real = opt._fast_launch
    opt._fast_launch = lambda *a: fast.append(True) or real(*a)
    for step in range(4):
        _set_grads(ps, dev, step)
        before = [p.detach().clone() for p in ps]
        opt.step()
        if len(fast) <= step:
            fast.append(False)
        torch._foreach_lerp_(ref, [p.detach() for p in ps], 1 - decay)
        emas = opt.ema_parameters()
        assert len(emas) == len(ps)
        moved = 0
        for p, b, r, e in zip(ps, before, ref, emas):
            assert e is opt.state[p]["ema"] and torch.equal(e, r)
            moved += int(not torch.equal(p, b)) + 2 * int(not torch.equal(e, p))
        assert moved > 2 * len(ps)                              # the step moved p, and the EMA lags behind it
    assert fast == [False, True, True, True]                    # the cached table from the second step on


def test_options_off_calls_only_adam_step(cuda_device, monkeypatch):
    from hkp import _lib, optim
    names = []

    def counting(name, *a):
        names.append(name)
        return _lib.call(name, *a)
    monkeypatch.setattr(optim, "call", counting)
    ps, pt = _params(cuda_device), _params(cuda_device)
    opt = optim.FusedAdam(ps, lr=1e-3, weight_decay=1e-4)
    ref = torch.optim.Adam(pt, lr=1e-3, weight_decay=1e-4, foreach=True)
    for step in range(2):
        _set_grads(ps, cuda_device, step)
        _set_grads(pt, cuda_device, step)
        opt.step()
        ref.step()
    assert names == ["hkp_adam_step"] * 2
    assert opt.grad_norm is None and opt.clip_coef is None and opt.ema_parameters() == []
    for a, b in zip(ps, pt):
        assert set(opt.state[a]) == set(ref.state[b]) == {"step", "exp_avg", "exp_avg_sq"}
    # with the options the new entry points run
    names.clear()
    on = optim.FusedAdam(_params(cuda_device), lr=1e-3, max_grad_norm=CLIP, ema_decay=0.9)
    _set_grads(on.param_groups[0]["params"], cuda_device, 0)
    on.step()
    assert names == ["hkp_grad_norm", "hkp_adam_step_ex"]


def _run(opt, ps, dev, steps):
    for step in steps:
        _set_grads(ps, dev, step)
        opt.step()


def test_state_dict_round_trip(cuda_device):
    from hkp.optim import FusedAdam
    dev = cuda_device
    kw = dict(lr=1e-3, weight_decay=1e-4, max_grad_norm=CLIP, ema_decay=0.9)
    pa = _params(dev)
    oa = FusedAdam(pa, **kw)
    _run(oa, pa, dev, range(4))                                 # the uninterrupted run
    pb = _params(dev)
    ob = FusedAdam(pb, **kw)
    _run(ob, pb, dev, range(2))
    sd = copy.deepcopy(ob.state_dict())
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "ema"}
    pc = [torch.nn.Parameter(p.detach().clone()) for p in pb[:-1]]
    pc.append(torch.nn.Parameter(torch.cat([pb[-1].detach()[:1], pb[-1].detach()])[1:]))    # misaligned again
    oc = FusedAdam(pc, lr=1e-3, weight_decay=1e-4)              # the options come with the loaded groups
    oc.load_state_dict(sd)
    _run(oc, pc, dev, range(2, 4))
    for a, c in zip(pa, pc):
        assert torch.equal(a, c)
        for key in ("exp_avg", "exp_avg_sq", "ema"):
            assert torch.equal(oa.state[a][key], oc.state[c][key]), key
    # into torch.optim.Adam, which steps on with it
    ot = torch.optim.Adam(pc, lr=1e-3, weight_decay=1e-4, foreach=True)
    ot.load_state_dict(copy.deepcopy(oc.state_dict()))
    _set_grads(pc, dev, 1)
    ot.step()
    # torch Adam's own dict (no EMA, no option keys) back: the EMA is re-created from the parameters
    pd = _params(dev, seed=9)
    od = torch.optim.Adam(pd, lr=1e-3, weight_decay=1e-4, foreach=True)
    _set_grads(pd, dev, 1)
    od.step()
    oe = FusedAdam(pd, **kw)
    oe.load_state_dict(od.state_dict())
    assert all("ema" not in oe.state[p] for p in pd)
    assert oe.param_groups[0]["ema_decay"] == 0.9 and oe.param_groups[0]["max_grad_norm"] == CLIP
    start = [p.detach().clone() for p in pd]
    _set_grads(pd, dev, 2)
    oe.step()
    torch._foreach_lerp_(start, [p.detach() for p in pd], 1 - 0.9)
    for p, r in zip(pd, start):
        assert torch.equal(oe.state[p]["ema"], r) and float(oe.state[p]["step"]) == 2.0


# ----------------------------------------------------------------- the network

BB, K, H, W, B = "resnet18", 2, 64, 80, 2


def _model(dev, wseed=23):
    from src.model import KeypointsGauss
    m = KeypointsGauss(K, H, W, backbone=BB, pretrained=False)
    m.load_state_dict(recipe.seeded_state_dict(BB, wseed))
    return m.to(dev)


def _batch(dev, n=B, iseed=21, kseed=22):
    x = recipe.to_tensor_nchw(recipe.seeded_images_u8(n, H, W, iseed)).to(dev)
    uv = torch.from_numpy(recipe.seeded_keypoints(n, K, H, W, kseed)).to(dev)
    return x, uv


def _first_norm(dev):
    from hkp import train
    t = train.Trainer(_model(dev))
    x, uv = _batch(dev)
    t.forward_backward(x, uv=uv)
    return float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in t.params)))


def test_trainer_step_equals_manual_chain(cuda_device):
    """Trainer(max_grad_norm=c, ema_decay=d).step == forward_backward, then g * coef (torch),
    a plain FusedAdam step and _foreach_lerp_; the manual chain runs on a twin model fed
    the gradients the Trainer left in p.grad (unscaled)."""
    from hkp import train
    from hkp.optim import FusedAdam
    dev = cuda_device
    n0 = _first_norm(dev)
    c, d = 0.5 * n0, 0.99                                       # below the first step's norm: the clip engages
    ma, mb = _model(dev), _model(dev)
    t = train.Trainer(ma, max_grad_norm=c, ema_decay=d)
    pb = list(mb.parameters())
    ob = FusedAdam(pb, lr=1e-4, weight_decay=1e-4)
    ema = [p.detach().clone() for p in pb]
    x, uv = _batch(dev)
    for step in range(2):
        t.step(x, uv=uv)
        if step == 0:
            assert abs(float(t.opt.grad_norm) - n0) <= 1e-4 * n0 and float(t.opt.clip_coef) < 0.51
        for a, b in zip(t.params, pb):
            b.grad = a.grad * t.opt.clip_coef
        ob.step()
        torch._foreach_lerp_(ema, [p.detach() for p in pb], 1 - d)
        for a, b, e in zip(t.params, pb, ema):
            assert torch.equal(a, b) and torch.equal(t.opt.state[a]["ema"], e)
            assert torch.equal(t.opt.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"])


def test_ema_weights_context(cuda_device):
    from hkp import train
    dev = cuda_device
    x, uv = _batch(dev)
    peak_kw = dict(max_peaks=3, radius=1, threshold=0.0)
    m, twin = _model(dev), _model(dev)
    t, t2 = train.Trainer(m, max_grad_norm=1.0, ema_decay=0.9), train.Trainer(twin, max_grad_norm=1.0, ema_decay=0.9)
    for _ in range(2):
        t.step(x, uv=uv)
    for _ in range(3):
        t2.step(x, uv=uv)                                       # the uninterrupted run
    raw = [p.detach().clone() for p in t.params]
    emas = [e.clone() for e in t.opt.ema_parameters()]
    assert any(not torch.equal(r, e) for r, e in zip(raw, emas))
    m2 = _model(dev)                                            # a second model loaded with the EMA tensors
    with torch.no_grad():
        for p2, e in zip(m2.parameters(), emas):
            p2.copy_(e)
        for b2, b in zip(m2.buffers(), m.buffers()):
            b2.copy_(b)
    want_pk, want_ct = m2.predict_peaks(x, **peak_kw)
    ptrs = [p.data_ptr() for p in t.params]
    with t.ema_weights():
        for p, e, r in zip(t.params, emas, raw):
            assert torch.equal(p, e) and torch.equal(t.opt.state[p]["ema"], r)
        pk, ct = m.predict_peaks(x, **peak_kw)
    assert torch.equal(pk, want_pk) and torch.equal(ct, want_ct)
    assert int(ct.sum()) > 0
    for p, r, e, ptr in zip(t.params, raw, emas, ptrs):
        assert torch.equal(p, r) and torch.equal(t.opt.state[p]["ema"], e) and p.data_ptr() == ptr
    with pytest.raises(RuntimeError, match="inside"):
        with t.ema_weights():
            assert torch.equal(t.params[0], emas[0])
            raise RuntimeError("inside")
    for p, r, e in zip(t.params, raw, emas):
        assert torch.equal(p, r) and torch.equal(t.opt.state[p]["ema"], e)
    t.step(x, uv=uv)                                            # the next step: the uninterrupted run's
    for a, b in zip(t.params, t2.params):
        assert torch.equal(a, b) and torch.equal(t.opt.state[a]["ema"], t2.opt.state[b]["ema"])


# ---------------------------------------------------------------- data parallel


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, out_dir, q):
    import sys
    sys.path[:0] = [REPO, PKG, os.path.join(REPO, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from hkp import train
        dev = torch.device("cuda:0")
        m = _model(dev, wseed=23 + rank)                        # broadcast_state makes them rank 0's
        t = train.Trainer(m, distributed=True, max_grad_norm=1e-3, ema_decay=0.9)
        x, uv = _batch(dev, n=2 * world)
        x, uv = x[2 * rank:2 * rank + 2], uv[2 * rank:2 * rank + 2].contiguous()
        norms, coefs = [], []
        for _ in range(2):
            t.step(x, uv=uv)
            norms.append(t.opt.grad_norm.clone())
            coefs.append(t.opt.clip_coef.clone())
        torch.cuda.synchronize()
        torch.save(dict(params=[p.detach().cpu() for p in t.params], ema=[e.cpu() for e in t.opt.ema_parameters()],
                        norms=[n.cpu() for n in norms], coefs=[c.cpu() for c in coefs]),
                   os.path.join(out_dir, "rank%d.pt" % rank))
        q.put(dict(rank=rank))
        dist.destroy_process_group()
    except Exception as e:            # report instead of hanging the parent on q.get
        q.put(dict(rank=rank, error=repr(e)))
        raise


def test_data_parallel_ranks_agree(cuda_device, tmp_path):
    """gloo world 2, both ranks on one GPU, 2 images each, two steps with clip and EMA: the
    norm is taken after the bucketed all-reduce, so every rank computes the same bits."""
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, str(tmp_path), q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(60)
    assert all("error" not in r for r in res), res
    assert all(p.exitcode == 0 for p in procs)
    r0, r1 = (torch.load(os.path.join(tmp_path, "rank%d.pt" % r), weights_only=True) for r in range(world))
    for key in ("params", "ema", "norms", "coefs"):
        assert len(r0[key]) == len(r1[key]) > 0
        assert all(torch.equal(a, b) for a, b in zip(r0[key], r1[key])), key
    assert all(0 < float(c) < 1 for c in r0["coefs"]) and all(float(n) > 1e-3 for n in r0["norms"])
    assert any(not torch.equal(p, e) for p, e in zip(r0["params"], r0["ema"]))


# ------------------------------------------------------------------------ fit()


def _write_split(root, split, n, seed):
    from PIL import Image
    img_dir, kp_dir = root / "data" / "toy" / split / "images", root / "data" / "toy" / split / "keypoints"
    img_dir.mkdir(parents=True)
    kp_dir.mkdir(parents=True)
    bgr = recipe.seeded_images_u8(n, H, W, seed)
    uv = recipe.seeded_keypoints(n, K, H, W, seed + 1)
    for i in range(n):
        Image.fromarray(np.ascontiguousarray(bgr[i][:, :, ::-1])).save(img_dir / ("%05d.jpg" % i), format="PNG")
        np.save(kp_dir / ("%05d.npy" % i), uv[i].reshape(-1).astype(np.float64))


def test_fit_writes_ema_checkpoint(cuda_device, tmp_path, monkeypatch, capsys):
    import train as train_mod
    from hkp.optim import FusedAdam
    dev = cuda_device
    x, uv = _batch(dev, n=4)
    data = [(x[:2].cpu(), uv[:2].cpu()), (x[2:].cpu(), uv[2:].cpu())]         # the two-batch synthetic set
    monkeypatch.setattr(train_mod, "_bucketer", None)
    m = _model(dev)
    opt = FusedAdam(m.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, ema_decay=0.9)
    monkeypatch.setattr(train_mod, "optimizer", opt)
    capsys.readouterr()
    train_mod.fit(data, data, m, epochs=2, checkpoint_path=str(tmp_path))
    out = capsys.readouterr().out
    assert [ln.split(":")[0] for ln in out.replace("\r", "\n").split("\n") if ln and not ln.startswith("[")] == \
        ["train loss", "test loss"] * 2
    assert sorted(os.listdir(tmp_path)) == ["model_2_1_0.pth", "model_2_1_0_ema.pth"]
    # epoch 1 moved the weights on: redo epoch 0 alone on a fresh model to compare the files
    (tmp_path / "again").mkdir()
    m1 = _model(dev)
    o1 = FusedAdam(m1.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, ema_decay=0.9)
    monkeypatch.setattr(train_mod, "optimizer", o1)
    train_mod.fit(data, data, m1, epochs=1, checkpoint_path=str(tmp_path / "again"))
    raw_file = torch.load(tmp_path / "again" / "model_2_1_0.pth", map_location="cpu", weights_only=True)
    ema_file = torch.load(tmp_path / "again" / "model_2_1_0_ema.pth", map_location="cpu", weights_only=True)
    raw_want = {k: v.cpu() for k, v in m1.state_dict().items()}
    with o1.ema_weights():
        ema_want = {k: v.cpu() for k, v in m1.state_dict().items()}
    assert list(raw_file) == list(ema_file) == list(raw_want)
    names = {n for n, _ in m1.named_parameters()}
    assert all(torch.equal(raw_file[k], raw_want[k]) for k in raw_want)       # the raw weights, to resume from
    assert all(torch.equal(ema_file[k], ema_want[k]) for k in names)          # the EMA tensors
    assert any(not torch.equal(ema_file[k], raw_file[k]) for k in names)
    # the first epoch of the two-epoch run wrote the same files
    for name, want in (("model_2_1_0.pth", raw_file), ("model_2_1_0_ema.pth", ema_file)):
        got = torch.load(tmp_path / name, map_location="cpu", weights_only=True)
        assert all(torch.equal(got[k], want[k]) for k in names), name


@pytest.mark.parametrize("ema_decay", [None, 0.9])
def test_main_builds_the_optimizer(cuda_device, tmp_path, monkeypatch, capsys, ema_decay):
    """Both options None: main() builds torch.optim.Adam as it always did and writes
    today's lines and files; with EMA_DECAY set it builds FusedAdam with the option."""
    import train as train_mod
    from hkp.optim import FusedAdam
    _write_split(tmp_path, "train", 2, 71)
    _write_split(tmp_path, "test", 2, 81)
    monkeypatch.chdir(tmp_path)
    for name, v in (("IMG_HEIGHT", H), ("IMG_WIDTH", W), ("NUM_KEYPOINTS", K), ("batch_size", 2), ("epochs", 1),
                    ("BACKBONE", BB), ("EMA_DECAY", ema_decay)):
        monkeypatch.setattr(train_mod, name, v)
    assert train_mod.MAX_GRAD_NORM is None
    capsys.readouterr()
    with pytest.warns(UserWarning, match="pretrained"):
        train_mod.main("toy")
    out = capsys.readouterr().out
    lines = [ln.split(":")[0] for ln in out.replace("\r", "\n").split("\n") if ln and not ln.startswith("[")]
    assert lines == ["train loss", "test loss"]
    files = sorted(os.listdir(tmp_path / "checkpoints" / "toy"))
    opt = train_mod.optimizer
    if ema_decay is None:
        assert type(opt) is torch.optim.Adam
        assert opt.defaults["lr"] == 1.0e-4 and opt.defaults["weight_decay"] == 1.0e-4
        assert files == ["model_2_1_0.pth"]
    else:
        assert type(opt) is FusedAdam
        g = opt.param_groups[0]
        assert (g["lr"], g["weight_decay"], g["ema_decay"], g["max_grad_norm"]) == (1.0e-4, 1.0e-4, 0.9, None)
        assert files == ["model_2_1_0.pth", "model_2_1_0_ema.pth"]
        assert len(opt.ema_parameters()) == len(list(train_mod.keypoints.parameters()))
