"""Line labels on the GPU: hkp_line_target against the numpy restatement of
tests/_lines_ref.py (which does not cull) bit for bit, against hkp_gauss_target_multi on
planes of points, its store paths, and the layers above it: Trainer, DeviceBatches,
LineMetrics, and a learning check.

Shapes (n, k, s, H, W): the kernel's tile is 32 x 32, 4 pixels of a row per thread.  One
pixel; odd widths (the scalar stores); 128 slots; several tiles a plane with ragged edges;
W % 4 == 0 (16-byte stores of both outputs) over 3 x 4 tiles; W % 4 == 2 (16-byte stores of
the doubles alone, the last pair of a row on its own)."""
import numpy as np
import pytest
import torch

import _lines_ref as ref
from oracle import recipe

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1, 1), (2, 3, 4, 17, 23), (1, 2, 128, 33, 131), (2, 4, 96, 75, 101), (1, 2, 8, 70, 100),
          (1, 3, 5, 35, 66)]
SIGMAS = (8.0, 0.75)
NAN = float("nan")
KINDS = 5


def _plane(kind, s, H, W, rng):
    """float32 [s,5] of one plane.  kind 0: horizontal, vertical, diagonal and zero-length
    segments, one across every tile border, two identical ones, an empty slot between them;
    1: every slot present, two near and the rest far (the cull); 2: no present slot: flags
    0, -1 and NaN over NaN coordinates; 3: two parallel segments equidistant from the first
    tile, segments partly outside, and wholly outside more than 1000 px away; 4: every slot
    present, all over the picture."""
    w, h = float(W - 1), float(H - 1)
    if kind == 0:
        rows = [ref.seg(0.1 * w, 0.3 * h, 0.9 * w, 0.3 * h), [NAN, NAN, NAN, NAN, 0.0], ref.seg(0.6 * w, 0.0, 0.6 * w, h),
                ref.seg(0.0, 0.0, w, h), ref.seg(0.25 * w, 0.75 * h, 0.25 * w, 0.75 * h), ref.seg(0.0, 0.0, w, h),
                [NAN, 1.0, 2.0, NAN, -1.0], ref.seg(w, 0.0, 0.0, h), ref.seg(0.5 * w + 0.25, 0.5 * h, 0.5 * w + 0.25, 0.5 * h)]
        rows = rows[:s] if s >= 2 else rows[:1]
        return ref.fill(rows, s, junk=(NAN, NAN, NAN, NAN, NAN))
    if kind == 1:
        far = rng.uniform(1500.0, 30000.0, (s, 1)) * rng.choice([-1.0, 1.0], (s, 2))
        rec = np.concatenate([far, far + rng.uniform(-40, 40, (s, 2)), np.ones((s, 1))], 1)
        rec[s // 2] = ref.seg(0.2 * w, 0.8 * h, 0.7 * w, 0.1 * h)
        if s > 3:
            rec[s - 1] = ref.seg(0.9 * w, 0.9 * h, 0.9 * w, 0.9 * h)
        return rec.astype(np.float32)
    if kind == 2:
        rec = np.full((s, 5), NAN, dtype=np.float32)
        rec[0::3, 4], rec[1::3, 4] = 0.0, -1.0
        return rec
    if kind == 3:
        rows = [ref.seg(-8.0, -5.0, -8.0, h + 5.0), ref.seg(39.0, -5.0, 39.0, h + 5.0), ref.seg(-20.0, 0.5 * h, 0.4 * w, 0.5 * h),
                ref.seg(0.7 * w, 0.6 * h, w + 300.0, h + 200.0), ref.seg(-1200.0, -1100.0, -1500.0, -1050.0),
                ref.seg(w + 2000.0, 0.0, w + 2000.0, h)]
        return ref.fill(rows[:s], s)
    a = rng.uniform(-6.0, [w + 6.0, h + 6.0], (s, 2))
    b = a + rng.uniform(-25.0, 25.0, (s, 2)) * (rng.uniform(0, 1, (s, 1)) > 0.2)
    return np.concatenate([a, b, np.ones((s, 1))], 1).astype(np.float32)


_CASES = {}


def _case(shape):
    """(lines float32 [n,k,s,5], kinds per plane, restated d2 float32 [n,k,H,W]); computed once."""
    if shape not in _CASES:
        n, k, s, H, W = shape
        rng = np.random.default_rng([7, s, H, W])
        kinds = [(p + (3 if shape == SHAPES[4] else 0)) % KINDS for p in range(n * k)]
        lines = np.stack([_plane(kd, s, H, W, rng) for kd in kinds]).reshape(n, k, s, 5)
        want = ref.d2(lines, H, W)
        want.setflags(write=False)
        lines.setflags(write=False)
        _CASES[shape] = (lines, kinds, want)
    return _CASES[shape]


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def test_fixture_holds_what_it_claims():
    kinds = set()
    for shape in SHAPES:
        lines, kd, want = _case(shape)
        kinds |= set(kd)
        empty = ~(lines[..., 4] > 0).any(-1)
        assert np.isposinf(want[empty]).all() and np.isfinite(want[~empty]).all()
    assert kinds == set(range(KINDS))
    lines, kd, _ = _case(SHAPES[2])
    assert (lines[0, 1, :, 4] > 0).all() and lines.shape[2] == 128         # all 128 present ...
    far = np.abs(lines[0, 1, :, :2]).min(-1) > 1000
    assert far.sum() == 126                                                  # ... and most of them far
    lines, kd, _ = _case(SHAPES[3])
    assert np.isnan(lines[kd.index(2) // 4, kd.index(2) % 4]).sum() > 96 * 4


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_equals_restatement(cuda_device, shape):
    from hkp import ops
    n, k, s, H, W = shape
    lines, kinds, want = _case(shape)
    ld = _dev(lines, cuda_device)
    empty = torch.from_numpy(~(lines[..., 4] > 0).any(-1))
    with torch.cuda.device(cuda_device):
        for sigma in SIGMAS:
            target, d2 = ops.line_target(ld, H, W, sigma, want_d2=True)
            assert target.dtype == torch.float64 and d2.dtype == torch.float32
            assert target.shape == d2.shape == (n, k, H, W)
            assert torch.equal(_bits(d2.cpu()), _bits(torch.from_numpy(want.copy())))
            t = target.cpu()
            if empty.any():
                assert torch.isposinf(d2.cpu()[empty]).all()
                assert (_bits(t[empty]) == 0).all()                          # +0.0, not -0.0
            # within one fp32 ulp of the float64 exp of the kernel's own fp32 quotient
            e = ref.target64(d2.cpu().numpy(), sigma)
            tn = t.numpy()
            assert np.array_equal(tn, tn.astype(np.float32).astype(np.float64))
            ulp = np.spacing(np.abs(e).astype(np.float32)).astype(np.float64)
            err = np.abs(tn - e) / ulp
            print("%s sigma %g: expf worst %.3f ulp" % (shape, sigma, err.max()))
            assert (err <= 1.0).all()
            assert tn.max() <= 1.0 and tn.min() >= 0.0


def _points(shape, m, dev):
    n, k, _, H, W = shape
    rng = np.random.default_rng([9, m, H, W])
    pts = np.zeros((n, k, m, 3), dtype=np.float32)
    pts[..., 0] = rng.uniform(-4, W + 3, (n, k, m))
    pts[..., 1] = rng.uniform(-4, H + 3, (n, k, m))
    pts[..., 2] = (rng.uniform(0, 1, (n, k, m)) > 0.25)
    pts[0, 0, :, :2] = np.rint(pts[0, 0, :, :2])                              # on pixel centres too
    if n * k > 1:
        pts[-1, -1, :, 2] = 0.0                                               # an absent plane
    return torch.from_numpy(pts).to(dev)


@pytest.mark.parametrize("m", [1, 16])
@pytest.mark.parametrize("shape", SHAPES[:2] + SHAPES[3:5])
def test_points_have_the_bits_of_gauss_target_multi(cuda_device, shape, m):
    """Every slot a zero-length segment.  m = 1: the same fp32 operations.  m = 16: the
    kernel takes expf of the smallest distance, gauss_target_multi the largest expf: equal
    as far as expf is monotone."""
    from hkp import lines as L
    from hkp import ops
    n, k, _, H, W = shape
    pts = _points(shape, m, cuda_device)
    with torch.cuda.device(cuda_device):
        for sigma in SIGMAS:
            got, d2 = ops.line_target(L.from_points(pts), H, W, sigma, want_d2=True)
            want = ops.gauss_target_multi(pts, H, W, sigma)
            bad = (_bits(got) != _bits(want)).nonzero()
            if len(bad):
                b = tuple(bad[0].tolist())
                print("first differing pixel", b, got[b].item(), want[b].item(), "d2", d2[b].item(), pts[b[0], b[1]].tolist())
            assert len(bad) == 0


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4], SHAPES[5]])
def test_same_bits_from_every_way_of_asking(cuda_device, shape):
    """A second run, one output alone, preallocated outputs, and views one element off a
    16-byte boundary (the scalar stores) with their guard values intact."""
    from hkp import ops
    n, k, s, H, W = shape
    lines, _, want = _case(shape)
    ld = _dev(lines, cuda_device)
    numel = n * k * H * W
    with torch.cuda.device(cuda_device):
        t0, d0 = ops.line_target(ld, H, W, 8.0, want_d2=True)
        assert t0.data_ptr() % 16 == 0 and d0.data_ptr() % 16 == 0
        t1, d1 = ops.line_target(ld, H, W, 8.0, want_d2=True)
        assert torch.equal(_bits(t1), _bits(t0)) and torch.equal(_bits(d1), _bits(d0))
        t2, none = ops.line_target(ld, H, W, 8.0)
        assert none is None and torch.equal(_bits(t2), _bits(t0))
        none, d2 = ops.line_target(ld, H, W, 8.0, want_target=False, want_d2=True)
        assert none is None and torch.equal(_bits(d2), _bits(d0))
        # sigma is not read without a target
        assert torch.equal(_bits(ops.line_target(ld, H, W, 0.75, want_target=False, want_d2=True)[1]), _bits(d0))
        out, out_d2 = torch.full_like(t0, 7.0), torch.full_like(d0, 7.0)
        rt, rd = ops.line_target(ld, H, W, 8.0, want_d2=True, out=out, out_d2=out_d2)
        assert rt is out and rd is out_d2
        assert torch.equal(_bits(out), _bits(t0)) and torch.equal(_bits(out_d2), _bits(d0))
        for off in (1, 3):
            bt = torch.full((numel + 8,), 7.0, dtype=torch.float64, device=cuda_device)
            bd = torch.full((numel + 8,), 7.0, dtype=torch.float32, device=cuda_device)
            vt, vd = bt[off:off + numel].view(n, k, H, W), bd[off:off + numel].view(n, k, H, W)
            assert vt.data_ptr() % 16 != 0 and vd.data_ptr() % 16 != 0
            ops.line_target(ld, H, W, 8.0, want_d2=True, out=vt, out_d2=vd)
            assert torch.equal(_bits(vt), _bits(t0)) and torch.equal(_bits(vd), _bits(d0))
            for buf in (bt, bd):
                assert (buf[:off] == 7).all() and (buf[off + numel:] == 7).all()
        # the outputs are checked before the launch
        for kw in (dict(out=out.float()), dict(out=out[:, :, :, :-1]), dict(out=out[:, :1].contiguous()),
                   dict(out_d2=out_d2), dict(out=out, want_target=False, want_d2=True)):
            with pytest.raises(ops.HkpError, match="line_target"):
                ops.line_target(ld, H, W, 8.0, **kw)


# ------------------------------------------------------------------ the layers above ----
HW_ = (96, 128)
SCENES2 = dict(classes=("cap", "tail"), cables=(2, 2), blobs=(0, 2), instances=2)
SCENES3 = dict(classes=("cap", "tail", "cable"), cables=(1, 2), blobs=(0, 2), instances=2)


def _r18(dev, k, seed=23):
    from src.model import KeypointsGauss
    m = KeypointsGauss(k, HW_[0], HW_[1], backbone="resnet18", pretrained=False)
    m.load_state_dict(recipe.seeded_state_dict("resnet18", seed))
    return m.to(dev)


def _batches(dev, scenes, seed, n, bs, fixed=False, **kw):
    from hkp.synth import CableScenes
    from src.dataset import DeviceBatches, SynthDataset
    return DeviceBatches(SynthDataset(CableScenes(seed=seed, **scenes), n, HW_, fixed=fixed, device=dev), bs, device=dev,
                         **kw)


def _grads(m):
    return [p.grad.clone() for p in m.parameters()]


def _spy(monkeypatch):
    from hkp import ops
    calls, real = [], ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    return calls


def test_trainer_step_with_points_as_lines(cuda_device, monkeypatch):
    """lines=from_points(pts) trains what pts=pts trains: every parameter gradient equal
    (hkp_heat_loss_multi's dheat is pinned bit-equal to the dense call elsewhere), and a step
    without lines makes the library calls it made before."""
    from hkp import lines as L
    from hkp.train import Trainer
    m = _r18(cuda_device, 2)
    calls = _spy(monkeypatch)
    with torch.cuda.device(cuda_device):
        img, pts = next(iter(_batches(cuda_device, SCENES2, 31, 4, 4, fixed=True)))
        assert (pts[..., 2] > 0).all(-1).any()                                 # a plane with two instances
        Trainer(m).forward_backward(img, pts=pts)                              # packs the weights: not compared
        del calls[:]
        loss_p = Trainer(m).forward_backward(img, None, None, None, pts=pts, weights=None, gid=None)   # the old form
        plain, names_plain = _grads(m), list(calls)
        assert "hkp_line_target" not in names_plain and names_plain.count("hkp_heat_loss_multi") == 1
        del calls[:]
        tr = Trainer(m)
        tr.step(img, pts=pts)                                                  # through step(): the same calls
        assert [c for c in calls if "adam" not in c] == names_plain
        m2 = _r18(cuda_device, 2)
        Trainer(m2).forward_backward(img, pts=pts)
        del calls[:]
        loss_l = Trainer(m2).forward_backward(img, lines=L.from_points(pts))
        at = names_plain.index("hkp_heat_loss_multi")
        assert list(calls) == names_plain[:at] + ["hkp_line_target", "hkp_heat_loss"] + names_plain[at + 1:]
        assert torch.equal(_bits(loss_l), _bits(loss_p))
        for p, g, want in zip(m2.parameters(), _grads(m2), plain):
            assert torch.equal(_bits(g), _bits(want)), tuple(p.shape)


def test_trainer_step_with_points_and_lines_is_the_manual_chain(cuda_device, monkeypatch):
    from hkp import lines as L
    from hkp import net, ops
    from hkp.autograd import heatmap_loss
    from hkp.train import Trainer
    m = _r18(cuda_device, 3)
    with torch.cuda.device(cuda_device):
        img, pts, lines = next(iter(_batches(cuda_device, SCENES3, 33, 4, 4, fixed=True)))
        assert lines.shape == (4, 3, 96, 5) and pts.shape == (4, 3, 2, 3) and (lines[:, 2, :, 4] > 0).any()
        for kind in ("bce", "mse"):
            tr = Trainer(m, loss=kind)
            loss = tr.forward_backward(img, pts=pts, lines=lines)
            got = _grads(m)
            trace = net.Trace(m.policy)
            hm, _, _ = net.keypoints_forward(m.resnet.net, img, 3, heat=True, trace=trace)
            lab = L.concat(L.from_points(pts), lines)
            assert lab.shape == (4, 3, 98, 5)
            target, _ = ops.line_target(lab, HW_[0], HW_[1], 8.0)
            want_loss, dheat = ops.heat_loss(hm, target, None, 8.0, kind)
            grads = net.keypoints_backward(m.resnet.net, trace, dheat, net.Grads())
            assert torch.equal(_bits(loss), _bits(want_loss))
            for p, g in zip(m.parameters(), got):
                assert torch.equal(_bits(grads[p]), _bits(g)), tuple(p.shape)
            # the target: the point planes are gauss_target_multi's, the cable plane the lines' own
            assert torch.equal(_bits(target[:, :2]), _bits(ops.gauss_target_multi(pts, HW_[0], HW_[1], 8.0)[:, :2]))
            assert torch.equal(_bits(target[:, 2]), _bits(ops.line_target(lines, HW_[0], HW_[1], 8.0)[0][:, 2]))
            # heatmap_loss: the same value, and its gradient through autograd
            hm2 = hm.detach().clone().requires_grad_(True)
            l2 = heatmap_loss(hm2, pts=pts, lines=lines, kind=kind)
            l2.backward()
            assert torch.equal(_bits(l2.detach()), _bits(want_loss)) and torch.equal(_bits(hm2.grad), _bits(dheat))
        # lines alone; and tags read pts alone
        Trainer(m).step(img, lines=lines)
        calls = _spy(monkeypatch)
        for kw in (dict(uv=pts[:, :, 0, :2].contiguous(), lines=lines), dict(lines=lines[:, :2].contiguous()),
                   dict(pts=pts, lines=lines, weights=torch.ones(4, 3, device=cuda_device))):
            with pytest.raises(ops.HkpError):
                Trainer(m).step(img, **kw)
        assert not calls                                                       # each raised before anything was launched


def test_device_batches_carry_lines(cuda_device):
    from hkp import lines as L
    from hkp import ops
    from hkp.geometry import GeometricAugmentation
    from hkp.synth import CableScenes
    from src.dataset import DeviceBatches, SynthDataset, transform
    cs = CableScenes(seed=9, **SCENES3)
    ds = SynthDataset(cs, 6, HW_, device=cuda_device)
    ga = GeometricAugmentation(seed=2, rotate=(-20, 20), hflip=0.5, keep_inside=False, flip_pairs=((0, 1),))
    with torch.cuda.device(cuda_device):
        whole = cs.plan(range(6), 0, HW_)
        want = ops.synth_cables_u8(whole)
        assert whole.lines.shape == (6, 3, 96, 5)
        for bs in (4, 1):
            got = [(i.clone(), p.clone(), ln.clone()) for i, p, ln in DeviceBatches(ds, bs, device=cuda_device)]
            assert len(got) == (2 if bs == 4 else 6)
            assert torch.equal(torch.cat([g[0] for g in got]), want)
            assert torch.equal(torch.cat([g[1] for g in got]).cpu(), torch.from_numpy(whole.pts))
            lines = torch.cat([g[2] for g in got])
            assert lines.dtype == torch.float32 and lines.is_cuda
            assert torch.equal(_bits(lines.cpu()), _bits(torch.from_numpy(whole.lines)))
            # geometric: the picture through the warp, points and lines through the plan
            got = [(i.clone(), p.clone(), ln.clone()) for i, p, ln in DeviceBatches(ds, bs, device=cuda_device, geometric=ga)]
            gplan = ga.plan(range(6), 0, uvs=whole.pts, hw=HW_)
            assert gplan.flipped.any() and not gplan.flipped.all()
            if bs == 4:
                assert torch.equal(got[0][0], ops.warp_affine_u8(want[:4].contiguous(), ga.plan(range(4), 0, uvs=whole.pts[:4], hw=HW_)))
            assert torch.equal(torch.cat([g[1] for g in got]).cpu(), torch.from_numpy(gplan.apply_points(whole.pts)))
            assert torch.equal(_bits(torch.cat([g[2] for g in got]).cpu()), _bits(torch.from_numpy(gplan.apply_lines(whole.lines))))
        moved = gplan.apply_lines(whole.lines)
        on = whole.lines[..., 4] > 0
        assert np.array_equal(moved[..., 4], whole.lines[..., 4]) and not np.array_equal(moved[on], whole.lines[on])
        # items
        raw, rpts, rlines = ds.raw(5)
        assert np.array_equal(raw, want[5].cpu().numpy())
        assert torch.equal(rpts.cpu(), torch.from_numpy(whole.pts[5])) and torch.equal(rlines.cpu(), torch.from_numpy(whole.lines[5]))
        item, ipts, ilines = ds[5]
        assert torch.equal(item, transform(raw)) and torch.equal(ipts, rpts) and torch.equal(ilines, rlines)
        dense = SynthDataset(cs, 6, HW_, return_uv=False, device=cuda_device)[5]
        assert len(dense) == 2
        lab = L.concat(L.from_points(rpts[None]), rlines[None])
        assert torch.equal(_bits(dense[1]), _bits(ops.line_target(lab, HW_[0], HW_[1], 8)[0][0]))
        # scenes without a line class: pairs, as before
        assert len(next(iter(_batches(cuda_device, SCENES2, 9, 2, 2)))) == 2


def _metrics_fixture():
    """Integer end points, axis-parallel and 45-degree segments: d2 is a multiple of 1/2."""
    H, W = 40, 70
    planes = [ref.fill([ref.seg(5, 20, 60, 20), ref.seg(33, 2, 33, 38)], 3), ref.fill([ref.seg(10, 5, 30, 25), ref.seg(50, 30, 50, 30)], 3),
              ref.fill([], 3)]
    lines = np.stack(planes)[None].astype(np.float32)
    return lines, ref.d2(lines, H, W), H, W


def test_line_metrics(cuda_device):
    from hkp import lines as L
    from hkp import ops
    lines, d2, H, W = _metrics_fixture()
    sigma, thr = 8.0, 0.5
    r2 = -float(ref.den(sigma)) * np.log(thr)
    finite = np.isfinite(d2)
    assert (np.abs(d2[finite] - r2) > 2.0 ** -10 * r2).all()                   # no pixel near the band's edge
    ld = _dev(lines, cuda_device)
    with torch.cuda.device(cuda_device):
        target, _ = ops.line_target(ld, H, W, sigma)
        m = L.LineMetrics(3, radius=float(np.sqrt(r2)), threshold=thr)
        m.update(target.float(), ld)
        res = m.compute()
        for c in (0, 1):
            n_in = int((d2[0, c] <= r2).sum())
            assert n_in > 0 and res[c]["hit"] == res[c]["pred"] == res[c]["line"] == n_in
            assert res[c]["completeness"] == res[c]["correctness"] == res[c]["iou"] == 1.0
        assert res[2]["line"] == 0 and res[2]["pred"] == 0 and np.isnan(res[2]["completeness"])
        # counts against numpy, over two updates, on a heat that is not the target
        rng = np.random.default_rng(5)
        m = L.LineMetrics(3, radius=4.0, threshold=0.6)
        want = np.zeros((3, 3), dtype=np.int64)
        for _ in range(2):
            heat = rng.uniform(0, 1, (1, 3, H, W)).astype(np.float32)
            heat[0, 0] = np.where(d2[0, 0] <= 30.0, 0.9, heat[0, 0] * 0.5)
            m.update(_dev(heat, cuda_device), ld)
            p, g = heat >= np.float32(0.6), d2 <= np.float32(16.0)
            want += np.stack([(p & g).sum((0, 2, 3)), p.sum((0, 2, 3)), g.sum((0, 2, 3))], 1)
        res = m.compute()
        assert [[r["hit"], r["pred"], r["line"]] for r in res] == want.tolist()
        assert res[0]["completeness"] == 1.0 and 0 < res[0]["correctness"] < 1.0
        assert res[1]["iou"] == want[1, 0] / (want[1, 1] + want[1, 2] - want[1, 0])
        m.reset()
        assert m.compute()[0]["line"] == 0


def test_training_lowers_the_held_out_cable_loss(cuda_device):
    """R18-8s, 96x128, classes (cap, tail, cable): 24 Trainer steps of batch 8 on fresh scenes
    with pts and lines; the BCE of the cable plane over 16 fixed held-out scenes must be lower
    afterwards (a sign condition; README "Line labels" records the two values)."""
    from hkp import ops
    from hkp.train import Trainer
    STEPS = 24
    model = _r18(cuda_device, 3)
    with torch.cuda.device(cuda_device):
        himg, hpts, hlines = next(iter(_batches(cuda_device, SCENES3, 11, 16, 16, fixed=True)))
        target = ops.line_target(hlines, HW_[0], HW_[1], 8.0)[0][:, 2]

        def held_out():
            with torch.no_grad():
                p = model(himg)[:, 2].double()
            return -(target * p.log().clamp(min=-100) + (1 - target) * (1 - p).log().clamp(min=-100)).mean().item()

        before = held_out()
        tr = Trainer(model, loss="bce", absent="zero")
        last = None
        for img, pts, lines in _batches(cuda_device, SCENES3, 10, 8 * STEPS, 8):
            last = tr.step(img, pts=pts, lines=lines)
        after = held_out()
    print("held-out cable-plane BCE before %.6f after %.6f; last train loss %.6f" % (before, after, last.item()))
    assert np.isfinite(after) and after < before


def _train_py(train_mod, tmp_path, monkeypatch, **extra):
    monkeypatch.chdir(tmp_path)                                            # no data/ directory here
    for name, v in dict(IMG_HEIGHT=96, IMG_WIDTH=128, NUM_KEYPOINTS=3, batch_size=4, epochs=1, BACKBONE="resnet18",
                        SYNTH={"train": 8, "test": 4, "seed": 5, "classes": ("cap", "tail", "cable"), "instances": 2,
                               "cables": (1, 2)}, **extra).items():
        monkeypatch.setattr(train_mod, name, v)
    torch.manual_seed(5)


def test_train_py_with_a_line_class(tmp_path, monkeypatch, capsys, cuda_device):
    """The items are dense targets (return_uv=False) and _loss takes them as it stands;
    EVAL and TAGS need point labels and are refused at start-up."""
    import train as train_mod
    _train_py(train_mod, tmp_path, monkeypatch)
    with pytest.warns(UserWarning, match="pretrained"):
        train_mod.main("scenes")
    out = capsys.readouterr().out
    train_loss = float(out.split("train loss:")[1].split()[0])
    test_loss = float(out.split("test loss:")[1].split()[0])
    assert np.isfinite(train_loss) and train_loss > 0 and np.isfinite(test_loss) and test_loss > 0
    assert (tmp_path / "checkpoints" / "scenes" / "model_2_1_0.pth").exists()
    for extra in (dict(EVAL={"thresholds": (8,)}, TAGS=None), dict(EVAL=None, TAGS={"classes": ("cap", "tail")})):
        _train_py(train_mod, tmp_path, monkeypatch, **extra)
        with pytest.raises(ValueError, match="holds a line class"):
            train_mod.main("scenes")
