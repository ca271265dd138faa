"""Domain randomisation on the GPU (csrc/augment.hip, hkp.augment): the kernel
against the numpy restatement (tests/_augment_ref.py), bit for bit — there is no
tolerance in this file — and the plumbing through DomainRandomization,
DeviceBatches and one training step."""
import functools
import io
import os

import numpy as np
import pytest
import torch

import _augment_ref as ref
from oracle import recipe

pytestmark = pytest.mark.gpu


def _shapes():
    from hkp import augment
    th, tw = augment.TILE_H, augment.TILE_W
    # all reflect; odd row bytes within one tile; one tile + 1; two tiles + 3
    return [(3, 3), (37, 53), (th + 1, tw + 1), (2 * th + 3, 2 * tw + 3)]


SHAPE_IDS = ["3x3", "37x53", "tile+1", "2tiles+3"]


@functools.lru_cache(maxsize=None)
def _images(b, h, w, seed=41):
    a = recipe.seeded_images_u8(b, h, w, seed)
    a.setflags(write=False)
    return a


def _run(imgs, plan, dev):
    from hkp import ops
    x = torch.from_numpy(np.array(imgs)).to(dev)
    out = ops.augment_u8(x, plan)
    assert out.dtype == torch.uint8 and out.shape == x.shape and out.data_ptr() != x.data_ptr()
    assert torch.equal(x.cpu(), torch.from_numpy(np.array(imgs)))      # the input is left alone
    return out.cpu().numpy()


def _check(imgs, stages, dev):
    from hkp import augment
    plan = augment.Plan.from_stages(stages)
    got = _run(imgs, plan, dev)
    want = ref.apply_plan(imgs, plan)
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, "%d bytes differ, first at (b, y, x, c) = %s: got %d, want %d" % (
        bad.shape[0], tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    return got


def _random_lut(seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(256).astype(np.uint8) for _ in range(3)])


def _identity_lut():
    return np.tile(np.arange(256, dtype=np.uint8), (3, 1))


def _stage(kind, b):
    """Stage `kind` with the parameters of image b (a different program per image)."""
    from hkp import augment
    if kind == "lut":
        return ("lut", _random_lut(100 + b))
    if kind == "hsv":
        return [("hsv", np.float32(6.0 * 20 / 255.0), 20.0, 1.0), ("hsv", np.float32(-6.0 * 20 / 255.0), -20.0, 1.0),
                ("hsv", 0.0, 0.0, np.float32(1.05))][b % 3]
    if kind == "blur":
        return ("blur",) + augment.blur_weights((0.6, 0.3, 0.45)[b % 3])
    return ("noise", np.float32((3.1875, 1.0, 0.37)[b % 3]), 0x1234 + b, 0xdeadbeef - b)


@pytest.mark.parametrize("hw", _shapes(), ids=SHAPE_IDS)
def test_identity(cuda_device, hw):
    imgs = _images(3, *hw)
    dropped = [("lut", _identity_lut()), ("blur", 1.0, 0.0, 0.0), ("noise", 0.0, 5, 6), ("lut", _identity_lut())]
    for stages in ([[], [], []], [dropped, dropped[:2], dropped[2:]]):
        assert np.array_equal(_check(imgs, stages, cuda_device), imgs)


def test_sampled_drops_are_identity(cuda_device):
    """sigma = 0 and s = 0 drop their stages: with every other operator off the
    sampled program is empty and the batch comes back as it went in."""
    from hkp import augment
    dr = augment.DomainRandomization(ops={"blur": (0, 0), "noise": (0, 0), "hue_sat": None, "contrast": None,
                                          "add": None, "gamma": None, "temperature": None, "mul_sat": None})
    plan = dr.plan([0, 1, 2])
    assert [p.nstages for p in plan.programs] == [0, 0, 0]
    imgs = _images(3, 37, 53)
    assert np.array_equal(_run(imgs, plan, cuda_device), imgs)


@pytest.mark.parametrize("hw", _shapes(), ids=SHAPE_IDS)
@pytest.mark.parametrize("kind", ["lut", "hsv", "blur", "noise"])
def test_each_stage_alone(cuda_device, kind, hw):
    imgs = _images(3, *hw)
    got = _check(imgs, [[_stage(kind, b)] for b in range(3)], cuda_device)
    assert not np.array_equal(got, imgs)


def test_hsv_sector_ties_and_wrap(cuda_device):
    """Every grey (d = 0), black, and the pure primaries / secondaries at several
    levels (max shared by two channels: the tie order; hue 0 minus a shift: the wrap)."""
    px = [(v, v, v) for v in range(256)]
    for lv in (255, 128, 20, 1):
        px += [(lv, 0, 0), (0, lv, 0), (0, 0, lv), (lv, lv, 0), (0, lv, lv), (lv, 0, lv)]
        px += [(lv, lv // 2, 0), (0, lv, lv // 2), (lv // 2, 0, lv), (lv, 0, lv // 2)]
    px.append((0, 0, 0))
    row = np.array(px, dtype=np.uint8)
    img = np.stack([row, row[::-1], np.roll(row, 7, axis=0)])                  # [3, N, 3]
    programs = [[("hsv", np.float32(6.0 * a / 255.0), float(a), 1.0)] for a in (20, -20)]
    programs += [[("hsv", 0.0, 0.0, np.float32(m))] for m in (0.95, 1.05)]
    programs += [[("hsv", np.float32(6.0 * -20 / 255.0), -20.0, 1.0), ("hsv", 0.0, 0.0, np.float32(1.05))]]
    imgs = np.stack([img] * len(programs))
    _check(imgs, programs, cuda_device)


@pytest.mark.parametrize("hw", _shapes()[2:], ids=SHAPE_IDS[2:])
@pytest.mark.parametrize("first", ["noise", "blur"])
def test_noise_and_blur_halo(cuda_device, first, hw):
    """NOISE then BLUR: the blur's halo pixels carry the noise of the pixel they are
    (a neighbouring tile's, or the reflected one's).  BLUR then NOISE: the noise runs
    in registers on the blurred tile."""
    imgs = _images(3, *hw)
    second = "blur" if first == "noise" else "noise"
    _check(imgs, [[_stage(first, b), _stage(second, b)] for b in range(3)], cuda_device)


@pytest.mark.parametrize("hw", [_shapes()[1], _shapes()[3]], ids=[SHAPE_IDS[1], SHAPE_IDS[3]])
def test_full_sampled_programs(cuda_device, hw):
    from hkp import _lib, augment
    dr = augment.DomainRandomization(seed=17)
    idx = list(range(16))
    plan = dr.plan(idx, epoch=2)
    kinds = [[p.stages[i].kind for i in range(p.nstages)] for p in plan.programs]
    assert all(len(k) >= 6 for k in kinds)
    firsts = {k[0] for k in kinds}
    assert len(firsts) >= 3                                                    # the order varies
    assert any(k.index(_lib.HKP_AUG_BLUR) > 0 for k in kinds if _lib.HKP_AUG_BLUR in k)
    imgs = _images(16, *hw)
    got = _run(imgs, plan, cuda_device)
    want = ref.apply_plan(imgs, plan)
    for b in range(16):
        assert np.array_equal(got[b], want[b]), (b, dr.sample(b, 2))
    # a sample's pixels do not depend on the batch it sits in
    sub = [11, 3, 7]
    again = _run(imgs[sub], dr.plan(sub, epoch=2), cuda_device)
    assert np.array_equal(again, got[sub])


def test_unaligned_batch_slice(cuda_device):
    """Rows that start at any address modulo 4 on either side: input and output
    views at odd byte offsets (the dword body / byte head and tail of every row)."""
    from hkp import augment, ops
    h, w = 5, 67
    imgs = _images(2, h, w)
    plan = augment.Plan.from_stages([[_stage("noise", 0), _stage("blur", 0), _stage("lut", 0)],
                                     [_stage("hsv", 1)]])
    want = ref.apply_plan(imgs, plan)
    n = imgs.size
    for off in (1, 2, 3):
        flat = torch.zeros(n + 8, dtype=torch.uint8, device=cuda_device)
        x = flat[off:off + n].view(2, h, w, 3)
        x.copy_(torch.from_numpy(np.array(imgs)))
        got = ops.augment_u8(x, plan)
        assert np.array_equal(got.cpu().numpy(), want), off
        assert int(flat[:off].sum()) == 0 and int(flat[off + n:].sum()) == 0


def _jpeg_folder(tmp_path, n, H, W):
    from PIL import Image
    os.makedirs(tmp_path / "images")
    os.makedirs(tmp_path / "labels")
    # smooth content (JPEG-friendly) with colour: a gradient plus seeded texture
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(n):
        tex = recipe.seeded_images_u8(1, H, W, 60 + i)[0] // 8
        rgb = np.stack([(xx * 3 + 20 * i) % 256, (yy * 5) % 256, (xx + yy + 40 * i) % 256], -1).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(np.clip(rgb.astype(np.int32) // 2 + 60 + tex, 0, 255).astype(np.uint8)).save(
            buf, format="JPEG", quality=85 + i, subsampling=2)
        (tmp_path / "images" / ("%05d.jpg" % i)).write_bytes(buf.getvalue())
        np.save(tmp_path / "labels" / ("%05d.npy" % i), np.array([[3.5 + i, 40.0], [-2.0, 7.25]]))


def test_device_batches_augment(cuda_device, tmp_path):
    from hkp import augment, ops
    from src.dataset import DeviceBatches, KeypointsDataset, transform
    K, H, W, n = 2, 48, 64, 5
    _jpeg_folder(tmp_path, n, H, W)
    ds = KeypointsDataset(str(tmp_path / "images"), str(tmp_path / "labels"), K, H, W, transform)
    plain_loader = DeviceBatches(ds, 2, shuffle=True, seed=5)
    plain = [[(i.clone(), u.clone()) for i, u in plain_loader] for _ in range(2)]      # epochs 0 and 1
    by_index = {}
    for decode in ("host", "device"):
        dr = augment.DomainRandomization(seed=9)
        loader = DeviceBatches(ds, 2, shuffle=True, seed=5, decode=decode, augment=dr)
        for epoch in range(2):
            order = np.random.default_rng(5 + epoch).permutation(n)
            got = list(loader)
            assert len(got) == len(plain[epoch]) == 3
            for bi, ((img, uv), (pimg, puv)) in enumerate(zip(got, plain[epoch])):
                idx = order[2 * bi:2 * bi + 2]
                plan = dr.plan(idx, epoch)
                assert torch.equal(img, ops.augment_u8(pimg, plan)) and torch.equal(uv, puv)
                assert np.array_equal(img.cpu().numpy(), ref.apply_plan(pimg.cpu().numpy(), plan))
                assert not torch.equal(img, pimg)
                for j, i in enumerate(idx):
                    by_index.setdefault((decode, epoch), {})[int(i)] = img[j].cpu()
    for decode in ("host", "device"):
        e0, e1 = by_index[(decode, 0)], by_index[(decode, 1)]
        assert sorted(e0) == sorted(e1) == list(range(n))
        assert all(not torch.equal(e0[i], e1[i]) for i in range(n))                    # two epochs differ
        assert all(torch.equal(e0[i], by_index[("host", 0)][i]) for i in range(n))
    # rebuilt with the same seed: the same pixels, also through decode workers and
    # another batch size; another seed: other pixels
    again = DeviceBatches(ds, 3, shuffle=True, seed=5, workers=2, augment=augment.DomainRandomization(seed=9))
    seen = {}
    order = np.random.default_rng(5).permutation(n)
    for bi, (img, uv) in enumerate(again):
        for j, i in enumerate(order[3 * bi:3 * bi + 3]):
            seen[int(i)] = img[j].cpu()
    assert all(torch.equal(seen[i], by_index[("host", 0)][i]) for i in range(n))
    other = next(iter(DeviceBatches(ds, 2, shuffle=True, seed=5, augment=augment.DomainRandomization(seed=10))))[0]
    assert not torch.equal(other[0].cpu(), by_index[("host", 0)][int(order[0])])
    # augment=None: today's batches
    for (a, ua), (b, ub) in zip(DeviceBatches(ds, 2, shuffle=True, seed=5, augment=None), plain[0]):
        assert torch.equal(a, b) and torch.equal(ua, ub)


def test_transform_call_kinds(cuda_device):
    from hkp import augment, ops
    from src.dataset import Compose, _to_tensor, domain_randomization
    imgs = _images(3, 37, 53)
    dr = augment.DomainRandomization(seed=4)
    want = ref.apply_plan(imgs, dr.plan([0, 1, 2], 0))
    # numpy HWC in, numpy out; images are numbered in call order
    a, b = dr(imgs[0]), dr(imgs[1])
    assert isinstance(a, np.ndarray) and a.dtype == np.uint8
    assert np.array_equal(a, want[0]) and np.array_equal(b, want[1])
    # device tensors: [H,W,3] and [B,H,W,3]
    dr2 = augment.DomainRandomization(seed=4)
    t = dr2(torch.from_numpy(imgs[0].copy()).to(cuda_device))
    assert t.is_cuda and t.shape == (37, 53, 3) and np.array_equal(t.cpu().numpy(), want[0])
    t = dr2(torch.from_numpy(imgs[1:].copy()).to(cuda_device))
    assert t.shape == (2, 37, 53, 3) and np.array_equal(t.cpu().numpy(), want[1:])
    # the drop-in for the reference's commented transform
    tf = Compose([augment.DomainRandomization(seed=4), _to_tensor])
    x = tf(imgs[0])
    dev = ops.augment_u8(torch.from_numpy(imgs[:1].copy()).to(cuda_device), dr.plan([0], 0))
    assert x.dtype == torch.float32 and x.shape == (3, 37, 53)
    assert torch.equal(x, ops.images_u8_to_nchw(dev)[0].cpu())
    assert torch.equal(domain_randomization(seed=4)(imgs[0]), x)


def test_one_training_step(cuda_device):
    from hkp import augment, ops, train
    from src.model import KeypointsGauss
    B, K, H, W = 2, 2, 64, 80
    u8 = torch.from_numpy(recipe.seeded_images_u8(B, H, W, 11)).to(cuda_device)
    uv = torch.from_numpy(recipe.seeded_keypoints(B, K, H, W, 13)).to(cuda_device)
    aug = ops.augment_u8(u8, augment.DomainRandomization(seed=2).plan(range(B), 0))
    assert aug.dtype == torch.uint8 and not torch.equal(aug, u8)
    losses = []
    for x in (u8, aug):
        m = KeypointsGauss(K, backbone="resnet18", pretrained=False)
        m.load_state_dict(recipe.seeded_state_dict("resnet18", 12))
        m = m.to(cuda_device)
        loss = train.Trainer(m).forward_backward(x, uv=uv)
        assert torch.isfinite(loss).all()
        for name, p in m.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
        losses.append(loss.item())
    assert losses[0] != losses[1]
