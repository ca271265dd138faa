"""The affine warp on the GPU (csrc/warp.hip, hkp.geometry): the kernel against the
numpy restatement (tests/_warp_ref.py) and against exact identities, bit for bit —
array_equal only, there is no tolerance in this file except the one-pixel support
of a bilinear tap in the labels-follow-pixels test — and the plumbing through
GeometricAugmentation, DeviceBatches, KeypointsDataset and one training step.

Sign convention, fixed once here: a positive rotate_deg turns the picture
counter-clockwise on the screen, so +90 on a square equals torch.rot90(img, 1,
dims=(rows, columns))."""
import functools

import numpy as np
import pytest
import torch

import _warp_ref as ref
from oracle import recipe

pytestmark = pytest.mark.gpu

FILL = (7, 200, 31)
INTERPS = ["bilinear", "nearest"]
BORDERS = ["constant", "replicate", "reflect101"]


@functools.lru_cache(maxsize=None)
def _images(b, h, w, seed=23):
    a = recipe.seeded_images_u8(b, h, w, seed)
    a.setflags(write=False)
    return a


def _compose(A, B):
    """Forward matrix of `B first, then A` (both 2x3)."""
    full = np.vstack([A, [0, 0, 1]]) @ np.vstack([B, [0, 0, 1]])
    return full[:2]


def _three(hs, ws, h, w):
    """Three different transforms source hs x ws -> output h x w: a rotation with
    scale, a shear with a non-integer translation that makes source coordinates
    negative, and a flip."""
    from hkp import geometry as G
    base = G.resize_matrix(hs, ws, h, w) if (hs, ws) != (h, w) else G.affine_matrix(h, w)
    return [_compose(G.affine_matrix(h, w, rotate_deg=23, scale=1.15), base),
            _compose(G.affine_matrix(h, w, shear_deg=12, translate_xy_px=(3.37, 2.61)), base),
            _compose(G.affine_matrix(h, w, hflip=True), base)]


def _check(src, mats, hw, interp, border, dev, fill=FILL):
    """Run the kernel; compare with the restatement fed the records' own numbers."""
    from hkp import geometry as G, ops
    h, w = hw
    plan = G.WarpPlan(mats, hw, fill=fill, interp=interp, border=border)
    coef = np.array([[int(x.m[i]) for i in range(6)] for x in plan.xforms], dtype=np.int64)
    x = torch.from_numpy(np.array(src)).to(dev)
    out = ops.warp_affine_u8(x, plan, out_hw=hw)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (len(src), h, w, 3)
    assert torch.equal(x.cpu(), torch.from_numpy(np.array(src)))              # the input is left alone
    got = out.cpu().numpy()
    want = ref.warp_batch(src, coef, h, w, INTERPS.index(interp), BORDERS.index(border), [fill] * len(src))
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, "%d bytes differ, first at (b, y, x, c) = %s: got %d, want %d" % (
        bad.shape[0], tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    return got


# (source, output): one full tile; partial tiles on both edges, byte stores; smaller
# than a tile; dword stores with partial tiles; one pixel; source != output, twice
SIZES = [((16, 64), (16, 64)), ((17, 65), (17, 65)), ((5, 7), (5, 7)), ((33, 132), (33, 132)), ((3, 4), (1, 1)),
         ((23, 37), (16, 64)), ((32, 96), (9, 13))]
SIZE_IDS = ["16x64", "17x65", "5x7", "33x132", "1x1", "23x37to16x64", "32x96to9x13"]


@pytest.mark.parametrize("sizes", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("interp", INTERPS)
def test_against_restatement(cuda_device, interp, border, sizes):
    (hs, ws), (h, w) = sizes
    got = _check(_images(3, hs, ws), _three(hs, ws, h, w), (h, w), interp, border, cuda_device)
    if border == "constant" and h * w > 1:
        assert np.any(np.all(got == FILL, axis=-1))                           # the fill is in the picture


@pytest.mark.parametrize("interp", INTERPS)
def test_reflect101_smallest_source(cuda_device, interp):
    _check(_images(3, 2, 2), _three(2, 2, 5, 7), (5, 7), interp, "reflect101", cuda_device)


def _warp(x, mats, hw, dev, **kw):
    from hkp import geometry as G, ops
    return ops.warp_affine_u8(x, G.WarpPlan(mats, hw, **kw))


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("interp", INTERPS)
def test_exact_identities(cuda_device, interp, border):
    """Independent of the restatement: flips, integer shifts and quarter turns move
    whole pixels (fx = fy = 0 returns p00 exactly)."""
    from hkp import geometry as G
    kw = dict(interp=interp, border=border, fill=FILL)
    for h, w in ((17, 65), (16, 64)):
        x = torch.from_numpy(np.array(_images(2, h, w))).to(cuda_device)
        two = lambda **a: [G.affine_matrix(h, w, **a)] * 2                       # noqa: E731
        assert torch.equal(_warp(x, two(), (h, w), cuda_device, **kw), x)
        hf = _warp(x, two(hflip=True), (h, w), cuda_device, **kw)
        assert torch.equal(hf, torch.flip(x, [2]))
        assert torch.equal(_warp(x, two(vflip=True), (h, w), cuda_device, **kw), torch.flip(x, [1]))
        assert torch.equal(_warp(hf, two(hflip=True), (h, w), cuda_device, **kw), x)      # twice: the input
        assert torch.equal(_warp(x, two(hflip=True, vflip=True), (h, w), cuda_device, **kw), torch.flip(x, [1, 2]))
    sq = torch.from_numpy(np.array(_images(2, 24, 24))).to(cuda_device)
    for deg, k in ((90, 1), (-90, -1), (180, 2)):
        got = _warp(sq, [G.affine_matrix(24, 24, rotate_deg=deg)] * 2, (24, 24), cuda_device, **kw)
        assert torch.equal(got, torch.rot90(sq, k, dims=(1, 2))), deg


def test_integer_translation_constant_fill(cuda_device):
    from hkp import geometry as G
    h, w = 17, 65
    x = torch.from_numpy(np.array(_images(2, h, w))).to(cuda_device)
    for interp in INTERPS:
        got = _warp(x, [G.affine_matrix(h, w, translate_xy_px=(5, -3))] * 2, (h, w), cuda_device, interp=interp,
                    fill=FILL)
        want = torch.empty_like(x)
        want[:] = torch.tensor(FILL, dtype=torch.uint8, device=cuda_device)
        want[:, :h - 3, 5:] = x[:, 3:, :w - 5]                                # dest (x, y) = source (x - 5, y + 3)
        assert torch.equal(got, want), interp


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("interp", INTERPS)
def test_source_entirely_outside(cuda_device, interp, border):
    """Ordinary input whose source coordinates all fall far outside the image: all
    fill in constant mode, the restatement's border pixels in the other two."""
    from hkp import geometry as G
    h, w = 24, 40
    far = np.array([8.0 * w, 8.0 * h])
    shrink = np.array([[1 / 64, 0, far[0] * (1 - 1 / 64)], [0, 1 / 64, far[1] * (1 - 1 / 64)]])
    mats = [G.affine_matrix(h, w, translate_xy_px=(10 * w, 0)), shrink,
            G.affine_matrix(h, w, translate_xy_px=(-10 * w, -10 * h))]
    got = _check(_images(3, h, w), mats, (h, w), interp, border, cuda_device)
    if border == "constant":
        assert np.all(got == FILL)
    else:
        assert not np.all(got == FILL)


def test_batch_dimension(cuda_device):
    from hkp import geometry as G
    n, h, w = 70, 5, 7
    rng = np.random.default_rng(8)
    mats = [G.affine_matrix(h, w, rng.uniform(-180, 180), rng.uniform(0.6, 1.6), rng.uniform(-2, 2, 2),
                            rng.uniform(-15, 15), rng.random() < 0.5, rng.random() < 0.5) for _ in range(n)]
    got = _check(_images(n, h, w), mats, (h, w), "bilinear", "constant", cuda_device)
    assert len({got[b].tobytes() for b in range(n)}) == n                     # one transform per image
    _check(_images(n, h, w), mats, (h, w), "nearest", "reflect101", cuda_device)


@pytest.mark.parametrize("interp", INTERPS)
def test_resize_u8(cuda_device, interp):
    from hkp import geometry as G, ops
    src = _images(2, 12, 20)
    x = torch.from_numpy(np.array(src)).to(cuda_device)
    for h, w in ((24, 40), (6, 10)):
        got = ops.resize_u8(x, h, w, interp=interp)
        # the half-pixel-centre map in Q16, written out: src = (dst + 0.5) * 12 / h - 0.5
        s = 12 * 65536 // h
        coef = [s, 0, (s - 65536) // 2, 0, s, (s - 65536) // 2]
        want = ref.warp_batch(src, [coef] * 2, h, w, INTERPS.index(interp), ref.REPLICATE)
        assert tuple(got.shape) == (2, h, w, 3) and np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(ops.resize_u8(x, 12, 20, interp=interp), x)
    if interp == "nearest":                                                   # 2x nearest repeats pixels
        up = ops.resize_u8(x, 24, 40, interp="nearest")
        assert torch.equal(up, x.repeat_interleave(2, 1).repeat_interleave(2, 2))


def test_argument_checks_on_the_device(cuda_device):
    from hkp import geometry as G, ops
    from hkp._lib import HKP_WARP_MAX_DIM, HkpError
    x = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=cuda_device)
    plan = G.WarpPlan([G.affine_matrix(8, 8)] * 2, (8, 8))
    with pytest.raises(HkpError, match="torch.uint8"):
        ops.warp_affine_u8(x.float(), plan)
    with pytest.raises(HkpError, match="4 dims"):
        ops.warp_affine_u8(x[0], plan)
    with pytest.raises(HkpError, match=r"\[B,H,W,3\]"):
        ops.warp_affine_u8(torch.zeros((2, 8, 8, 4), dtype=torch.uint8, device=cuda_device), plan)
    with pytest.raises(HkpError, match="contiguous"):
        ops.warp_affine_u8(x.permute(0, 2, 1, 3)[:, :, ::2], plan)
    with pytest.raises(HkpError, match="2 transforms for a batch of 1"):
        ops.warp_affine_u8(x[:1], plan)
    for bad in ((0, 8), (8, HKP_WARP_MAX_DIM + 1)):
        with pytest.raises(HkpError, match="out_hw"):
            ops.warp_affine_u8(x, plan, out_hw=bad)
    with pytest.raises(HkpError, match="reflect101"):
        ops.warp_affine_u8(x[:, :1].contiguous(), G.WarpPlan([G.affine_matrix(8, 8)] * 2, (8, 8), border="reflect101"))
    with pytest.raises(HkpError, match="torch.uint8"):
        ops.resize_u8(x.float(), 4, 4)
    with pytest.raises(HkpError, match=r"\[B,H,W,3\]"):
        ops.resize_u8(torch.zeros((2, 8, 8, 1), dtype=torch.uint8, device=cuda_device), 4, 4)
    with pytest.raises(HkpError, match="outside"):
        ops.resize_u8(x, 4, HKP_WARP_MAX_DIM + 1)
    with pytest.raises(HkpError, match="overlap"):                            # out must not alias in
        from hkp import _lib
        import ctypes
        P = ctypes.c_void_p
        _lib.call("hkp_warp_affine_u8", 2, 8, 8, P(x.data_ptr()), 8, 8, P(x.data_ptr() + 64), plan.xforms,
                  P(plan.device_array(cuda_device).data_ptr()), 0, 0, None)
    assert int(x.sum()) == 0


def test_labels_follow_pixels(cuda_device):
    """One lit pixel at an integer label: after rotate 20, scale 1.1 and hflip
    (bilinear) the brightest output pixel lies within 1 px (Chebyshev) of the
    transformed label — one pixel is the support of a bilinear tap."""
    from hkp import geometry as G, ops
    h, w = 48, 64
    label = np.array([[[40.0, 20.0]]], dtype=np.float32)                       # (u, v)
    img = np.zeros((1, h, w, 3), dtype=np.uint8)
    img[0, 20, 40] = 255
    M = G.affine_matrix(h, w, rotate_deg=20, scale=1.1, hflip=True)
    plan = G.WarpPlan([M], (h, w), flipped=[True])
    out = ops.warp_affine_u8(torch.from_numpy(img).to(cuda_device), plan).cpu().numpy()
    s = out[0].astype(np.int64).sum(-1)
    assert s.max() > 0
    v, u = np.unravel_index(np.argmax(s), s.shape)
    want = plan.apply_uv(label)[0, 0]
    assert max(abs(u - want[0]), abs(v - want[1])) <= 1.0, ((u, v), want)
    assert abs(want[0] - 40.0) > 5                                             # it moved
    # the same through the sampler's call surface, image and labels together
    ga = G.GeometricAugmentation(rotate=(20, 20), scale=(1.1, 1.1), translate=(0, 0), hflip=1.0)
    out2, uv2 = ga(img[0], label[0])
    assert isinstance(out2, np.ndarray) and np.array_equal(out2, out[0])
    assert uv2.dtype == np.float32 and np.array_equal(uv2, plan.apply_uv(label)[0])
    t_img, t_uv = ga(torch.from_numpy(img).to(cuda_device), torch.from_numpy(label), index=[0], epoch=0)
    assert t_img.is_cuda and np.array_equal(t_img.cpu().numpy(), out) and np.array_equal(t_uv.numpy(), uv2[None])
    only = ga(img[0], index=0)                                                 # without labels: the image alone
    assert isinstance(only, np.ndarray) and np.array_equal(only, out[0])


def _by_index(loader, order, bs):
    px, lab = {}, {}
    for bi, (img, uv) in enumerate(loader):
        for j, i in enumerate(order[bs * bi:bs * bi + bs]):
            px[int(i)], lab[int(i)] = img[j].cpu(), uv[j].cpu()
    return px, lab


def test_device_batches_geometric(cuda_device, tmp_path):
    from test_gpu_augment import _jpeg_folder
    from hkp import augment, geometry as G, ops
    from src.dataset import DeviceBatches, KeypointsDataset, transform
    K, H, W, n = 2, 48, 64, 6
    _jpeg_folder(tmp_path, n, H, W)
    ds = KeypointsDataset(str(tmp_path / "images"), str(tmp_path / "labels"), K, H, W, transform)
    stored = np.stack(ds.labels_np)
    make = lambda: G.GeometricAugmentation(seed=3, hflip=0.5, flip_pairs=[(0, 1)], fill=FILL)   # noqa: E731
    plain = list(DeviceBatches(ds, 2, shuffle=True, seed=5))
    order = np.random.default_rng(5).permutation(n)
    ga = make()
    got = list(DeviceBatches(ds, 2, shuffle=True, seed=5, geometric=ga))
    assert len(got) == len(plain) == 3
    for bi, ((img, uv), (pimg, puv)) in enumerate(zip(got, plain)):
        idx = order[2 * bi:2 * bi + 2]
        assert np.array_equal(puv.cpu().numpy(), stored[idx])
        plan = ga.plan(idx, 0, uvs=stored[idx], hw=(H, W))
        assert torch.equal(img, ops.warp_affine_u8(pimg, plan))
        coef = [[int(x.m[i]) for i in range(6)] for x in plan.xforms]
        assert np.array_equal(img.cpu().numpy(), ref.warp_batch(pimg.cpu().numpy(), coef, H, W, fills=[FILL] * 2))
        assert np.array_equal(uv.cpu().numpy(), plan.apply_uv(stored[idx]))   # labels through the same transform
        assert uv.dtype == torch.float32 and not torch.equal(img, pimg)
    ref_px, ref_lab = _by_index(got, order, 2)
    assert any(not np.array_equal(ref_lab[i].numpy(), stored[i]) for i in range(n))
    # the same pixels and labels per dataset index: another batch size, the device decode
    # (decode workers only hand over host batches; the plan is made in this process)
    for bs, kw in ((3, {}), (2, {"decode": "device"}), (3, {"decode": "device"})):
        px, lab = _by_index(DeviceBatches(ds, bs, shuffle=True, seed=5, geometric=make(), **kw), order, bs)
        assert sorted(px) == list(range(n))
        for i in range(n):
            assert torch.equal(px[i], ref_px[i]) and torch.equal(lab[i], ref_lab[i]), (bs, kw, i)
    # the second epoch draws again
    loader = DeviceBatches(ds, 2, shuffle=False, geometric=make())
    e0, l0 = _by_index(loader, np.arange(n), 2)
    e1, l1 = _by_index(loader, np.arange(n), 2)
    assert all(not torch.equal(e0[i], e1[i]) for i in range(n))
    # geometric=None: today's batches, bit for bit
    for (a, ua), (b, ub) in zip(DeviceBatches(ds, 2, shuffle=True, seed=5, geometric=None), plain):
        assert torch.equal(a, b) and torch.equal(ua, ub)
    # with augment: the warp first, then the domain randomisation, labels from the warp
    dr = augment.DomainRandomization(seed=9)
    both = list(DeviceBatches(ds, 2, shuffle=True, seed=5, geometric=make(), augment=dr))
    for bi, ((img, uv), (pimg, puv)) in enumerate(zip(both, plain)):
        idx = order[2 * bi:2 * bi + 2]
        plan = ga.plan(idx, 0, uvs=stored[idx], hw=(H, W))
        assert torch.equal(img, ops.augment_u8(ops.warp_affine_u8(pimg, plan), dr.plan(idx, 0)))
        assert torch.equal(uv, got[bi][1])


def test_keypoints_dataset_geometric(cuda_device, tmp_path):
    from test_gpu_augment import _jpeg_folder
    from hkp import geometry as G
    from src.dataset import KeypointsDataset, imread_bgr, transform
    K, H, W, n = 2, 48, 64, 3
    _jpeg_folder(tmp_path, n, H, W)
    ga = G.GeometricAugmentation(seed=4, hflip=0.5, flip_pairs=[(0, 1)])
    args = (str(tmp_path / "images"), str(tmp_path / "labels"), K, H, W, transform)
    ds_uv = KeypointsDataset(*args, return_uv=True, geometric=ga)
    ds_g = KeypointsDataset(*args, geometric=ga)
    plain = KeypointsDataset(*args, return_uv=True)
    moved = 0
    for i in range(n):
        plan = ga.plan([i], 0, uvs=plain.labels_np[i][None], hw=(H, W))
        want_uv = plan.apply_uv(plain.labels_np[i][None])[0]
        img, uv = ds_uv[i]
        assert uv.is_cuda and uv.dtype == torch.float32 and np.array_equal(uv.cpu().numpy(), want_uv)
        coef = [[int(x.m[j]) for j in range(6)] for x in plan.xforms]
        want_img = ref.warp(imread_bgr(ds_uv.imgs[i]), coef[0], H, W)
        assert torch.equal(img, transform(want_img))
        raw_img, raw_uv = ds_uv.raw(i)
        assert np.array_equal(raw_img, want_img) and np.array_equal(raw_uv.cpu().numpy(), want_uv)
        img_g, gauss = ds_g[i]
        assert torch.equal(img_g, img) and tuple(gauss.shape) == (K, H, W)
        for k in range(K):                                 # the target's peak: the pixel nearest to the moved label
            v, u = np.unravel_index(int(gauss[k].argmax()), (H, W))
            assert abs(u - want_uv[k, 0]) <= 0.5 and abs(v - want_uv[k, 1]) <= 0.5
        moved += not np.array_equal(want_uv, plain.labels_np[i])
        assert torch.equal(plain[i][1].cpu(), torch.from_numpy(plain.labels_np[i]))    # geometric=None: as stored
    assert moved > 0
    before = [ds_uv[i][1].cpu() for i in range(n)]
    ds_uv.set_epoch(1)
    after = [ds_uv[i][1].cpu() for i in range(n)]
    assert any(not torch.equal(a, b) for a, b in zip(before, after))
    assert all(np.array_equal(after[i].numpy(), ga.plan([i], 1, uvs=plain.labels_np[i][None], hw=(H, W)).apply_uv(
        plain.labels_np[i][None])[0]) for i in range(n))


def test_one_training_step(cuda_device):
    from hkp import geometry as G, ops, train
    from src.model import KeypointsGauss
    B, K, H, W = 2, 2, 64, 96
    u8 = torch.from_numpy(recipe.seeded_images_u8(B, H, W, 11)).to(cuda_device)
    uv = recipe.seeded_keypoints(B, K, H, W, 13)
    # (keep_inside off: the seeded keypoints sit near the edges; labels that leave the image are clipped)
    plan = G.GeometricAugmentation(seed=2, hflip=0.5, keep_inside=False).plan(range(B), 0, uvs=uv, hw=(H, W))
    x = ops.warp_affine_u8(u8, plan)
    assert x.dtype == torch.uint8 and x.shape == u8.shape and not torch.equal(x, u8)
    m = KeypointsGauss(K, backbone="resnet18", pretrained=False)
    m.load_state_dict(recipe.seeded_state_dict("resnet18", 12))
    m = m.to(cuda_device)
    loss = train.Trainer(m).step(x, uv=torch.from_numpy(plan.apply_uv(uv)).to(cuda_device))
    assert torch.isfinite(loss).all()
