"""The antialiased resize on the GPU (csrc/resample.hip, hkp.resample): the kernel's
output against Pillow's Image.resize(..., reducing_gap=None) directly and against
the numpy restatement (tests/_resample_ref.py), bit for bit — array_equal only —
over the smallest shapes at which the kernel takes another path, and the plumbing
through DeviceBatches, KeypointsDataset and one training step."""
import ctypes
import functools
import io
import os

import numpy as np
import pytest
import torch

import _resample_ref as ref
from oracle import recipe

pytestmark = pytest.mark.gpu

TH, TW = 32, 64                  # RS_TH, RS_TW of csrc/resample.hip: one block's tile of one output image
FILTERS = ["box", "bilinear", "hamming", "bicubic", "lanczos"]
FILL = (7, 200, 31)


@functools.lru_cache(maxsize=None)
def _image(hs, ws, seed=1):
    a = ref.images(hs, ws, seed)
    a.setflags(write=False)
    return a


def _pillow(img, h, w, name, mode="stretch", fill=(0, 0, 0)):
    from PIL import Image
    x0, y0, wd, hd = ref.placement(img.shape[0], img.shape[1], h, w, mode)
    out = np.empty((h, w, 3), dtype=np.uint8)
    out[:] = np.asarray(fill, dtype=np.uint8)
    out[y0:y0 + hd, x0:x0 + wd] = np.asarray(Image.fromarray(np.asarray(img), "RGB").resize(
        (wd, hd), getattr(Image, name.upper()), reducing_gap=None))
    return out


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, "%s: %d bytes differ, first at (b, y, x, c) = %s: got %d, want %d" % (
        what, bad.shape[0], tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _check(imgs, h, w, name, dev, mode="stretch", fill=(0, 0, 0)):
    """One launch over `imgs` (any sizes); the result against Pillow and the restatement."""
    from hkp import ops, resample
    plan = resample.ResamplePlan([im.shape[:2] for im in imgs], (h, w), filter=name, mode=mode, fill=fill)
    flat = torch.from_numpy(np.concatenate([np.asarray(im).reshape(-1) for im in imgs])).to(dev)
    before = flat.clone()
    out = ops.resample_ragged_u8(flat, plan)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (len(imgs), h, w, 3)
    assert torch.equal(flat, before)                                          # the input is left alone
    got = out.cpu().numpy()
    _same(got, np.stack([_pillow(im, h, w, name, mode, fill) for im in imgs]), "Pillow")
    _same(got, np.stack([ref.resample(im, h, w, name, mode, fill) for im in imgs]), "restatement")
    return got


# (hs, ws, h, w)
SHAPES = {
    "w=TW+1,h=TH+1": (40, 150, TH + 1, TW + 1),               # partial tiles on both edges, byte stores
    "w=2TW-1": (70, 300, TH + 1, 2 * TW - 1),
    "w=2TW,dwords": (50, 100, TH + 1, 2 * TW),                # dword stores, two tiles across, partial tile down
    "w%4!=0": (31, 45, 17, 22),
    "1x1": (64, 64, 1, 1),
    "one row": (30, 200, 1, 68),                              # dword stores of a single row
    "up": (10, 12, 25, 31),
    "non-integer": (121, 163, 48, 64),
    "x unchanged": (33, 47, 60, 47),
    "y unchanged": (33, 47, 33, 20),
    "identity": (5, 5, 5, 5),
    "tall span": (300, 7, 5, 7),                              # one output row spans 60 (x support) source rows
    "wide span": (7, 300, 5, 7),                              # ksize over the LDS budget: kx from global memory
}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", FILTERS)
def test_against_pillow_and_restatement(cuda_device, name, shape):
    hs, ws, h, w = SHAPES[shape]
    _check([_image(hs, ws), _image(hs, ws, 2)], h, w, name, cuda_device)


def test_kx_staging_threshold(cuda_device):
    """The tile's kx rows sit in LDS while 64 columns x ksize words fit 32 KiB, i.e.
    ksize <= 128: bilinear at a reduction of 63 has ksize 127, at 64 it has 129."""
    from hkp import resample
    for ws, ks in ((252, 127), (256, 129)):
        assert int(resample.axis_table(ws, 4, "bilinear")[0]) == ks
        _check([_image(6, ws)], 6, 4, "bilinear", cuda_device)
        _check([_image(6, ws), _image(9, 40)], 6, 4, "bilinear", cuda_device)      # the batch's largest ksize decides


@pytest.mark.parametrize("name", ["bilinear", "lanczos"])
def test_unaligned_output_takes_the_byte_path(cuda_device, name):
    """w % 4 == 0 but the output pointer is offset by one byte: byte stores, same bytes."""
    from hkp import _lib, resample
    hs, ws, h, w = 50, 100, TH + 1, 2 * TW
    img = _image(hs, ws)
    plan = resample.ResamplePlan([(hs, ws)], (h, w), filter=name)
    x = torch.from_numpy(np.array(img)).to(cuda_device).reshape(-1)
    buf = torch.full((h * w * 3 + 8,), 0xAB, dtype=torch.uint8, device=cuda_device)
    recs, tables = plan.device_arrays(cuda_device)
    P = ctypes.c_void_p
    assert buf.data_ptr() % 4 == 0
    _lib.call("hkp_resample_u8", 1, P(x.data_ptr()), plan.in_bytes, plan.records, P(recs.data_ptr()),
              P(plan.tables.ctypes.data), P(tables.data_ptr()), plan.tables.size, h, w, P(buf.data_ptr() + 1),
              P(torch.cuda.current_stream().cuda_stream))
    got = buf.cpu().numpy()
    assert got[0] == 0xAB and np.all(got[1 + h * w * 3:] == 0xAB)             # nothing outside the output
    _same(got[1:1 + h * w * 3].reshape(1, h, w, 3), _pillow(img, h, w, name)[None], "Pillow")


@pytest.mark.parametrize("name", FILTERS)
def test_ragged_batch(cuda_device, name):
    """One launch, three images of three sizes; the one already at the output size
    comes back unchanged."""
    h, w = 48, 64
    imgs = [_image(121, 163), _image(h, w), _image(30, 200)]
    got = _check(imgs, h, w, name, cuda_device)
    assert np.array_equal(got[1], imgs[1])


@pytest.mark.parametrize("name", ["bilinear", "bicubic"])
def test_fit_mode(cuda_device, name):
    h, w = TH + 8, TW + 8                                                     # 40 x 72: rectangle edges inside tiles
    imgs = [_image(50, 400), _image(300, 70), _image(80, 144)]                # wider, taller, the output's own aspect
    got = _check(imgs, h, w, name, cuda_device, mode="fit", fill=FILL)
    assert np.all(got[0][0] == FILL) and np.all(got[0][-1] == FILL) and not np.all(got[0][h // 2] == FILL)
    assert np.all(got[1][:, 0] == FILL) and np.all(got[1][:, -1] == FILL) and not np.all(got[1][:, w // 2] == FILL)
    assert ref.placement(80, 144, h, w, "fit") == (0, 0, w, h)
    _check(imgs[:2], 41, 73, name, cuda_device, mode="fit", fill=FILL)        # byte stores


def test_resample_u8_wrapper(cuda_device):
    from hkp import ops
    src = np.stack([_image(40, 150), _image(40, 150, 2)])
    x = torch.from_numpy(src).to(cuda_device)
    got = ops.resample_u8(x, 20, 64, filter="hamming")
    _same(got.cpu().numpy(), np.stack([_pillow(im, 20, 64, "hamming") for im in src]), "Pillow")
    assert torch.equal(ops.resample_u8(x, 40, 150, filter="lanczos"), x)
    fit = ops.resample_u8(x, 32, 32, mode="fit", fill=FILL)
    _same(fit.cpu().numpy(), np.stack([_pillow(im, 32, 32, "bilinear", "fit", FILL) for im in src]), "Pillow")
    # resize_u8 stays the two-tap warp: it aliases where the antialiased resize does not
    assert not torch.equal(ops.resize_u8(x, 10, 30), ops.resample_u8(x, 10, 30))


def test_argument_checks_on_the_device(cuda_device):
    from hkp import ops, resample
    from hkp._lib import HKP_WARP_MAX_DIM, HkpError
    x = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=cuda_device)
    with pytest.raises(HkpError, match="torch.uint8"):
        ops.resample_u8(x.float(), 4, 4)
    with pytest.raises(HkpError, match="4 dims"):
        ops.resample_u8(x[0], 4, 4)
    with pytest.raises(HkpError, match=r"\[B,H,W,3\]"):
        ops.resample_u8(torch.zeros((2, 8, 8, 4), dtype=torch.uint8, device=cuda_device), 4, 4)
    with pytest.raises(HkpError, match="contiguous"):
        ops.resample_u8(x.permute(0, 2, 1, 3)[:, :, ::2], 4, 4)
    with pytest.raises(HkpError, match="unknown filter"):
        ops.resample_u8(x, 4, 4, filter="area")
    with pytest.raises(HkpError, match="unknown mode"):
        ops.resample_u8(x, 4, 4, mode="crop")
    with pytest.raises(HkpError, match="outside 1.."):
        ops.resample_u8(x, 4, HKP_WARP_MAX_DIM + 1)
    plan = resample.ResamplePlan([(8, 8), (8, 8)], (4, 4))
    with pytest.raises(HkpError, match="the buffer has"):
        ops.resample_ragged_u8(x.reshape(-1)[:-3], plan)
    with pytest.raises(HkpError, match="1 dims"):
        ops.resample_ragged_u8(x, plan)
    plan.records[1].wd = 5                                                     # the C side's check, from the wrapper
    with pytest.raises(HkpError, match="image 1: rectangle"):
        ops.resample_ragged_u8(x.reshape(-1), plan)
    assert int(x.sum()) == 0


# ------------------------------------------------------------- the data path ----
SIZES = [(48, 64), (48, 64), (96, 128), (96, 128), (60, 100), (60, 100)]         # per file; the network's: 48 x 64


def _mixed_folder(tmp_path, sizes):
    """JPEG files of different sizes with labels in each file's own pixel coordinates
    (one label outside the image: it has to be clipped after the resize)."""
    from PIL import Image
    os.makedirs(tmp_path / "images")
    os.makedirs(tmp_path / "labels")
    for i, (H, W) in enumerate(sizes):
        yy, xx = np.mgrid[0:H, 0:W]
        tex = recipe.seeded_images_u8(1, H, W, 60 + i)[0] // 8
        rgb = np.stack([(xx * 3 + 20 * i) % 256, (yy * 5) % 256, (xx + yy + 40 * i) % 256], -1).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(np.clip(rgb.astype(np.int32) // 2 + 60 + tex, 0, 255).astype(np.uint8)).save(
            buf, format="JPEG", quality=85 + i, subsampling=2)
        (tmp_path / "images" / ("%05d.jpg" % i)).write_bytes(buf.getvalue())
        np.save(tmp_path / "labels" / ("%05d.npy" % i), np.array([[0.6 * W + i, 0.8 * H], [-2.0, H + 5.0]]))


def _by_index(loader, bs):
    px, lab = {}, {}
    for bi, (img, uv) in enumerate(loader):
        assert img.dtype == torch.uint8 and uv.dtype == torch.float32
        for j in range(img.shape[0]):
            px[bs * bi + j], lab[bs * bi + j] = img[j].cpu(), uv[j].cpu()
    return px, lab


@pytest.mark.parametrize("rs_kw", [dict(filter="bilinear"), dict(filter="lanczos", mode="fit", fill=FILL)],
                         ids=["bilinear-stretch", "lanczos-fit"])
def test_device_batches_resize(cuda_device, tmp_path, rs_kw):
    from hkp import augment, geometry as G, ops, resample
    from src.dataset import DeviceBatches, KeypointsDataset, imread_bgr, transform
    K, H, W, n = 2, 48, 64, len(SIZES)
    _mixed_folder(tmp_path, SIZES)
    rs = resample.Resize(**rs_kw)
    ds = KeypointsDataset(str(tmp_path / "images"), str(tmp_path / "labels"), K, H, W, transform, resize=rs)
    stored = np.stack(ds.labels_np)
    assert stored[2, 0, 0] > W and stored[0, 1, 0] == -2.0                     # source coordinates, not clipped at load
    want_px, want_uv = [], []
    for i in range(n):
        dec = imread_bgr(ds.imgs[i])
        assert dec.shape[:2] == SIZES[i]
        want_px.append(_pillow(dec, H, W, rs.filter, rs.mode, rs.fill))        # Pillow's resize of the host decode
        want_uv.append(rs.plan([SIZES[i]], (H, W)).apply_uv(stored[i][None])[0])
        assert np.array_equal(want_uv[i], ref.apply_uv(stored[i], SIZES[i][0], SIZES[i][1], H, W, rs.mode))
    for kw in ({}, {"decode": "device"}):
        for bs in (1, 3, 2):                                                   # one size per batch; mixed; pairs of one size
            px, lab = _by_index(DeviceBatches(ds, bs, resize=rs, **kw), bs)
            assert sorted(px) == list(range(n))
            for i in range(n):
                _same(px[i].numpy(), want_px[i], "%s bs=%d image %d" % (kw, bs, i))
                assert np.array_equal(lab[i].numpy(), want_uv[i]), (kw, bs, i)
    # geometric and augment chained after it: they see the resampled batch and the mapped labels
    ga = G.GeometricAugmentation(seed=3, hflip=0.5, flip_pairs=[(0, 1)], fill=FILL)
    dr = augment.DomainRandomization(seed=9)
    first = None
    for kw in ({}, {"decode": "device"}):
        for bs in (1, 3):
            got = list(DeviceBatches(ds, bs, resize=rs, geometric=ga, augment=dr, **kw))
            px, lab = {}, {}
            for bi, (img, uv) in enumerate(got):
                idx = list(range(bs * bi, bs * bi + img.shape[0]))
                base = torch.from_numpy(np.stack([want_px[i] for i in idx])).to(cuda_device)
                uv0 = np.stack([want_uv[i] for i in idx])
                gplan = ga.plan(idx, 0, uvs=uv0, hw=(H, W))
                assert torch.equal(img, ops.augment_u8(ops.warp_affine_u8(base, gplan), dr.plan(idx, 0)))
                assert np.array_equal(uv.cpu().numpy(), gplan.apply_uv(uv0))
                for j, i in enumerate(idx):
                    px[i], lab[i] = img[j].cpu(), uv[j].cpu()
            if first is None:
                first = (px, lab)
            for i in range(n):                                                 # the same for any batch size and decode
                assert torch.equal(px[i], first[0][i]) and torch.equal(lab[i], first[1][i]), (kw, bs, i)


def test_device_batches_without_resize_unchanged(cuda_device, tmp_path):
    from test_gpu_augment import _jpeg_folder
    from src.dataset import DeviceBatches, KeypointsDataset, imread_bgr, transform
    K, H, W, n = 2, 48, 64, 3
    _jpeg_folder(tmp_path, n, H, W)
    ds = KeypointsDataset(str(tmp_path / "images"), str(tmp_path / "labels"), K, H, W, transform, resize=None)
    assert ds.labels_np[0][1, 0] == 0.0                                        # clipped at load, as before
    for kw in ({}, {"decode": "device"}):
        for (img, uv), i in zip(DeviceBatches(ds, 1, resize=None, **kw), range(n)):
            assert np.array_equal(img[0].cpu().numpy(), imread_bgr(ds.imgs[i]))
            assert np.array_equal(uv[0].cpu().numpy(), ds.labels_np[i])


def test_keypoints_dataset_resize(cuda_device, tmp_path):
    from hkp import geometry as G, resample
    from src.dataset import KeypointsDataset, imread_bgr, transform
    K, H, W = 2, 48, 64
    sizes = SIZES[1:4] + SIZES[4:5]
    _mixed_folder(tmp_path, sizes)
    rs = resample.Resize(filter="bicubic", mode="fit", fill=FILL)
    args = (str(tmp_path / "images"), str(tmp_path / "labels"), K, H, W, transform)
    ds_uv = KeypointsDataset(*args, return_uv=True, resize=rs)
    ds_g = KeypointsDataset(*args, resize=rs)
    ga = G.GeometricAugmentation(seed=4, hflip=0.5, flip_pairs=[(0, 1)])
    ds_both = KeypointsDataset(*args, return_uv=True, resize=rs, geometric=ga)
    for i, (hs, ws) in enumerate(sizes):
        dec = imread_bgr(ds_uv.imgs[i])
        want_img = _pillow(dec, H, W, "bicubic", "fit", FILL)
        want_uv = ref.apply_uv(ds_uv.labels_np[i], hs, ws, H, W, "fit")
        img, uv = ds_uv[i]
        assert uv.is_cuda and uv.dtype == torch.float32 and np.array_equal(uv.cpu().numpy(), want_uv)
        assert torch.equal(img, transform(want_img))
        raw_img, raw_uv = ds_uv.raw(i)
        assert np.array_equal(raw_img, want_img) and np.array_equal(raw_uv.cpu().numpy(), want_uv)
        img_g, gauss = ds_g[i]
        assert torch.equal(img_g, img) and tuple(gauss.shape) == (K, H, W)
        v, u = np.unravel_index(int(gauss[0].argmax()), (H, W))                # the target's peak: the mapped label
        assert abs(u - want_uv[0, 0]) <= 0.5 and abs(v - want_uv[0, 1]) <= 0.5
        # with geometric: the warp of the resampled image, labels through both maps
        gplan = ga.plan([i], 0, uvs=want_uv[None], hw=(H, W))
        both_img, both_uv = ds_both.raw(i)
        assert both_img.shape == (H, W, 3) and np.array_equal(both_uv.cpu().numpy(), gplan.apply_uv(want_uv[None])[0])


def test_one_training_step(cuda_device):
    from hkp import ops, resample, train
    from src.model import KeypointsGauss
    B, K, H, W = 2, 2, 64, 96
    u8 = torch.from_numpy(recipe.seeded_images_u8(B, 2 * H + 9, 2 * W + 5, 11)).to(cuda_device)
    uv = recipe.seeded_keypoints(B, K, 2 * H + 9, 2 * W + 5, 13)
    plan = resample.Resize("hamming").plan([tuple(u8.shape[1:3])] * B, (H, W))
    x = ops.resample_ragged_u8(u8.reshape(-1), plan)
    assert x.dtype == torch.uint8 and tuple(x.shape) == (B, H, W, 3)
    m = KeypointsGauss(K, backbone="resnet18", pretrained=False)
    m.load_state_dict(recipe.seeded_state_dict("resnet18", 12))
    m = m.to(cuda_device)
    loss = train.Trainer(m).step(x, uv=torch.from_numpy(plan.apply_uv(uv)).to(cuda_device))
    assert torch.isfinite(loss).all()


def test_analysis_maps_predictions_back(tmp_path, monkeypatch, cuda_device):
    """analysis.main with RESIZE set: an image of another size is resampled on the
    device, and its keypoints.npy row is the prediction on the resampled frame
    mapped back into the source image's pixels; an image of the model's size is
    untouched."""
    import analysis as analysis_mod
    from PIL import Image
    from hkp import resample
    from src.dataset import transform
    from src.model import KeypointsGauss
    BB, K, H, W = "resnet34", 4, 64, 96
    for name, v in (("IMG_HEIGHT", H), ("IMG_WIDTH", W), ("RESIZE", "hamming"), ("RESIZE_PARAMS", {"mode": "fit"})):
        monkeypatch.setattr(analysis_mod, name, v)
    assert (analysis_mod.BACKBONE, analysis_mod.NUM_KEYPOINTS) == (BB, K)
    sd = recipe.seeded_state_dict(BB, 91)
    (tmp_path / "ck").mkdir()
    torch.save(sd, tmp_path / "ck" / "m.pth")
    (tmp_path / "imgs").mkdir()
    srcs = [recipe.seeded_images_u8(1, H, W, 92)[0], recipe.seeded_images_u8(1, 150, 330, 93)[0]]
    for i, bgr in enumerate(srcs):
        Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(tmp_path / "imgs" / ("f%d.png" % i))
    kp = analysis_mod.main("m.pth", str(tmp_path / "imgs"), out_dir=str(tmp_path / "preds"),
                           checkpoint_dir=str(tmp_path / "ck"))
    assert kp.shape == (2, K, 2) and kp.dtype == np.int32
    m = KeypointsGauss(K, H, W, backbone=BB, pretrained=False)
    m.load_state_dict(sd)
    m = m.to(cuda_device)
    plan = resample.Resize("hamming", mode="fit").plan([(150, 330)], (H, W))
    frames = [srcs[0], _pillow(srcs[1], H, W, "hamming", "fit")]
    for i, frame in enumerate(frames):
        with torch.no_grad():                  # batch 1 per image, train-mode BN, as analysis.main runs it
            _, yx = m.heatmaps_and_keypoints(transform(frame).to(cuda_device)[None])
        yx = yx.cpu().numpy()
        if i == 1:
            uv = plan.invert_uv(yx[..., ::-1].astype(np.float32))
            yx = np.rint(uv[..., ::-1]).astype(np.int32)
        assert np.array_equal(kp[i:i + 1], yx), i
        assert (tmp_path / "preds" / ("out%04d.png" % i)).exists()
    assert np.array_equal(np.load(tmp_path / "preds" / "keypoints.npy"), kp)
