"""The antialiased resize without a GPU: the numpy restatement (tests/_resample_ref.py)
against Pillow bit for bit, hkp.resample's axis tables against the restatement's,
the label maps, hkp_resample_u8's validation of its host copies (nothing is
launched), and the ragged collate of the data path."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _resample_ref as ref

PIL_FILTERS = {"box": "BOX", "bilinear": "BILINEAR", "hamming": "HAMMING", "bicubic": "BICUBIC", "lanczos": "LANCZOS"}
# (hs, ws, h, w): down, down by 10, x only, y only, up, a 7x300 source, 1x9, to 1x1, non-integer, identity, and
# (beyond the issue's ten) a 300x7 source, whose one-row span is far longer than a kernel tile
CASES = [(97, 131, 30, 40), (480, 640, 48, 64), (33, 47, 33, 20), (33, 47, 60, 47), (10, 12, 25, 31), (7, 300, 5, 7),
         (1, 9, 3, 2), (64, 64, 1, 1), (121, 163, 48, 64), (5, 5, 5, 5), (300, 7, 5, 7)]


@functools.lru_cache(maxsize=None)
def _image(hs, ws):
    a = ref.images(hs, ws, 1)
    a.setflags(write=False)
    return a


def pillow_resize(img, h, w, name):
    from PIL import Image
    return np.asarray(Image.fromarray(np.asarray(img), "RGB").resize((w, h), getattr(Image, PIL_FILTERS[name]),
                                                                     reducing_gap=None))


@pytest.mark.parametrize("case", CASES, ids=["%dx%dto%dx%d" % c for c in CASES])
@pytest.mark.parametrize("name", list(PIL_FILTERS))
def test_restatement_equals_pillow(name, case):
    hs, ws, h, w = case
    img = _image(hs, ws)
    got = ref.resize(img, h, w, name)
    want = pillow_resize(img, h, w, name)
    assert got.shape == want.shape == (h, w, 3)
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, "%d bytes differ, first at %s" % (bad.shape[0], tuple(bad[0]))


@pytest.mark.parametrize("name", list(PIL_FILTERS))
def test_tables_equal_the_restatement(name):
    from hkp import resample
    assert set(resample.FILTERS) == set(ref.FILTERS) == set(PIL_FILTERS)
    pairs = {(c[1], c[3]) for c in CASES} | {(c[0], c[2]) for c in CASES} | {(1280, 640), (1080, 480), (640, 1)}
    for n_in, n_out in sorted(pairs):
        words = resample.axis_table(n_in, n_out, name)
        assert words.dtype == np.int32 and not words.flags.writeable
        ksize, bounds, kk = resample.table_parts(words)
        rk, rb, rkk = ref.axis_table(n_in, n_out, name)
        assert words.size == 2 + 2 * n_out + n_out * ksize and int(words[1]) == n_out
        assert ksize == rk and np.array_equal(bounds, rb) and np.array_equal(kk, rkk), (n_in, n_out)
        assert np.all(bounds[:, 0] >= 0) and np.all(bounds[:, 1] <= ksize) and np.all(bounds.sum(1) <= n_in)
    assert resample.axis_table(47, 20, name) is resample.axis_table(47, 20, name)       # cached


def test_identity_table_returns_the_source():
    from hkp import resample
    img = _image(33, 47)
    for n in (33, 47):
        ksize, bounds, kk = resample.table_parts(resample.identity_table(n))
        rk, rb, rkk = ref.identity_table(n)
        assert ksize == rk == 1 and np.array_equal(bounds, rb) and np.array_equal(kk, rkk)
    tab = tuple(np.asarray(p, dtype=np.int64) if i else p for i, p in
                enumerate(resample.table_parts(resample.identity_table(47))))
    assert np.array_equal(ref._pass(img, tab, 1), img)
    tab = tuple(np.asarray(p, dtype=np.int64) if i else p for i, p in
                enumerate(resample.table_parts(resample.identity_table(33))))
    assert np.array_equal(ref._pass(img, tab, 0), img)
    # a plan gives an axis that keeps its size the identity table
    plan = resample.ResamplePlan([(33, 47)], (60, 47), filter="lanczos")
    ksize, bounds, kk = resample.table_parts(plan.tables[plan.records[0].xtab:])
    assert ksize == 1 and np.all(bounds[:, 1] == 1) and np.all(kk == 1 << 22)


@pytest.mark.parametrize("name", list(PIL_FILTERS))
def test_int32_accumulators_suffice(name):
    """sum |k| * 255 + 2^21 < 2^31 for every output index: no partial sum of a pass
    can leave int32, whatever the pixels."""
    from hkp import resample
    for n_out, n_in in ((64, 64), (64, 160), (40, 280), (16, 960)):         # reductions 1, 2.5, 7, 60
        _, _, kk = resample.table_parts(resample.axis_table(n_in, n_out, name))
        worst = int(np.abs(kk.astype(np.int64)).sum(1).max())
        assert worst * 255 + (1 << 21) < 1 << 31, (n_in, n_out, worst)
    _, _, kk = resample.table_parts(resample.axis_table(64, 64 * 3, name))   # and upsampling
    assert int(np.abs(kk.astype(np.int64)).sum(1).max()) * 255 + (1 << 21) < 1 << 31


def test_fit_geometry_and_label_maps():
    from hkp import resample
    h, w = 48, 64
    # wider than the output's aspect: full width, bars above and below; taller: bars left and right
    assert resample.placement(100, 400, h, w, "fit") == (0, 16, 64, 16) == ref.placement(100, 400, h, w, "fit")
    assert resample.placement(300, 100, h, w, "fit") == (24, 0, 16, 48) == ref.placement(300, 100, h, w, "fit")
    assert resample.placement(300, 100, h, w, "stretch") == (0, 0, 64, 48)
    assert resample.placement(10000, 3, h, w, "fit")[2] == 1                   # never narrower than a pixel
    sizes = [(100, 400), (300, 100), (48, 64), (200, 330)]
    rng = np.random.default_rng(3)
    for mode in ("stretch", "fit"):
        plan = resample.ResamplePlan(sizes, (h, w), mode=mode)
        assert [tuple(r) for r in plan.rects] == [ref.placement(a, b, h, w, mode) for a, b in sizes]
        uv = np.stack([np.stack([rng.uniform(0, b - 1, 5), rng.uniform(0, a - 1, 5)], -1) for a, b in sizes])
        uv = uv.astype(np.float32)
        fwd = plan.apply_uv(uv)
        assert fwd.dtype == np.float32 and fwd.shape == uv.shape
        for b, (hs, ws) in enumerate(sizes):
            assert np.array_equal(fwd[b], ref.apply_uv(uv[b], hs, ws, h, w, mode))
        # labels inside the source stay inside the rectangle: nothing clipped, so the round trip returns them
        back = plan.invert_uv(fwd)
        assert np.abs(back.astype(np.float64) - uv).max() < 1e-4
        small = resample.ResamplePlan([(48, 64), (30, 40)], (h, w), mode=mode)
        uv2 = np.array([[[10.25, 7.5], [63.0, 47.0]], [[0.0, 0.0], [39.0, 29.0]]], dtype=np.float32)
        assert np.abs(small.invert_uv(small.apply_uv(uv2)) - uv2).max() < 1e-4
        t = plan.apply_uv(torch.from_numpy(uv))                               # a tensor comes back as a tensor
        assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), fwd)
    # the identity keeps labels; clipping as dataset.py:65-66 clips
    same = resample.ResamplePlan([(h, w)], (h, w))
    uv = np.array([[[3.5, 7.25], [-4.0, 100.0], [70.0, -1.0]]], dtype=np.float32)
    want = uv.copy()
    want[..., 0] = np.clip(want[..., 0], 0, w - 1)
    want[..., 1] = np.clip(want[..., 1], 0, h - 1)
    assert np.array_equal(same.apply_uv(uv), want)
    half = resample.ResamplePlan([(2 * h, 2 * w)], (h, w))
    assert np.array_equal(half.apply_uv(np.array([[[127.0, 95.0], [300.0, -9.0]]], dtype=np.float32)),
                          np.array([[[63.0, 47.0], [63.0, 0.0]]], dtype=np.float32))  # (127.5*0.5 - 0.5 = 63.25 -> 63)
    assert np.allclose(half.invert_uv(np.array([[[0.0, 0.0]]], dtype=np.float32)), 0.5)
    with pytest.raises(Exception, match="expected"):
        half.apply_uv(np.zeros((2, 3, 2), dtype=np.float32))


@pytest.mark.parametrize("mode", ["stretch", "fit"])
@pytest.mark.parametrize("name", ["bilinear", "lanczos"])
def test_label_follows_a_blob(name, mode):
    """A bright 9x9 blob centred on an integer label: after the resize its intensity
    centroid lies within 1 output pixel of the mapped label."""
    from hkp import resample
    hs, ws, h, w = 150, 260, 48, 64
    img = np.zeros((hs, ws, 3), dtype=np.uint8)
    u, v = 171, 52
    img[v - 4:v + 5, u - 4:u + 5] = 255
    out = ref.resample(img, h, w, name, mode, fill=(0, 0, 0)).astype(np.float64).sum(-1)
    assert out.sum() > 0
    ys, xs = np.mgrid[0:h, 0:w]
    cu, cv = (out * xs).sum() / out.sum(), (out * ys).sum() / out.sum()
    plan = resample.ResamplePlan([(hs, ws)], (h, w), filter=name, mode=mode)
    want = plan.apply_uv(np.array([[[u, v]]], dtype=np.float32))[0, 0]
    assert abs(cu - want[0]) <= 1.0 and abs(cv - want[1]) <= 1.0, ((cu, cv), want)


def _call(plan, in_ptr=1 << 20, out_ptr=1 << 40, records=True, tables=True, table_words=None, hw=None, in_bytes=None):
    """hkp_resample_u8 with made-up device addresses: every case below fails the host
    validation, which comes before anything is launched or read on the device."""
    from hkp import _lib
    P = ctypes.c_void_p
    h, w = plan.hw if hw is None else hw
    return _lib.call("hkp_resample_u8", plan.n, P(in_ptr), plan.in_bytes if in_bytes is None else in_bytes,
                     plan.records if records else None, P(1 << 30), P(plan.tables.ctypes.data) if tables else None,
                     P(1 << 31), plan.tables.size if table_words is None else table_words, h, w, P(out_ptr), None)


def test_bad_arguments_raise_not_crash():
    from hkp import _lib, resample
    assert ctypes.sizeof(_lib.ResampleImage) == 64
    mk = lambda: resample.ResamplePlan([(20, 30), (12, 9)], (8, 12), filter="bicubic", mode="fit")   # noqa: E731
    with pytest.raises(_lib.HkpError, match="null pointer"):
        _call(mk(), in_ptr=0)
    with pytest.raises(_lib.HkpError, match="null pointer"):
        _call(mk(), records=False)
    with pytest.raises(_lib.HkpError, match="null pointer"):
        _call(mk(), tables=False)
    p = mk()
    p.records[1].xtab = p.tables.size                              # a table offset past table_words
    with pytest.raises(_lib.HkpError, match="image 1, x table: table offset"):
        _call(p)
    p = mk()
    with pytest.raises(_lib.HkpError, match="table_words"):        # a table that runs past the end
        _call(p, table_words=p.tables.size - 1)
    p = mk()
    ytab = p.records[0].ytab
    p.tables[ytab + 2 + 2 * 3 + 1] += 20                           # y output 3: xmin + cnt > hs
    with pytest.raises(_lib.HkpError, match=r"image 0, y table: output index 3: .*xmin \+ cnt <= 20"):
        _call(p)
    p = mk()
    p.tables[p.records[1].xtab + 2 + 2 * 5] += 1                   # x output 5 (the last): xmin + cnt > ws
    with pytest.raises(_lib.HkpError, match=r"image 1, x table: output index 5: .*xmin \+ cnt <= 9"):
        _call(p)
    p = mk()
    p.tables[p.records[1].xtab + 2] = -1                           # a negative xmin
    with pytest.raises(_lib.HkpError, match="image 1, x table: output index 0: xmin=-1"):
        _call(p)
    p = mk()
    p.tables[p.records[0].xtab + 1] += 1                           # a table's out != wd
    with pytest.raises(_lib.HkpError, match="out="):
        _call(p)
    p = mk()
    p.records[1].x0 = 12                                           # the rectangle leaves the output
    with pytest.raises(_lib.HkpError, match="image 1: rectangle"):
        _call(p)
    with pytest.raises(_lib.HkpError, match="image 0: rectangle"):
        _call(mk(), hw=(7, 12))
    p = mk()
    p.records[0].reserved[2] = 5
    with pytest.raises(_lib.HkpError, match="image 0 has a non-zero reserved"):
        _call(p)
    p = mk()
    with pytest.raises(_lib.HkpError, match="in_bytes"):           # the last image passes the input's end
        _call(p, in_bytes=p.in_bytes - 1)
    with pytest.raises(_lib.HkpError, match="overlap"):
        _call(mk(), out_ptr=(1 << 20) + 100)
    with pytest.raises(_lib.HkpError, match="outside 1.."):
        _call(mk(), hw=(8, _lib.HKP_WARP_MAX_DIM + 1))
    # the host wrappers: no GPU tensor, unknown names
    with pytest.raises(_lib.HkpError, match="unknown filter"):
        resample.ResamplePlan([(4, 4)], (2, 2), filter="cubic")
    with pytest.raises(_lib.HkpError, match="unknown mode"):
        resample.ResamplePlan([(4, 4)], (2, 2), mode="crop")
    with pytest.raises(ValueError):
        resample.Resize(filter="cubic")
    from hkp import ops
    with pytest.raises(_lib.HkpError, match="on the GPU"):
        ops.resample_u8(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), 2, 2)


def test_ragged_collate_and_the_collate_choice():
    from hkp import resample
    from src import dataset as D
    sizes = [(5, 7), (9, 4), (6, 6)]
    imgs = [ref.images(a, b, 4) for a, b in sizes]
    uvs = [np.full((2, 2), i, dtype=np.float32) for i in range(3)]
    tag, flat, sz, uv = D._collate_ragged(list(zip(imgs, uvs)))
    assert tag == "ragged" and flat.dtype == torch.uint8 and flat.dim() == 1
    assert sz.dtype == torch.int64 and sz.tolist() == [list(s) for s in sizes] and tuple(uv.shape) == (3, 2, 2)
    plan = resample.Resize("box").plan(sz.numpy(), (4, 4))
    assert plan.in_bytes == flat.numel() == sum(a * b * 3 for a, b in sizes)
    assert plan.offsets().tolist() == [0, 5 * 7 * 3, 5 * 7 * 3 + 9 * 4 * 3]
    for im, off in zip(imgs, plan.offsets()):
        assert np.array_equal(flat.numpy()[off:off + im.size].reshape(im.shape), im)
    assert np.array_equal(ref.resample_ragged(flat.numpy(), sizes, 4, 4, "box"),
                          np.stack([ref.resize(im, 4, 4, "box") for im in imgs]))

    class _DS:
        imgs, labels_np, img_height, img_width = [], [], 4, 4

    assert D.DeviceBatches(_DS(), 2)._view_collate()[1] is D._collate_u8
    assert D.DeviceBatches(_DS(), 2, decode="device", resize=None)._view_collate()[1] is D._collate_coef
    rs = resample.Resize()
    assert D.DeviceBatches(_DS(), 2, resize=rs)._view_collate()[1] is D._collate_ragged
    assert D.DeviceBatches(_DS(), 2, decode="device", resize=rs)._view_collate()[1] is D._collate_coef_ragged
