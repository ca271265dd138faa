"""The BatchNorm family (csrc/bn.hip, csrc/bn_bwd.hip), the stem pool and absmax,
kernel by kernel at the edges of their dispatch, each against a plain restatement
from tests/_bn_ref.py: bit for bit where the kernel's arithmetic is fp32 in a fixed
order (apply, split, backward apply, pool, absmax), to a stated bound where it sums.

The whole-network tests pass through these kernels at the workloads' shapes and with
tolerances set by train-mode-BN conditioning.  Here: the FIX / non-FIX forms of the
two applies with their pair loops and tails, capped grids and second grid-stride
trips, every form of the two finalizes (register-held 8 / 16 / 32, the 256- and
1024-thread loops, the two-level merge, CPB 1 / 2 / 4 / 8), every channel width of
the backward reduce, the rejections, and the non-finite rule (ReLU(NaN) = 0).
Each figure is printed before it is asserted (pytest -s shows them).

Not pinned: the 64-bit index instantiation of bn_relu_maxpool_kernel (>= 2^31
elements: an 8 GB tensor), and the segmented (mixed tile height) finalize, which
test_gpu_mix_tiles.py covers."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bn_ref as ref
from _bn_ref import rand

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _equal(what, got, want):
    """Bit-for-bit up to the sign of zero (torch.equal), NaN in the same places."""
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.is_floating_point():
        bad = int(((got != want) & ~(got.isnan() & want.isnan())).sum())
    else:
        bad = int((got != want).sum())
    print("%s: %d of %d differ" % (what, bad, got.numel()))
    assert bad == 0, (what, bad)


def _ulps(what, got, want, most=1):
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, what
    worst, n = ref.ulp_diff(got, want)
    print("%s: max %d ulp, %d of %d differ" % (what, worst, n, got.numel()))
    assert worst <= most, (what, worst)
    return n


def mixed_ss(c, seed):
    """scale | shift with scales of both signs, none near 0."""
    sc = (rand(c, seed=seed).abs() * 0.5 + 0.5) * torch.where(rand(c, seed=seed + 1000) > 0, 1.0, -1.0)
    return torch.cat([sc, rand(c, seed=seed + 2000)])


# ------------------------------------------------------------ A. bn_apply ----

RES_FORMS = ("none", "raw", "affine", "packed")
OUT_FORMS = ("fp32", "split1", "split3", "split3only")
# block 256, at most 4096 blocks, n4 = m*C/4, stride = blocks*256, FIX <=> stride % (C/4) == 0
APPLY_ROWS = [
    # m, C, plan ("cross": every residual x output form the width allows)
    (1, 4, "cross"),          # n4 = 1: one live thread; FIX (256 % 1), tail only
    (7, 96, "cross"),         # n4 = 168, one block: 256 % 24 != 0 -> non-FIX, 88 idle threads
    (32, 96, "cross"),        # n4 = 768, 3 blocks: 768 % 24 == 0 -> FIX with i0 % C4, C4 = 24 not a power of two
    (3, 2048, "cross"),       # C/4 = 512 wider than a block: n4 = 1536, 6 blocks, 1536 % 512 == 0 -> FIX
    (43700, 96, [("packed", "split3")]),       # n4 = 1,048,800 > 4096*256: capped grid, 1048576 % 24 != 0 ->
                                               # non-FIX, a second trip for 224 threads
    (16400, 256, [("affine", "split1")]),      # n4 = 1,049,600: capped, FIX (C4 = 64); 1024 threads take the
                                               # pair loop, every other thread the tail only
    (131075, 64, [("none", "split3only"), ("raw", "fp32")]),   # n4 = 2*stride + 48: FIX (C4 = 16), every thread
                                                               # one pair, 48 threads a pair and the tail
]


def _apply_case(d, ops, inp, relu, resf, outf, tag):
    y, ss, res, rss, packed = inp["y"], inp["ss"], inp["res"], inp["rss"], inp["packed"]
    kw, rkw = {}, {}
    if resf == "raw":
        kw, rkw = dict(res=inp["res_d"]), dict(res=res)
    elif resf == "affine":
        kw, rkw = dict(res=inp["res_d"], res_ss=inp["rss_d"]), dict(res=res, res_ss=rss)
    elif resf == "packed":
        kw, rkw = dict(res=inp["packed_d"]), dict(res_split=packed)
    want = ref.apply(y, ss, relu=relu, **rkw)
    what = "bn_apply %s relu=%d res=%s out=%s" % (tag, relu, resf, outf)
    if outf == "fp32":
        _equal(what, ops.bn_apply(inp["y_d"], inp["ss_d"], relu=relu, **kw), want)
    elif outf == "split3only":
        sp = ops.bn_apply(inp["y_d"], inp["ss_d"], relu=relu, split=3, keep_fp32=False, **kw)
        assert sp._hkp_split_passes == 3
        _equal(what, sp, ref.split(want, 3))
    else:
        passes = 1 if outf == "split1" else 3
        o = ops.bn_apply(inp["y_d"], inp["ss_d"], relu=relu, split=passes, **kw)
        _equal(what, o, want)
        assert o._hkp_split[1] == passes
        _equal(what + " (split)", o._hkp_split[0], ref.split(want, passes))


def _apply_inputs(d, ops, m, c, seed):
    inp = dict(y=rand(m, c, seed=seed) * 2 + 0.3, ss=mixed_ss(c, seed + 1), res=rand(m, c, seed=seed + 2) * 3,
               rss=mixed_ss(c, seed + 3), packed=None)
    for k in ("y", "ss", "res", "rss"):
        inp[k + "_d"] = inp[k].to(d)
    if c % 32 == 0:     # the packed residual is a split=3 tensor the kernel itself made (identity BN, no ReLU)
        ident = torch.cat([torch.ones(c), torch.zeros(c)])
        inp["packed_d"] = ops.bn_apply(inp["res_d"], ident.to(d), relu=False, split=3, keep_fp32=False)
        inp["packed"] = inp["packed_d"].cpu()
        _equal("bn_apply: packed residual", inp["packed"], ref.split(inp["res"], 3))
    return inp


@pytest.mark.parametrize("m,c,plan", APPLY_ROWS, ids=["%dx%d" % r[:2] for r in APPLY_ROWS])
def test_bn_apply_edges(cuda_device, m, c, plan):
    from hkp import ops
    inp = _apply_inputs(cuda_device, ops, m, c, 100 + c)
    if plan == "cross":
        plan = [(r, o) for r in RES_FORMS for o in OUT_FORMS if c % 32 == 0 or (r != "packed" and o == "fp32")]
    for resf, outf in plan:
        for relu in (True, False):
            _apply_case(cuda_device, ops, inp, relu, resf, outf, "(%d, %d)" % (m, c))


# -------------------------------------------------------- B. bn_apply_f16 ----

# block 256, at most 512 blocks, n8 = m*C/8, FIX <=> (blocks*256) % (C/8) == 0
APPLY16_ROWS = [
    (1, 8, "cross"),          # one live thread
    (5, 96, "cross"),         # n8 = 60, one block: 256 % 12 != 0 -> non-FIX
    (64, 96, "cross"),        # n8 = 768, 3 blocks: 768 % 12 == 0 -> FIX with C/8 = 12
    (10930, 96, [("raw", True)]),              # n8 = 131,160 > 512*256: capped, 131072 % 12 != 0 -> non-FIX, second trip
    (2050, 512, [("affine", False)]),          # n8 = 131,200: capped, FIX (C/8 = 64); pair loop for 128 threads
    (32771, 64, [("none", True), ("raw", False)]),   # n8 = 2*stride + 24: every thread one pair, 24 the tail too
]


@pytest.mark.parametrize("m,c,plan", APPLY16_ROWS, ids=["%dx%d" % r[:2] for r in APPLY16_ROWS])
def test_bn_apply_f16_edges(cuda_device, m, c, plan):
    from hkp import ops
    d = cuda_device
    y, res = (rand(m, c, seed=200 + c) * 2 + 0.3).half(), (rand(m, c, seed=201 + c) * 3).half()
    ss, rss = mixed_ss(c, 202 + c), mixed_ss(c, 203 + c)
    y_d, res_d, ss_d, rss_d = y.to(d), res.to(d), ss.to(d), rss.to(d)
    if plan == "cross":
        plan = [(r, k) for r in RES_FORMS[:3] for k in (False, True)]
    for resf, keep in plan:
        for relu in (True, False):
            kw = {} if resf == "none" else dict(res=res_d) if resf == "raw" else dict(res=res_d, res_ss=rss_d)
            rkw = {} if resf == "none" else dict(res=res) if resf == "raw" else dict(res=res, res_ss=rss)
            h16, o32 = ref.apply_f16(y, ss, relu=relu, **rkw)
            what = "bn_apply_f16 (%d, %d) relu=%d res=%s keep_fp32=%d" % (m, c, relu, resf, keep)
            out = ops.bn_apply_f16(y_d, ss_d, relu=relu, keep_fp32=keep, **kw)
            if keep:
                _equal(what + " (fp32)", out, o32)
                assert out._hkp_split[1] == 1
                out = out._hkp_split[0]
            assert out._hkp_split_passes == 1
            _equal(what, out, h16)


# --------------------------------------- C. bn_finalize on synthetic partials ----

# one-kernel form: CPB = 1 / 2 / 4 / 8 for C < 256 / < 512 / < 1024 / >= 1024, TL = 256/CPB tile lanes;
# per = ceil(tiles / TL) partials per lane: <= 8 -> NB 8, <= 16 -> NB 16, <= 32 -> NB 32, else the
# 256-thread loop; tiles >= 4096 -> the 1024-thread loop.  Two-level: chunks of 128 tiles.
FIN_CASES = [
    (64, 2048),      # CPB 1: per = 8 -> NB 8
    (64, 2049),      # per = 9 -> NB 16
    (64, 4095),      # per = 16 -> NB 16, the last lane one short
    (64, 4096),      # 1024 threads
    (256, 1024),     # CPB 2, TL 128: per = 8 -> NB 8
    (256, 2048),     # per = 16 -> NB 16
    (256, 2049),     # per = 17 -> NB 32
    (256, 4096),     # 1024 threads, CPB 2
    (512, 2048),     # CPB 4, TL 64: per = 32 -> NB 32
    (512, 2049),     # per = 33 -> the 256-thread loop (NB 0)
    (512, 4097),     # 1024 threads, CPB 4; 33 chunks, the last of one tile
    (1024, 1024),    # CPB 8, TL 32: per = 32 -> NB 32
    (1024, 1025),    # per = 33 -> the 256-thread loop
    (1024, 4096),    # 1024 threads, CPB 8
    (1030, 300),     # 129 blocks, the last with six live channels; per = 10 -> NB 16
    (100, 130),      # two-level: 2 chunks (128 + 2 tiles), the second channel block 36 of 64 live
]
FIN_SEEN = {"cases": 0, "one_ulp": 0, "values": 0}


def _fin_count(tiles, rows, kind):
    return tiles * rows - 37 % rows if kind == "ragged" else (tiles - 1) * rows + 1


def _fin_partials(tiles, c, rows, count, seed):
    n_t = torch.clamp(count - torch.arange(tiles) * rows, max=rows).float()[:, None]
    g = torch.Generator().manual_seed(seed)
    s = n_t * (torch.randn(tiles, c, generator=g) + 1.5)
    q = n_t * (torch.rand(tiles, c, generator=g) * 1.5 + 0.5)
    return torch.stack([s, q], -1).contiguous()


@pytest.mark.parametrize("c,tiles", FIN_CASES)
def test_bn_finalize_forms(cuda_device, c, tiles):
    from hkp import ops
    d = cuda_device
    i = FIN_CASES.index((c, tiles))
    # every (C, tiles): a power-of-two and another tile height, one of the two ragged counts each
    configs = [(128, "ragged"), (96, "one")] if i % 2 == 0 else [(4, "one"), (96, "ragged")]
    gamma, beta = mixed_ss(c, 300 + i)[:c], rand(c, seed=301 + i)
    rm0, rv0 = rand(c, seed=302 + i), rand(c, seed=303 + i).abs() + 0.5
    for rows, kind in configs:
        count = _fin_count(tiles, rows, kind)
        assert (tiles - 1) * rows < count <= tiles * rows
        part = _fin_partials(tiles, c, rows, count, 304 + i)
        want = ref.finalize(part, count, rows, gamma, beta, 0.1, 1e-5, rm0, rv0)
        part_d = part.to(d)
        part_d._hkp_tile_rows = rows
        tag = "bn_finalize C=%d tiles=%d rows=%d count=%d" % (c, tiles, rows, count)
        outs = []
        for form, two_level in (("one-kernel", 1 << 40), ("two-level", 1)):
            rm, rv, nbt = rm0.to(d), rv0.to(d), torch.full((1,), 41, device=d, dtype=torch.int64)
            ss, mi = ops.bn_finalize(part_d, count, gamma.to(d), beta.to(d), rm, rv, nbt, two_level_tiles=two_level)
            n = _ulps("%s %s mean_invstd" % (tag, form), mi, want["mi"])
            _equal("%s %s scale_shift" % (tag, form), ss, ref.ss_from_mi(mi.cpu(), gamma, beta))
            n += _ulps("%s %s running_mean" % (tag, form), rm, want["rm"])
            n += _ulps("%s %s running_var" % (tag, form), rv, want["rv"])
            assert nbt.item() == 42
            FIN_SEEN["one_ulp"] += n
            FIN_SEEN["values"] += 4 * c
            ss2, mi2 = ops.bn_finalize(part_d, count, gamma.to(d), beta.to(d), two_level_tiles=two_level)
            _equal("%s %s second run" % (tag, form), torch.cat([ss2, mi2]), torch.cat([ss, mi]).cpu())
            outs.append((mi.cpu(), rm.cpu(), rv.cpu()))
        for a, b, nm in zip(outs[0], outs[1], ("mean_invstd", "running_mean", "running_var")):
            _ulps("%s one-kernel vs two-level %s" % (tag, nm), a, b)
    FIN_SEEN["cases"] += 1
    print("bn_finalize so far: %d of %d values 1 ulp from the float64 restatement"
          % (FIN_SEEN["one_ulp"], FIN_SEEN["values"]))


@pytest.mark.parametrize("c,tiles,rows", [(512, 2049, 96), (64, 4096, 128)])   # the 256- and the 1024-thread loop
def test_bn_stats_forms(cuda_device, c, tiles, rows):
    from hkp import ops
    count = _fin_count(tiles, rows, "ragged")
    part = _fin_partials(tiles, c, rows, count, 330 + c)
    want = ref.finalize(part, count, rows, None, None)
    want = np.concatenate([want["mean"], want["m2"], [float(count)]])
    part_d = part.to(cuda_device)
    part_d._hkp_tile_rows = rows
    for form, two_level in (("one-kernel", 1 << 40), ("two-level", 1)):
        st = ops.bn_stats(part_d, count, two_level_tiles=two_level).cpu().numpy()
        err = np.abs(st - want) / np.abs(want)
        print("bn_stats C=%d tiles=%d %s: max relative error %.3e" % (c, tiles, form, err.max()))
        assert st.shape == want.shape and err.max() <= 1e-12


# ------------------------------------------------- D. bn_bwd kernel by kernel ----

def _stats64(y, eps=1e-5):
    """mean | invstd of y [M, C] from float64 statistics, rounded (M = 1 is legal)."""
    y64 = y.double()
    mean = y64.mean(0)
    var = ((y64 - mean) ** 2).mean(0)
    return torch.cat([mean, 1.0 / torch.sqrt(var + float(np.float32(eps)))]).float()


REDUCE_SEEN = {"s": 0.0, "d": 0.0}


# C/4 threads per row (tpr), rpar = 256/tpr rows in flight, G channel groups per thread
@pytest.mark.parametrize("c", [4,       # tpr 1, rpar 256 > 64 rows: 192 threads without a row
                               32,      # tpr 8, rpar 32
                               128,     # tpr 32, rpar 8
                               512,     # tpr 128, rpar 2
                               1024,    # tpr 256, rpar 1
                               2048])   # G = 2: tpr 256, two groups per thread
def test_bn_bwd_reduce_widths(cuda_device, c):
    from hkp import ops
    from hkp._lib import call
    d = cuda_device
    ss = mixed_ss(c, 400 + c)
    for m in (1, 63, 64, 65, 130):      # one row; a tile one short, full, one over; three tiles, the last of two rows
        y, g = rand(m, c, seed=401 + m) * 2 + 0.3, rand(m, c, seed=402 + m)
        mi = _stats64(y)
        out = ref.apply(y, ss, relu=True)
        y_d, g_d, mi_d, ss_d, out_d = y.to(d), g.to(d), mi.to(d), ss.to(d), out.to(d)
        tiles = (m + 63) // 64
        parts = {}
        for mode in ("none", "out_mask", "relu_ss"):
            mask = None if mode == "none" else out if mode == "out_mask" else ss
            dz_w, sums, sabs, max_w = ref.bwd_tile_sums(g, mask, y, mi[:c])
            for want_dz in (True, False):
                for want_max in (True, False):
                    part = torch.full((tiles, c, 2), NAN, device=d)
                    maxima = torch.full((tiles, c, 2), NAN, device=d) if want_max else None
                    bound = torch.full((1,), 0x7F7FFFFF, device=d, dtype=torch.int32) if want_max else None
                    dz = torch.full((m, c), NAN, device=d) if want_dz else None
                    call("hkp_bn_bwd_reduce", m, c, P(g_d), P(out_d if mode == "out_mask" else None),
                         P(ss_d if mode == "relu_ss" else None), P(y_d), P(mi_d), P(dz), P(part), P(maxima), P(bound),
                         ops._stream())
                    tag = "bn_bwd_reduce C=%d M=%d %s dz=%d maxima=%d" % (c, m, mode, want_dz, want_max)
                    p = part.cpu().numpy().astype(np.float64)
                    assert np.isfinite(p).all(), tag
                    es, ed = np.abs(p[..., 0] - sums[..., 0]), np.abs(p[..., 1] - sums[..., 1])
                    # an fp32 sum of <= 64 terms in any order, plus two roundings per product
                    bs, bd = 64 * 2.0 ** -24 * sabs[..., 0], 66 * 2.0 ** -24 * sabs[..., 1]
                    rs = float((es / np.where(bs > 0, bs, 1)).max())
                    rd = float((ed / np.where(bd > 0, bd, 1)).max())
                    print("%s: error / bound %.4f (sum dz), %.4f (sum dz*(y-mean))" % (tag, rs, rd))
                    assert (es <= bs).all() and (ed <= bd).all(), tag
                    REDUCE_SEEN["s"], REDUCE_SEEN["d"] = max(REDUCE_SEEN["s"], rs), max(REDUCE_SEEN["d"], rd)
                    if want_dz:
                        _equal(tag + " dz", dz, dz_w)
                    if want_max:
                        _equal(tag + " maxima", maxima, max_w)
                        assert bound.item() == 0, tag              # dy_bound_bits is zeroed for finalize's atomicMax
                    parts.setdefault(mode, part.cpu())
                    _equal(tag + " same partials as the first launch", part, parts[mode])
        _equal("bn_bwd_reduce C=%d M=%d: mask forms 1 and 2, partials" % (c, m), parts["relu_ss"], parts["out_mask"])
    print("bn_bwd_reduce so far: worst error / bound %.4f (sum dz), %.4f (sum dz*(y-mean))"
          % (REDUCE_SEEN["s"], REDUCE_SEEN["d"]))


# per = ceil(tiles / (256/CPB)): <= 8 -> NB 8, <= 16 -> NB 16, else the 256-thread loop; >= 4096 tiles -> 1024 threads
BWD_FIN_CASES = [
    (64, 2048, True),     # CPB 1: per 8 -> NB 8
    (64, 2049, True),     # per 9 -> NB 16
    (64, 4095, True),     # per 16 -> NB 16
    (64, 4096, True),     # 1024 threads
    (256, 1024, True),    # CPB 2: per 8 -> NB 8
    (256, 1025, True),    # per 9 -> NB 16
    (256, 2049, True),    # per 17 -> the 256-thread loop
    (256, 4096, True),    # 1024 threads, CPB 2
    (512, 512, True),     # CPB 4: per 8 -> NB 8
    (512, 513, True),     # per 9 -> NB 16
    (512, 1025, True),    # per 17 -> the 256-thread loop
    (512, 4097, True),    # 1024 threads, CPB 4
    (2048, 256, True),    # CPB 8: per 8 -> NB 8
    (2048, 257, True),    # per 9 -> NB 16
    (2048, 513, True),    # per 17 -> the 256-thread loop
    (2048, 4096, True),   # 1024 threads, CPB 8
    (1028, 300, False),   # the last block four live channels; no maxima: the bound word is zeroed
]
BWD_FIN_SEEN = {"one_ulp": 0, "values": 0}


def _bwd_fin_inputs(c, tiles, seed):
    g = torch.Generator().manual_seed(seed)
    part = torch.randn(tiles, c, 2, generator=g) + 0.5
    maxima = torch.rand(tiles, c, 2, generator=g) * 3
    mi = torch.cat([torch.randn(c, generator=g), torch.rand(c, generator=g) * 1.5 + 0.5])
    return part, maxima, mi, mixed_ss(c, seed + 1)[:c]


@pytest.mark.parametrize("c,tiles,with_max", BWD_FIN_CASES)
def test_bn_bwd_finalize_forms(cuda_device, c, tiles, with_max):
    from hkp import ops
    from hkp._lib import call
    d = cuda_device
    m = tiles * 64 - 5
    part, maxima, mi, gamma = _bwd_fin_inputs(c, tiles, 500 + c + tiles)
    if not with_max:
        maxima = None
    want = ref.bwd_coef(part, maxima, m, mi, gamma)
    part_d, mi_d, gamma_d = part.to(d), mi.to(d), gamma.to(d)
    max_d = maxima.to(d) if with_max else None
    dgamma, dbeta, coef = torch.full((c,), NAN, device=d), torch.full((c,), NAN, device=d), torch.full((3 * c,), NAN, device=d)
    # with maxima the reduce pass has zeroed the word; without, finalize zeroes it itself
    word = torch.full((1,), 0 if with_max else 0x7F7FFFFF, device=d, dtype=torch.int32)
    call("hkp_bn_bwd_finalize", c, m, P(part_d), P(max_d), P(mi_d), P(gamma_d), P(dgamma), P(dbeta), P(coef), P(word),
         ops._stream())
    tag = "bn_bwd_finalize C=%d tiles=%d" % (c, tiles)
    sl = want["slack"]
    for nm, got, w, s in (("dbeta", dbeta, want["dbeta"], sl[0]), ("dgamma", dgamma, want["dgamma"], sl[1]),
                          ("coef", coef, want["coef"], np.concatenate([sl[2], sl[3], sl[4]]))):
        got = got.cpu()
        err = (got.double() - w.double()).abs().numpy()
        tol = np.spacing(np.abs(w.numpy())).astype(np.float64) + s       # 1 fp32 ulp + tiles * 2^-53 * sum |partial|
        n = int((got != w).sum())
        print("%s %s: %d of %d differ, max error / tolerance %.3f" % (tag, nm, n, got.numel(), (err / tol).max()))
        assert np.isfinite(got.numpy()).all() and (err <= tol).all(), (tag, nm)
        BWD_FIN_SEEN["one_ulp"] += n
        BWD_FIN_SEEN["values"] += got.numel()
    got_word = word.cpu().view(torch.float32)
    if with_max:
        own = torch.from_numpy(np.array([ref.bwd_bound(coef.cpu(), want["md"], want["mv"])], dtype=np.float32))
        _ulps(tag + " bound word vs the formula on the kernel's coef", got_word, own)
    else:
        print("%s bound word without maxima: %r" % (tag, word.item()))
        assert word.item() == 0
    print("bn_bwd_finalize so far: %d of %d values differ from the float64 restatement"
          % (BWD_FIN_SEEN["one_ulp"], BWD_FIN_SEEN["values"]))


@pytest.mark.parametrize("c,tiles", [(256, 2049), (2048, 4096)])      # the 256-thread loop; 1024 threads
def test_bn_bwd_stats(cuda_device, c, tiles):
    from hkp import ops
    from hkp._lib import call
    d = cuda_device
    m = tiles * 64 - 5
    part, maxima, mi, _ = _bwd_fin_inputs(c, tiles, 500 + c + tiles)
    p = part.numpy().astype(np.float64)
    x = maxima.numpy().astype(np.float64)
    want = np.concatenate([p[..., 0].sum(0), p[..., 1].sum(0), x[..., 0].max(0), x[..., 1].max(0), [float(m)]])
    st = torch.full((4 * c + 1,), NAN, device=d, dtype=torch.float64)
    part_d, max_d, mi_d = part.to(d), maxima.to(d), mi.to(d)
    call("hkp_bn_bwd_stats", c, m, P(part_d), P(max_d), P(mi_d), P(st), ops._stream())
    err = np.abs(st.cpu().numpy() - want) / np.abs(want)
    print("bn_bwd_stats C=%d tiles=%d: max relative error %.3e" % (c, tiles, err.max()))
    assert err.max() <= 1e-12


# block 256; at most 512 blocks with the fused max (stride 131,072), 4096 without (stride 1,048,576)
@pytest.mark.parametrize("m,c", [(1, 4),          # one live thread; no split (C % 32)
                                 (130, 128),      # 17 blocks
                                 (4100, 128),     # n4 = 131,200: a second trip with the fused max (128 threads)
                                 (4100, 1024)])   # n4 = 1,049,600: a second trip without it, fp32 and split_only
def test_bn_bwd_apply_edges(cuda_device, m, c):
    from hkp import ops
    from hkp._lib import call
    d = cuda_device
    y, g = rand(m, c, seed=600 + c) * 2 + 0.3, rand(m, c, seed=601 + c)
    mi, ss, gamma = _stats64(y), mixed_ss(c, 602 + c), mixed_ss(c, 603 + c)[:c]
    out = ref.apply(y, ss, relu=True)
    y_d, g_d, mi_d, ss_d, out_d, gamma_d = (t.to(d) for t in (y, g, mi, ss, out, gamma))
    tiles = (m + 63) // 64
    st = ops._stream()
    for mode in ("none", "out_mask", "relu_ss"):
        mk = (P(out_d if mode == "out_mask" else None), P(ss_d if mode == "relu_ss" else None))
        mask = None if mode == "none" else out if mode == "out_mask" else ss
        dz_w = ref.bwd_tile_sums(g, mask, y, mi[:c])[0]
        part, maxima = torch.empty(tiles, c, 2, device=d), torch.empty(tiles, c, 2, device=d)
        word = torch.full((1,), 0x7F7FFFFF, device=d, dtype=torch.int32)
        dgamma, dbeta, coef = torch.empty(c, device=d), torch.empty(c, device=d), torch.empty(3 * c, device=d)
        call("hkp_bn_bwd_reduce", m, c, P(g_d), mk[0], mk[1], P(y_d), P(mi_d), None, P(part), P(maxima), P(word), st)
        call("hkp_bn_bwd_finalize", c, m, P(part), P(maxima), P(mi_d), P(gamma_d), P(dgamma), P(dbeta), P(coef), P(word), st)
        bound = word.cpu().view(torch.float32).item()
        dy_w = ref.bwd_apply(dz_w, y, mi[:c], coef.cpu())         # on the kernel's own coefficients
        tag = "bn_bwd_apply (%d, %d) %s" % (m, c, mode)
        # fp32 dy, no max: the 4096-block grid
        dy = torch.full((m, c), NAN, device=d)
        call("hkp_bn_bwd_apply", m, c, P(g_d), mk[0], mk[1], P(y_d), P(mi_d), P(coef), P(dy), None, None, st)
        _equal(tag + " dy", dy, dy_w)
        # fused max|dy|: the 512-block grid; the word starts from 0, as finalize without maxima leaves it
        amax = torch.full((1,), 0x7F7FFFFF, device=d, dtype=torch.int32)
        coef2 = torch.empty(3 * c, device=d)
        call("hkp_bn_bwd_finalize", c, m, P(part), None, P(mi_d), P(gamma_d), P(dgamma), P(dbeta), P(coef2), P(amax), st)
        _equal(tag + " coef without maxima", coef2, coef.cpu())
        dy2 = torch.full((m, c), NAN, device=d)
        call("hkp_bn_bwd_apply", m, c, P(g_d), mk[0], mk[1], P(y_d), P(mi_d), P(coef), P(dy2), P(amax), None, st)
        _equal(tag + " dy (fused max)", dy2, dy_w)
        want_bits = dy_w.abs().max().reshape(1).view(torch.int32)
        print("%s fused max bits %#x, dy.abs().max() bits %#x, bound %.6g" % (tag, amax.item(), want_bits.item(), bound))
        assert amax.item() == want_bits.item()
        assert bound >= dy_w.abs().max().item()
        assert torch.equal(amax, ops.absmax(dy2))
        if c % 32 == 0:
            scale = ref.pow2_scale(bound)
            sp_w = ref.split(dy_w * scale, 3)
            for keep in (False, True):      # split_only, and the split with the fp32 dy beside it
                sp = torch.zeros(m, 2 * c, device=d, dtype=torch.float16)
                dy3 = torch.full((m, c), NAN, device=d) if keep else None
                call("hkp_bn_bwd_apply", m, c, P(g_d), mk[0], mk[1], P(y_d), P(mi_d), P(coef), P(dy3), P(word), P(sp), st)
                _equal("%s split of dy * 2^%d, fp32 dy=%d" % (tag, int(np.log2(scale)), keep), sp, sp_w)
                if keep:
                    _equal(tag + " dy beside the split", dy3, dy_w)
            assert word.cpu().view(torch.float32).item() == bound      # the split form only reads the word


@pytest.mark.parametrize("m,c", [(65, 512), (130, 1024)])
def test_bn_bwd_chain_against_autograd(cuda_device, m, c):
    """ops.bn_bwd (the three launches) against float64 autograd of F.batch_norm + ReLU.
    1e-5 * max(1, max |ref|), test_bn_backward's tolerance for dy, kept because the
    conditioning is the forward statistics' (fp32 mean and invstd), not these kernels'."""
    from hkp import ops
    d = cuda_device
    y32, g = rand(m, c, seed=700 + c) * 2 + 0.3, rand(m, c, seed=701 + c)
    gamma32, beta32 = rand(c, seed=702) * 0.2 + 1, rand(c, seed=703) * 0.1
    y, gamma, beta = (t.double().requires_grad_(True) for t in (y32, gamma32, beta32))
    z = F.batch_norm(y.t()[None], None, None, gamma, beta, True, 0.1, float(np.float32(1e-5)))[0].t()
    F.relu(z).backward(g.double())
    mi = _stats64(y32)
    ss = ref.ss_from_mi(mi, gamma32, beta32)
    out = ref.apply(y32, ss, relu=True)
    dy, dgamma, dbeta, _ = ops.bn_bwd(g.to(d), out.to(d), y32.to(d), mi.to(d), gamma32.to(d))
    dy2, dgamma2, dbeta2, _ = ops.bn_bwd(g.to(d), None, y32.to(d), mi.to(d), gamma32.to(d), relu_ss=ss.to(d))
    for nm, got, got2, want in (("dy", dy, dy2, y.grad), ("dgamma", dgamma, dgamma2, gamma.grad),
                                ("dbeta", dbeta, dbeta2, beta.grad)):
        err = (got.cpu().double() - want).abs().max().item()
        tol = 1e-5 * max(1.0, want.abs().max().item())
        print("bn_bwd chain (%d, %d) %s: err %.3e bound %.3e" % (m, c, nm, err, tol))
        assert err <= tol, (nm, err, tol)
        assert torch.equal(got2, got)


# ---------------------------------------------------------------- E. pool ----

# block 256, at most 4096 blocks: a second grid-stride trip needs more than 1,048,576 work items
@pytest.mark.parametrize("shape", [(1, 2050, 2050, 4),     # 1025 * 1025 = 1,050,625 windows, C/4 = 1: second trip of
                                                           # the forward; 4,202,500 pixels: trips 2-5 of the backward
                                   (2, 364, 364, 64)])     # 2 * 182 * 182 * 16 = 1,060,192 forward items
def test_pool_second_trip(cuda_device, shape):
    from hkp import ops
    d = cuda_device
    n, h, w, c = shape
    y = rand(*shape, seed=800 + c)
    ss = mixed_ss(c, 801 + c)
    out_w, route_w = ref.maxpool(y, ss)
    pool = ops.bn_relu_maxpool(y.to(d), ss.to(d), route=True)
    _equal("bn_relu_maxpool %s" % (shape,), pool, out_w)
    _equal("bn_relu_maxpool %s route" % (shape,), pool._hkp_route, route_w)
    dpool = rand(*out_w.shape, seed=802 + c)
    dz_w = ref.maxpool_bwd(dpool, route_w, shape)
    dz = ops.maxpool_bwd(dpool.to(d), pool._hkp_route, shape)
    _equal("maxpool_bwd %s" % (shape,), dz, dz_w)
    z = (y * ss[:c] + ss[c:]).requires_grad_(True)
    p = F.max_pool2d(F.relu(z).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(p.detach(), out_w)
    (dz_t,) = torch.autograd.grad(p, z, dpool)
    err, tol = (dz.cpu() - dz_t).abs().max().item(), 1e-6 * dz_t.abs().max().item()
    print("maxpool_bwd %s vs autograd: err %.3e bound %.3e" % (shape, err, tol))
    assert err <= tol


# -------------------------------------------------------------- F. absmax ----

# block 256, at most 512 blocks: stride 131,072 vectors of 4
@pytest.mark.parametrize("n", [4,                    # one live thread
                               8,
                               1028,                 # two blocks, the second one live thread
                               524292,               # n/4 = 131,073: one thread makes a second trip
                               3 * 524288 + 4])      # three full trips and one vector
def test_absmax_is_abs_max(cuda_device, n):
    from hkp import ops
    d = cuda_device

    def check(what, x):
        got = ops.absmax(x.to(d)).cpu()
        want = x.abs().max().reshape(1).view(torch.int32)
        print("absmax n=%d %s: bits %#x, x.abs().max() bits %#x" % (n, what, got.item() & 0xFFFFFFFF,
                                                                    want.item() & 0xFFFFFFFF))
        assert got.dtype == torch.int32 and got.item() == want.item(), what

    base = rand(n, seed=900)
    top = base.abs().max().item()
    for where in (0, n - 1, n // 2):        # a negative maximum in the first, the last, a middle element
        x = base.clone()
        x[where] = -(top + 1.5)
        check("negative maximum at %d" % where, x)
    check("all zeros", torch.zeros(n))
    check("all -0.0", -torch.zeros(n))
    x = torch.zeros(n)
    x[n - 2] = -1e-41
    check("a denormal maximum", x)
    x = base.clone()
    x[n // 3] = INF
    check("+inf", x)
    x[n // 3] = -INF
    check("-inf", x)


# ------------------------------------------------------ G. bn_eval_params ----

@pytest.mark.parametrize("c", [1, 64, 300])     # one thread; a quarter block; two blocks, the second 44 live
@pytest.mark.parametrize("affine", [True, False])
def test_bn_eval_params(cuda_device, c, affine):
    from hkp import ops
    d = cuda_device
    gamma, beta = (mixed_ss(c, 1000)[:c], rand(c, seed=1001)) if affine else (None, None)
    rm, rv = rand(c, seed=1002), rand(c, seed=1003).abs() + 1e-3
    ss_w, mi_w = ref.eval_params(gamma, beta, rm, rv)
    ss, mi = ops.bn_eval_params(gamma.to(d) if affine else None, beta.to(d) if affine else None, rm.to(d), rv.to(d))
    tag = "bn_eval_params C=%d affine=%d" % (c, affine)
    _equal(tag + " mean", mi[:c], rm)
    _ulps(tag + " invstd", mi[c:], mi_w[c:])
    _equal(tag + " scale_shift", ss, ref.ss_from_mi(mi.cpu(), gamma, beta))


# ---------------------------------------------------------- H. rejections ----

SENTINEL = -777.0


def _rejects(what, fn, *outs):
    """fn raises HkpError and leaves every tensor of outs as it was."""
    from hkp._lib import HkpError
    before = [o.clone() for o in outs]
    with pytest.raises(HkpError):
        fn()
    torch.cuda.synchronize()
    for o, b in zip(outs, before):
        assert torch.equal(o, b), what + ": an output was written"
    print("%s: rejected, nothing written" % what)


def test_bn_forward_rejections(cuda_device):
    from hkp import ops
    from hkp._lib import call, lib
    d, st = cuda_device, ops._stream()
    z = lambda *s, dt=torch.float32: torch.full(s, SENTINEL, device=d, dtype=dt)   # noqa: E731
    y6, ss6, o6 = z(3, 6), z(12), z(3, 6)
    _rejects("bn_apply C % 4 != 0", lambda: ops.bn_apply(y6, ss6, out=o6), o6)
    y8, ss8, o8, sp8 = z(3, 8), z(16), z(3, 8), z(3, 16, dt=torch.float16)
    _rejects("bn_apply split with C % 32 != 0 (wrapper)", lambda: ops.bn_apply(y8, ss8, out=o8, split=3), o8)
    for passes in (1, 3):
        _rejects("hkp_bn_apply split passes %d with C not a multiple of 32" % passes,
                 lambda: call("hkp_bn_apply", 3, 8, P(y8), P(ss8), None, None, None, 1, P(o8), P(sp8), passes, st), o8, sp8)
    y32, ss32, o32, sp32 = z(3, 32), z(64), z(3, 32), z(3, 64, dt=torch.float16)
    _rejects("hkp_bn_apply split passes 2",
             lambda: call("hkp_bn_apply", 3, 32, P(y32), P(ss32), None, None, None, 1, P(o32), P(sp32), 2, st), o32, sp32)
    _rejects("bn_apply res_ss without res", lambda: ops.bn_apply(y32, ss32, res_ss=ss32, out=o32), o32)
    _rejects("bn_apply scale_shift one short", lambda: ops.bn_apply(y32, ss32[:-1], out=o32), o32)
    _rejects("bn_apply res_ss one short", lambda: ops.bn_apply(y32, ss32, res=y32, res_ss=ss32[:-1], out=o32), o32)
    _rejects("hkp_bn_apply packed and raw residual together",
             lambda: call("hkp_bn_apply", 3, 32, P(y32), P(ss32), P(y32), None, P(sp32), 1, P(o32), None, 0, st), o32)
    y12, ss12, o12, f12 = z(3, 12, dt=torch.float16), z(24), z(3, 12, dt=torch.float16), z(3, 12)
    _rejects("bn_apply_f16 C % 8 != 0 (wrapper)", lambda: ops.bn_apply_f16(y12, ss12))
    _rejects("hkp_bn_apply_f16 C % 8 != 0",
             lambda: call("hkp_bn_apply_f16", 3, 12, P(y12), P(ss12), None, None, 1, P(o12), P(f12), st), o12, f12)
    # finalize: 10 tiles of 128 rows hold 1153..1280 rows
    c, part = 64, z(10, 64, 2)
    ss, mi, rm, rv = z(128), z(128), z(64), z(64)
    nbt = torch.full((1,), 7, device=d, dtype=torch.int64)
    for count, why in ((1281, "tiles * tile_rows < count"), (1152, "(tiles - 1) * tile_rows >= count")):
        _rejects("hkp_bn_finalize " + why,
                 lambda: call("hkp_bn_finalize", c, count, 10, 128, P(part), None, None, 0.1, 1e-5, P(rm), P(rv), P(nbt),
                              P(ss), P(mi), st), ss, mi, rm, rv, nbt)
    need = lib().hkp_bn_finalize_workspace_bytes(c, 10)
    ws = z((need + 7) // 8, dt=torch.float64)
    _rejects("hkp_bn_finalize_ws workspace one byte short",
             lambda: call("hkp_bn_finalize_ws", c, 1200, 10, 128, P(part), None, None, 0.1, 1e-5, P(rm), P(rv), P(nbt),
                          P(ss), P(mi), P(ws), need - 1, st), ss, mi, rm, rv, nbt, ws)
    x6, word = z(6), torch.full((1,), 12345, device=d, dtype=torch.int32)
    _rejects("absmax n % 4 != 0 (wrapper)", lambda: ops.absmax(x6))
    _rejects("hkp_absmax n % 4 != 0", lambda: call("hkp_absmax", 6, P(x6), P(word), st), word)


def test_bn_backward_rejections(cuda_device):
    from hkp import ops
    from hkp._lib import call
    d, st = cuda_device, ops._stream()
    z = lambda *s, dt=torch.float32: torch.full(s, SENTINEL, device=d, dtype=dt)   # noqa: E731
    word = torch.full((1,), 12345, device=d, dtype=torch.int32)
    for c in (96, 4096):       # C/4 = 24 does not divide 256; C/4 = 1024 is wider than the G = 2 form
        g, mi, dz, part, maxima = z(2, c), z(2 * c), z(2, c), z(1, c, 2), z(1, c, 2)
        _rejects("hkp_bn_bwd_reduce C=%d" % c,
                 lambda: call("hkp_bn_bwd_reduce", 2, c, P(g), None, None, P(g), P(mi), P(dz), P(part), P(maxima), P(word),
                              st), dz, part, maxima, word)
    c = 64
    g, mi, ss, dz, part, maxima = z(2, c), z(2 * c), z(2 * c), z(2, c), z(1, c, 2), z(1, c, 2)
    _rejects("hkp_bn_bwd_reduce both masks",
             lambda: call("hkp_bn_bwd_reduce", 2, c, P(g), P(g), P(ss), P(g), P(mi), P(dz), P(part), P(maxima), P(word), st),
             dz, part, maxima, word)
    _rejects("hkp_bn_bwd_reduce bound word without maxima",
             lambda: call("hkp_bn_bwd_reduce", 2, c, P(g), None, None, P(g), P(mi), P(dz), P(part), None, P(word), st),
             dz, part, word)
    coef, dy, sp = z(3 * c), z(2, c), z(2, 2 * c, dt=torch.float16)
    _rejects("hkp_bn_bwd_apply dy_split without the bound word",
             lambda: call("hkp_bn_bwd_apply", 2, c, P(g), None, None, P(g), P(mi), P(coef), P(dy), None, P(sp), st), dy, sp)
    _rejects("hkp_bn_bwd_apply both masks",
             lambda: call("hkp_bn_bwd_apply", 2, c, P(g), P(g), P(ss), P(g), P(mi), P(coef), P(dy), None, None, st), dy)


# ---------------------------------------------------- I. non-finite values ----

def test_nonfinite_forward(cuda_device):
    """+-inf as torch (relu(-inf) = 0, +inf kept); NaN by this project's rule: 0 with
    the ReLU (o > 0 ? o : 0), NaN without it — the fused-input-BN convs rely on it."""
    from hkp import ops
    d = cuda_device
    m, c = 9, 32
    y = rand(m, c, seed=1100)
    ss = mixed_ss(c, 1101)
    ss[:4] = ss[:4].abs()           # channels 0..3: positive scales
    inf_y = y.clone()
    inf_y[0, 0], inf_y[1, 1], inf_y[2, 4] = INF, -INF, INF
    inf_y[3] = INF
    inf_y[4] = -INF
    for relu in (True, False):
        t = inf_y * ss[:c] + ss[c:]
        want = torch.relu(t) if relu else t
        assert not want.isnan().any() and torch.equal(ref.apply(inf_y, ss, relu=relu), want)
        _equal("bn_apply +-inf relu=%d" % relu, ops.bn_apply(inf_y.to(d), ss.to(d), relu=relu, split=0), want)
        t16 = inf_y.half().float() * ss[:c] + ss[c:]
        want16 = torch.relu(t16) if relu else t16
        got = ops.bn_apply_f16(inf_y.half().to(d), ss.to(d), relu=relu, keep_fp32=True)
        _equal("bn_apply_f16 +-inf relu=%d (fp32)" % relu, got, want16)
        _equal("bn_apply_f16 +-inf relu=%d" % relu, got._hkp_split[0], want16.half())
    nan_y = y.clone()
    nan_y[0, 0], nan_y[5, 7] = NAN, NAN
    res = rand(m, c, seed=1102)
    on, off = ops.bn_apply(nan_y.to(d), ss.to(d), relu=True).cpu(), ops.bn_apply(nan_y.to(d), ss.to(d), relu=False).cpu()
    print("bn_apply NaN: relu on -> %r, %r; off -> %r, %r" % (on[0, 0].item(), on[5, 7].item(), off[0, 0].item(),
                                                               off[5, 7].item()))
    assert on[0, 0] == 0 and on[5, 7] == 0 and off[0, 0].isnan() and off[5, 7].isnan()
    _equal("bn_apply NaN relu on", on, ref.apply(nan_y, ss, relu=True))
    _equal("bn_apply NaN relu off", off, ref.apply(nan_y, ss, relu=False))
    _equal("bn_apply NaN + residual relu on", ops.bn_apply(nan_y.to(d), ss.to(d), res=res.to(d), relu=True),
           ref.apply(nan_y, ss, res=res, relu=True))
    for relu in (True, False):
        h16, o32 = ref.apply_f16(nan_y.half(), ss, relu=relu)
        got = ops.bn_apply_f16(nan_y.half().to(d), ss.to(d), relu=relu, keep_fp32=True)
        _equal("bn_apply_f16 NaN relu=%d (fp32)" % relu, got, o32)
        _equal("bn_apply_f16 NaN relu=%d" % relu, got._hkp_split[0], h16)
        assert (o32[0, 0] == 0 and h16[5, 7] == 0) if relu else (o32[0, 0].isnan() and h16[5, 7].isnan())


def test_nonfinite_pool(cuda_device):
    from hkp import ops
    d = cuda_device
    shape = (1, 9, 11, 8)
    y = rand(*shape, seed=1110)
    ss = torch.cat([torch.ones(8), torch.zeros(8)])
    ss[1] = -1.0
    y[0, 2, 2, 0], y[0, 4, 6, 0], y[0, 6, 3, 1], y[0, 0, 0, 1] = INF, -INF, INF, -INF     # +-inf, both scale signs
    y[0, 3, 3, 2] = NAN                    # one NaN in four windows
    y[0, :, :, 3] = NAN                    # nothing but NaN: every window 0, route 255
    out_w, route_w = ref.maxpool(y, ss)
    clean = torch.nan_to_num(y[..., :2], nan=0.0, posinf=INF, neginf=-INF)
    t = F.max_pool2d(F.relu(clean * ss[:2]).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(out_w[..., :2], t) and out_w[0, 1, 1, 0] == INF     # +-inf as torch
    pool = ops.bn_relu_maxpool(y.to(d), ss.to(d), route=True)
    _equal("bn_relu_maxpool non-finite", pool, out_w)
    _equal("bn_relu_maxpool non-finite route", pool._hkp_route, route_w)
    got, rt = pool.cpu(), pool._hkp_route.cpu()
    print("bn_relu_maxpool NaN channel: max %r, routes %r" % (got[..., 3].max().item(), rt[..., 3].unique().tolist()))
    assert not got.isnan().any() and (got[..., 3] == 0).all() and (rt[..., 3] == 255).all()
    dpool = rand(*out_w.shape, seed=1111)
    dz = ops.maxpool_bwd(dpool.to(d), pool._hkp_route, shape)
    _equal("maxpool_bwd non-finite", dz, ref.maxpool_bwd(dpool, route_w, shape))
    assert (dz.cpu()[..., 3] == 0).all() and dz.cpu()[0, 3, 3, 2] == 0      # nothing is routed to a NaN


def test_nonfinite_backward_masks(cuda_device):
    """A NaN in y: the forward wrote 0 there, so `out > 0` blocks its gradient, and the
    mask recomputed from y (NaN > 0 is false) blocks the same ones."""
    from hkp import ops
    from hkp._lib import call
    d, st = cuda_device, ops._stream()
    m, c = 70, 32
    y, g = rand(m, c, seed=1120), rand(m, c, seed=1121)
    y[3, 5], y[66, 9] = NAN, NAN
    ss = mixed_ss(c, 1122)
    mi = _stats64(torch.nan_to_num(y))
    out_d = ops.bn_apply(y.to(d), ss.to(d), relu=True)
    assert out_d[3, 5] == 0 and out_d[66, 9] == 0
    dzs = []
    g_d, y_d, mi_d, ss_d = g.to(d), y.to(d), mi.to(d), ss.to(d)
    for om, rs in ((out_d, None), (None, ss_d)):
        dz, part = torch.full((m, c), NAN, device=d), torch.empty(2, c, 2, device=d)
        call("hkp_bn_bwd_reduce", m, c, P(g_d), P(om), P(rs), P(y_d), P(mi_d), P(dz), P(part), None, None, st)
        dzs.append(dz.cpu())
    want = ref.bwd_tile_sums(g, ss, y, mi[:c])[0]
    print("NaN in y: dz there %r / %r" % (dzs[0][3, 5].item(), dzs[1][66, 9].item()))
    _equal("bn_bwd_reduce NaN, out_mask", dzs[0], want)
    _equal("bn_bwd_reduce NaN, relu_ss", dzs[1], want)
    assert dzs[0][3, 5] == 0 and dzs[0][66, 9] == 0 and not dzs[0].isnan().any()
