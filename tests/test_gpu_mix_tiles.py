"""HKP_TILE_MIX_A3 (conv_x3_a3_mix_kernel: 256-, 192- and 160-row A3 tiles in one
launch) against the 256-row A3 body, and the segmented BN partial lists that go
with it (hkp_bn_finalize_seg / hkp_bn_stats_seg)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

MIX_CASES = [
    # (n, h, w, cin, cout, k, stride, pad, dil), the kernel the policy runs
    ((2, 150, 200, 32, 512, 3, 1, 2, 2), "mix"),    # M = 60,000, two column tiles, dilated: borders inside image rows
    ((2, 240, 240, 32, 256, 1, 1, 0, 1), "mix"),    # M = 115,200, one column tile, a single K-step
    # M = 57,344 = 128 x 256 + 128 x 192 on 256 CUs (the last tile full) — but a 64-channel
    # 3x3 with pad = dil = 1 on a patch-divisible output is the halo-tile body's under this
    # policy as under HKP_TILE_192_A3 and _256_A3; the dilated twin below runs the mix launch
    ((1, 224, 256, 64, 512, 3, 1, 1, 1), "halo"),
    ((1, 224, 256, 64, 512, 3, 1, 2, 2), "mix"),
    # on 256 CUs the planner's rule (fewest 16-row blocks per CU) gives the first two
    # shapes one region of 160-row tiles; these two give all three regions there:
    ((2, 150, 256, 32, 512, 3, 1, 2, 2), "mix"),    # M = 76,800, two column tiles: 128 x 256, 128 x 192, 122 x 160
    ((2, 240, 320, 256, 256, 1, 1, 0, 1), "mix"),   # M = 153,600, one column tile (256 / 256 / 244), with the dgrad
]


def _bn_stats(part, m):
    """mean | invstd of a conv's BN tile partials (bn_finalize, gamma 1, beta 0)."""
    from hkp import ops
    one = torch.ones(part.shape[1], device=part.device)
    return ops.bn_finalize(part, m, one, torch.zeros_like(one))[1]


@pytest.mark.parametrize("case", MIX_CASES)
def test_mix_tiles(cuda_device, case):
    """Every output of a mix launch is the 256-row A3 body's, bit for bit (the same
    MFMA sequence per output element), for f16x3 and both two-product sets; its BN
    partials come in the segments the library's layout query reports and finalize
    to the 128-row tiles' statistics; two launches give the same bits; the stride-1
    dgrad with its residual addend likewise (256-divisible Cin)."""
    from hkp import ops
    from hkp._lib import HKP_KOP_FWD_X3, HKP_TILE_256_A3, HKP_TILE_MIX_A3, HKP_X3_W16, HKP_X3_X16, ConvDesc
    (n, h, w, cin, cout, k, st, pad, dil), body = case
    d = cuda_device
    g = torch.Generator(device=d).manual_seed(47)
    x = torch.relu(torch.randn(n, h, w, cin, device=d, generator=g))
    wt = torch.randn(cout, k, k, cin, device=d, generator=g) * (2.0 / (k * k * cout)) ** 0.5
    ss = torch.cat([torch.ones(cin, device=d), torch.zeros(cin, device=d)])
    xs = ops.bn_apply(x, ss, relu=False, split=3, keep_fp32=False)
    del x
    wp = ops.weight_pack_x3(wt)
    desc = ConvDesc(n, h, w, cin, cout, k, k, st, pad, dil, 0, HKP_TILE_MIX_A3)
    assert ops.kernel_name(desc, HKP_KOP_FWD_X3) == "conv_x3_%s_kernel<3>" % ("a3_mix" if body == "mix" else body)
    segs = ops.conv_stat_layout(desc, HKP_KOP_FWD_X3)
    # the 256-row reference without the split-K tail (its segment sums reorder the K loop)
    y0, p0 = ops.conv2d_fwd_x3(xs, wp, st, pad, dil, sk=False, tile=HKP_TILE_256_A3)
    y1, p1 = ops.conv2d_fwd_x3(xs, wp, st, pad, dil, tile=HKP_TILE_MIX_A3)
    y2, p2 = ops.conv2d_fwd_x3(xs, wp, st, pad, dil, tile=HKP_TILE_MIX_A3)
    m = y0.numel() // cout
    print("segments", segs, "M", m)
    assert sum(r * t for r, t in segs[:-1]) < m <= sum(r * t for r, t in segs)
    assert p1.shape == (sum(t for _, t in segs), cout, 2)
    assert (ops.stat_segments(p1) or ((ops.stat_tile_rows(p1), p1.shape[0]),)) == segs
    assert torch.equal(y1, y0)
    assert torch.equal(y2, y1) and torch.equal(p2, p1)
    s1, s0 = _bn_stats(p1, m), _bn_stats(p0, m)
    print("stats max diff", (s1 - s0).abs().max().item())
    assert torch.allclose(s1, s0, rtol=1e-6, atol=1e-7)
    del y1, y2
    for prod in (HKP_X3_W16, HKP_X3_X16):
        a, _ = ops.conv2d_fwd_x3(xs, wp, st, pad, dil, sk=False, tile=HKP_TILE_256_A3, products=prod)
        b, _ = ops.conv2d_fwd_x3(xs, wp, st, pad, dil, tile=HKP_TILE_MIX_A3, products=prod)
        assert torch.equal(a, b), prod
        del a, b
    if st == 1 and cin % 256 == 0:          # (the dgrad outputs cin channels)
        gy = torch.randn(n, h, w, cout, device=d, generator=g) * 1e-3
        add = torch.randn(n, h, w, cin, device=d, generator=g) * 1e-3
        amax = ops.absmax(gy)
        dys = ops.split_pack_x3(gy, amax)
        wf = ops.weight_flip_pack_x3(wt)
        dx0 = ops.conv2d_bwd_data_x3(dys, wf, (n, h, w, cin), pad, dil, add=add, amax=amax, sk=False,
                                     tile=HKP_TILE_256_A3)
        dx1 = ops.conv2d_bwd_data_x3(dys, wf, (n, h, w, cin), pad, dil, add=add, amax=amax, tile=HKP_TILE_MIX_A3)
        dx2 = ops.conv2d_bwd_data_x3(dys, wf, (n, h, w, cin), pad, dil, add=add, amax=amax, tile=HKP_TILE_MIX_A3)
        assert torch.equal(dx1, dx0) and torch.equal(dx2, dx1)


def test_mix_one_round_plans_as_auto(cuda_device):
    """A 64 -> 256 conv one round deep (150 256-row tiles) is no mix launch: the
    forced policy plans as AUTO — AUTO's kernel, one list of 128-row partials, AUTO's bits."""
    from hkp import ops
    from hkp._lib import HKP_KOP_FWD_X3, HKP_TILE_MIX_A3, ConvDesc
    n, h, w, cin, cout = 2, 120, 160, 64, 256
    d = cuda_device
    g = torch.Generator(device=d).manual_seed(48)
    x = torch.relu(torch.randn(n, h, w, cin, device=d, generator=g))
    wt = torch.randn(cout, 1, 1, cin, device=d, generator=g) * (2.0 / cout) ** 0.5
    ss = torch.cat([torch.ones(cin, device=d), torch.zeros(cin, device=d)])
    xs = ops.bn_apply(x, ss, relu=False, split=3, keep_fp32=False)
    wp = ops.weight_pack_x3(wt)
    auto = ops.kernel_name(ConvDesc(n, h, w, cin, cout, 1, 1, 1, 0, 1, 0, 0), HKP_KOP_FWD_X3)
    desc = ConvDesc(n, h, w, cin, cout, 1, 1, 1, 0, 1, 0, HKP_TILE_MIX_A3)
    assert ops.kernel_name(desc, HKP_KOP_FWD_X3) == auto and "mix" not in auto
    assert ops.conv_stat_layout(desc, HKP_KOP_FWD_X3) == ((128, 300),)
    y0, p0 = ops.conv2d_fwd_x3(xs, wp, tile=0)
    y1, p1 = ops.conv2d_fwd_x3(xs, wp, tile=HKP_TILE_MIX_A3)
    assert p1.shape == (300, cout, 2) and ops.stat_segments(p1) is None and ops.stat_tile_rows(p1) == 128
    assert torch.equal(y1, y0) and torch.equal(p1, p0)


def _partials(y, bounds):
    """fp32 (sum, M2 about the tile mean) of the row ranges [bounds[i], bounds[i+1]) of y [M, C]."""
    out = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        t = y[a:b].double()
        out.append(torch.stack([t.sum(0), ((t - t.mean(0)) ** 2).sum(0)], dim=1))
    return torch.stack(out).float().contiguous()


def test_segmented_finalize(cuda_device):
    """hkp_bn_finalize_seg / hkp_bn_stats_seg on a three-segment list (5 x 128, 3 x 96,
    4 x 80 rows with the last tile cut to 37): scale/shift, mean/invstd and the
    running statistics are the one-segment finalize's of the same y tiled at 128
    rows and an fp64 mean / variance's, in the one-kernel and the two-level merge;
    a one-segment table through the new entry point gives hkp_bn_finalize's bits."""
    from hkp import ops
    from hkp._lib import call
    d = cuda_device
    c = 64
    segs = ((128, 5), (96, 3), (80, 4))
    count = 128 * 5 + 96 * 3 + 80 * 3 + 37
    g = torch.Generator(device=d).manual_seed(49)
    y = torch.randn(count, c, device=d, generator=g) * (0.5 + torch.rand(c, device=d, generator=g)) + \
        torch.randn(c, device=d, generator=g)
    bounds, row = [0], 0
    for rows, tiles in segs:
        for _ in range(tiles):
            row = min(count, row + rows)
            bounds.append(row)
    assert bounds[-1] == count and bounds[-2] == count - 37
    part = _partials(y, bounds)
    part._hkp_segments = segs
    ref = _partials(y, list(range(0, count, 128)) + [count])
    gamma = 0.5 + torch.rand(c, device=d, generator=g)
    beta = torch.randn(c, device=d, generator=g)

    def fin(p, **kw):
        rm, rv = torch.zeros(c, device=d), torch.ones(c, device=d)
        nbt = torch.zeros((), device=d, dtype=torch.int64)
        ss, mi = ops.bn_finalize(p, count, gamma, beta, rm, rv, nbt, **kw)
        assert nbt.item() == 1
        return ss, mi, rm, rv

    want = fin(ref)
    mean = y.double().mean(0)
    var = y.double().var(0, unbiased=False)
    invstd = (var + 1e-5).rsqrt()
    scale = gamma.double() * invstd
    f64 = (torch.cat([scale, beta.double() - mean * scale]), torch.cat([mean, invstd]), 0.1 * mean,
           0.9 + 0.1 * var * count / (count - 1))
    for kw in ({}, {"two_level_tiles": 1}):                   # one-kernel merge, two-level merge
        got = fin(part, **kw)
        for a, b, e in zip(got, want, f64):
            print(kw, "vs one segment", (a - b).abs().max().item(), "vs fp64", (a.double() - e).abs().max().item())
            assert torch.allclose(a, b, rtol=1e-6, atol=1e-7)
            assert torch.allclose(a.double(), e, rtol=1e-6, atol=1e-7)
        st = ops.bn_stats(part, count, **kw)
        assert st[2 * c].item() == count
        assert torch.allclose(st[:c], mean, rtol=1e-6, atol=1e-7)
        assert torch.allclose(st[c:2 * c], var * count, rtol=1e-6, atol=1e-7 * count)
    # one segment through the new entry point: the old kernels, the old bits
    table = (ctypes.c_int32 * 2)(128, ref.shape[0])
    ss = torch.empty(2 * c, device=d)
    mi = torch.empty(2 * c, device=d)
    call("hkp_bn_finalize_seg", c, count, 1, table, ref.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 0.1, 1e-5,
         None, None, None, ss.data_ptr(), mi.data_ptr(), None, 0, None)
    ss0, mi0 = ops.bn_finalize(ref, count, gamma, beta)
    assert torch.equal(ss, ss0) and torch.equal(mi, mi0)


def test_halo_body_reports_its_own_partial_rows(cuda_device):
    """A 64-channel 3x3 at 32 x 64 under HKP_TILE_160_A3 runs the halo-tile body, which
    writes 128-row partials: the layout query says so, the list has ceil(M / 128)
    tiles, and it finalizes to the statistics of y."""
    from hkp import ops
    from hkp._lib import HKP_KOP_FWD_X3, HKP_TILE_160_A3, ConvDesc
    n, h, w, cin, cout = 1, 32, 64, 64, 64
    d = cuda_device
    g = torch.Generator(device=d).manual_seed(50)
    x = torch.relu(torch.randn(n, h, w, cin, device=d, generator=g))
    wt = torch.randn(cout, 3, 3, cin, device=d, generator=g) * (2.0 / (9 * cout)) ** 0.5
    ss = torch.cat([torch.ones(cin, device=d), torch.zeros(cin, device=d)])
    xs = ops.bn_apply(x, ss, relu=False, split=3, keep_fp32=False)
    wp = ops.weight_pack_x3(wt)
    desc = ConvDesc(n, h, w, cin, cout, 3, 3, 1, 1, 1, 0, HKP_TILE_160_A3)
    assert ops.kernel_name(desc, HKP_KOP_FWD_X3) == "conv_x3_halo_kernel<3>"
    y, p = ops.conv2d_fwd_x3(xs, wp, 1, 1, 1, tile=HKP_TILE_160_A3)
    y0, p0 = ops.conv2d_fwd_x3(xs, wp, 1, 1, 1, tile=0)
    m = n * h * w
    assert p.shape == (m // 128, cout, 2) and ops.stat_tile_rows(p) == 128
    assert torch.equal(y, y0) and torch.equal(p, p0)
    mi = _bn_stats(p, m)
    yd = y.reshape(m, cout).double()
    want = torch.cat([yd.mean(0), (yd.var(0, unbiased=False) + 1e-5).rsqrt()])
    assert torch.allclose(mi.double(), want, rtol=1e-6, atol=1e-7)
