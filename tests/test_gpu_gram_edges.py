"""The Gram BN path (hkp_gram_f16 -> hkp_bn_from_gram -> hkp_conv2d_fwd_f16_bn) at
its dispatch edges, bit for bit.

On small-integer activations and weights every stage is exact (tests/_gram_ref.py),
so a wrong index, mask, tile decode or split bound changes bits:

* hkp_gram_f16 == the integer moments at every branch of gram_plan (both tile
  widths with off-diagonal tiles, up to 136 tiles, both reduce variants, the
  16384-row cap, fewer rows than one K-step, ragged and exact last splits), with NaN
  rows on both sides of the activation;
* hkp_bn_from_gram from hand-built dyadic moments and a hand-built packed weight
  (masked columns, a partial column block, K % 16 != 0, count 1, the variance clamp);
* the chain on one integer activation, tied to the statistics of the conv's output;
* hkp_conv2d_fwd_f16_bn == the exact conv -> fp16 -> tests/_bn_ref.apply_f16, for
  the Bottleneck channel pairs, every tile policy, relu on and off;
* one real-valued case at mean / spread = 80 against the a-priori fp32 bound.
"""
import time

import numpy as np
import pytest
import torch

import _bn_ref
import _gram_ref as ref
from _gram_ref import f32, f64
from test_gpu_precision import LIVE_TILES

pytestmark = pytest.mark.gpu

GUARD = 64                                    # NaN rows on each side: 64 * C * 2 bytes keeps the base 128-B aligned
INV_EPS = f32(1.0 / np.sqrt(f64(f32(1e-5))))  # invstd of a zero variance


def _guarded(m, c, seed, dev):
    """An integer activation as rows [GUARD, GUARD + m) of a buffer whose other rows
    are NaN: a read past either end turns a sum into NaN."""
    buf = torch.full((m + 2 * GUARD, c), float("nan"), device=dev, dtype=torch.float16)
    a = buf[GUARD:GUARD + m]
    a.copy_(ref.int_activation(m, c, seed, device=dev))
    assert a.is_contiguous() and a.data_ptr() % 128 == 0
    return buf, a


# ------------------------------------------------------------ hkp_gram_f16 ----

def test_plan_matches_workspace_bytes(cuda_device):
    from hkp._lib import lib
    for m, c in ref.GRAM_SHAPES + [(4096, 64), (198, 128), (768, 256), (300, 512), (30000, 256)]:
        assert lib().hkp_gram_f16_workspace_bytes(m, c) == ref.plan(m, c).ws_bytes, (m, c)


@pytest.mark.parametrize("m,c", ref.GRAM_SHAPES)
def test_gram_int_exact(cuda_device, m, c):
    """mean and E of an integer activation equal colsum / m and a^T a / m (exact
    integer sums, one fp64 division) in every bit; E is symmetric; two runs agree.
    The reference is computed on the CPU, for the 192 MB case on the GPU in fp64 row
    chunks (exact either way).  (49153, 2048) is the longest case: 0.24 s measured,
    reference included."""
    from hkp import ops
    t0 = time.time()
    buf, a = _guarded(m, c, 1000 + m + c, cuda_device)
    mean, e2 = ops.gram_f16(a)
    big = m * c > 1 << 24
    mu_ref, e_ref = ref.gram_exact(a if big else a.cpu())
    mean_c, e2_c = (mean, e2) if big else (mean.cpu(), e2.cpu())
    assert not torch.isnan(mean_c).any() and not torch.isnan(e2_c).any()
    bad = (e2_c != e_ref).nonzero()
    assert bad.numel() == 0, "E differs at %d entries, first (i, j) %s; plan %s" % (
        bad.shape[0], bad[:4].tolist(), ref.plan(m, c))
    assert torch.equal(mean_c, mu_ref), (mean_c != mu_ref).nonzero()[:8].flatten().tolist()
    assert torch.equal(e2, e2.T)
    mean2, e22 = ops.gram_f16(a)
    assert torch.equal(mean, mean2) and torch.equal(e2, e22)
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + m:]).all()
    torch.cuda.synchronize()
    print("gram (%d, %d): %.2f s" % (m, c, time.time() - t0))


# -------------------------------------------------------- hkp_bn_from_gram ----

def _affine(k, seed):
    gamma, beta = _bn_ref.rand(k, seed=seed) * 0.3 + 1, _bn_ref.rand(k, seed=seed + 1)
    rm, rv = _bn_ref.rand(k, seed=seed + 2), _bn_ref.rand(k, seed=seed + 3).abs() + 0.5
    return gamma, beta, rm, rv


def _check_stats(k, ss, mi, rm, rv, want, gamma, beta, tag, inv_ulps):
    """The assertions every bn_from_gram comparison makes (arguments on the CPU):
    mean, scale/shift and running_mean in every bit, invstd to inv_ulps fp32 ulps,
    running_var to 1."""
    assert torch.equal(mi[:k], want["mi"][:k]), (tag, "mean", _bn_ref.ulp_diff(mi[:k], want["mi"][:k]))
    ulps, n = _bn_ref.ulp_diff(mi[k:], want["mi"][k:])
    assert ulps <= inv_ulps, (tag, "invstd", ulps, n)
    assert torch.equal(ss, _bn_ref.ss_from_mi(mi, gamma, beta)), (tag, "ss")
    if rm is not None:
        assert torch.equal(rm, want["rm"]), (tag, "running_mean", _bn_ref.ulp_diff(rm, want["rm"]))
        ulps_v, _ = _bn_ref.ulp_diff(rv, want["rv"])
        assert ulps_v <= 1, (tag, "running_var", ulps_v)
    return ulps


def _run_bn_from_gram(dev, mu, E, wp, count, gamma, beta, rm, rv):
    from hkp import ops
    to = lambda t: None if t is None else t.clone().to(dev)
    g, b, rm_d, rv_d = to(gamma), to(beta), to(rm), to(rv)
    nbt = torch.full((1,), 5, device=dev, dtype=torch.int64)
    ss, mi = ops.bn_from_gram(mu, E, wp, count, g, b, rm_d, rv_d, nbt)
    assert nbt.item() == 6                                   # incremented exactly once
    back = lambda t: None if t is None else t.cpu()
    return ss.cpu(), mi.cpu(), back(rm_d), back(rv_d)


@pytest.mark.parametrize("k", [16, 72, 256])
@pytest.mark.parametrize("c", [64, 192, 256, 320, 1024, 2048])
def test_bn_from_gram_dyadic(cuda_device, c, k):
    """Moments built by hand from a 64-row integer matrix (mu = colsum / 64,
    E = A^T A / 64, one entry lowered by 2^-10) and a hand-built PackedWeight (fp16
    integers in [-4, 4], inverse scales 2^-3 .. 2^-14 by channel): all dyadic, so every
    fp64 product and sum of the two kernels is exact in any order — per channel the
    terms of q = w^T E w are integers times one power of two, their magnitudes sum
    to at most C^2 * 16 * 9 * 2^10 < 2^53.  mean, scale/shift and running_mean must
    match in every bit, and running_var to 1 fp32 ulp (numpy's fp64 sqrt and division
    are the reference's, the device's are not pinned by this project).  invstd was
    allowed 1 ulp for the same reason, measured bit-equal on the MI355X at every case,
    and is therefore asserted equal.
    Channel 0 has variance exactly 0, channel 1's is negative before the clamp,
    channel 2's weight row is all zero."""
    from hkp import ops
    d = cuda_device
    a = ref.int_activation(64, c, seed=c)
    a[:, 0], a[:, 1] = 2, 3
    mu, E = ref.gram_exact(a)
    E[1, 1] -= 2.0 ** -10
    assert c <= 2048 and E.max() <= 9 and torch.equal(E * 1024, (E * 1024).floor())
    assert c * c * 16 * 9 * 1024 < 2 ** 53
    g = torch.Generator().manual_seed(100 + k)
    w16 = torch.randint(-4, 5, (k, 1, 1, c), generator=g).half()
    w16[0], w16[1], w16[2] = 0, 0, 0
    w16[0, 0, 0, 0], w16[1, 0, 0, 1] = 3, -2
    inv = torch.tensor([2.0 ** -(3 + i % 12) for i in range(k)], dtype=torch.float32)
    wp = ops.PackedWeight(w16.to(d), inv.to(d))
    mu_d, E_d = mu.to(d), E.to(d)
    gamma, beta, rm, rv = _affine(k, 7)
    worst = 0
    for count in (64, 1, 38400):
        for affine in (True, False):
            for running in (True, False):
                gm, bt = (gamma, beta) if affine else (None, None)
                r_m, r_v = (rm, rv) if running else (None, None)
                want = ref.bn_from_gram_exact(mu, E, w16, inv, count, gm, bt, 0.1, 1e-5, r_m, r_v)
                ss, mi, rm2, rv2 = _run_bn_from_gram(d, mu_d, E_d, wp, count, gm, bt, r_m, r_v)
                worst = max(worst, _check_stats(k, ss, mi, rm2, rv2, want, gm, bt, (c, k, count, affine, running), 0))
                # the clamp: variance 0, negative, and an all-zero row
                assert want["var"][0] == 0 and want["var"][1] == 0 and want["var"][2] == 0
                assert (mi[k:k + 3].numpy() == INV_EPS).all(), mi[k:k + 3]
                assert mi[2] == 0 and mi[0] == 6 * 2.0 ** -3 and mi[1] == -6 * 2.0 ** -4
                assert torch.isfinite(ss).all() and torch.isfinite(mi).all()
                if running and count == 1:                   # the unbiased fallback: var itself
                    assert rv2[2] == f32((1.0 - f64(f32(0.1))) * f64(rv[2].item()))
    print("bn_from_gram C=%d K=%d: invstd worst %d ulp" % (c, k, worst))


# ------------------------------------------------------------------ chain ----

CHAIN = [((1, 64, 64), 64, 256), ((2, 9, 11), 128, 512), ((2, 16, 24), 256, 1024), ((1, 15, 20), 512, 2048)]


def _packed_int_weight(k, c, seed, dev):
    """weight_pack_f16 of an integer weight: its power-of-two scaling keeps the
    integers exact (asserted)."""
    from hkp import ops
    w = ref.int_weight(k, c, seed)
    wp = ops.weight_pack_f16(w.to(dev))
    assert torch.equal(wp.split.float() * wp.inv_scale[:, None, None, None], w.to(dev))
    return w, wp


@pytest.mark.parametrize("nhw,c,k", CHAIN)
def test_chain_int_exact(cuda_device, nhw, c, k):
    """gram_f16 -> bn_from_gram on an integer activation against bn_from_gram_exact
    of gram_exact, with test_bn_from_gram_dyadic's assertions, and against the fp64
    population statistics of the conv's own (exact, integer) output.

    m = 4096 keeps every value dyadic: exact throughout.  For m = 198, 768, 300 the
    column sums and a^T a are exact integers on both sides (fp32 below 2^24 inside a
    split, fp64 across splits) and both sides divide them by m in fp64 once, so mu and
    E are the same bits.  The fp64 dot products over them then round (about C * 2^-53
    relative) in the kernel's order and in numpy's; the difference vanishes in the cast
    to fp32 unless a mean sits that close to the midpoint of two fp32 values.  An exact
    tie cannot occur: mean_k * 2^e is N / m with |N| <= 768 m, and a value of that form
    that is dyadic needs far fewer than 25 bits.  The fixed seeds are not within
    1e-12 of one either, so the mean is asserted bit-equal for every case.  invstd:
    equal at m = 4096, 1 fp32 ulp where the dot products round."""
    from hkp import ops
    d = cuda_device
    n, h, wd_ = nhw
    m = n * h * wd_
    a = ref.int_activation(m, c, 31 + m, device=d)
    w, wp = _packed_int_weight(k, c, 17 + k, d)
    gamma, beta, rm, rv = _affine(k, 23)
    mean, e2 = ops.gram_f16(a)
    mu_ref, e_ref = ref.gram_exact(a.cpu())
    assert torch.equal(mean.cpu(), mu_ref) and torch.equal(e2.cpu(), e_ref)
    want = ref.bn_from_gram_exact(mu_ref, e_ref, wp.split.cpu(), wp.inv_scale.cpu(), m, gamma, beta, 0.1, 1e-5, rm, rv)
    ss, mi, rm2, rv2 = _run_bn_from_gram(d, mean, e2, wp, m, gamma, beta, rm, rv)
    _check_stats(k, ss, mi, rm2, rv2, want, gamma, beta, (m, c, k), 0 if m == 4096 else 1)
    # the thing the algebra replaces: the statistics of the conv's output
    x = a.reshape(n, h, wd_, c)
    x._hkp_split_passes = 1
    y, _ = ops.conv2d_fwd_f16(x, wp)
    y64 = y.reshape(m, k).double().cpu()
    exact = a.double().cpu() @ w.reshape(k, c).double().T
    assert exact.abs().max() <= 2048 and torch.equal(y64, exact)
    mean_y, var_y = y64.sum(0) / m, y64.var(0, unbiased=False)     # an exact integer sum, one division
    assert torch.equal(mi[:k], mean_y.float()), _bn_ref.ulp_diff(mi[:k], mean_y.float())
    inv_y = (1.0 / torch.sqrt(var_y + float(f32(1e-5)))).float()
    assert _bn_ref.ulp_diff(mi[k:], inv_y)[0] <= 1, _bn_ref.ulp_diff(mi[k:], inv_y)


# -------------------------------------------------- hkp_conv2d_fwd_f16_bn ----

PAIRS = [(64, 256), (128, 512), (256, 1024), (512, 2048)]
SHAPES = [(1, 3, 5), (2, 9, 11), (2, 16, 24)]          # M = 15 (below any tile), 198 (ragged), 768 = 3 * 256


def _kernel(n, h, w, c, k, tile, sk):
    from hkp import ops
    from hkp._lib import HKP_KOP_FWD_F16, HKP_LAYOUT_NHWC, ConvDesc
    return ops.kernel_name(ConvDesc(n, h, w, c, k, 1, 1, 1, 0, 1, HKP_LAYOUT_NHWC, tile), HKP_KOP_FWD_F16, sk)


def _real_ss(k, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.rand(k, generator=g) + 0.5, torch.rand(k, generator=g) - 0.5])


@pytest.mark.parametrize("nhw", SHAPES)
@pytest.mark.parametrize("c,k", PAIRS)
def test_fused_epilogue_vs_exact_conv(cuda_device, c, k, nhw):
    """The fused output equals fused_apply_ref of the exact integer conv result in
    every fp16 bit: residual none / raw / scaled, relu on and off, the planner's tile
    and every live tile policy, stream-K workspace given and withheld."""
    from hkp import ops
    from hkp._lib import HkpError
    d = cuda_device
    n, h, wd_ = nhw
    m = n * h * wd_
    a = ref.int_activation(m, c, 57 + m + c)
    w, wp = _packed_int_weight(k, c, 71 + k, d)
    exact = a.double() @ w.reshape(k, c).double().T
    assert exact.abs().max() <= 2048
    exact = exact.reshape(n, h, wd_, k)
    ss, rss = _real_ss(k, 3), _real_ss(k, 4)
    res = (_bn_ref.rand(n, h, wd_, k, seed=5)).half()
    x = a.reshape(n, h, wd_, c).to(d)
    x._hkp_split_passes = 1
    ss_d, rss_d, res_d = ss.to(d), rss.to(d), res.to(d)
    launched = skipped = 0
    names = set()
    for res_kind in ("none", "raw", "scaled"):
        r_c, rs_c = (None, None) if res_kind == "none" else (res, None) if res_kind == "raw" else (res, rss)
        r_d, rs_d = (None, None) if res_kind == "none" else (res_d, None) if res_kind == "raw" else (res_d, rss_d)
        for relu in (True, False):
            want = ref.fused_apply_ref(exact, ss, r_c, rs_c, relu).to(d)
            for tile in (0,) + tuple(LIVE_TILES):
                for sk in (True, False):
                    try:
                        names.add((tile, sk, _kernel(n, h, wd_, c, k, tile, sk)))
                    except HkpError:                         # the library rejects this policy for the shape
                        skipped += 1
                        continue
                    got = ops.conv2d_fwd_f16_bn(x, wp, ss_d, res=r_d, res_ss=rs_d, relu=relu, tile=tile, sk=sk)
                    launched += 1
                    assert got.dtype == torch.float16 and got.shape == want.shape
                    if not torch.equal(got, want):
                        bad = (got != want).nonzero()
                        raise AssertionError("C=%d K=%d M=%d res=%s relu=%s tile=%d sk=%s (%s): %d wrong, first %s" % (
                            c, k, m, res_kind, relu, tile, sk, _kernel(n, h, wd_, c, k, tile, sk), bad.shape[0],
                            bad[:4].tolist()))
    bodies = sorted({nm for _, _, nm in names})
    print("fused C=%d K=%d M=%d: %d launches, %d policies rejected, %d bodies: %s" % (
        c, k, m, launched, skipped, len(bodies), ", ".join(bodies)))
    assert launched > 0 and launched + skipped == 6 * 2 * (1 + len(LIVE_TILES))


def test_fused_auto_policy_reaches_several_bodies(cuda_device):
    """The planner's own choice (tile = 0) over the table is not one body."""
    seen = {}
    for c, k in PAIRS:
        for n, h, w in SHAPES:
            seen[(c, k, n * h * w)] = _kernel(n, h, w, c, k, 0, True)
    bodies = sorted(set(seen.values()))
    print("tile=0 bodies over the table: %s" % ", ".join(bodies))
    for key, nm in sorted(seen.items()):
        print("  C=%d K=%d M=%d -> %s" % (key + (nm,)))
    assert len(bodies) > 1, bodies


@pytest.mark.parametrize("relu", [True, False])
def test_fused_epilogue_nan_rule(cuda_device, relu):
    """A NaN shift in one channel: `o > 0 ? o : 0` gives 0 with the ReLU and NaN
    without, as _bn_ref.relu_rule."""
    from hkp import ops
    d = cuda_device
    (n, h, wd_), c, k = (2, 9, 11), 64, 256
    m = n * h * wd_
    a = ref.int_activation(m, c, 5)
    w, wp = _packed_int_weight(k, c, 6, d)
    exact = (a.double() @ w.reshape(k, c).double().T).reshape(n, h, wd_, k)
    ss = _real_ss(k, 8)
    ss[k + 5] = float("nan")
    res = _bn_ref.rand(n, h, wd_, k, seed=9).half()
    want = ref.fused_apply_ref(exact, ss, res, None, relu)
    x = a.reshape(n, h, wd_, c).to(d)
    x._hkp_split_passes = 1
    got = ops.conv2d_fwd_f16_bn(x, wp, ss.to(d), res=res.to(d), relu=relu).cpu()
    assert ref.same_bits_f16(got, want)
    col = got[..., 5]
    assert (col == 0).all() if relu else col.isnan().all()
    assert not got[..., :5].isnan().any() and not got[..., 6:].isnan().any()


# ------------------------------------------------------- real-valued case ----

def test_gram_variance_at_high_mean_to_spread(cuda_device):
    """m = 30000, C = 256, K = 1024, activations 4 + 0.05 randn (fp16), weights
    randn * sqrt(2 / C): the variance from the Gram route against the fp64 variance
    of the fp64 product of the same fp16 operands.  E carries the fp32 rounding of
    its in-split accumulation, rows - 1 additions of at most 2^-23 relative each (the
    MFMA's rounding mode is not documented, hence not 2^-24), so
        |var - var64| <= (rows - 1) * 2^-23 * sum_ij |w_i| |w_j| E_ij
    with rows from plan() and the right side in fp64 from the reference's E.  That is
    the assertion; nothing tighter is claimed.  Measured on an MI355X, worst channel:
    |var - var64| / var64 = 1.9e-4 on the Gram route (8e-6 of the bound, which is 27
    times var64 here) and 5.5e-7 on the unfused route ("Gram statistics")."""
    from hkp import ops
    d = cuda_device
    n, h, wd_, c, k = 1, 150, 200, 256, 1024
    m = n * h * wd_
    rows = ref.plan(m, c).rows
    assert rows == 192
    g = torch.Generator(device=d).manual_seed(77)
    x = (4 + 0.05 * torch.randn(n, h, wd_, c, device=d, generator=g)).half()
    x._hkp_split_passes = 1
    wt = torch.randn(k, 1, 1, c, device=d, generator=g) * (2.0 / c) ** 0.5
    wp = ops.weight_pack_f16(wt)
    a = x.reshape(m, c)
    w64 = wp.split.double().reshape(k, c) * wp.inv_scale.double()[:, None]
    y64 = a.double() @ w64.T
    var64 = y64.var(0, unbiased=False)
    mu_ref, e_ref = ref.gram_exact(a)
    bound = (rows - 1) * 2.0 ** -23 * ((w64.abs() @ e_ref) * w64.abs()).sum(1)
    mean, e2 = ops.gram_f16(a)
    # the Gram route's variance in fp64 from the kernel's own moments (this evaluation's
    # rounding, 1e-16 of the bound's sum, is twelve orders below the bound)
    var_g = ((w64 @ e2) * w64).sum(1) - (w64 @ mean) ** 2
    err_g = (var_g - var64).abs()
    assert (err_g <= bound).all(), (err_g / bound).max().item()
    # the same through hkp_bn_from_gram: var = 1 / invstd^2 - eps, invstd rounded to fp32
    # (2^-24 relative, so 2^-23 of var + eps; 2^-22 allowed)
    eps = float(f32(1e-5))
    _, mi = ops.bn_from_gram(mean, e2, wp, m, None, None)
    var_b = 1.0 / mi[k:].double() ** 2 - eps
    err_b = (var_b - var64).abs()
    assert (err_b <= bound + 2.0 ** -22 * (var64 + eps)).all()
    # the unfused route, for the record: conv tile partials -> bn_finalize
    _, part = ops.conv2d_fwd_f16(x, wp)
    _, mi_u = ops.bn_finalize(part, m, None, None)
    var_u = 1.0 / mi_u[k:].double() ** 2 - eps
    err_u = (var_u - var64).abs()
    print("high mean/spread (m=%d C=%d K=%d, rows %d): |var - var64| / var64 worst channel: gram (fp64 of E) %.3g, "
          "gram (bn_from_gram) %.3g, unfused (partials -> bn_finalize) %.3g; median %.3g / %.3g / %.3g; "
          "bound / var64 worst %.3g, err / bound worst %.3g"
          % (m, c, k, rows, (err_g / var64).max().item(), (err_b / var64).max().item(), (err_u / var64).max().item(),
             (err_g / var64).median().item(), (err_b / var64).median().item(), (err_u / var64).median().item(),
             (bound / var64).max().item(), (err_g / bound).max().item()))
