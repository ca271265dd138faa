"""CPU restatements of the BatchNorm family (csrc/bn.hip, csrc/bn_bwd.hip), the stem
pool and absmax — shared by test_bn_ref_cpu.py and test_gpu_bn.py.  numpy / torch
CPU only; nothing here touches a GPU.

Two kinds of restatement:

* bit-exact fp32, torch CPU ops in the kernel's order, one rounding per op (eager
  torch never contracts a*b + c across two ops): apply, apply_f16, split, ss_from_mi,
  bwd_apply, maxpool, maxpool_bwd.  The kernels must give these bits.
* float64: finalize, eval_params, bwd_tile_sums, bwd_coef.  The kernels merge in
  float64 in another order (or sum in fp32), so they are compared to a stated bound.

The ReLU everywhere is this project's `o > 0 ? o : 0`: NaN gives 0 (torch.relu keeps
it), and the pool's `t > m` never lets a NaN win.
"""
import math

import numpy as np
import torch

f32, f64 = np.float32, np.float64
BWD_TILE = 64          # rows per reduction tile of hkp_bn_bwd_reduce


def rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def ordered(x):
    """fp32 -> int64 that orders like the floats (+0 and -0 both 0): ulp distances."""
    i = x.contiguous().view(torch.int32).long()
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def ulp_diff(a, b):
    """Largest distance in fp32 ulps between two fp32 tensors, and how many differ."""
    d = (ordered(a) - ordered(b)).abs()
    return int(d.max()), int((d > 0).sum())


def relu_rule(o):
    """o > 0 ? o : 0 — NaN and -0.0 give +0."""
    return torch.where(o > 0, o, torch.zeros_like(o))


# ---------------------------------------------------------------- forward ----

def split(o, passes):
    """store_split4: hi = f16(o), lo = f16(o - hi).  passes 1 -> hi [.., C];
    passes 3 -> packed [.., C/32, (hi32 | lo32)] flattened to [.., 2C]."""
    hi = o.half()
    if passes == 1:
        return hi
    lo = (o - hi.float()).half()
    c = o.shape[-1]
    assert passes == 3 and c % 32 == 0
    lead = tuple(o.shape[:-1])
    return torch.cat([hi.reshape(lead + (c // 32, 32)), lo.reshape(lead + (c // 32, 32))], -1).reshape(lead + (2 * c,))


def unsplit(packed):
    """(hi, lo) fp16 [.., C] of a packed split [.., 2C]."""
    lead, c = tuple(packed.shape[:-1]), packed.shape[-1] // 2
    p = packed.reshape(lead + (c // 32, 64))
    return p[..., :32].reshape(lead + (c,)), p[..., 32:].reshape(lead + (c,))


def apply(y, ss, res=None, res_ss=None, res_split=None, relu=True):
    """bn_apply_kernel: o = y*sc + sh (two roundings), then o += res | (res*rsc + rsh) |
    (hi + lo), then the ReLU rule."""
    c = y.shape[-1]
    o = y * ss[:c] + ss[c:]
    if res_split is not None:
        hi, lo = unsplit(res_split)
        o = o + (hi.float() + lo.float())
    elif res is not None and res_ss is not None:
        o = o + (res * res_ss[:c] + res_ss[c:])
    elif res is not None:
        o = o + res
    return relu_rule(o) if relu else o


def apply_f16(y16, ss, res=None, res_ss=None, relu=True):
    """bn_apply_f16_kernel: the same on y16.float() -> (fp16 result, fp32 copy)."""
    o = apply(y16.float(), ss, None if res is None else res.float(), res_ss, None, relu)
    return o.half(), o


def ss_from_mi(mi, gamma, beta):
    """bn_fin_store / bn_eval_kernel's fp32 tail: alpha = inv*g, shift = b - mean*alpha."""
    c = mi.numel() // 2
    mean, inv = mi[:c], mi[c:]
    alpha = inv * (gamma if gamma is not None else torch.ones(c))
    shift = (beta if beta is not None else torch.zeros(c)) - mean * alpha
    return torch.cat([alpha, shift])


def finalize(part, count, tile_rows, gamma, beta, momentum=0.1, eps=1e-5, rm=None, rv=None):
    """hkp_bn_finalize in float64 from fp32 partials [T, C, 2] = (sum, M2 about the
    tile mean) of tiles of tile_rows rows (the last one ragged).  Returns a dict:
    mean, m2 (float64), mi, ss (fp32 torch), rm, rv (fp32 torch or None)."""
    p = part.numpy().astype(f64)
    tiles, c, _ = p.shape
    n_t = np.minimum(tile_rows, count - np.arange(tiles, dtype=np.int64) * tile_rows).astype(f64)[:, None]
    assert n_t.min() >= 1
    s, q = p[:, :, 0], p[:, :, 1]
    mean = s.sum(0) / f64(count)
    m2 = (q + n_t * (s / n_t - mean[None, :]) ** 2).sum(0)
    var = m2 / f64(count)
    inv = 1.0 / np.sqrt(var + f64(f32(eps)))
    mi = torch.from_numpy(np.concatenate([mean.astype(f32), inv.astype(f32)]))
    out = dict(mean=mean, m2=m2, mi=mi, ss=ss_from_mi(mi, gamma, beta), rm=None, rv=None)
    if rm is not None:
        mom = f64(f32(momentum))
        unbiased = m2 / f64(count - 1) if count > 1 else var
        out["rm"] = torch.from_numpy((mom * mean + (1.0 - mom) * rm.numpy().astype(f64)).astype(f32))
        out["rv"] = torch.from_numpy((mom * unbiased + (1.0 - mom) * rv.numpy().astype(f64)).astype(f32))
    return out


def eval_params(gamma, beta, rm, rv, eps=1e-5):
    """hkp_bn_eval_params -> (ss, mi): inv = f32(1/sqrt(f64(rv) + f64(f32(eps))))."""
    inv = (1.0 / np.sqrt(rv.numpy().astype(f64) + f64(f32(eps)))).astype(f32)
    mi = torch.cat([rm, torch.from_numpy(inv)])
    return ss_from_mi(mi, gamma, beta), mi


# --------------------------------------------------------------- backward ----

def relu_mask(mask, y):
    """The two mask forms: an activation [M, C] (out > 0), or the forward's [2C]
    scale|shift (fl(fl(y*scale) + shift) > 0, fp32)."""
    c = y.shape[-1]
    if mask.dim() == 1:
        return (y * mask[:c] + mask[c:]) > 0
    return mask > 0


def bwd_tile_sums(g, mask, y, mean):
    """hkp_bn_bwd_reduce per 64-row tile and channel.  g, y [M, C] fp32; mask None,
    an activation or a scale|shift vector; mean [C] fp32.  Returns dz (fp32 torch),
    sums [T, C, 2] = (sum dz, sum dz*(y-mean)) and abs [T, C, 2] (the same of absolute
    values) in float64, maxima [T, C, 2] = (max|dz|, max|y-mean|) in fp32."""
    m, c = y.shape
    dz = g if mask is None else torch.where(relu_mask(mask, y), g, torch.zeros_like(g))
    ym = y - mean                                   # one fp32 subtraction
    tiles = (m + BWD_TILE - 1) // BWD_TILE
    pad = tiles * BWD_TILE - m

    def tiled(t):
        t = t.numpy()
        return np.concatenate([t, np.zeros((pad, c), t.dtype)]).reshape(tiles, BWD_TILE, c)

    d, v = tiled(dz), tiled(ym)
    d64, p64 = d.astype(f64), d.astype(f64) * v.astype(f64)
    sums = np.stack([d64.sum(1), p64.sum(1)], -1)
    sabs = np.stack([np.abs(d64).sum(1), np.abs(p64).sum(1)], -1)
    maxima = np.stack([np.abs(d).max(1), np.abs(v).max(1)], -1)
    return dz, sums, sabs, torch.from_numpy(maxima)


def bwd_bound(coef, md, mv):
    """bn_bwd_finalize_kernel's bound word: max_c f32((md + |cg| + mv*|ck|)*|cs|*1.0001)
    in float64 on the fp32 coefficients; md, mv float64 [C]."""
    c = coef.numel() // 3
    k = coef.numpy().astype(f64)
    cg, ck, cs = k[:c], k[c:2 * c], k[2 * c:]
    return f32(((md + np.abs(cg) + mv * np.abs(ck)) * np.abs(cs) * 1.0001).astype(f32).max())


def bwd_coef(part, maxima, m, mi, gamma):
    """hkp_bn_bwd_finalize in float64 from fp32 partials [T, C, 2] (and maxima or
    None).  Returns dict: dgamma, dbeta, coef [3C] (fp32 torch), bound (np.float32 or
    None), slack (float64 [5, C]: tiles*2^-53*sum|partial| carried to dbeta, dgamma,
    cg, ck, cs), md, mv (float64 [C] or None)."""
    p = part.numpy().astype(f64)
    tiles, c, _ = p.shape
    S, D = p[:, :, 0].sum(0), p[:, :, 1].sum(0)
    inv = mi[c:].numpy().astype(f64)
    gm = gamma.numpy().astype(f64) if gamma is not None else np.ones(c)
    dgamma, dbeta = (D * inv).astype(f32), S.astype(f32)
    cg, ck, cs = (S / f64(m)).astype(f32), (D * inv * inv / f64(m)).astype(f32), (inv * gm).astype(f32)
    coef = torch.from_numpy(np.concatenate([cg, ck, cs]))
    e = tiles * 2.0 ** -53
    aS, aD = np.abs(p[:, :, 0]).sum(0) * e, np.abs(p[:, :, 1]).sum(0) * e
    slack = np.stack([aS, aD * inv, aS / m, aD * inv * inv / m, np.zeros(c)])
    out = dict(dgamma=torch.from_numpy(dgamma), dbeta=torch.from_numpy(dbeta), coef=coef, slack=slack, bound=None,
               md=None, mv=None)
    if maxima is not None:
        x = maxima.numpy().astype(f64)
        out["md"], out["mv"] = x[:, :, 0].max(0), x[:, :, 1].max(0)
        out["bound"] = bwd_bound(coef, out["md"], out["mv"])
    return out


def bwd_apply(dz, y, mean, coef):
    """bn_bwd_apply_kernel: ((dz - gm) - (y - mean)*k)*sc, five fp32 roundings."""
    c = y.shape[-1]
    return ((dz - coef[:c]) - (y - mean) * coef[c:2 * c]) * coef[2 * c:]


def pow2_scale(bound):
    """pow2_scale_for: 2^e with bound*2^e in [2^13, 2^14); 1 for 0, inf or NaN."""
    b = float(bound)
    if not (b > 0.0) or not (b < math.inf):
        return 1.0
    e = 14 - math.frexp(b)[1]
    return math.ldexp(1.0, max(-100, min(100, e)))


# ------------------------------------------------------------------- pool ----

def maxpool(y, ss):
    """hkp_bn_relu_maxpool on NHWC y: max over the 3x3/s2/p1 window of
    relu(y*a + b) by the kernel's scan (first maximum in (dr, ds) order wins, a NaN
    never does; equal to F.max_pool2d for NaN-free input) -> (out, route uint8):
    route = dr*3 + ds of the maximum, 255 where the maximum is not > 0."""
    n, h, w, c = y.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    t = torch.full((n, h + 2, w + 2, c), -math.inf)
    t[:, 1:h + 1, 1:w + 1] = relu_rule(y * ss[:c] + ss[c:])
    m = torch.full((n, ho, wo, c), -math.inf)
    tap = torch.zeros((n, ho, wo, c), dtype=torch.uint8)
    for dr in range(3):
        for ds in range(3):
            v = t[:, dr:dr + 2 * ho:2, ds:ds + 2 * wo:2]
            win = v > m
            m = torch.where(win, v, m)
            tap[win] = dr * 3 + ds
    return m, torch.where(m > 0, tap, torch.full_like(tap, 255))


def maxpool_bwd(dpool, route, shape):
    """hkp_maxpool_bwd: every input pixel sums, in fp32, dpool of the (<= 4) windows
    routed to it, in window order (ho, wo) ascending — for one pixel that is the tap
    order dr descending, then ds descending."""
    n, h, w, c = shape
    ho, wo = dpool.shape[1:3]
    dz = torch.zeros((n, h + 2, w + 2, c))
    zero = torch.zeros_like(dpool)
    for dr in (2, 1, 0):
        for ds in (2, 1, 0):
            dz[:, dr:dr + 2 * ho:2, ds:ds + 2 * wo:2] += torch.where(route == dr * 3 + ds, dpool, zero)
    return dz[:, 1:h + 1, 1:w + 1].contiguous()
