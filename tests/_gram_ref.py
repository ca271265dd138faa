"""Plain references of the Gram BN path (csrc/gram.hip and the fused BN-apply
epilogue of csrc/conv_x3.hip and csrc/x3_duo.h) — shared by test_gram_ref_cpu.py and
test_gpu_gram_edges.py.  numpy / torch only; nothing here imports hkp.

The path is exact on small integers: fp16 holds them, their products are exact,
fp32 MFMA accumulation of integers is exact in any order while the sums stay below
2^24, and the fp64 stages are exact far beyond that.  With integer activations
every kernel of the family must therefore reproduce these references bit for bit.
"""
import collections

import numpy as np
import torch

import _bn_ref

f32, f64 = np.float32, np.float64

MAX_SPLIT_ROWS = 16384       # gram_plan's cap on the rows of one split
ACT_MAX = 3                  # int_activation draws from {0 .. ACT_MAX}

Plan = collections.namedtuple("Plan", "tc nb tiles rows splits variant last ws_bytes")


def plan(m, c):
    """gram_plan (csrc/gram.hip) restated: tile width, channel blocks, upper-triangle
    tiles, rows per split (a multiple of 32, at most 16384), splits, the reduce
    variant (gram_reduce_kernel<4> from 64 splits on, else <1>), the rows of the last
    split and hkp_gram_f16_workspace_bytes."""
    assert m > 0 and c > 0 and c % 64 == 0
    tc = 128 if c % 128 == 0 else 64
    nb = c // tc
    tiles = nb * (nb + 1) // 2
    sp = max(1, 512 // tiles)
    rows = min((m + sp - 1) // sp, MAX_SPLIT_ROWS)
    rows = (rows + 31) // 32 * 32
    splits = (m + rows - 1) // rows
    ws = splits * tiles * tc * tc * 4 + splits * nb * tc * 4 + 256
    return Plan(tc, nb, tiles, rows, splits, 4 if splits >= 64 else 1, m - (splits - 1) * rows, ws)


def tile_of(t, nb):
    """gram_tile: upper-triangle tile t -> (ib, jb), ib <= jb, row-major."""
    i = 0
    while t >= nb - i:
        t -= nb - i
        i += 1
    return i, i + t


# (m, C) of hkp_gram_f16 and the branch each shape is there for
GRAM_SHAPES = [
    (1, 64), (31, 64), (32, 64), (33, 64),     # below / at / past one 32-row K-step; 33: a second split of 1 row
    (2016, 64), (2017, 64),                    # 63 splits -> reduce<1>, 64 -> reduce<4>, TC = 64
    (2048, 64),                                # 64 full splits, no ragged tail
    (97, 320),                                 # TC = 64, nb = 5: off-diagonal 64-wide tiles, last split of 1 row
    (2700, 192),                               # TC = 64, nb = 3, reduce<4> over several tiles
    (2700, 384),                               # TC = 128, nb = 3, reduce<4>
    (300, 1024),                               # nb = 8, 36 tiles (the model's widest)
    (130, 2048),                               # nb = 16, 136 tiles, rows = 64
    (49153, 2048),                             # rows capped at 16384, 4 splits, last split of 1 row
]


def int_activation(m, c, seed, device="cpu"):
    """fp16 [m, c] of integers drawn from {0, 1, 2, 3}, different per row and per
    channel.  Inside one split (plan(m, c).rows rows) a second moment is at most
    9 * rows and a column sum 3 * rows: both stay below 2^24, where fp32 adds
    integers exactly — asserted here."""
    rows = plan(m, c).rows
    assert rows <= MAX_SPLIT_ROWS
    assert ACT_MAX * ACT_MAX * rows <= 9 * 16384 == 147456 < 2 ** 24      # a second moment inside a split
    assert ACT_MAX * rows <= 3 * 16384 < 2 ** 24                          # a column sum inside a split
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(0, ACT_MAX + 1, (m, c), generator=g, device=device, dtype=torch.int8).half()


def gram_exact(a, chunk=8192):
    """(mean, E) of a [m, c] in fp64 on a's device: mean = colsum / m and
    E = (a^T a) / m — the sums taken in fp64 over row chunks (exact for integer a:
    every partial sum is an integer far below 2^53), then one fp64 division, as
    gram_reduce_kernel's "sum / M"."""
    m, c = a.shape
    s = torch.zeros(c, dtype=torch.float64, device=a.device)
    g = torch.zeros(c, c, dtype=torch.float64, device=a.device)
    for r0 in range(0, m, chunk):
        x = a[r0:r0 + chunk].double()
        s += x.sum(0)
        g += x.T @ x
    # a tensor divisor: torch's GPU kernels divide by a Python scalar as a multiplication
    # with its reciprocal (two roundings), an element-wise tensor division is one
    return s / torch.full_like(s, m), g / torch.full_like(g, m)


def int_weight(k, c, seed, nnz=64, wmax=4):
    """fp32 [k, 1, 1, c] of integers in [-wmax, wmax], at most nnz non-zeros per
    row: with activations in {0 .. 3} every output of the 1x1 conv is an integer of
    magnitude <= 3 * wmax * nnz (768 <= 2048: exact in fp16)."""
    assert ACT_MAX * wmax * nnz <= 2048
    rng = np.random.default_rng(seed)
    w = np.zeros((k, c), f32)
    for r in range(k):
        cols = rng.choice(c, size=min(nnz, c), replace=False)
        w[r, cols] = rng.integers(-wmax, wmax + 1, size=cols.size)
    assert (np.count_nonzero(w, axis=1) <= nnz).all() and np.abs(w).max() <= wmax
    return torch.from_numpy(w).reshape(k, 1, 1, c)


def _np(x, dtype):
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x).astype(dtype)


def bn_from_gram_exact(mu, E, w16, inv_scale, count, gamma, beta, momentum=0.1, eps=1e-5, rm=None, rv=None):
    """hkp_bn_from_gram in numpy fp64.  w_k = f16 weight row x its inverse scale;
    mean_k = w_k . mu, var_k = max(w_k^T E w_k - mean_k^2, 0); then bn_fin_store's
    arithmetic (csrc/common.h): m2 = var * count, var = m2 / count,
    inv = 1 / sqrt(var + f64(f32(eps))), the fp32 casts, and the running statistics
    (unbiased = m2 / (count - 1) when count > 1, else var).  Returns a dict: mean, var
    (float64, var clamped, before the count round trip), mi, ss (fp32 torch), rm, rv
    (fp32 torch or None)."""
    mu, E = _np(mu, f64), _np(E, f64)
    k = w16.shape[0]
    w = (_np(w16, f32).reshape(k, -1) * _np(inv_scale, f32)[:, None]).astype(f64)   # exact: fp16 x 2^e
    mean = w @ mu
    q = ((w @ E) * w).sum(1)
    var = np.maximum(q - mean * mean, 0.0)
    m2 = var * f64(count)
    v = m2 / f64(count)
    inv = 1.0 / np.sqrt(v + f64(f32(eps)))
    mi = torch.from_numpy(np.concatenate([mean.astype(f32), inv.astype(f32)]))
    g = None if gamma is None else gamma.detach().cpu()
    b = None if beta is None else beta.detach().cpu()
    out = dict(mean=mean, var=var, mi=mi, ss=_bn_ref.ss_from_mi(mi, g, b), rm=None, rv=None)
    if rm is not None:
        mom = f64(f32(momentum))
        unbiased = m2 / f64(count - 1) if count > 1 else v
        out["rm"] = torch.from_numpy((mom * mean + (1.0 - mom) * _np(rm, f64)).astype(f32))
        out["rv"] = torch.from_numpy((mom * unbiased + (1.0 - mom) * _np(rv, f64)).astype(f32))
    return out


def fused_apply_ref(y_exact, ss, res=None, res_ss=None, relu=True):
    """hkp_conv2d_fwd_f16_bn's output from the exact conv result: the epilogue
    stages y in fp16 first (x3_store_tile_f16_bn), then runs bn_apply_f16's
    arithmetic on it -> fp16."""
    return _bn_ref.apply_f16(y_exact.float().half(), ss, res, res_ss, relu)[0]


def same_bits_f16(a, b):
    """Equal fp16 bit patterns, except that any NaN equals any NaN (payloads are not pinned)."""
    na, nb = a.isnan(), b.isnan()
    zero = torch.zeros_like(a)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(
        torch.where(na, zero, a).view(torch.int16), torch.where(nb, zero, b).view(torch.int16))
