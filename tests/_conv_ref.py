"""Plain fp64 references, inputs, error bounds and case tables of the exact-fp32
MFMA convs (csrc/conv_fwd.hip, csrc/conv_bwd.hip) — shared by test_conv_ref_cpu.py
and test_gpu_conv_fp32.py.  Helpers only; torch on the CPU, hkp only inside desc().

Tensors are kept in torch's own layouts (x NCHW, w OIHW, dy NCHW); nhwc() / krsc()
give the kernels' layouts.

Two kinds of input:

* integers (x, dy, add in [-3, 3], w in [-2, 2]) stored as fp32.  Every product is at
  most 9 in magnitude, so a partial sum of L products plus the addend is at most
  9 L + 3; while that is below 2^24 every product and every partial sum IN ANY ORDER
  is an integer fp32 holds exactly, and the kernel must equal the fp64 reference bit
  for bit: no tolerance.
* floats (relu'd N(0,1) activations, He-scaled weights), judged elementwise by
  err_bound(): the a-priori bound of an fp32 dot product summed in any order.
"""
import collections
import functools

import torch
import torch.nn.functional as F

U = 2.0 ** -24                # fp32 unit roundoff
TILE_ROWS = 128               # CONV_BM: rows of one BN statistic tile
WG_STAGE = 32                 # WG_BKM: pixels per LDS stage of the wgrad kernels

Case = collections.namedtuple("Case", "n h w cin cout r s stride pad dil")

# ---------------------------------------------------------------- the tables ----
# rows are (n, h, w, cin, cout, r, s, stride, pad, dil)

FWD_NHWC = [Case(*t) for t in [
    (1, 1, 1, 32, 64, 1, 1, 1, 0, 1),       # M = 1: one live row; tile sum == y, M2 == 0 exactly
    (1, 1, 127, 32, 64, 1, 1, 1, 0, 1),     # M = 127
    (1, 8, 16, 32, 128, 1, 1, 1, 0, 1),     # M = 128 exactly, BN 128
    (1, 3, 43, 64, 192, 1, 1, 1, 0, 1),     # M = 129: second tile cnt == 1; K 192 -> BN 64, 3 column tiles; grid 6
    (2, 9, 11, 32, 64, 3, 3, 1, 1, 1),      # Cin 32: one chunk per tap
    (3, 9, 11, 96, 192, 3, 3, 1, 1, 1),     # Cin 96: 3 chunks per tap; grid 3x3 = 9 (xcd_remap with nwg % 8 != 0)
    (1, 10, 12, 64, 64, 3, 3, 1, 0, 1),     # pad 0
    (1, 5, 6, 64, 64, 3, 3, 1, 2, 1),       # pad > dil*(r-1)/2: border outputs read padding only
    (1, 2, 2, 64, 128, 3, 3, 1, 4, 4),      # image inside one dilated tap: only the centre tap is live
    (2, 30, 40, 64, 128, 1, 1, 2, 0, 1),    # 1x1 stride 2, even H, W
    (1, 31, 41, 64, 128, 3, 3, 2, 1, 1),    # 3x3 stride 2, odd H, W
    (1, 15, 20, 64, 64, 3, 3, 2, 2, 2),     # stride 2 with dilation 2
    (1, 9, 14, 64, 64, 1, 3, 1, 1, 1),      # R != S (1x3)
    (1, 9, 14, 64, 64, 3, 1, 1, 1, 1),      # R != S (3x1)
]]

FWD_STEM = [Case(*t) for t in [             # layout "nchw": x [n,c,h,w], w OIHW
    (2, 9, 11, 3, 64, 7, 7, 2, 3, 1),       # Kreal 147: 147 % 4 == 3, last chunk 19 wide
    (1, 20, 26, 1, 64, 7, 7, 2, 3, 1),      # C 1, Kreal 49; M = 130
    (1, 12, 14, 8, 128, 7, 7, 2, 3, 1),     # C 8 (the cap), K 128 template, Kreal 392
    (2, 6, 7, 3, 64, 3, 3, 1, 1, 1),        # Kreal 27 < 32: one partial chunk
    (1, 6, 7, 8, 64, 5, 5, 1, 2, 1),        # Kreal 200
]]

DGRAD = [Case(*t) for t in [
    (2, 17, 23, 64, 32, 3, 3, 1, 1, 1),     # Cout 32: one chunk per tap; Cin 64 -> width 64
    (2, 9, 11, 128, 96, 3, 3, 1, 1, 1),     # Cout 96; Cin 128 -> width 128; M = 198
    (1, 1, 1, 64, 64, 1, 1, 1, 0, 1),       # one dx pixel
    (1, 15, 20, 192, 64, 3, 3, 1, 2, 2),    # Cin 192 (width 64, 3 column tiles), dilation 2
    (2, 30, 40, 64, 128, 1, 1, 2, 0, 1),    # stride-2 1x1, even H, W: last dx row/col and all odd rows/cols == add
    (2, 31, 41, 64, 128, 1, 1, 2, 0, 1),    # the same, odd
    (1, 30, 40, 128, 64, 3, 3, 2, 1, 1),    # stride-2 3x3, width 128: last dy row/col half used
    (1, 15, 20, 64, 64, 3, 3, 2, 2, 2),     # stride 2, dilation 2
    (1, 14, 17, 64, 64, 3, 3, 3, 1, 1),     # stride 3 (the loader's `% stride` with three residues)
]]

# the split counts are the library's planner's (test_conv_ref_cpu.py holds them to it)
WGRAD_NHWC = [Case(*t) for t in [
    (1, 1, 1, 64, 64, 1, 1, 1, 0, 1),       # M = 1: one split, one stage, 31 empty pixel rows       <64,64>
    (1, 16, 16, 64, 64, 3, 3, 1, 1, 1),     # M = 256: 1 split exactly full
    (1, 1, 257, 64, 128, 1, 1, 1, 0, 1),    # 2 splits, last 97 px                                   <128,64>
    (1, 3, 171, 128, 64, 1, 1, 1, 0, 1),    # 3 splits, last 129 px                                  <64,128>
    (1, 30, 30, 64, 64, 1, 1, 1, 0, 1),     # 4 splits
    (1, 25, 44, 64, 64, 1, 1, 1, 0, 1),     # 5 splits: the reduce's lane 0 takes two slabs
    (1, 48, 48, 64, 64, 3, 3, 1, 1, 1),     # 9 splits
    (2, 30, 40, 128, 128, 3, 3, 1, 2, 2),   # 10 splits, dilation 2                                  <128,128>
    (1, 4, 2, 64, 64, 3, 3, 1, 4, 4),       # M = 8: a last (only) split shorter than one stage; most taps read padding
    (1, 31, 33, 64, 64, 3, 3, 2, 1, 1),     # stride 2, odd
    (1, 9, 14, 64, 64, 1, 3, 1, 1, 1),      # R != S
    (1, 9, 14, 64, 64, 3, 1, 1, 1, 1),
]]

WGRAD_STEM = [Case(*t) for t in [           # layout "nchw": dw OIHW
    (2, 9, 11, 3, 64, 7, 7, 2, 3, 1),       # Kreal 147: third column tile 19 live of 64
    (1, 20, 26, 1, 64, 7, 7, 2, 3, 1),      # Kreal 49 < 64
    (2, 24, 28, 8, 128, 7, 7, 2, 3, 1),     # K 128 template, Kreal 392, 2 splits
    (2, 50, 70, 3, 64, 7, 7, 2, 3, 1),      # 7 splits (the shape of test_gpu_backward.test_stem_wgrad)
]]

# (K, R, S, C) of hkp_conv_weight_flip; the last has 1,179,648 elements > 4096 * 256
# threads: the second grid-stride trip
FLIP_SHAPES = [(64, 3, 3, 64), (32, 1, 3, 64), (64, 3, 1, 96), (256, 3, 3, 512)]

TABLES = {"fwd_nhwc": FWD_NHWC, "fwd_stem": FWD_STEM, "dgrad": DGRAD, "wgrad_nhwc": WGRAD_NHWC,
          "wgrad_stem": WGRAD_STEM}


def case_id(c):
    return "%dx%dx%dx%d-k%d-%dx%d-s%dp%dd%d" % c


# ------------------------------------------------------------------ geometry ----

def out_hw(c):
    return ((c.h + 2 * c.pad - c.dil * (c.r - 1) - 1) // c.stride + 1,
            (c.w + 2 * c.pad - c.dil * (c.s - 1) - 1) // c.stride + 1)


def out_pixels(c):
    ho, wo = out_hw(c)
    return c.n * ho * wo


def red_len(c, op):
    """The reduction length L of one output element of op ("fwd", "dgrad", "wgrad")."""
    return {"fwd": c.r * c.s * c.cin, "dgrad": c.r * c.s * c.cout, "wgrad": out_pixels(c)}[op]


def int_exact(c):
    """The 2^24 condition of the integer inputs, for all three ops of the case and for
    the BN tile sums (128 rows of |y| <= 6 L)."""
    worst = max(red_len(c, op) for op in ("fwd", "dgrad", "wgrad"))
    return 9 * worst + 3 < 2 ** 24 and TILE_ROWS * 6 * red_len(c, "fwd") < 2 ** 24


def desc(c, layout="nhwc"):
    """The hkp_conv_desc of the case."""
    from hkp import _lib
    return _lib.ConvDesc(c.n, c.h, c.w, c.cin, c.cout, c.r, c.s, c.stride, c.pad, c.dil,
                         _lib.HKP_LAYOUT_NHWC if layout == "nhwc" else _lib.HKP_LAYOUT_NCHW)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


krsc, oihw = nhwc, nchw       # the same permutations on a weight


# -------------------------------------------------------------------- inputs ----

def _shapes(c):
    ho, wo = out_hw(c)
    return dict(x=(c.n, c.cin, c.h, c.w), w=(c.cout, c.cin, c.r, c.s), dy=(c.n, c.cout, ho, wo),
                add=(c.n, c.cin, c.h, c.w))


@functools.lru_cache(maxsize=None)
def int_tensors(case, seed):
    """dict(x, w, dy, add) of integer-valued fp32 tensors (read-only: cached)."""
    assert int_exact(case), case
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in _shapes(case).items():
        a = 2 if name == "w" else 3
        out[name] = torch.randint(-a, a + 1, shape, generator=g).float()
    return out


@functools.lru_cache(maxsize=None)
def float_tensors(case, seed):
    """dict(x, w, dy, add): relu'd N(0,1) activations, He-scaled weights, N(0,1) gradients."""
    g = torch.Generator().manual_seed(seed)
    sh = _shapes(case)
    return dict(x=torch.randn(sh["x"], generator=g).relu(),
                w=torch.randn(sh["w"], generator=g) * (2.0 / (case.r * case.s * case.cin)) ** 0.5,
                dy=torch.randn(sh["dy"], generator=g), add=torch.randn(sh["add"], generator=g))


# ----------------------------------------------------------- fp64 references ----

def fwd64(x, w, c):
    """y [n, cout, ho, wo] in fp64."""
    return F.conv2d(x.double(), w.double(), None, c.stride, c.pad, c.dil)


def dgrad64(dy, w, c, add=None):
    """dx [n, cin, h, w] in fp64 (+ add)."""
    dx = torch.nn.grad.conv2d_input((c.n, c.cin, c.h, c.w), w.double(), dy.double(), c.stride, c.pad, c.dil)
    return dx if add is None else dx + add.double()


def wgrad64(x, dy, c):
    """dw OIHW in fp64."""
    return torch.nn.grad.conv2d_weight(x.double(), (c.cout, c.cin, c.r, c.s), dy.double(), c.stride, c.pad, c.dil)


def rows(y):
    """NCHW [n, k, ho, wo] -> the GEMM's [M, K] (row = output pixel, NHWC order)."""
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


def tile_partials64(y_mk):
    """Per 128-row tile of y [M, K] (fp64): (sum [T, K], M2 about the tile's own mean
    [T, K], mean [T, K], rows per tile [T])."""
    y = y_mk.double()
    sums, m2s, means, cnts = [], [], [], []
    for m0 in range(0, y.shape[0], TILE_ROWS):
        t = y[m0:m0 + TILE_ROWS]
        mu = t.mean(0)
        sums.append(t.sum(0))
        m2s.append(((t - mu) ** 2).sum(0))
        means.append(mu)
        cnts.append(t.shape[0])
    return torch.stack(sums), torch.stack(m2s), torch.stack(means), cnts


# -------------------------------------------------------------------- bounds ----

def err_bound(L, absref):
    """|fl(dot) - dot| <= gamma_L * sum |a_i b_i| for an fp32 dot product of length L
    summed in any order (Higham, Accuracy and Stability, sec. 3.1), taken as
    (L + 2) u with u = 2^-24: the + 2 covers the optional addend and the rounding of
    the reference to fp32-representable output.  absref: the same conv of |a| and |b|
    in fp64.  Elementwise; the only tolerance of the float-input tests."""
    return (L + 2) * U * absref


def m2_bound(cnt, m2, mean):
    """Bound on |part[t, :, 1] - M2| for a tile of cnt rows whose y is exact.

    The kernel takes mu' = fl(s / cnt) from the exact sum s, |mu' - mu| <= 2u |mu|
    (u = 2^-24; 2u allows a division that is not correctly rounded), then
    q = sum fl(fl(y_i - mu')^2) over cnt terms in some order.  Exactly,
    sum (y_i - mu')^2 = M2 + cnt (mu' - mu)^2 =: Q' since sum (y_i - mu) = 0.  Each term
    carries one rounding of the difference (squared: two factors), one of the square,
    and at most cnt - 1 of the summation (rows past M add exact zeros): a relative
    error of at most gamma_{cnt+2} on Q'.  Hence
        |q - M2| <= gamma_{cnt+2} (M2 + e) + e,   e = cnt (2u |mu|)^2.
    cnt == 1 gives mu' == y and q == 0 exactly; the tests assert that separately."""
    n = cnt + 2
    gamma = n * U / (1 - n * U)
    e = cnt * (2 * U * mean.abs()) ** 2
    return gamma * (m2 + e) + e
