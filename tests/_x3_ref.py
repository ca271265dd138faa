"""Plain fp64 references, hand-built operand planes, packing helpers, error bounds and case
tables of the f16x3 / plain-fp16 convs (csrc/conv_x3.hip, csrc/wgrad_x3.hip) — shared by
test_x3_ref_cpu.py and
test_gpu_x3_exact.py.  Helpers only; torch on the CPU, hkp only inside desc() / plans().

The kernels take their operands PRE-SPLIT as two independent fp16 planes (hi, lo) and add
every product they keep into one fp32 accumulator:

    P = 3 (f16x3)       hx*hw + hx*lw + lx*hw
    P = 2 (HKP_X3_W16)  hx*hw + lx*hw
    P = 4 (HKP_X3_X16)  hx*hw + hx*lw
    P = 1 (plain fp16)  x16*w16

and the epilogue multiplies by power-of-two scales (per output channel, and 1 / the
gradient's scale) and adds the addend.  Nothing ties lo to hi inside the kernel, so a test
may fill both planes with UNRELATED small integers: every product and every partial sum is
then an integer below 2^24 in any order and any grouping (one tile, K segments, slabs),
which fp32 holds exactly, and the kernel must equal the fp64 reference of exactly those
products bit for bit.  A swapped plane, a dropped or doubled product, a wrong tap, channel
group, row or column shows as a nonzero difference at a named element.

Planes are kept in torch's own layouts (activations NCHW, weights OIHW); pack_* give the
kernels' layouts:

    activation  [N, H, W, C/32, hi32 | lo32]           (P = 1: [N, H, W, C])
    weight      [K, R, S, C/32, hi32 | lo32]           (P = 1: [K, R, S, C])
    flipped     [C, R, S, K/32, hi32 | lo32], tap (i, j) = the filter's tap (R-1-i, S-1-j)
"""
import collections
import functools

import torch
import torch.nn.functional as F

U = 2.0 ** -24                # fp32 unit roundoff
POLICIES = (2, 3, 4, 5, 6, 9, 10, 11, 13, 15, 16, 17, 0)      # every live tile policy, AUTO last
PATCH_H, PATCH_W = 8, 32      # HALO_PH x HALO_PW and STEM_PH x STEM_PW of csrc/x3_plan.h

# A row: entry (x3 | w16 | x16 | f16 | ...), (n, h, w, cin, cout, k, stride, pad, dil), tile
# policy, stream-K workspace, and the integer ranges of its planes (|hi| <= hi, |lo| <= lo):
# the ranges are a field so that a row that fails int_exact() narrows them — the check
# itself is never turned off.
Row = collections.namedtuple("Row", "name entry shape tile sk hi lo")
HI, LO, ADD = 3, 2, 3

# ---------------------------------------------------------------- the tables ----
# (n, h, w, cin, cout, k, stride, pad, dil), what the row reaches
EDGE_SHAPES = [
    (1, 1, 1, 32, 64, 1, 1, 0, 1),          # M = 1, one K-step: the ring's fill is longer than the loop
    (1, 1, 257, 32, 64, 1, 1, 0, 1),        # third 128-row tile has one row: its M2 is exactly +0, its sum is y
    (1, 5, 6, 64, 64, 3, 1, 2, 1),          # border outputs that read padding only
    (1, 2, 2, 64, 128, 3, 1, 4, 4),         # image inside one dilated tap
    (3, 9, 11, 96, 192, 3, 1, 1, 1),        # 3 channel groups, Cout 192 (BN 64, 3 column tiles)
    (1, 31, 41, 64, 128, 3, 2, 1, 1),       # stride 2, odd H and W
    (1, 9, 14, 32, 192, 3, 1, 2, 2),        # one channel group, dilation 2
    (1, 16, 64, 64, 64, 3, 1, 1, 1),        # halo body ...
    (1, 17, 64, 64, 64, 3, 1, 1, 1),        # ... and h = 17: the plan leaves it
    (1, 8, 32, 64, 64, 3, 1, 1, 1),         # halo, exactly one patch
]
FWD_ENTRIES = ("x3", "w16", "x16", "f16")
PRODUCTS = {"x3": 3, "w16": 2, "x16": 4, "f16": 1, "f16bn": 1, "dgrad": 3, "dgrad_s2": 3, "wgrad": 3,
            "x3_bnin": 3, "f16_bnin": 1}
NPROD = {3: 3, 2: 2, 4: 2, 1: 1}            # products per channel each mode keeps

WG_EDGE = [
    (1, 1, 1, 64, 64, 1, 1, 0, 1),          # M = 1
    (1, 4, 2, 64, 64, 3, 1, 4, 4),          # M = 8, shorter than one stage, mostly padding
]
WG_CUS = (0, 1, 40, -1)                     # the planner's, one split, a budget, the tiled body forced

STEM_SHAPES = [
    (1, 16, 64, 3, 64, 7, 2, 3, 1),         # 8 x 32 outputs: one patch
    (1, 18, 70, 3, 64, 7, 2, 3, 1),         # 9 x 35 outputs: no whole patch (the one-tile pair body)
    (1, 20, 26, 1, 64, 7, 2, 3, 1),         # one channel, 10 x 13 outputs
]


def case_id(shape):
    return "%dx%dx%dx%d-k%d-%dx%d-s%dp%dd%d" % (shape[:6] + (shape[5],) + shape[6:])


# ------------------------------------------------------------------ geometry ----

def out_hw(shape):
    n, h, w, cin, cout, k, st, pad, dil = shape
    return (h + 2 * pad - dil * (k - 1) - 1) // st + 1, (w + 2 * pad - dil * (k - 1) - 1) // st + 1


def out_pixels(shape):
    ho, wo = out_hw(shape)
    return shape[0] * ho * wo


def red_len(shape, op):
    """The reduction length L (channels x taps, or pixels) of one output element of op."""
    n, h, w, cin, cout, k, st, pad, dil = shape
    return {"fwd": k * k * cin, "dgrad": k * k * cout, "wgrad": out_pixels(shape)}[op]


def int_exact(row, op, tile_rows=128):
    """The 2^24 condition of a row's integer planes: an element is at most
    (hi*hi + 2*hi*lo) L + add (21 L + 3 with the default ranges), a BN tile sum at most
    rows * (hi*hi + 2*hi*lo) L (before the power-of-two scales, which are exact)."""
    per = row.hi * row.hi + 2 * row.hi * row.lo
    L = red_len(row.shape, op)
    ok = per * L + ADD < 2 ** 24
    if op == "fwd":
        ok = ok and tile_rows * per * L < 2 ** 24
    return ok


def desc(shape, tile=0, layout="nhwc"):
    from hkp import _lib
    n, h, w, cin, cout, k, st, pad, dil = shape
    return _lib.ConvDesc(n, h, w, cin, cout, k, k, st, pad, dil,
                         _lib.HKP_LAYOUT_NHWC if layout == "nhwc" else _lib.HKP_LAYOUT_NCHW, tile)


def kop(entry):
    from hkp import _lib
    return {"x3": _lib.HKP_KOP_FWD_X3, "w16": _lib.HKP_KOP_FWD_X3_W16, "x16": _lib.HKP_KOP_FWD_X3_X16,
            "f16": _lib.HKP_KOP_FWD_F16, "f16bn": _lib.HKP_KOP_FWD_F16_BN, "x3_bnin": _lib.HKP_KOP_FWD_X3,
            "f16_bnin": _lib.HKP_KOP_FWD_F16, "dgrad": _lib.HKP_KOP_DGRAD_X3, "stem_planes": _lib.HKP_KOP_STEM_X3,
            "stem_image": _lib.HKP_KOP_STEM_X3_IMAGE, "stem_u8": _lib.HKP_KOP_STEM_X3_IMAGE_U8}[entry]


def accepts(entry, shape):
    """The entry's documented shape rules (the wrappers' and entry points' argument checks)."""
    n, h, w, cin, cout, k, st, pad, dil = shape
    if PRODUCTS.get(entry, 3) == 1 and cin % 64:          # the plain-fp16 entries take whole 64-channel lines
        return False
    if entry == "dgrad":                                  # hkp_conv2d_bwd_data_x3: stride 1, its padding rule
        return not (st != 1 or cout % 32 or cin % 64 or dil * (k - 1) - pad < 0)
    return entry.startswith("stem") or (cin % 32 == 0 and cout % 64 == 0)


def plans(entry, shape, tile, sk, cus):
    """The launches the plan gives (ops.launch_plan); [] only where accepts() says the entry
    rejects the row — any other refusal raises, so a regression that makes an entry reject an
    edge shape cannot shrink the tables silently."""
    from hkp import ops
    if not accepts(entry, shape):
        return []
    return ops.launch_plan(desc(shape, tile, "nchw" if entry.startswith("stem") else "nhwc"), kop(entry), sk, cus)


def body_of(plan):
    """What tells two launches of one shape apart: kernel names, and whether an in-launch
    tail, a second region or the stream-K workspace is in play."""
    return tuple((l["name"], l["main_blocks"] > 0, l["tail_groups"] > 0, l["uses_ws"] > 0, l["mix_b1"] > 0)
                 for l in plan)


def edge_rows(entries=FWD_ENTRIES, shapes=None, cus=256):
    """Every edge shape under every live tile policy each entry accepts, one row per body
    the plan actually names (on `cus` CUs): [(Row, body)]."""
    out = []
    for entry in entries:
        for shape in (EDGE_SHAPES if shapes is None else shapes):
            seen = set()
            for tile in POLICIES:
                if not accepts(entry, shape):
                    continue
                plan = plans(entry, shape, tile, True, cus)
                assert plan, "no plan for %s %s under policy %d" % (entry, shape, tile)
                if body_of(plan) in seen:
                    continue
                seen.add(body_of(plan))
                out.append((Row("%s-%s-t%d" % (entry, case_id(shape), tile), entry, shape, tile, True, HI, LO),
                            body_of(plan)))
    return out


# ------------------------------------------------------------------- packing ----

def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def pack_x3(hi, lo):
    """(hi, lo) [.., C] -> packed split [.., C/32, hi32 | lo32] as [.., 2C] fp16."""
    c = hi.shape[-1]
    assert c % 32 == 0 and hi.shape == lo.shape
    lead = tuple(hi.shape[:-1])
    g = torch.stack([hi.reshape(lead + (c // 32, 32)), lo.reshape(lead + (c // 32, 32))], dim=-2)
    return g.reshape(lead + (2 * c,)).half().contiguous()


def unpack_x3(t):
    """packed split [.., 2C] -> (hi, lo) [.., C]."""
    lead = tuple(t.shape[:-1])
    g = t.reshape(lead + (t.shape[-1] // 64, 2, 32))
    return g[..., 0, :].reshape(lead + (-1,)), g[..., 1, :].reshape(lead + (-1,))


def pack_act(hi, lo, P=3):
    """NCHW planes -> the activation operand (P = 1: the hi plane alone, plain fp16 NHWC)."""
    t = nhwc(hi).half() if P == 1 else pack_x3(nhwc(hi), nhwc(lo))
    t._hkp_split_passes = 1 if P == 1 else 3
    return t


def unpack_act(t, P=3):
    """The activation operand -> NCHW (hi, lo) fp32 planes (P = 1: lo is zero)."""
    if P == 1:
        return nchw(t.float()), torch.zeros_like(nchw(t.float()))
    hi, lo = unpack_x3(t)
    return nchw(hi.float()), nchw(lo.float())


def pack_w(hw, lw, P=3):
    """OIHW planes -> [K, R, S, 2C] (P = 1: [K, R, S, C])."""
    return nhwc(hw).half() if P == 1 else pack_x3(nhwc(hw), nhwc(lw))


def unpack_w(t, P=3):
    if P == 1:
        return nchw(t.float()), torch.zeros_like(nchw(t.float()))
    hi, lo = unpack_x3(t)
    return nchw(hi.float()), nchw(lo.float())


def _flip(w):                 # OIHW [K, C, R, S] -> [C, R, S, K], tap (i, j) = the filter's (R-1-i, S-1-j)
    return w.flip(2, 3).permute(1, 2, 3, 0).contiguous()


def _unflip(t):               # the inverse
    return t.permute(3, 0, 1, 2).flip(2, 3).contiguous()


def pack_w_flip(hw, lw):
    """OIHW planes -> the dgrad operand [C, R, S, 2K]."""
    return pack_x3(_flip(hw), _flip(lw))


def unpack_w_flip(t):
    hi, lo = unpack_x3(t)
    return _unflip(hi.float()), _unflip(lo.float())


def phase_slices(k, pad, ph):
    """Rows and columns of the flipped pack that output phase ph = py*2 + px of a stride-2
    conv's dgrad reads (hkp_phase_taps; the selection of test_gpu_precision.test_x3_dgrad_strided)."""
    rows = [k - 1 - r for r in range(k - 1, -1, -1) if (((ph >> 1) + pad - r) % 2) == 0]
    cols = [k - 1 - s for s in range(k - 1, -1, -1) if (((ph & 1) + pad - s) % 2) == 0]
    return rows, cols


def pow2_scale(amax):
    """The gradient scale the kernels derive from max|dy| (pow2_scale_for, csrc/common.h):
    2^e putting amax in [2^13, 2^14); 1 for 0."""
    if not amax > 0:
        return 1.0
    _, e = torch.frexp(torch.tensor(float(amax)))
    return 2.0 ** (14 - int(e))


# -------------------------------------------------------------------- inputs ----

@functools.lru_cache(maxsize=4)
def int_planes(shape, seed, op, hi=HI, lo=LO):
    """Hand-built integer planes (read-only: cached) of op "fwd" | "dgrad" | "wgrad":
    hx, lx [n, cin, h, w]; hw, lw OIHW; hdy, ldy [n, cout, ho, wo]; add [n, cin, h, w];
    inv [channels of the output]: powers of two in 2^-2 .. 2^2.  hi planes in [-hi, hi], lo
    planes in [-lo, lo] and UNRELATED to hi; a handful of lo == 0 channels and of all-zero
    filters are mixed in."""
    n, h, w, cin, cout, k, st, pad, dil = shape
    ho, wo = out_hw(shape)
    g = torch.Generator().manual_seed(seed)

    def ri(a, *shp):
        return torch.randint(-a, a + 1, shp, generator=g).float()

    def some(c):
        return torch.randperm(c, generator=g)[:max(1, c // 16)]

    p = {}
    if op in ("fwd", "wgrad"):
        p["hx"], p["lx"] = ri(hi, n, cin, h, w), ri(lo, n, cin, h, w)
        p["lx"][:, some(cin)] = 0
    if op in ("dgrad", "wgrad"):
        p["hdy"], p["ldy"] = ri(hi, n, cout, ho, wo), ri(lo, n, cout, ho, wo)
        p["ldy"][:, some(cout)] = 0
    if op in ("fwd", "dgrad"):
        p["hw"], p["lw"] = ri(hi, cout, cin, k, k), ri(lo, cout, cin, k, k)
        p["lw"][:, some(cin)] = 0
        zf = some(cout)
        p["hw"][zf] = 0
        p["lw"][zf] = 0
        p["inv"] = 2.0 ** torch.randint(-2, 3, (cout if op == "fwd" else cin,), generator=g).float()
    if op == "dgrad":
        p["add"] = ri(ADD, n, cin, h, w)
    return p


def abs_planes(p):
    return {k: v.abs() for k, v in p.items()}


# ----------------------------------------------------------- fp64 references ----

def _conv(x, w, shape):
    n, h, wd, cin, cout, k, st, pad, dil = shape
    return F.conv2d(x.double(), w.double(), None, st, pad, dil)


def ref64(p, shape, op, P=3, gscale=1.0):
    """fp64 reference of exactly the products mode P keeps (the sums of planes below are
    exact in fp64: fp16 values span 2^-24 .. 2^16), in torch's layouts:
      fwd    y [n, cout, ho, wo] = inv[k] * acc
      dgrad  dx [n, cin, h, w]   = inv[c] * acc / gscale + add       (P = 3)
      wgrad  dw OIHW             = acc / gscale                      (P = 3)
    gscale: the power of two dy was scaled by before its split (pow2_scale)."""
    n, h, w, cin, cout, k, st, pad, dil = shape
    if op == "fwd":
        hx, lx, hw, lw = (p[q].double() for q in ("hx", "lx", "hw", "lw"))
        if P == 3:
            acc = _conv(hx, hw + lw, shape) + _conv(lx, hw, shape)
        elif P == 2:
            acc = _conv(hx + lx, hw, shape)
        elif P == 4:
            acc = _conv(hx, hw + lw, shape)
        else:
            acc = _conv(hx, hw, shape)
        return acc * p["inv"].double().view(1, -1, 1, 1)
    assert P == 3
    if op == "dgrad":
        hdy, ldy, hw, lw = (p[q].double() for q in ("hdy", "ldy", "hw", "lw"))
        size = (n, cin, h, w)
        acc = (torch.nn.grad.conv2d_input(size, hw + lw, hdy, st, pad, dil)
               + torch.nn.grad.conv2d_input(size, hw, ldy, st, pad, dil))
        dx = acc * p["inv"].double().view(1, -1, 1, 1) / gscale
        return dx + p["add"].double() if p.get("add") is not None else dx
    hx, lx, hdy, ldy = (p[q].double() for q in ("hx", "lx", "hdy", "ldy"))
    size = (cout, cin, k, k)
    acc = (torch.nn.grad.conv2d_weight(hx, size, hdy + ldy, st, pad, dil)
           + torch.nn.grad.conv2d_weight(lx, size, hdy, st, pad, dil))
    return acc / gscale


def rows(y):
    """NCHW [n, k, ho, wo] -> the GEMM's [M, K] (row = output pixel, NHWC order)."""
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


def stat_tiles64(y, layout):
    """Per BN statistic tile of y [n, K, ho, wo]: (sum [T, K], M2 about the tile's own mean
    [T, K], mean [T, K], rows per tile [T], max|y| [T, K], the tile height each tile was cut
    at [T]) in fp64, grouped the way the body groups rows.  layout:

      ("raster", ((rows, tiles), ...))   consecutive runs of output pixels in NHWC order:
          x3_bn_partials (conv_x3.hip, `tile128 = part_base + ((m0 - m_base) >> 7)`) and
          x3_bn_partials_w (`tile128 = part_base + (m0 - m_base) / (2 * WROWS) + h`, and
          `pt = part_base + (m0 - m_base) / WROWS + wm` for the 160-row tiles) write one
          partial per 128 / 96 / 80 rows of the launch's row range; a mix launch's regions
          follow each other (`m_base`, `part_base` of X3Args), every region but the last
          made of whole tiles — ops.conv_stat_layout / ops.stat_segments give the table,
          a plain launch is ((ops.stat_tile_rows(part), ceil(M / rows)),).
      ("patch",)   the halo and stem patch bodies: m-tile mt is the 8 x 32 patch (img,
          h0, w0) in raster order of patches (`img = mt / tpi ... h0 = (rem / pwn) * PH`),
          tile row m the pixel (h0 + m / 32, w0 + m % 32), and the partial tiles are its
          two 128-row halves: patch rows 0-3 and 4-7."""
    n, kk, ho, wo = y.shape
    y = y.double()
    if layout[0] == "patch":
        assert ho % PATCH_H == 0 and wo % PATCH_W == 0
        t = y.permute(0, 2, 3, 1).reshape(n, ho // PATCH_H, 2, PATCH_H // 2, wo // PATCH_W, PATCH_W, kk)
        t = t.permute(0, 1, 4, 2, 3, 5, 6).reshape(-1, 128, kk)
        tiles = list(t)
        nominal = [128] * len(tiles)
    else:
        ym, tiles, nominal, m0 = rows(y), [], [], 0
        for nrows, ntiles in layout[1]:
            for _ in range(ntiles):
                if m0 < ym.shape[0]:
                    tiles.append(ym[m0:m0 + nrows])
                    nominal.append(nrows)
                m0 += nrows
        assert m0 >= ym.shape[0], "the layout covers %d of %d rows" % (m0, ym.shape[0])
    mu = torch.stack([t.mean(0) for t in tiles])
    return (torch.stack([t.sum(0) for t in tiles]),
            torch.stack([((t - t.mean(0)) ** 2).sum(0) for t in tiles]), mu,
            [t.shape[0] for t in tiles], torch.stack([t.abs().amax(0) for t in tiles]), nominal)


# -------------------------------------------------------------------- bounds ----

def err_bound_x3(nprod, L, absref):
    """The dot-product bound of _conv_ref.err_bound at length nprod * L: every product of
    two fp16 values is exact in the MFMA, so an output element is an fp32 sum of nprod * L
    exact terms in some order, and |fl(sum) - sum| <= gamma_{nprod L} sum |terms|, taken as
    (nprod L + 2) u: the + 2 covers the addend and the rounding of the reference to an
    fp32-representable output (the power-of-two scales are exact).  absref: the same
    reference on the absolute values of the planes.  Elementwise."""
    return (nprod * L + 2) * U * absref


def f16_round_bound(ref, bound):
    """What one rounding of the fp32 result to fp16 adds (the plain-fp16 entries' output):
    half an fp16 ulp of the rounded value, 2^-11 (|ref| + bound), and 2^-25 in fp16's
    subnormal range."""
    return 2.0 ** -11 * (ref.abs() + bound) + 2.0 ** -25


def stat_body(name, tile_rows):
    """How the body named `name` (the plan's kernel name) reduces a statistic tile cut at
    tile_rows rows: ("direct",) — x3_bn_partials, the squares taken about the tile's own mean:
    the 32x32x16-MFMA forms of conv_x3_tile, `conv_x3_kernel<BN, STEM, PAIR, 32, ..>` — or
    ("merged", leaf rows, merge levels) — x3_bn_partials_w: a lane's 4 NI rows (16 of a 128-row
    tile, 12 of a 96-row one) merged over lanes l ^ 16, l ^ 32 and the half's two waves, three
    levels; the 160-row A3 tiles (80-row statistic tiles): 20-row leaves, two levels, a wave is
    a tile; duo_bn_partials: 4 UM = 32-row leaves, two levels."""
    if name.startswith("conv_x3_kernel<") and name.split(",")[3].strip() == "32":
        return ("direct",)
    if "duo" in name:
        return ("merged", 32, 2)
    return {128: ("merged", 16, 3), 96: ("merged", 12, 3), 80: ("merged", 20, 2)}[tile_rows]


def m2_bound_x3(cnt, m2, mean, ymax, body):
    """Bound on |part[t, :, 1] - M2| for a tile of cnt rows whose y is exact, by the body
    (stat_body) that wrote it.

    ("direct",): _conv_ref.m2_bound as it stands, gamma_{cnt+2} (M2 + e) + e with
    e = cnt (2u |mean|)^2.

    ("merged", leaf, levels): disjoint row groups (leaves of at most `leaf` rows) are reduced
    to (sum, M2 about the group's own mean) — the direct bound per leaf with cnt = its rows
    and its own mean, |mu_l| <= Y = max|y| of the tile — and merged pairwise by x3_chan_merge,
        d = fl(fl(s_b i_b) - fl(s_a i_a)),  q = fl(fl(q_a + q_b) + fl(fl(d d) f)),
    over `levels` levels.  Exactly, M2 = M2_a + M2_b + D^2 f with D = mu_b - mu_a and
    f = n_a n_b / n <= n / 4; all three terms are >= 0.  The sums s are exact (compared
    separately, bit for bit); i = 1/n and f are exact on full tiles and carry a rounding each
    on ragged ones, so with |mu_a|, |mu_b| <= Y
        |d - D| <= eta := 8 u Y    (two roundings per mean, one of the difference, |D| <= 2Y),
        |d^2 - D^2| f <= (2 |D| eta + eta^2) f <= sqrt(n M2_node) eta + n eta^2 / 4
    (f D^2 <= M2_node, f <= n / 4).  Over the disjoint nodes of one level, Cauchy-Schwarz
    gives sum sqrt(n_i M2_i) <= sqrt(cnt M2): a level adds at most sqrt(cnt M2) eta +
    cnt eta^2 / 4 in absolute terms, and every quantity passes through at most 6 more
    roundings per level (the two additions, the square, the product with f, f's own, one to
    spare).  With the leaves' sum of M2 <= M2 and sum of e_l <= cnt (2 u Y)^2:
        |q - M2| <= gamma_{min(leaf, cnt) + 2 + 6 levels} (M2 + A) + A,
        A = cnt (2 u Y)^2 + levels (sqrt(cnt M2) eta + cnt eta^2 / 4).
    Y, not |mean|, because the sub-tiles' means are bounded by the tile's largest |y| only.
    cnt == 1: the leaf's mean is y itself and every merge has f = 0: q == +0 exactly in
    either body; the tests assert that separately."""
    if body[0] == "direct":
        import _conv_ref
        return _conv_ref.m2_bound(cnt, m2, mean)
    _, leaf, levels = body
    n = min(leaf, cnt) + 2 + 6 * levels
    gamma = n * U / (1 - n * U)
    eta = 8 * U * ymax
    a = cnt * (2 * U * ymax) ** 2 + levels * ((cnt * m2).sqrt() * eta + cnt * eta ** 2 / 4)
    return gamma * (m2 + a) + a


def f16bn_bound(ref_y, b_y, s, t, res):
    """Bound on the fused-BN fp16 epilogue out = f16(relu(f16(y) s + t + res)) against
    relu(ref_y s + t + res) in fp64, from b_y >= |y - ref_y| (err_bound_x3): the first fp16
    rounding (f16_round_bound), the affine step in fp32 — |s| times the error so far plus
    the roundings of its multiply and two adds, each at most u times an intermediate no larger
    than (|y16 s| + |t| + |res|)(1 + u)^2: 3 u (1 + O(u)), taken as 4 u — the ReLU
    (1-Lipschitz), and the second fp16 rounding of the result."""
    e1 = b_y + f16_round_bound(ref_y, b_y)
    mag = (ref_y.abs() + e1) * s.abs() + t.abs() + res.abs()
    e2 = s.abs() * e1 + 4 * U * mag
    return e2 + 2.0 ** -11 * (mag + e2) + 2.0 ** -25
