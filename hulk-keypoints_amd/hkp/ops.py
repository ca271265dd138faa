"""Tensor-level wrappers over the C ABI (one function per kernel family).

Every wrapper validates device/dtype/contiguity/shape on the host BEFORE the
launch (a mis-shaped launch can fault the GPU), launches on PyTorch's current
stream, and allocates outputs with the caching allocator.  No fallback path.
"""
import ctypes

import torch

from ._lib import (HKP_KOP_DGRAD_X3, HKP_KOP_FWD_F16, HKP_KOP_FWD_F16_BN, HKP_KOP_FWD_X3, HKP_KOP_FWD_X3_W16,
                   HKP_KOP_FWD_X3_X16, HKP_KOP_STEM_X3, HKP_KOP_STEM_X3_IMAGE, HKP_KOP_STEM_X3_IMAGE_U8,
                   HKP_KOP_WGRAD_X3, HKP_X3_ALL, HKP_LAYOUT_NCHW, HKP_LAYOUT_NHWC, HKP_TILE_160_A3, HKP_TILE_192_A3,
                   HKP_TILE_MIX_A3, ConvDesc, HkpError, call)

CONV_TILE_ROWS = 128  # BM of conv_fwd.hip (rows per BN statistic tile)

# Optional launch observer (bench.py's roofline timer): called as
# observer(kernel_symbol, algorithmic_flops, algorithmic_bytes, launch_fn).
_observer = None


def set_observer(fn):
    global _observer
    _observer = fn


def conv_kernel_symbol(layout, cout):
    bn = 128 if cout % 128 == 0 else 64
    return "conv_fwd_kernel<128, %d, %s>" % (bn, "true" if layout != "nhwc" else "false")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# Stream-K workspace of the x3 convs, one per (device, stream): zeroed once (its
# arrival counters must start at zero; every launch leaves them zero).  Launches
# sharing one stream never run concurrently, as the workspace requires.
_sk_ws = {}


def _sk_workspace(enable=True):
    from ._lib import lib
    if not enable:
        return ctypes.c_void_p(0), ctypes.c_int64(0)
    st = torch.cuda.current_stream()
    key = (st.device_index, st.cuda_stream)
    ws = _sk_ws.get(key)
    if ws is None:
        nb = lib().hkp_conv_x3_sk_workspace_bytes()
        ws = torch.zeros(nb, device=torch.device("cuda", st.device_index), dtype=torch.uint8)
        _sk_ws[key] = ws
    return ctypes.c_void_p(ws.data_ptr()), ctypes.c_int64(ws.numel())


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _need(t, dtype, name, ndim=None):
    if not isinstance(t, torch.Tensor):
        raise HkpError("%s: expected a tensor" % name)
    if t.device.type != "cuda":
        raise HkpError("%s: tensor must be on the GPU (got %s)" % (name, t.device))
    if t.dtype != dtype:
        raise HkpError("%s: expected %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise HkpError("%s: tensor must be contiguous" % name)
    if ndim is not None and t.dim() != ndim:
        raise HkpError("%s: expected %d dims, got %s" % (name, ndim, tuple(t.shape)))


def conv_out_hw(h, w, r, s, stride, pad, dil):
    """conv_geometry of csrc/conv_fwd.hip with its rejections: the wrappers size their
    outputs from this before the library sees the descriptor."""
    if stride <= 0 or dil <= 0 or pad < 0:
        raise HkpError("conv: bad stride/dilation/pad")
    # C division truncates, floor division does not: a footprint larger than the padded image is empty
    eh, ew = h + 2 * pad - dil * (r - 1) - 1, w + 2 * pad - dil * (s - 1) - 1
    if eh < 0 or ew < 0:
        raise HkpError("conv: empty output")
    return eh // stride + 1, ew // stride + 1


def conv2d_fwd(x, w, stride=1, pad=0, dil=1, layout="nhwc", stats=True, out=None):
    """x NHWC [N,H,W,C] (or NCHW for the stem) fp32; w KRSC [K,R,S,C] (stem: OIHW).

    Returns (y NHWC [N,Ho,Wo,K], partials [tiles,K,2] or None)."""
    _need(x, torch.float32, "conv2d_fwd.x", 4)
    _need(w, torch.float32, "conv2d_fwd.w", 4)
    if layout == "nhwc":
        n, h, wd, c = x.shape
        k, r, s, cw = w.shape
        lay = HKP_LAYOUT_NHWC
    else:
        n, c, h, wd = x.shape
        k, cw, r, s = w.shape
        lay = HKP_LAYOUT_NCHW
    if cw != c:
        raise HkpError("conv2d_fwd: weight Cin %d != input C %d" % (cw, c))
    ho, wo = conv_out_hw(h, wd, r, s, stride, pad, dil)
    d = ConvDesc(n, h, wd, c, k, r, s, stride, pad, dil, lay)
    y = out if out is not None else torch.empty((n, ho, wo, k), device=x.device, dtype=torch.float32)
    _need(y, torch.float32, "conv2d_fwd.y", 4)
    if tuple(y.shape) != (n, ho, wo, k):
        raise HkpError("conv2d_fwd: out shape %s != %s" % (tuple(y.shape), (n, ho, wo, k)))
    part = None
    if stats:
        tiles = (n * ho * wo + CONV_TILE_ROWS - 1) // CONV_TILE_ROWS
        part = torch.empty((tiles, k, 2), device=x.device, dtype=torch.float32)
    def launch():
        call("hkp_conv2d_fwd", ctypes.byref(d), _ptr(x), _ptr(w), _ptr(y), _ptr(part), _stream())

    if _observer is None:
        launch()
    else:
        flops = 2.0 * n * ho * wo * k * r * s * c
        _observer(conv_kernel_symbol(layout, k), flops, 4.0 * (x.numel() + w.numel() + y.numel()), launch)
    return y, part


class PackedWeight(tuple):
    """(split, inv_scale): a weight in the packed split layout (fp16, each output
    channel scaled by a power of two) and the per-output-channel inverse scales."""

    def __new__(cls, split, inv_scale):
        return super().__new__(cls, (split, inv_scale))

    @property
    def split(self):
        return self[0]

    @property
    def inv_scale(self):
        return self[1]


def kernel_name(d, op, sk=True):
    """The kernel symbol a launch with ConvDesc d runs (hkp_conv_kernel_name: the first
    launch of the plan the launcher itself reads, so the name cannot drift from what runs)."""
    from ._lib import lib
    buf = ctypes.create_string_buffer(128)
    n = lib().hkp_conv_kernel_name(ctypes.byref(d), op, int(bool(sk)), buf, 128)
    if n < 0:
        raise HkpError("hkp_conv_kernel_name failed: %s" % lib().hkp_last_error().decode(errors="replace"))
    return buf.value.decode()


def launch_plan(d, op, sk=True, cus=0):
    """The launches entry point op runs for ConvDesc d on cus CUs (0: this device's;
    hkp_conv_x3_launch_plan, the plan the launcher itself reads): a list of dicts, one per
    launch — name, the _lib.X3_LAUNCH_FIELDS values, and the plan-wide segments
    ((rows, tiles), ...), cus, m, m_tiles, bn, bm.  Empty where the entry point would
    reject the shape."""
    from ._lib import HKP_X3_LAUNCH_PLAN_LEN, X3_LAUNCH_FIELDS, lib
    out, i, n = [], 0, 1
    while i < n:
        buf = ctypes.create_string_buffer(128)
        v = (ctypes.c_int64 * HKP_X3_LAUNCH_PLAN_LEN)()
        n = lib().hkp_conv_x3_launch_plan(ctypes.byref(d), op, int(bool(sk)), cus, i, buf, 128, v)
        if n < 0:
            raise HkpError("hkp_conv_x3_launch_plan failed: %s" % lib().hkp_last_error().decode(errors="replace"))
        if n == 0:
            break
        one = dict(zip(X3_LAUNCH_FIELDS, v), name=buf.value.decode(),
                   segments=tuple((v[22 + 2 * j], v[23 + 2 * j]) for j in range(v[28])),
                   cus=v[29], m=v[30], m_tiles=v[31], bn=v[32], bm=v[33])
        out.append(one)
        i += 1
    return out


def weight_pack_x3(w):
    """fp32 KRSC weight → PackedWeight: [K, R, S, 2C] fp16 ([..][C/32][hi32|lo32]) + [K] scales."""
    _need(w, torch.float32, "weight_pack_x3.w", 4)
    k, r, s, c = w.shape
    ws = torch.empty((k, r, s, 2 * c), device=w.device, dtype=torch.float16)
    sc = torch.empty(k, device=w.device, dtype=torch.float32)
    call("hkp_weight_pack_x3", k, r * s * c, c, _ptr(w), _ptr(ws), _ptr(sc), _stream())
    return PackedWeight(ws, sc)


def split_of(x):
    """(split tensor, passes) of an activation: x itself when it IS a split-only
    activation (fp16), else the split a producer attached to fp32 x, else None."""
    if x.dtype == torch.float16:
        return x, x._hkp_split_passes
    return getattr(x, "_hkp_split", None)


def channels_of(x):
    """Channel count of an fp32 activation or of a split-only one."""
    if x.dtype == torch.float16 and x._hkp_split_passes == 3:
        return x.shape[-1] // 2
    return x.shape[-1]


def _stat_partials(n_rows, k, device, part_out, name, tile_rows=CONV_TILE_ROWS, segments=None):
    """BN tile partials [tiles, k, 2] of an n_rows-pixel conv output, tile_rows rows
    per tile: part_out (a caller's slice of a larger buffer) or a new tensor.  A
    tile size other than CONV_TILE_ROWS rides on the tensor (_hkp_tile_rows) to
    bn_finalize / bn_stats, and so does a segmented list's table (_hkp_segments:
    ((rows, tiles), ...) of a mixed-height launch, hkp_conv_x3_stat_layout)."""
    tiles = (n_rows + tile_rows - 1) // tile_rows
    if segments is not None and len(segments) > 1:
        tiles = sum(t for _, t in segments)
    else:
        segments = None
    if part_out is None:
        part = torch.empty((tiles, k, 2), device=device, dtype=torch.float32)
    else:
        _need(part_out, torch.float32, name, 3)
        if tuple(part_out.shape) != (tiles, k, 2):
            raise HkpError("%s: shape %s != %s" % (name, tuple(part_out.shape), (tiles, k, 2)))
        part = part_out
    if tile_rows != CONV_TILE_ROWS:
        part._hkp_tile_rows = tile_rows
    if segments is not None:
        part._hkp_segments = tuple(segments)
    return part


def stat_tile_rows(part):
    """Rows per BN statistic tile of conv partials (hkp_conv_x3_stat_tile_rows)."""
    return getattr(part, "_hkp_tile_rows", CONV_TILE_ROWS)


def stat_segments(part):
    """The (rows, tiles) segments of a mixed-height conv's partials, or None for a
    list of one tile height."""
    return getattr(part, "_hkp_segments", None)


def conv_stat_layout(d, kop):
    """hkp_conv_x3_stat_layout: the ((rows, tiles), ...) segments of a forward conv's
    BN partial list."""
    from ._lib import lib
    seg = (ctypes.c_int32 * 6)()
    n = lib().hkp_conv_x3_stat_layout(ctypes.byref(d), kop, seg)
    if n < 1:
        raise HkpError("hkp_conv_x3_stat_layout failed (rc=%d): %s"
                       % (n, lib().hkp_last_error().decode(errors="replace")))
    return tuple((seg[2 * i], seg[2 * i + 1]) for i in range(n))


def _seg_table(segments):
    flat = [v for rt in segments for v in rt]
    return (ctypes.c_int32 * len(flat))(*flat)


def conv2d_fwd_x3(xs, wp, stride=1, pad=0, dil=1, stats=True, out=None, part_out=None, sk=True, tile=0,
                  products=HKP_X3_ALL):
    """f16x3 NHWC conv on packed split operands: xs [N,H,W,2C] (from a producer with
    split=3), wp = weight_pack_x3(w) → fp32 y [N,Ho,Wo,K] (+ BN partials, into
    part_out when given).  sk=False: never stream-K (one tile per block);
    tile: HKP_TILE_* policy (0 = the planner); products: HKP_X3_ALL (f16x3), or
    HKP_X3_W16 / HKP_X3_X16 (two of the three products: the weights / the
    activation at fp16, hkp_conv2d_fwd_x3_products)."""
    ws, wsc = wp
    _need(xs, torch.float16, "conv2d_fwd_x3.x_split", 4)
    _need(ws, torch.float16, "conv2d_fwd_x3.w_split", 4)
    _need(wsc, torch.float32, "conv2d_fwd_x3.w_inv_scale", 1)
    n, h, wd, c2 = xs.shape
    k, r, s, cw2 = ws.shape
    if cw2 != c2:
        raise HkpError("conv2d_fwd_x3: weight Cin %d != input C %d" % (cw2 // 2, c2 // 2))
    c = c2 // 2
    ho, wo = conv_out_hw(h, wd, r, s, stride, pad, dil)
    d = ConvDesc(n, h, wd, c, k, r, s, stride, pad, dil, HKP_LAYOUT_NHWC, tile)
    y = out if out is not None else torch.empty((n, ho, wo, k), device=xs.device, dtype=torch.float32)
    kop = HKP_KOP_FWD_X3 if products == HKP_X3_ALL else HKP_KOP_FWD_X3_W16 if products == 2 else HKP_KOP_FWD_X3_X16
    part = None
    if stats:
        rows, segs = CONV_TILE_ROWS, None
        if tile in (HKP_TILE_192_A3, HKP_TILE_160_A3, HKP_TILE_MIX_A3):
            # 96- / 80-row statistic tiles, or a mixed-height launch's segments (the library says)
            segs = conv_stat_layout(d, kop)
            rows = segs[0][0]
        part = _stat_partials(n * ho * wo, k, xs.device, part_out, "conv2d_fwd_x3.part_out", rows, segs)

    if products == HKP_X3_ALL:
        def launch():
            call("hkp_conv2d_fwd_x3", ctypes.byref(d), _ptr(xs), _ptr(ws), _ptr(wsc), _ptr(y), _ptr(part),
                 *_sk_workspace(sk), _stream())
    else:
        def launch():
            call("hkp_conv2d_fwd_x3_products", ctypes.byref(d), _ptr(xs), _ptr(ws), _ptr(wsc), int(products),
                 _ptr(y), _ptr(part), *_sk_workspace(sk), _stream())

    if _observer is None:
        launch()
    else:
        _observer(kernel_name(d, kop, sk), 2.0 * n * ho * wo * k * r * s * c,
                  2.0 * (xs.numel() + ws.numel()) + 4.0 * y.numel(), launch)
    return y, part


def bnin_kernel(n, h, w, c, k, r, s, stride, pad, dil, f16=False, tile=0, sk=True):
    """The kernel a fused-input-BN conv (hkp_conv2d_fwd_x3_bnin / _f16_bnin) of this
    shape runs, or None where it has none: the fused conv runs where the unfused
    one runs the halo-tile body (conv_x3_halo_bnin_kernel<P>) — the same tiles
    and summation order, so the same bits."""
    cg = 64 if f16 else 32
    if c % cg or k % 64:
        return None
    try:
        ho, wo = conv_out_hw(h, w, r, s, stride, pad, dil)
    except HkpError:
        return None
    d = ConvDesc(n, h, w, c, k, r, s, stride, pad, dil, HKP_LAYOUT_NHWC, tile)
    name = kernel_name(d, HKP_KOP_FWD_F16 if f16 else HKP_KOP_FWD_X3, sk)
    if name.startswith("conv_x3_halo_kernel<"):
        return name.replace("_kernel<", "_bnin_kernel<")
    return None


def conv2d_fwd_bnin(y_in, in_ss, wp, stride=1, pad=1, dil=1, stats=True, sk=True, tile=0):
    """Inference conv whose input is the producer conv's raw output y_in with the
    producer's BN + ReLU applied inside the conv (hkp_conv2d_fwd_x3_bnin for fp32
    y_in with wp = weight_pack_x3(w); hkp_conv2d_fwd_f16_bnin for fp16 y_in with
    wp = weight_pack_f16(w)): the same y (and BN partials) as
    conv2d_fwd_x3(bn_apply(y_in, in_ss, relu, split=3)) / conv2d_fwd_f16(
    bn_apply_f16(y_in, in_ss, relu)) with the same sk / tile, bit for bit, without
    the apply pass (shapes: bnin_kernel)."""
    ws, wsc = wp
    f16 = y_in.dtype == torch.float16
    _need(y_in, torch.float16 if f16 else torch.float32, "conv2d_fwd_bnin.y_in", 4)
    _need(in_ss, torch.float32, "conv2d_fwd_bnin.in_scale_shift", 1)
    _need(ws, torch.float16, "conv2d_fwd_bnin.w", 4)
    n, h, wd, c = y_in.shape
    k, r, s, cw = ws.shape
    if cw != (c if f16 else 2 * c):
        raise HkpError("conv2d_fwd_bnin: weight Cin %d != input C %d" % (cw if f16 else cw // 2, c))
    if in_ss.numel() != 2 * c:
        raise HkpError("conv2d_fwd_bnin: in_scale_shift size %d != 2C" % in_ss.numel())
    ho, wo = conv_out_hw(h, wd, r, s, stride, pad, dil)
    d = ConvDesc(n, h, wd, c, k, r, s, stride, pad, dil, HKP_LAYOUT_NHWC, tile)
    y = torch.empty((n, ho, wo, k), device=y_in.device, dtype=torch.float16 if f16 else torch.float32)
    part = _stat_partials(n * ho * wo, k, y_in.device, None, "conv2d_fwd_bnin") if stats else None
    fn = "hkp_conv2d_fwd_f16_bnin" if f16 else "hkp_conv2d_fwd_x3_bnin"

    def launch():
        call(fn, ctypes.byref(d), _ptr(y_in), _ptr(in_ss), _ptr(ws), _ptr(wsc), _ptr(y), _ptr(part),
             *_sk_workspace(sk), _stream())

    if _observer is None:
        launch()
    else:
        name = kernel_name(d, HKP_KOP_FWD_F16 if f16 else HKP_KOP_FWD_X3, sk).replace("_kernel<", "_bnin_kernel<")
        _observer(name, 2.0 * n * ho * wo * k * r * s * c,
                  y_in.element_size() * y_in.numel() + 2.0 * ws.numel() + y.element_size() * y.numel(), launch)
    return y, part


def weight_pack_f16(w):
    """fp32 KRSC weight → PackedWeight: [K, R, S, C] fp16 (each output channel scaled
    by a power of two) + [K] inverse scales — the plain-fp16 conv's operand."""
    _need(w, torch.float32, "weight_pack_f16.w", 4)
    k, r, s, c = w.shape
    out = torch.empty((k, r, s, c), device=w.device, dtype=torch.float16)
    sc = torch.empty(k, device=w.device, dtype=torch.float32)
    call("hkp_weight_pack_f16", k, r * s * c, _ptr(w), _ptr(out), _ptr(sc), _stream())
    return PackedWeight(out, sc)


def conv2d_fwd_f16(x16, wp, stride=1, pad=0, dil=1, stats=True, sk=True, tile=0):
    """Plain-fp16 NHWC conv (BASELINE config C4): x16 fp16 [N,H,W,C] (a producer's
    split=1 output), wp = weight_pack_f16(w) → y fp16 [N,Ho,Wo,K] (autocast
    semantics) + BN partials from the fp32 accumulators."""
    ws, wsc = wp
    _need(x16, torch.float16, "conv2d_fwd_f16.x", 4)
    _need(ws, torch.float16, "conv2d_fwd_f16.w", 4)
    _need(wsc, torch.float32, "conv2d_fwd_f16.w_inv_scale", 1)
    n, h, wd, c = x16.shape
    k, r, s, cw = ws.shape
    if cw != c:
        raise HkpError("conv2d_fwd_f16: weight Cin %d != input C %d" % (cw, c))
    ho, wo = conv_out_hw(h, wd, r, s, stride, pad, dil)
    d = ConvDesc(n, h, wd, c, k, r, s, stride, pad, dil, HKP_LAYOUT_NHWC, tile)
    y = torch.empty((n, ho, wo, k), device=x16.device, dtype=torch.float16)
    part = _stat_partials(n * ho * wo, k, x16.device, None, "conv2d_fwd_f16") if stats else None

    def launch():
        call("hkp_conv2d_fwd_f16", ctypes.byref(d), _ptr(x16), _ptr(ws), _ptr(wsc), _ptr(y), _ptr(part),
             *_sk_workspace(sk), _stream())

    if _observer is None:
        launch()
    else:
        _observer(kernel_name(d, HKP_KOP_FWD_F16, sk), 2.0 * n * ho * wo * k * r * s * c,
                  2.0 * (x16.numel() + ws.numel() + y.numel()), launch)
    return y, part


def conv2d_fwd_f16_bn(x16, wp, ss, res=None, res_ss=None, relu=True, stride=1, pad=0, dil=1, sk=True, tile=0):
    """conv2d_fwd_f16 with the output's BN apply fused into the epilogue
    (hkp_conv2d_fwd_f16_bn): fp16 out = [relu](y*scale + shift [+ res | + res*rscale
    + rshift]) — what conv2d_fwd_f16 + bn_apply_f16 return with the same ss, y
    never written.  ss [2K] must be known before the conv (bn_from_gram, or
    eval-mode BN).  Returns the fp16 activation (a split=1 operand)."""
    ws, wsc = wp
    _need(x16, torch.float16, "conv2d_fwd_f16_bn.x", 4)
    _need(ws, torch.float16, "conv2d_fwd_f16_bn.w", 4)
    _need(wsc, torch.float32, "conv2d_fwd_f16_bn.w_inv_scale", 1)
    _need(ss, torch.float32, "conv2d_fwd_f16_bn.scale_shift", 1)
    n, h, wd, c = x16.shape
    k, r, s_, cw = ws.shape
    if cw != c:
        raise HkpError("conv2d_fwd_f16_bn: weight Cin %d != input C %d" % (cw, c))
    if ss.numel() != 2 * k:
        raise HkpError("conv2d_fwd_f16_bn: scale_shift size %d != 2K" % ss.numel())
    ho, wo = conv_out_hw(h, wd, r, s_, stride, pad, dil)
    if res is not None:
        _need(res, torch.float16, "conv2d_fwd_f16_bn.res", 4)
        if tuple(res.shape) != (n, ho, wo, k):
            raise HkpError("conv2d_fwd_f16_bn: residual %s != %s" % (tuple(res.shape), (n, ho, wo, k)))
    if res_ss is not None:
        _need(res_ss, torch.float32, "conv2d_fwd_f16_bn.res_scale_shift", 1)
        if res is None or res_ss.numel() != 2 * k:
            raise HkpError("conv2d_fwd_f16_bn: res_scale_shift needs a residual and 2K entries")
    d = ConvDesc(n, h, wd, c, k, r, s_, stride, pad, dil, HKP_LAYOUT_NHWC, tile)
    out = _split_out((n, ho, wo, k), x16.device, 1)

    def launch():
        call("hkp_conv2d_fwd_f16_bn", ctypes.byref(d), _ptr(x16), _ptr(ws), _ptr(wsc), _ptr(ss), _ptr(res),
             _ptr(res_ss), int(bool(relu)), _ptr(out), *_sk_workspace(sk), _stream())

    if _observer is None:
        launch()
    else:
        _observer(kernel_name(d, HKP_KOP_FWD_F16_BN, sk), 2.0 * n * ho * wo * k * r * s_ * c,
                  2.0 * (x16.numel() + ws.numel() + out.numel() + (res.numel() if res is not None else 0)), launch)
    return out


def gram_f16(a16):
    """Mean and second moments of the channels of an fp16 activation [.., C] over
    all its pixels (hkp_gram_f16) → (mean fp64 [C], E = a^T a / M fp64 [C, C])."""
    from ._lib import lib
    _need(a16, torch.float16, "gram_f16.a")
    c = a16.shape[-1]
    m = a16.numel() // c
    nb = lib().hkp_gram_f16_workspace_bytes(m, c)
    if nb < 0:
        raise HkpError("gram_f16: unsupported shape (m=%d c=%d)" % (m, c))
    ws = torch.empty((nb + 7) // 8, device=a16.device, dtype=torch.float64)
    mean = torch.empty(c, device=a16.device, dtype=torch.float64)
    second = torch.empty((c, c), device=a16.device, dtype=torch.float64)
    call("hkp_gram_f16", m, c, _ptr(a16), _ptr(mean), _ptr(second), _ptr(ws), nb, _stream())
    return mean, second


def bn_from_gram(mean, second, wp, count, gamma, beta, running_mean=None, running_var=None,
                 num_batches_tracked=None, momentum=0.1, eps=1e-5):
    """Train-mode BN parameters of the output of a 1x1 conv with packed fp16 weight
    wp (weight_pack_f16 of [K,1,1,C]) from its input's mean / second moments
    (gram_f16) → (scale_shift [2K], mean_invstd [2K]); running stats updated as
    bn_finalize does."""
    ws, wsc = wp
    _need(mean, torch.float64, "bn_from_gram.mean", 1)
    _need(second, torch.float64, "bn_from_gram.second", 2)
    _need(ws, torch.float16, "bn_from_gram.w", 4)
    k, r, s_, c = ws.shape
    if (r, s_) != (1, 1) or mean.numel() != c or tuple(second.shape) != (c, c):
        raise HkpError("bn_from_gram: needs a 1x1 weight over the gram's %d channels (got %s)"
                       % (mean.numel(), tuple(ws.shape)))
    for t, nm in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        if t is not None:
            _need(t, torch.float32, "bn_from_gram." + nm, 1)
            if t.numel() != k:
                raise HkpError("bn_from_gram.%s: %d != K=%d" % (nm, t.numel(), k))
    from ._lib import lib
    ss = torch.empty(2 * k, device=ws.device, dtype=torch.float32)
    mi = torch.empty(2 * k, device=ws.device, dtype=torch.float32)
    nb = lib().hkp_bn_from_gram_workspace_bytes(k, c)
    work = torch.empty((max(nb, 8) + 7) // 8, device=ws.device, dtype=torch.float64)
    call("hkp_bn_from_gram", k, c, int(count), _ptr(mean), _ptr(second), _ptr(ws), _ptr(wsc), _ptr(gamma), _ptr(beta),
         momentum, eps, _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked), _ptr(ss), _ptr(mi),
         _ptr(work), work.numel() * 8, _stream())
    return ss, mi


def stem_x3_ok(x_shape, w_shape, stride, pad, dil):
    """Whether the stem conv (NCHW x, OIHW w) takes the f16x3 stem kernel."""
    def one(v):
        return int(v[0]) if isinstance(v, (tuple, list)) else int(v)
    k, c, r, s = w_shape
    return (r, s, one(stride), one(pad), one(dil)) == (7, 7, 2, 3, 1) and 1 <= c <= 4 and k % 64 == 0 \
        and x_shape[1] == c


def stem_weight_pack_x3(w):
    """OIHW [K,C<=4,7,7] fp32 stem weight → PackedWeight [K,7,64] fp16 + [K] scales."""
    _need(w, torch.float32, "stem_weight_pack_x3.w", 4)
    k, c = w.shape[:2]
    out = torch.empty((k, 7, 64), device=w.device, dtype=torch.float16)
    sc = torch.empty(k, device=w.device, dtype=torch.float32)
    call("hkp_stem_weight_pack_x3", k, c, _ptr(w), _ptr(out), _ptr(sc), _stream())
    return PackedWeight(out, sc)


# A/B (tools/infer_ab.py stem_img=0): the image-direct stem off by default in this process
STEM_IMAGE_DIRECT = True


def conv2d_fwd_stem_x3(x, wp, k, stats=True, part_out=None, tile=0, image_direct=None):
    """f16x3 stem conv (7x7/s2/p3) → NHWC fp32 y (+ BN partials).  x: the NCHW fp32
    image, or the uint8 NHWC (BGR) batch cv2.imread gives — ToTensor's /255 is then
    fused into the stem's operand split.  tile: 0 = the patch body
    where the output tiles into 8 x 32 patches, HKP_TILE_64_PAIR = the one-tile
    stem (the BN partials then group raster-order rows instead of patches).  On the
    patch body the image is split per tile in LDS (hkp_conv2d_fwd_stem_x3_image:
    no packed planes in HBM) unless image_direct=False (pack + planes, the same
    bits)."""
    from ._lib import lib
    ws, wsc = wp
    u8 = x.dtype == torch.uint8
    _need(x, torch.uint8 if u8 else torch.float32, "conv2d_fwd_stem_x3.x", 4)
    _need(ws, torch.float16, "conv2d_fwd_stem_x3.w_split", 3)
    if u8:
        n, h, wd, c = x.shape
    else:
        n, c, h, wd = x.shape
    d = ConvDesc(n, h, wd, c, k, 7, 7, 2, 3, 1, HKP_LAYOUT_NCHW, tile)
    ho, wo = conv_out_hw(h, wd, 7, 7, 2, 3, 1)
    y = torch.empty((n, ho, wo, k), device=x.device, dtype=torch.float32)
    part = _stat_partials(n * ho * wo, k, x.device, part_out, "conv2d_fwd_stem_x3.part_out") if stats else None
    if image_direct is None:
        image_direct = STEM_IMAGE_DIRECT
    if image_direct and lib().hkp_stem_x3_image_ok(ctypes.byref(d)):
        xin = x.contiguous()
        op = HKP_KOP_STEM_X3_IMAGE_U8 if u8 else HKP_KOP_STEM_X3_IMAGE

        def launch():
            call("hkp_conv2d_fwd_stem_x3_image", ctypes.byref(d), _ptr(xin), 1 if u8 else 0, _ptr(ws), _ptr(wsc),
                 _ptr(y), _ptr(part), _stream())
        nbytes = float(xin.numel() * xin.element_size()) + 2.0 * ws.numel() + 4.0 * y.numel()
    else:
        xs = torch.empty(lib().hkp_stem_pack_x3_elems(ctypes.byref(d)), device=x.device, dtype=torch.float16)
        call("hkp_stem_pack_x3_u8" if u8 else "hkp_stem_pack_x3", ctypes.byref(d), _ptr(x), _ptr(xs), _stream())
        op = HKP_KOP_STEM_X3

        def launch():
            call("hkp_conv2d_fwd_stem_x3", ctypes.byref(d), _ptr(xs), _ptr(ws), _ptr(wsc), _ptr(y), _ptr(part),
                 _stream())
        nbytes = 2.0 * (xs.numel() + ws.numel()) + 4.0 * y.numel()
    if _observer is None:
        launch()
    else:
        _observer(kernel_name(d, op), 2.0 * n * ho * wo * k * 49 * c, nbytes, launch)
    return y, part


def images_u8_to_nchw(img):
    """ToTensor on the device: uint8 [B,H,W,C] (BGR, cv2.imread) → fp32 [B,C,H,W] / 255."""
    _need(img, torch.uint8, "images_u8_to_nchw.img", 4)
    n, h, w, c = img.shape
    x = torch.empty((n, c, h, w), device=img.device, dtype=torch.float32)
    call("hkp_images_u8_to_nchw", n, h, w, c, _ptr(img), _ptr(x), _stream())
    return x


def augment_u8(img, plan):
    """Domain randomisation (dataset.py:18-31): img uint8 [B,H,W,3] BGR and the batch's
    hkp.augment.Plan (one program per image) → the augmented uint8 [B,H,W,3], one
    launch on the current stream.  The plan's arrays are uploaded on that stream."""
    _need(img, torch.uint8, "augment_u8.img", 4)
    n, h, w, c = img.shape
    if c != 3:
        raise HkpError("augment_u8: img must be [B,H,W,3], got %s" % (tuple(img.shape),))
    if n < 1 or h < 3 or w < 3:
        raise HkpError("augment_u8: need B >= 1 and H, W >= 3 (reflect-101 borders), got %s" % (tuple(img.shape),))
    if getattr(plan, "n", None) != n:
        raise HkpError("augment_u8: the plan holds %s programs for a batch of %d" % (getattr(plan, "n", None), n))
    progs, luts = plan.device_arrays(img.device)
    table = plan.table.on(img.device)
    out = torch.empty_like(img)
    call("hkp_augment_u8", n, h, w, _ptr(img), _ptr(out), plan.programs, _ptr(progs), _ptr(luts), _ptr(table),
         _stream())
    return out


def warp_affine_u8(img, plan, out_hw=None):
    """Batched affine warp (csrc/warp.hip): img uint8 [B,Hs,Ws,3] and the batch's
    hkp.geometry.WarpPlan (one transform per image) → uint8 [B,H,W,3] with
    (H, W) = out_hw, default the plan's own size; one launch on the current stream.
    The plan's records are uploaded on that stream."""
    from ._lib import HKP_WARP_BORDER_REFLECT101, HKP_WARP_MAX_DIM
    _need(img, torch.uint8, "warp_affine_u8.img", 4)
    n, hs, ws, c = img.shape
    if c != 3:
        raise HkpError("warp_affine_u8: img must be [B,H,W,3], got %s" % (tuple(img.shape),))
    if n < 1 or not (1 <= hs <= HKP_WARP_MAX_DIM and 1 <= ws <= HKP_WARP_MAX_DIM):
        raise HkpError("warp_affine_u8: need B >= 1 and H, W in 1..%d, got %s" % (HKP_WARP_MAX_DIM, tuple(img.shape)))
    if getattr(plan, "n", None) != n:
        raise HkpError("warp_affine_u8: the plan holds %s transforms for a batch of %d" % (getattr(plan, "n", None), n))
    h, w = plan.hw if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    if not (1 <= h <= HKP_WARP_MAX_DIM and 1 <= w <= HKP_WARP_MAX_DIM):
        raise HkpError("warp_affine_u8: out_hw %dx%d outside 1..%d" % (h, w, HKP_WARP_MAX_DIM))
    if plan.border == HKP_WARP_BORDER_REFLECT101 and (hs < 2 or ws < 2):
        raise HkpError("warp_affine_u8: reflect101 needs a source of at least 2x2, got %dx%d" % (hs, ws))
    xf = plan.device_array(img.device)
    out = torch.empty((n, h, w, 3), device=img.device, dtype=torch.uint8)
    call("hkp_warp_affine_u8", n, hs, ws, _ptr(img), h, w, _ptr(out), plan.xforms, _ptr(xf), plan.interp,
         plan.border, _stream())
    return out


def warp_mask_u8(mask, plan, fill=0, out_hw=None, lut=None, out=None):
    """The ignore masks of a batch through its images' transforms (hkp_warp_mask_u8): mask
    uint8 [B,Hs,Ws] and the batch's hkp.geometry.WarpPlan -> uint8 [B,H,W], one launch on the
    current stream.  The plan's matrices and border are used, its interp is not: a mask is
    always sampled nearest, by the image warp's own rule.  fill (0..255): the byte a pixel
    outside the source gets under border="constant" (0: trained, 255: ignored for every
    class).  lut: uint8 [B,256] on mask's device, the table each source byte goes through
    (hkp.masks.flip_lut per flipped image; WarpPlan.apply_mask builds it), or None.  out: a
    contiguous uint8 [B,H,W] tensor to write into (it may be an unaligned view)."""
    from ._lib import HKP_WARP_BORDER_REFLECT101, HKP_WARP_MAX_DIM
    if isinstance(fill, bool) or not isinstance(fill, int) or not 0 <= fill <= 255:
        raise HkpError("warp_mask_u8: fill is an integer in 0..255, got %r" % (fill,))
    _need(mask, torch.uint8, "warp_mask_u8.mask", 3)
    n, hs, ws = mask.shape
    if n < 1 or not (1 <= hs <= HKP_WARP_MAX_DIM and 1 <= ws <= HKP_WARP_MAX_DIM):
        raise HkpError("warp_mask_u8: need B >= 1 and H, W in 1..%d, got %s" % (HKP_WARP_MAX_DIM, tuple(mask.shape)))
    if getattr(plan, "n", None) != n:
        raise HkpError("warp_mask_u8: the plan holds %s transforms for a batch of %d" % (getattr(plan, "n", None), n))
    h, w = plan.hw if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    if not (1 <= h <= HKP_WARP_MAX_DIM and 1 <= w <= HKP_WARP_MAX_DIM):
        raise HkpError("warp_mask_u8: out_hw %dx%d outside 1..%d" % (h, w, HKP_WARP_MAX_DIM))
    if plan.border == HKP_WARP_BORDER_REFLECT101 and (hs < 2 or ws < 2):
        raise HkpError("warp_mask_u8: reflect101 needs a source of at least 2x2, got %dx%d" % (hs, ws))
    if lut is not None:
        _need(lut, torch.uint8, "warp_mask_u8.lut", 2)
        if tuple(lut.shape) != (n, 256) or lut.device != mask.device:
            raise HkpError("warp_mask_u8: lut must be uint8 [%d,256] on %s, got %s on %s"
                           % (n, mask.device, tuple(lut.shape), lut.device))
    xf = plan.device_array(mask.device)
    if out is None:
        out = torch.empty((n, h, w), device=mask.device, dtype=torch.uint8)
    else:
        _need(out, torch.uint8, "warp_mask_u8.out", 3)
        if tuple(out.shape) != (n, h, w) or out.device != mask.device:
            raise HkpError("warp_mask_u8: out must be uint8 [%d,%d,%d] on %s, got %s on %s"
                           % (n, h, w, mask.device, tuple(out.shape), out.device))
    call("hkp_warp_mask_u8", n, hs, ws, _ptr(mask), h, w, _ptr(out), plan.xforms, _ptr(xf), plan.border, fill,
         _ptr(lut), _stream())
    return out


def mask_regions_u8(regions, H, W, out=None):
    """Ignore masks from region records (hkp_mask_regions_u8): regions float32 [N,R,6] =
    (kind, a, b, c, d, bits) on the device, 1 <= R <= 64, as hkp.masks.pack builds them ->
    uint8 [N,H,W], every byte written in one launch on the current stream.  kind 1: the box
    a <= x <= c, b <= y <= d; kind 2: the disc (x-a)^2 + (y-b)^2 <= c^2 (fp32); any other
    kind: an empty slot.  A pixel gets the OR of the bits of the regions that hold it.
    out: a uint8 [N,H,W] tensor to write into (it may be an unaligned view, as long as it is
    contiguous)."""
    from ._lib import HKP_MASK_MAX_DIM, HKP_MASK_MAX_REGIONS
    H, W = int(H), int(W)
    if not (1 <= H <= HKP_MASK_MAX_DIM and 1 <= W <= HKP_MASK_MAX_DIM):
        raise HkpError("mask_regions_u8: H, W must be in 1..%d, got %dx%d" % (HKP_MASK_MAX_DIM, H, W))
    if not isinstance(regions, torch.Tensor) or regions.dtype != torch.float32 or regions.dim() != 3 or \
            regions.shape[2] != 6 or not 1 <= regions.shape[1] <= HKP_MASK_MAX_REGIONS or regions.shape[0] < 1:
        raise HkpError("mask_regions_u8: regions must be float32 [N,R,6] with 1 <= R <= %d, got %s"
                       % (HKP_MASK_MAX_REGIONS, "%s %s" % (regions.dtype, tuple(regions.shape))
                          if isinstance(regions, torch.Tensor) else type(regions).__name__))
    _need(regions, torch.float32, "mask_regions_u8.regions", 3)
    n, r = regions.shape[:2]
    if out is None:
        out = torch.empty((n, H, W), device=regions.device, dtype=torch.uint8)
    else:
        _need(out, torch.uint8, "mask_regions_u8.out", 3)
        if tuple(out.shape) != (n, H, W) or out.device != regions.device:
            raise HkpError("mask_regions_u8: out must be uint8 [%d,%d,%d] on %s, got %s on %s"
                           % (n, H, W, regions.device, tuple(out.shape), out.device))
    call("hkp_mask_regions_u8", n, r, H, W, _ptr(regions), _ptr(out), _stream())
    return out


def synth_cables_u8(plan, out=None):
    """Procedural cable scenes (csrc/synth.hip): the batch's hkp.synth.SynthPlan (one scene
    per image) → uint8 [B,H,W,3] BGR on the current device, one launch on the current
    stream; the plan's records are uploaded on that stream.  out: a uint8 [B,H,W,3] device
    tensor to render into (rows may start at any byte address), else a new one."""
    from ._lib import HKP_SYNTH_MAX_DIM
    n, (h, w) = getattr(plan, "n", None), getattr(plan, "hw", (0, 0))
    if not n or not (1 <= h <= HKP_SYNTH_MAX_DIM and 1 <= w <= HKP_SYNTH_MAX_DIM):
        raise HkpError("synth_cables_u8: need a SynthPlan of B >= 1 images of H, W in 1..%d, got %r %r"
                       % (HKP_SYNTH_MAX_DIM, n, (h, w)))
    if out is None:
        out = torch.empty((n, h, w, 3), device=torch.device("cuda", torch.cuda.current_device()), dtype=torch.uint8)
    else:
        _need(out, torch.uint8, "synth_cables_u8.out", 4)
        if tuple(out.shape) != (n, h, w, 3):
            raise HkpError("synth_cables_u8: out must be %s, got %s" % ((n, h, w, 3), tuple(out.shape)))
    scenes, segs = plan.device_arrays(out.device)
    call("hkp_synth_cables_u8", n, h, w, _ptr(out), plan.scenes, _ptr(scenes), plan.segs, _ptr(segs), plan.nsegs,
         _stream())
    return out


def resize_u8(img, h, w, interp="bilinear"):
    """img uint8 [B,Hs,Ws,3] → [B,h,w,3]: the affine warp with the half-pixel-centre
    resize matrix and replicated borders.  No antialiasing: large reductions alias."""
    from . import geometry
    from ._lib import HKP_WARP_MAX_DIM
    if interp not in geometry.INTERP:
        raise HkpError("resize_u8: unknown interp %r (known: %s)" % (interp, ", ".join(geometry.INTERP)))
    _need(img, torch.uint8, "resize_u8.img", 4)
    n, hs, ws, c = img.shape
    if c != 3 or n < 1 or hs < 1 or ws < 1:
        raise HkpError("resize_u8: img must be a non-empty [B,H,W,3], got %s" % (tuple(img.shape),))
    h, w = int(h), int(w)
    if not (1 <= h <= HKP_WARP_MAX_DIM and 1 <= w <= HKP_WARP_MAX_DIM):
        raise HkpError("resize_u8: output %dx%d outside 1..%d" % (h, w, HKP_WARP_MAX_DIM))
    m = geometry.resize_matrix(hs, ws, h, w)
    plan = geometry.WarpPlan([m] * n, (h, w), interp=interp, border="replicate")
    return warp_affine_u8(img, plan)


def resample_ragged_u8(flat, plan):
    """Antialiased resize (csrc/resample.hip) of a batch of images of different
    sizes: flat uint8 [plan.in_bytes] on the device, the images of plan.sizes packed
    one after the other, and the batch's hkp.resample.ResamplePlan → uint8
    [B,h,w,3] with (h, w) = plan.hw; one launch on the current stream, bit for bit
    Pillow's Image.resize(..., reducing_gap=None).  The plan's records and tables
    are uploaded on that stream."""
    _need(flat, torch.uint8, "resample_ragged_u8.flat", 1)
    n = getattr(plan, "n", None)
    if n is None or n < 1:
        raise HkpError("resample_ragged_u8: expected a ResamplePlan, got %s" % type(plan).__name__)
    if flat.numel() != plan.in_bytes:
        raise HkpError("resample_ragged_u8: the plan's %d images take %d bytes, the buffer has %d"
                       % (n, plan.in_bytes, flat.numel()))
    h, w = plan.hw
    recs, tables = plan.device_arrays(flat.device)
    out = torch.empty((n, h, w, 3), device=flat.device, dtype=torch.uint8)
    call("hkp_resample_u8", n, _ptr(flat), plan.in_bytes, plan.records, _ptr(recs),
         ctypes.c_void_p(plan.tables.ctypes.data), _ptr(tables), plan.tables.size, h, w, _ptr(out), _stream())
    return out


def resample_u8(img, h, w, filter="bilinear", mode="stretch", fill=(0, 0, 0)):
    """img uint8 [B,Hs,Ws,3] → [B,h,w,3], antialiased: Pillow's Image.resize((w, h),
    filter, reducing_gap=None) bit for bit.  filter: "box", "bilinear", "hamming",
    "bicubic", "lanczos"; mode "stretch", or "fit" (aspect ratio kept, the rest
    filled with `fill`, (B, G, R))."""
    from . import resample
    _need(img, torch.uint8, "resample_u8.img", 4)
    n, hs, ws, c = img.shape
    if c != 3 or n < 1 or hs < 1 or ws < 1:
        raise HkpError("resample_u8: img must be a non-empty [B,H,W,3], got %s" % (tuple(img.shape),))
    plan = resample.ResamplePlan([(hs, ws)] * n, (h, w), filter=filter, mode=mode, fill=fill)
    return resample_ragged_u8(img.reshape(-1), plan)


def heat_overlay(heat, img, yx):
    """Prediction.plot's picture on the GPU: heat [B,K,H,W] fp32,
    img uint8 [B,H,W,3] BGR, yx int32 [B,K,2] argmax → uint8 [B, H*K/2, 2W, 3]
    (K = 1: [B,H,W,3]) — the reference's two-column grid of JET overlays."""
    _need(heat, torch.float32, "heat_overlay.heat", 4)
    _need(img, torch.uint8, "heat_overlay.img", 4)
    _need(yx, torch.int32, "heat_overlay.yx", 3)
    n, k, h, w = heat.shape
    if tuple(img.shape) != (n, h, w, 3) or tuple(yx.shape) != (n, k, 2):
        raise HkpError("heat_overlay: img %s / yx %s do not match heat %s" % (tuple(img.shape), tuple(yx.shape),
                                                                            tuple(heat.shape)))
    if k != 1 and k % 2:
        raise HkpError("heat_overlay: K must be 1 or even (two equal columns)")
    out = torch.empty((n, h, w, 3) if k == 1 else (n, h * (k // 2), 2 * w, 3), device=heat.device,
                      dtype=torch.uint8)
    mm = torch.empty(n * k * 2, device=heat.device, dtype=torch.float32)
    call("hkp_heat_overlay", n, k, h, w, _ptr(heat), _ptr(img), _ptr(yx), _ptr(mm), _ptr(out), _stream())
    return out


def soft_argmax(heat, beta=1.0):
    """heat [N,K,H,W] fp32 → float32 [N,K,2] (x, y): softmax(beta*h)-weighted mean
    position per plane — Prediction.expectation (prediction.py:31-38) with its
    axis mix-up fixed."""
    _need(heat, torch.float32, "soft_argmax.heat", 4)
    n, k, h, w = heat.shape
    out = torch.empty((n, k, 2), device=heat.device, dtype=torch.float32)
    call("hkp_soft_argmax", n, k, h, w, float(beta), _ptr(heat), _ptr(out), _stream())
    return out


HEAT_PEAKS_MAX_NODES = 32768          # PEAKS_CAP of csrc/head.hip: h * w of one plane


def heat_peaks(low, H, W, max_peaks=4, radius=1, threshold=0.0):
    """lowres logits [N,K,h,w] fp32 (what keypoints_forward returns as `low`) →
    (peaks float32 [N,K,max_peaks,3], counts int32 [N,K]): per plane the up to
    max_peaks best local maxima of its (2 radius + 1)^2 windows with
    sigmoid(logit) >= threshold, best first, each as (x, y, score) — (x, y), the
    order of soft_argmax and the labels, NOT the (y, x) of the argmax — with x, y
    sub-lattice positions in pixels of the H x W output (align_corners frame) and
    score the heatmap's value at the node.  Unused slots hold (-1, -1, 0).  The
    definition is hkp_heat_peaks's (include/hulkkp.h); no heatmap is formed."""
    _need(low, torch.float32, "heat_peaks.lowres", 4)
    n, k, h, w = low.shape
    if min(n, k, h, w) < 1 or h * w > HEAT_PEAKS_MAX_NODES:
        raise HkpError("heat_peaks: lowres %s: need non-empty planes of at most %d nodes"
                       % (tuple(low.shape), HEAT_PEAKS_MAX_NODES))
    H, W, max_peaks, radius, threshold = int(H), int(W), int(max_peaks), int(radius), float(threshold)
    if not 1 <= max_peaks <= 16 or not 1 <= radius <= 8 or not 0.0 <= threshold <= 1.0 or H < 1 or W < 1:
        raise HkpError("heat_peaks: need 1 <= max_peaks <= 16, 1 <= radius <= 8, 0 <= threshold <= 1, H, W >= 1 "
                       "(got max_peaks=%d radius=%d threshold=%g H=%d W=%d)" % (max_peaks, radius, threshold, H, W))
    peaks = torch.empty((n, k, max_peaks, 3), device=low.device, dtype=torch.float32)
    counts = torch.empty((n, k), device=low.device, dtype=torch.int32)
    call("hkp_heat_peaks", n, k, h, w, H, W, radius, max_peaks, threshold, _ptr(low), _ptr(peaks), _ptr(counts),
         _stream())
    return peaks, counts


# the packed views of logits_merge, one flat fp32 buffer per (device, stream), grown
# on demand: launches sharing a stream never run concurrently
_merge_buf = {}


def logits_merge(lows, plan_or_table, perm=None, mode="prob", out=None):
    """Test-time augmentation's merge (csrc/tta.hip): lows, one fp32 [N,K,h_v,w_v]
    tensor per view, and the launch's hkp.tta.MergePlan — or its pieces: a sequence
    of (h_v, w_v, ay, by, ax, bx, weight) per view with perm, integers [views, K],
    both on the host — → fp32 [N,K,h,w] on the plan's base lattice; the definition
    is hkp_logits_merge's (include/hulkkp.h).  mode: "prob" or "logit".  The views
    are copied into one reused flat buffer (at most 8 small copies), then one launch
    on the current stream; the plan's table and perm are uploaded once.  out: an
    fp32 tensor of the result's shape to write into (any 4-byte alignment)."""
    from . import tta
    if mode not in tta.MODES:
        raise HkpError("logits_merge: unknown mode %r (known: %s)" % (mode, ", ".join(tta.MODES)))
    lows = list(lows)
    if not 1 <= len(lows) <= tta.HKP_MERGE_MAX_VIEWS:
        raise HkpError("logits_merge: %d views outside 1..%d" % (len(lows), tta.HKP_MERGE_MAX_VIEWS))
    for i, t in enumerate(lows):
        _need(t, torch.float32, "logits_merge.lows[%d]" % i, 4)
        if t.device != lows[0].device or tuple(t.shape[:2]) != tuple(lows[0].shape[:2]) or t.numel() == 0:
            raise HkpError("logits_merge: view %d is %s on %s, view 0 %s on %s: need non-empty views of one batch on "
                           "one device" % (i, tuple(t.shape), t.device, tuple(lows[0].shape), lows[0].device))
    n, k = lows[0].shape[:2]
    if isinstance(plan_or_table, tta.MergePlan):
        plan = plan_or_table
        if perm is not None:
            raise HkpError("logits_merge: a MergePlan carries its own perm")
    else:
        if perm is None:
            raise HkpError("logits_merge: a view table needs perm")
        plan = tta.MergePlan(n, k, lows[0].shape[2:] if out is None else out.shape[2:], plan_or_table, perm)
    if (plan.n, plan.k, plan.n_views) != (n, k, len(lows)):
        raise HkpError("logits_merge: the plan is for %d views of [%d,%d,..], got %d of [%d,%d,..]"
                       % (plan.n_views, plan.n, plan.k, len(lows), n, k))
    for i, t in enumerate(lows):
        if tuple(t.shape[2:]) != plan.lattices[i]:
            raise HkpError("logits_merge: view %d has lattice %s, the plan %s" % (i, tuple(t.shape[2:]), plan.lattices[i]))
    h, w = plan.hw
    dev = lows[0].device
    if out is None:
        out = torch.empty((n, k, h, w), device=dev, dtype=torch.float32)
    else:
        _need(out, torch.float32, "logits_merge.out", 4)
        if tuple(out.shape) != (n, k, h, w) or out.device != dev:
            raise HkpError("logits_merge: out must be %s on %s, got %s on %s" % ((n, k, h, w), dev, tuple(out.shape),
                                                                               out.device))
    st = torch.cuda.current_stream(dev)
    key = (st.device_index, st.cuda_stream)
    buf = _merge_buf.get(key)
    if buf is None or buf.numel() < plan.total:
        buf = _merge_buf[key] = torch.empty(plan.total, device=dev, dtype=torch.float32)
    for r, t in zip(plan.records, lows):
        buf[r.off:r.off + t.numel()].copy_(t.reshape(-1))
    table, perm_d = plan.device_arrays(dev)
    call("hkp_logits_merge", n, k, h, w, plan.n_views, tta.MODES[mode], _ptr(buf), _ptr(table), _ptr(perm_d), _ptr(out),
         ctypes.c_void_p(st.cuda_stream))
    return out


# two-level finalize (hkp_bn_finalize_ws) from this many partial tiles on: C4 +2.2 %
# (R50 C = 2048 convs, 4,800+ tiles); at 300-1,200 tiles (C2 layer2-4, the C3
# shard) the one-kernel merge already fills the chip and its single launch won
# (C2 neutral, C3 training -1.2 % with the two-level form everywhere)
FIN_TWO_LEVEL_TILES = 2048


def bn_finalize(part, count, gamma, beta, running_mean=None, running_var=None, num_batches_tracked=None,
                momentum=0.1, eps=1e-5, want_mean_invstd=True, two_level_tiles=FIN_TWO_LEVEL_TILES):
    """Train-mode BN statistics from conv partials → (scale_shift [2C], mean_invstd [2C]).
    Lists of >= two_level_tiles tiles take the two-level merge (hkp_bn_finalize_ws)."""
    _need(part, torch.float32, "bn_finalize.partials", 3)
    tiles, c, _ = part.shape
    ss = torch.empty(2 * c, device=part.device, dtype=torch.float32)
    mi = torch.empty(2 * c, device=part.device, dtype=torch.float32) if want_mean_invstd else None
    for t, nm in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        if t is not None:
            _need(t, torch.float32, "bn_finalize." + nm, 1)
            if t.numel() != c:
                raise HkpError("bn_finalize.%s: %d != C=%d" % (nm, t.numel(), c))
    if num_batches_tracked is not None:
        _need(num_batches_tracked, torch.int64, "bn_finalize.num_batches_tracked")
    segs = stat_segments(part)
    if segs is not None:
        # a mixed-height conv's segmented list: the same merges, tile rows from the table
        ws, nb = None, 0
        if tiles >= two_level_tiles:
            from ._lib import lib
            nb = lib().hkp_bn_finalize_workspace_bytes(c, tiles)
            ws = torch.empty((nb + 7) // 8, device=part.device, dtype=torch.float64)
        call("hkp_bn_finalize_seg", c, count, len(segs), _seg_table(segs), _ptr(part), _ptr(gamma), _ptr(beta),
             momentum, eps, _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked), _ptr(ss), _ptr(mi),
             _ptr(ws), nb, _stream())
        return ss, mi
    if tiles >= two_level_tiles:
        # two-level merge (chunks of 128 tiles over [C/64][chunks] blocks, then per channel)
        from ._lib import lib
        nb = lib().hkp_bn_finalize_workspace_bytes(c, tiles)
        ws = torch.empty((nb + 7) // 8, device=part.device, dtype=torch.float64)
        call("hkp_bn_finalize_ws", c, count, tiles, stat_tile_rows(part), _ptr(part), _ptr(gamma), _ptr(beta), momentum,
             eps, _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked), _ptr(ss), _ptr(mi), _ptr(ws),
             nb, _stream())
        return ss, mi
    call("hkp_bn_finalize", c, count, tiles, stat_tile_rows(part), _ptr(part), _ptr(gamma), _ptr(beta), momentum, eps,
         _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked), _ptr(ss), _ptr(mi), _stream())
    return ss, mi


def bn_stats(part, count, two_level_tiles=FIN_TWO_LEVEL_TILES):
    """SyncBN: this rank's per-channel BN statistics from its conv tile partials →
    fp64 [2C+1] = [mean | M2 | count] (hkp_bn_stats; gathered in rank order and
    merged by bn_finalize_ranks)."""
    _need(part, torch.float32, "bn_stats.partials", 3)
    tiles, c, _ = part.shape
    st = torch.empty(2 * c + 1, device=part.device, dtype=torch.float64)
    ws, nb = None, 0
    if tiles >= two_level_tiles:
        from ._lib import lib
        nb = lib().hkp_bn_finalize_workspace_bytes(c, tiles)
        ws = torch.empty((nb + 7) // 8, device=part.device, dtype=torch.float64)
    segs = stat_segments(part)
    if segs is not None:
        call("hkp_bn_stats_seg", c, count, len(segs), _seg_table(segs), _ptr(part), _ptr(st), _ptr(ws), nb, _stream())
        return st
    call("hkp_bn_stats", c, count, tiles, stat_tile_rows(part), _ptr(part), _ptr(st), _ptr(ws), nb, _stream())
    return st


def bn_finalize_ranks(stats, gamma, beta, running_mean=None, running_var=None, num_batches_tracked=None,
                      momentum=0.1, eps=1e-5):
    """SyncBN: the ranks' bn_stats blocks [R, 2C+1] (rank order) merged in fixed
    order → (scale_shift [2C], mean_invstd [2C]) of the global batch, as bn_finalize."""
    _need(stats, torch.float64, "bn_finalize_ranks.stats", 2)
    r, l = stats.shape
    if l % 2 != 1:
        raise HkpError("bn_finalize_ranks.stats: row length %d is not 2C+1" % l)
    c = (l - 1) // 2
    for t, nm in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        if t is not None:
            _need(t, torch.float32, "bn_finalize_ranks." + nm, 1)
            if t.numel() != c:
                raise HkpError("bn_finalize_ranks.%s: %d != C=%d" % (nm, t.numel(), c))
    if num_batches_tracked is not None:
        _need(num_batches_tracked, torch.int64, "bn_finalize_ranks.num_batches_tracked")
    ss = torch.empty(2 * c, device=stats.device, dtype=torch.float32)
    mi = torch.empty(2 * c, device=stats.device, dtype=torch.float32)
    call("hkp_bn_finalize_ranks", c, r, _ptr(stats.contiguous()), _ptr(gamma), _ptr(beta), momentum, eps,
         _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked), _ptr(ss), _ptr(mi), _stream())
    return ss, mi


def bn_eval_params(gamma, beta, running_mean, running_var, eps=1e-5):
    c = running_mean.numel()
    ss = torch.empty(2 * c, device=running_mean.device, dtype=torch.float32)
    mi = torch.empty(2 * c, device=running_mean.device, dtype=torch.float32)
    call("hkp_bn_eval_params", c, _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), eps, _ptr(ss),
         _ptr(mi), _stream())
    return ss, mi


def _split_out(shape, device, split):
    """Split output of a producer: passes 1 → fp16 [.., C]; passes 3 → packed [.., 2C]."""
    shp = tuple(shape[:-1]) + (shape[-1] * (2 if split == 3 else 1),)
    t = torch.empty(shp, device=device, dtype=torch.float16)
    t._hkp_split_passes = split
    return t


def _check_split(split, c, who):
    if split not in (0, 1, 3):
        raise HkpError("%s: split must be 0, 1 or 3" % who)
    if split and c % 32:
        raise HkpError("%s: split output needs C %% 32 == 0 (C=%d)" % (who, c))


def bn_apply(y, ss, res=None, res_ss=None, relu=True, out=None, split=0, keep_fp32=True):
    """out = [relu](y*scale+shift [+ res | + res*rscale+rshift]).
    split = 1 or 3 also writes the next conv's operand (attached as out._hkp_split);
    keep_fp32=False (with split): the fp32 activation is not written and the split
    tensor itself is returned (an activation only a conv consumes).  res may be a
    split-only activation (packed, split=3): the residual is then read as hi + lo."""
    _need(y, torch.float32, "bn_apply.y")
    c = y.shape[-1]
    m = y.numel() // c
    _check_split(split, c, "bn_apply")
    if ss.numel() != 2 * c:
        raise HkpError("bn_apply: scale_shift size %d != 2C" % ss.numel())
    if res_ss is not None and res_ss.numel() != 2 * c:
        raise HkpError("bn_apply: res_scale_shift size %d != 2C" % res_ss.numel())
    res_sp = None
    if res is not None and res.dtype == torch.float16:
        if res_ss is not None or getattr(res, "_hkp_split_passes", 0) != 3:
            raise HkpError("bn_apply: a split residual must be a packed (split=3) raw residual")
        _need(res, torch.float16, "bn_apply.res_split")
        if tuple(res.shape[:-1]) != tuple(y.shape[:-1]) or res.shape[-1] != 2 * c:
            raise HkpError("bn_apply: split residual shape %s vs %s" % (tuple(res.shape), tuple(y.shape)))
        res, res_sp = None, res
    elif res is not None:
        _need(res, torch.float32, "bn_apply.res")
        if res.shape != y.shape:
            raise HkpError("bn_apply: residual shape %s != %s" % (tuple(res.shape), tuple(y.shape)))
    if not keep_fp32 and not split:
        raise HkpError("bn_apply: keep_fp32=False needs a split output")
    o = None if not keep_fp32 else (out if out is not None else torch.empty_like(y))
    sp = _split_out(y.shape, y.device, split) if split else None
    call("hkp_bn_apply", m, c, _ptr(y), _ptr(ss), _ptr(res), _ptr(res_ss), _ptr(res_sp), int(bool(relu)), _ptr(o),
         _ptr(sp), int(split), _stream())
    if o is None:
        return sp
    if split:
        o._hkp_split = (sp, split)
    return o


def bn_apply_f16(y16, ss, res=None, res_ss=None, relu=True, keep_fp32=False):
    """Plain-fp16 path (config C4): fp16 out = [relu](y16*scale+shift [+ res | +
    res*rscale+rshift]), res an fp16 activation or (with res_ss) the downsample's
    fp16 y.  Returns the fp16 activation (a split=1 operand of the next conv), or
    with keep_fp32 the fp32 copy carrying it as its split (the head reads fp32)."""
    _need(y16, torch.float16, "bn_apply_f16.y")
    c = y16.shape[-1]
    m = y16.numel() // c
    if ss.numel() != 2 * c:
        raise HkpError("bn_apply_f16: scale_shift size %d != 2C" % ss.numel())
    if res is not None:
        _need(res, torch.float16, "bn_apply_f16.res")
        if res.shape != y16.shape:
            raise HkpError("bn_apply_f16: residual shape %s != %s" % (tuple(res.shape), tuple(y16.shape)))
    if res_ss is not None and (res is None or res_ss.numel() != 2 * c):
        raise HkpError("bn_apply_f16: res_scale_shift needs a residual and 2C entries")
    out = _split_out(y16.shape, y16.device, 1)
    o32 = torch.empty(y16.shape, device=y16.device, dtype=torch.float32) if keep_fp32 else None
    call("hkp_bn_apply_f16", m, c, _ptr(y16), _ptr(ss), _ptr(res), _ptr(res_ss), int(bool(relu)), _ptr(out),
         _ptr(o32), _stream())
    if o32 is None:
        return out
    o32._hkp_split = (out, 1)
    return o32


def bn_relu_maxpool(y, ss, split=0, route=False, keep_fp32=True):
    """maxpool3x3/s2/p1(relu(y*scale+shift)); route=True (training) also records
    each window's gradient tap as out._hkp_route (uint8, out's shape) for maxpool_bwd.
    keep_fp32=False (with split): only the split is written and returned."""
    _need(y, torch.float32, "bn_relu_maxpool.y", 4)
    n, h, w, c = y.shape
    _check_split(split, c, "bn_relu_maxpool")
    if not keep_fp32 and (not split or route):
        raise HkpError("bn_relu_maxpool: keep_fp32=False needs a split output and no route")
    shape = (n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c)
    out = torch.empty(shape, device=y.device, dtype=torch.float32) if keep_fp32 else None
    sp = _split_out(shape, y.device, split) if split else None
    rt = torch.empty(shape, device=y.device, dtype=torch.uint8) if route else None
    call("hkp_bn_relu_maxpool", n, h, w, c, _ptr(y), _ptr(ss), _ptr(out), _ptr(sp), int(split), _ptr(rt),
         _stream())
    if out is None:
        return sp
    if split:
        out._hkp_split = (sp, split)
    if route:
        out._hkp_route = rt
    return out


HEAD_FC_LDS_FLOATS = 16384  # hkp_head_fc's k*c limit (head.hip: its [K][C] rows in 64 KiB of LDS)


def head_fc(feat, w_kc, bias_k):
    """feat NHWC [N,h,w,C]; w [K,C]; bias [K] → lowres NCHW [N,K,h,w].
    hkp_head_fc stages its rows in 64 KiB of LDS (K*C <= 16384 floats): more rows
    than that (C = 2048 with K > 8) run in row chunks, concatenated along K."""
    _need(feat, torch.float32, "head_fc.feat", 4)
    _need(w_kc, torch.float32, "head_fc.w", 2)
    _need(bias_k, torch.float32, "head_fc.bias", 1)
    n, h, w, c = feat.shape
    k = w_kc.shape[0]
    if w_kc.shape[1] != c or bias_k.numel() != k:
        raise HkpError("head_fc: weight %s / bias %s do not match C=%d" % (tuple(w_kc.shape), bias_k.numel(), c))
    if k * c > HEAD_FC_LDS_FLOATS:
        rows = min(16, HEAD_FC_LDS_FLOATS // max(c, 1))
        if rows == 0:
            raise HkpError("head_fc: C=%d: one row does not fit the kernel's LDS (%d floats)"
                           % (c, HEAD_FC_LDS_FLOATS))
        # (row slices of contiguous [K,C] / [K] tensors are contiguous)
        return torch.cat([head_fc(feat, w_kc[k0:k0 + rows], bias_k[k0:k0 + rows]) for k0 in range(0, k, rows)], 1)
    low = torch.empty((n, k, h, w), device=feat.device, dtype=torch.float32)
    call("hkp_head_fc", n, h * w, c, k, _ptr(feat), _ptr(w_kc), _ptr(bias_k), _ptr(low), _stream())
    return low


def head_fusable(c, k):
    """hkp_bn_apply_head covers this (channels, keypoints) pair."""
    return c % 512 == 0 and c <= 2048 and 0 < k <= 16


def bn_apply_head(y, ss, res, res_ss, w_kc, bias_k):
    """Inference tail: lowres [N,K,h,w] = head_fc(relu(y*scale+shift + residual))
    without writing the feature map.  y fp32 or fp16 NHWC; res: None, a raw
    residual of y's dtype, a packed split-only activation (fp32 y), or (with
    res_ss) the downsample's y."""
    n, h, w, c = y.shape
    k = w_kc.shape[0]
    if y.dtype not in (torch.float32, torch.float16):
        raise HkpError("bn_apply_head: y must be fp32 or fp16")
    _need(y, y.dtype, "bn_apply_head.y", 4)
    _need(w_kc, torch.float32, "bn_apply_head.w", 2)
    _need(bias_k, torch.float32, "bn_apply_head.bias", 1)
    if not head_fusable(c, k) or w_kc.shape[1] != c or bias_k.numel() != k or ss.numel() != 2 * c:
        raise HkpError("bn_apply_head: C=%d K=%d weight %s bias %d ss %d" % (c, k, tuple(w_kc.shape), bias_k.numel(),
                                                                         ss.numel()))
    kind = 0
    if res is not None:
        if res.dtype == torch.float16 and y.dtype == torch.float32:
            if res_ss is not None or getattr(res, "_hkp_split_passes", 0) != 3 or res.shape[-1] != 2 * c:
                raise HkpError("bn_apply_head: a split residual must be a packed (split=3) raw residual")
            kind = 3
        else:
            if res.dtype != y.dtype or res.shape != y.shape:
                raise HkpError("bn_apply_head: residual %s %s vs y %s %s" % (res.dtype, tuple(res.shape), y.dtype,
                                                                           tuple(y.shape)))
            kind = 2 if res_ss is not None else 1
        _need(res, res.dtype, "bn_apply_head.res")
        if tuple(res.shape[:-1]) != tuple(y.shape[:-1]):
            raise HkpError("bn_apply_head: residual pixels %s vs %s" % (tuple(res.shape), tuple(y.shape)))
    if res_ss is not None and (res is None or res_ss.numel() != 2 * c):
        raise HkpError("bn_apply_head: res_scale_shift needs a residual and 2C entries")
    low = torch.empty((n, k, h, w), device=y.device, dtype=torch.float32)
    call("hkp_bn_apply_head", n, h * w, c, k, int(y.dtype == torch.float16), _ptr(y), _ptr(ss), _ptr(res),
         _ptr(res_ss), kind, _ptr(w_kc), _ptr(bias_k), _ptr(low), _stream())
    return low


def upsample_sigmoid(low, H, W, heat=True, argmax=True, sigmoid=True, out=None):
    """lowres [N,K,h,w] → (heat [N,K,H,W] (into out when given) or None, argmax
    int32 [N,K,2] (y,x) or None)."""
    _need(low, torch.float32, "upsample_sigmoid.lowres", 4)
    n, k, h, w = low.shape
    hm = None
    if heat:
        hm = out if out is not None else torch.empty((n, k, H, W), device=low.device, dtype=torch.float32)
        _need(hm, torch.float32, "upsample_sigmoid.out", 4)
        if tuple(hm.shape) != (n, k, H, W):
            raise HkpError("upsample_sigmoid: out shape %s != %s" % (tuple(hm.shape), (n, k, H, W)))
    ws = yx = None
    if argmax:
        from ._lib import lib
        ws = torch.empty(lib().hkp_upsample_argmax_ws_bytes(n, k, H, W) // 8, device=low.device, dtype=torch.int64)
        yx = torch.empty((n, k, 2), device=low.device, dtype=torch.int32)
    call("hkp_upsample_sigmoid", n, k, h, w, H, W, int(bool(sigmoid)), _ptr(low), _ptr(hm), _ptr(ws), _ptr(yx), _stream())
    return hm, yx


def gauss_target(uv, H, W, sigma):
    """uv float32 [N,K,2] (u=x, v=y) → float64 [N,K,H,W]."""
    _need(uv, torch.float32, "gauss_target.uv", 3)
    n, k, _ = uv.shape
    out = torch.empty((n, k, H, W), device=uv.device, dtype=torch.float64)
    call("hkp_gauss_target", n, k, H, W, float(sigma), _ptr(uv), _ptr(out), _stream())
    return out


def _need_pts(pts, name):
    """Instance labels float32 [N,K,M,3] (u, v, flag), 1 <= M <= 16, on the GPU."""
    from ._lib import MAX_INSTANCES
    _need(pts, torch.float32, name, 4)
    if pts.shape[3] != 3 or not 1 <= pts.shape[2] <= MAX_INSTANCES or pts.shape[0] < 1 or pts.shape[1] < 1:
        raise HkpError("%s: expected [N,K,M,3] with 1 <= M <= %d, got %s" % (name, MAX_INSTANCES, tuple(pts.shape)))


def gauss_target_multi(pts, H, W, sigma):
    """pts float32 [N,K,M,3] (u=x, v=y, flag; flag > 0: present) → float64 [N,K,H,W]:
    the maximum of the present instances' Gaussians, 0 for a plane with none."""
    _need_pts(pts, "gauss_target_multi.pts")
    n, k, m, _ = pts.shape
    if int(H) < 1 or int(W) < 1 or not float(sigma) > 0:
        raise HkpError("gauss_target_multi: bad size %sx%s or sigma %s" % (H, W, sigma))
    out = torch.empty((n, k, int(H), int(W)), device=pts.device, dtype=torch.float64)
    call("hkp_gauss_target_multi", n, k, m, int(H), int(W), float(sigma), _ptr(pts), _ptr(out), _stream())
    return out


def _lines_shape(lines, name):
    """Line labels are a tensor [N,K,S,5], 1 <= S <= 128 (the shape alone: nothing is read)."""
    from ._lib import HKP_LINE_MAX_S
    if not isinstance(lines, torch.Tensor):
        raise HkpError("%s: expected a tensor" % name)
    if lines.dim() != 4 or lines.shape[3] != 5 or not 1 <= lines.shape[2] <= HKP_LINE_MAX_S or lines.shape[0] < 1 \
            or lines.shape[1] < 1:
        raise HkpError("%s: expected [N,K,S,5] with 1 <= S <= %d, got %s" % (name, HKP_LINE_MAX_S, tuple(lines.shape)))


def _need_lines(lines, name):
    """Line labels float32 [N,K,S,5] (x0, y0, x1, y1, flag), 1 <= S <= 128, on the GPU."""
    _lines_shape(lines, name)
    _need(lines, torch.float32, name, 4)


def line_target(lines, H, W, sigma=8.0, want_target=True, want_d2=False, out=None, out_d2=None):
    """lines float32 [N,K,S,5] (x0, y0, x1, y1, flag; flag > 0: present) → (target, d2):
    d2 float32 [N,K,H,W], the squared distance to the nearest present segment (+inf for a
    plane with none), and target float64 [N,K,H,W] = exp(-d2 / (2 sigma^2)) (0 for a plane
    with none); whichever is not wanted is None.  A zero-length segment is a point.  out /
    out_d2: preallocated outputs (contiguous, of the output's shape and dtype)."""
    import math
    if not (want_target or want_d2):
        raise HkpError("line_target: neither target nor d2 is wanted")
    if int(H) < 1 or int(W) < 1 or int(H) * int(W) > 1 << 30:
        raise HkpError("line_target: bad size %sx%s (H, W >= 1, H*W <= 2^30)" % (H, W))
    if not (float(sigma) > 0 and math.isfinite(float(sigma))):
        raise HkpError("line_target: sigma %s must be finite and > 0" % (sigma,))
    _need_lines(lines, "line_target.lines")
    n, k, s, _ = lines.shape
    H, W = int(H), int(W)
    for o, want, dtype, name in ((out, want_target, torch.float64, "out"), (out_d2, want_d2, torch.float32, "out_d2")):
        if o is None:
            continue
        if not want:
            raise HkpError("line_target: %s given but not wanted" % name)
        _need(o, dtype, "line_target." + name, 4)
        if tuple(o.shape) != (n, k, H, W) or o.device != lines.device:
            raise HkpError("line_target: %s %s on %s does not go with lines %s on %s, %dx%d"
                           % (name, tuple(o.shape), o.device, tuple(lines.shape), lines.device, H, W))
    if want_target and out is None:
        out = torch.empty((n, k, H, W), device=lines.device, dtype=torch.float64)
    if want_d2 and out_d2 is None:
        out_d2 = torch.empty((n, k, H, W), device=lines.device, dtype=torch.float32)
    call("hkp_line_target", n, k, s, H, W, float(sigma), _ptr(lines), _ptr(out), _ptr(out_d2), _stream())
    return out, out_d2


# ------------------------------------------------------------------ backward


def _shape4(shape, name):
    """`shape` as a tuple of four positive ints (a descriptor is built from it unchecked)."""
    try:
        sh = tuple(shape)
    except TypeError:
        sh = None
    if sh is None or len(sh) != 4 or not all(isinstance(v, int) and not isinstance(v, bool) and v > 0 for v in sh):
        raise HkpError("%s: expected four positive ints, got %r" % (name, shape))
    return sh


def _fwd_desc(x_shape, w_shape, stride, pad, dil, layout):
    if layout == "nhwc":
        n, h, wd, c = x_shape
        k, r, s, _ = w_shape
        lay = HKP_LAYOUT_NHWC
    else:
        n, c, h, wd = x_shape
        k, _, r, s = w_shape
        lay = HKP_LAYOUT_NCHW
    return ConvDesc(n, h, wd, c, k, r, s, stride, pad, dil, lay)


def conv_weight_flip(w):
    """KRSC [K,R,S,C] → flipped CRSK [C,R,S,K] (the dgrad weight)."""
    _need(w, torch.float32, "conv_weight_flip.w", 4)
    k, r, s, c = w.shape
    d = ConvDesc(1, 1, 1, c, k, r, s, 1, 0, 1, HKP_LAYOUT_NHWC)
    wf = torch.empty((c, r, s, k), device=w.device, dtype=torch.float32)
    call("hkp_conv_weight_flip", ctypes.byref(d), _ptr(w), _ptr(wf), _stream())
    return wf


def conv2d_bwd_data(dy, w_flip, x_shape, stride=1, pad=0, dil=1, add=None):
    """dL/dx (NHWC) of conv2d_fwd; ``add`` (same shape as x, nullable) is summed in."""
    _need(dy, torch.float32, "conv2d_bwd_data.dy", 4)
    _need(w_flip, torch.float32, "conv2d_bwd_data.w_flip", 4)
    x_shape = _shape4(x_shape, "conv2d_bwd_data.x_shape")
    c, r, s, k = w_flip.shape
    if c != x_shape[3]:
        raise HkpError("conv2d_bwd_data: w_flip Cin %d != x_shape C %d" % (c, x_shape[3]))
    d = _fwd_desc(x_shape, (k, r, s, c), stride, pad, dil, "nhwc")
    ho, wo = conv_out_hw(x_shape[1], x_shape[2], r, s, stride, pad, dil)
    if tuple(dy.shape) != (x_shape[0], ho, wo, k):
        raise HkpError("conv2d_bwd_data: dy shape %s != %s" % (tuple(dy.shape), (x_shape[0], ho, wo, k)))
    if add is not None:
        _need(add, torch.float32, "conv2d_bwd_data.add", 4)
        if tuple(add.shape) != tuple(x_shape):
            raise HkpError("conv2d_bwd_data: add shape mismatch")
    dx = torch.empty(tuple(x_shape), device=dy.device, dtype=torch.float32)
    call("hkp_conv2d_bwd_data", ctypes.byref(d), _ptr(dy), _ptr(w_flip), _ptr(add), _ptr(dx), _stream())
    return dx


def absmax(x):
    """max |x| as a device uint32 (IEEE bits) — feeds the split kernels' power-of-two scaling."""
    _need(x, torch.float32, "absmax.x")
    out = torch.empty(1, device=x.device, dtype=torch.int32)
    call("hkp_absmax", x.numel(), _ptr(x), _ptr(out), _stream())
    return out


def split_pack_x3(x, amax=None):
    """fp32 NHWC x (scaled by the power of two of amax, if given) → packed split [.., 2C]."""
    _need(x, torch.float32, "split_pack_x3.x")
    c = x.shape[-1]
    out = torch.empty(tuple(x.shape[:-1]) + (2 * c,), device=x.device, dtype=torch.float16)
    call("hkp_split_pack_x3", x.numel(), c, _ptr(x), _ptr(amax), _ptr(out), _stream())
    out._hkp_split_passes = 3
    return out


def weight_flip_pack_x3(w):
    """KRSC [K,R,S,C] fp32 → packed flipped [C,R,S,2K] fp16 for conv2d_bwd_data_x3."""
    _need(w, torch.float32, "weight_flip_pack_x3.w", 4)
    k, r, s, c = w.shape
    d = ConvDesc(1, 1, 1, c, k, r, s, 1, 0, 1, HKP_LAYOUT_NHWC)
    out = torch.empty((c, r, s, 2 * k), device=w.device, dtype=torch.float16)
    sc = torch.empty(c, device=w.device, dtype=torch.float32)
    call("hkp_weight_flip_pack_x3", ctypes.byref(d), _ptr(w), _ptr(out), _ptr(sc), _stream())
    return PackedWeight(out, sc)


def phase_taps(r, pad, phase, stride=2):
    """Taps of output phase `phase` along a filter axis of r taps (hkp_phase_taps)."""
    from ._lib import lib
    return lib().hkp_phase_taps(r, pad, stride, phase)


def weight_pack_x3_batch(items, outs=None, keep_launch=None):
    """Many weight packs in one launch pair (hkp_weight_pack_x3_batch): items =
    [(kind, w)] with kind "x3" (= weight_pack_x3(w)) or "flip_x3"
    (= weight_flip_pack_x3(w)), or ("phase_x3", w, (phase, pad)) — output phase
    phase = py*2+px of a stride-2 conv's dgrad operand (conv2d_bwd_data_x3_strided);
    returns the PackedWeights in order.  outs (optional, same order; None entries
    allowed) are PackedWeights to overwrite.  keep_launch (a dict, optional)
    receives a `relaunch()` that repeats this exact launch (same pointers) — for
    callers that repack the same weights in place every step."""
    from ._lib import PackJob, lib
    jobs = (PackJob * max(1, len(items)))()
    res = []
    for i, item in enumerate(items):
        kind, w = item[0], item[1]
        _need(w, torch.float32, "weight_pack_x3_batch.w", 4)
        k, r, s, c = w.shape
        if kind == "x3":
            code, shape, n_sc = 0, (k, r, s, 2 * c), k
        elif kind == "flip_x3":
            code, shape, n_sc = 1, (c, r, s, 2 * k), c
        elif kind == "phase_x3":
            ph, pad = item[2]
            r2, s2 = phase_taps(r, pad, ph >> 1), phase_taps(s, pad, ph & 1)
            if r2 <= 0 or s2 <= 0:
                raise HkpError("weight_pack_x3_batch: phase %d has no taps" % ph)
            code, shape, n_sc = 2, (c, r2, s2, 2 * k), c
            jobs[i].r, jobs[i].s, jobs[i].pad, jobs[i].phase = r, s, pad, ph
        else:
            raise HkpError("weight_pack_x3_batch: unknown kind %r" % (kind,))
        o = outs[i] if outs is not None else None
        if o is None or tuple(o.split.shape) != shape or o.split.device != w.device:
            o = PackedWeight(torch.empty(shape, device=w.device, dtype=torch.float16),
                             torch.empty(n_sc, device=w.device, dtype=torch.float32))
        res.append(o)
        jobs[i].w, jobs[i].out, jobs[i].inv_scale = _ptr(w), _ptr(o.split), _ptr(o.inv_scale)
        jobs[i].kind, jobs[i].k, jobs[i].rs, jobs[i].c = code, k, r * s, c
    if not items:
        return res
    nb = lib().hkp_weight_pack_x3_batch_ws_bytes(len(items), jobs)
    ws = torch.empty(max(4, nb), device=items[0][1].device, dtype=torch.uint8)
    n = len(items)

    def relaunch():
        call("hkp_weight_pack_x3_batch", n, jobs, _ptr(ws), nb, _stream())

    relaunch()
    if keep_launch is not None:
        keep_launch["relaunch"] = relaunch
    return res


def weight_phase_pack_x3(w, pad):
    """The four output-phase dgrad operands of a stride-2 KRSC conv weight (None for a
    phase no tap reaches), for conv2d_bwd_data_x3_strided."""
    k, r, s, c = w.shape
    phases = [ph for ph in range(4) if phase_taps(r, pad, ph >> 1) > 0 and phase_taps(s, pad, ph & 1) > 0]
    packs = weight_pack_x3_batch([("phase_x3", w, (ph, pad)) for ph in phases])
    out = [None] * 4
    for ph, pk in zip(phases, packs):
        out[ph] = pk
    return out


def conv2d_bwd_data_x3_strided(dys, phase_packs, x_shape, w_shape, pad=0, add=None, amax=None, sk=True, tile=0):
    """f16x3 dL/dx of a stride-2 (dilation-1) NHWC conv with KRSC weight shape
    w_shape, one stride-1 conv per output phase: dys = split_pack_x3(dy, amax),
    phase_packs = weight_phase_pack_x3(w, pad).  sk=False: no stream-K (one tile
    per block, e.g. while another stream's kernel shares the CUs)."""
    _need(dys, torch.float16, "conv2d_bwd_data_x3_strided.dy_split", 4)
    k, r, s, c = w_shape
    if len(phase_packs) != 4:
        raise HkpError("conv2d_bwd_data_x3_strided: need 4 phase packs (None for empty phases)")
    for ph, p in enumerate(phase_packs):
        taps = (phase_taps(r, pad, ph >> 1), phase_taps(s, pad, ph & 1))
        want = None if min(taps) <= 0 else (c,) + taps + (2 * k,)
        if (p is None) != (want is None) or (p is not None and tuple(p.split.shape) != want):
            raise HkpError("conv2d_bwd_data_x3_strided: phase %d pack %s, expected %s" % (
                ph, None if p is None else tuple(p.split.shape), want))
    d = _fwd_desc(x_shape, (k, r, s, c), 2, pad, 1, "nhwc")
    d.tile = tile
    ho, wo = conv_out_hw(x_shape[1], x_shape[2], r, s, 2, pad, 1)
    if tuple(dys.shape) != (x_shape[0], ho, wo, 2 * k):
        raise HkpError("conv2d_bwd_data_x3_strided: dy split shape %s != %s" % (tuple(dys.shape),
                                                                               (x_shape[0], ho, wo, 2 * k)))
    if add is not None:
        _need(add, torch.float32, "conv2d_bwd_data_x3_strided.add", 4)
        if tuple(add.shape) != tuple(x_shape):
            raise HkpError("conv2d_bwd_data_x3_strided: add shape mismatch")
    dx = torch.empty(tuple(x_shape), device=dys.device, dtype=torch.float32)
    sp = (ctypes.c_void_p * 4)(*[None if p is None else p.split.data_ptr() for p in phase_packs])
    sc = (ctypes.c_void_p * 4)(*[None if p is None else p.inv_scale.data_ptr() for p in phase_packs])
    call("hkp_conv2d_bwd_data_x3_strided", ctypes.byref(d), _ptr(dys), sp, sc, _ptr(amax), _ptr(add), _ptr(dx),
         *_sk_workspace(sk), _stream())
    return dx


def conv2d_bwd_data_x3(dys, wfp, x_shape, pad=0, dil=1, add=None, amax=None, sk=True, tile=0):
    """f16x3 dL/dx of a stride-1 NHWC conv from packed dy (split_pack_x3 with `amax`)
    and wfp = weight_flip_pack_x3(w).  sk=False: no stream-K; tile: HKP_TILE_*."""
    wfs, wfsc = wfp
    _need(dys, torch.float16, "conv2d_bwd_data_x3.dy_split", 4)
    _need(wfs, torch.float16, "conv2d_bwd_data_x3.wf_split", 4)
    c, r, s, k2 = wfs.shape
    k = k2 // 2
    d = _fwd_desc(x_shape, (k, r, s, c), 1, pad, dil, "nhwc")
    d.tile = tile
    ho, wo = conv_out_hw(x_shape[1], x_shape[2], r, s, 1, pad, dil)
    if tuple(dys.shape) != (x_shape[0], ho, wo, 2 * k):
        raise HkpError("conv2d_bwd_data_x3: dy split shape %s != %s" % (tuple(dys.shape), (x_shape[0], ho, wo, 2 * k)))
    if add is not None:
        _need(add, torch.float32, "conv2d_bwd_data_x3.add", 4)
        if tuple(add.shape) != tuple(x_shape):
            raise HkpError("conv2d_bwd_data_x3: add shape mismatch")
    dx = torch.empty(tuple(x_shape), device=dys.device, dtype=torch.float32)

    def launch():
        call("hkp_conv2d_bwd_data_x3", ctypes.byref(d), _ptr(dys), _ptr(wfs), _ptr(wfsc), _ptr(amax), _ptr(add),
             _ptr(dx), *_sk_workspace(sk), _stream())

    if _observer is None:
        launch()
    else:
        _observer(kernel_name(d, HKP_KOP_DGRAD_X3, sk),
                  2.0 * x_shape[0] * x_shape[1] * x_shape[2] * c * r * s * k,
                  2.0 * (dys.numel() + wfs.numel()) + 4.0 * dx.numel(), launch)
    return dx


# The wgrad's split-K slabs, one buffer per (device, launching stream), grown to the
# largest request: the launches on a stream run in order, each reading its slabs back
# (the reduce) before the next writes them.  A per-call allocation instead left each
# side-stream workspace pending on its stream's progress when freed: the caching
# allocator levelled off at 38 GB of blocks after ~25 C3 training steps, 28 GB with
# this buffer (5.6 GB without the overlap; step time unchanged; tools/alloc_probe.py).
_wg_ws = {}


def _wgrad_workspace(device, nbytes, alloc_stream=None):
    st = torch.cuda.current_stream(device)
    key = (st.device_index, st.cuda_stream)
    ws = _wg_ws.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        if ws is not None:
            ws.record_stream(st)                     # the last launches on st may still read it
        n = max(nbytes, 4) // 4
        if alloc_stream is None:
            ws = torch.empty(n, device=device, dtype=torch.float32)
        else:
            with torch.cuda.stream(alloc_stream):
                ws = torch.empty(n, device=device, dtype=torch.float32)
            ws.record_stream(st)
        _wg_ws[key] = ws
    return ws


def conv2d_bwd_filter_x3(xs, dys, w_shape, stride=1, pad=0, dil=1, amax=None, alloc_stream=None, cus=0):
    """f16x3 dL/dw (KRSC) from packed x (forward operand) and packed dy (split_pack_x3 with `amax`).
    cus: the CUs the grid should occupy (pixel-range splits = max(1, cus / tiles);
    0: the planner's count, filling whole rounds of every CU; -1: the planner's
    count on the tiled body — the halo body of 3x3 stride-1 convs off).
    alloc_stream: take dw (and a new workspace buffer) from that stream's memory pool (marked
    as used by the launching stream) — a side-stream wgrad then shares the main
    stream's cached blocks instead of growing a second pool (C5 at 245 GB: the
    second pool forced allocator flushes every step, 5x slower)."""
    from ._lib import lib
    _need(xs, torch.float16, "conv2d_bwd_filter_x3.x_split", 4)
    _need(dys, torch.float16, "conv2d_bwd_filter_x3.dy_split", 4)
    n, h, wd, c2 = xs.shape
    d = _fwd_desc((n, h, wd, c2 // 2), tuple(w_shape), stride, pad, dil, "nhwc")
    d.tile = int(cus)
    ho, wo = conv_out_hw(h, wd, d.r, d.s, stride, pad, dil)
    if tuple(dys.shape) != (n, ho, wo, 2 * d.k):
        raise HkpError("conv2d_bwd_filter_x3: dy split shape %s != %s" % (tuple(dys.shape), (n, ho, wo, 2 * d.k)))
    nbytes = lib().hkp_conv_bwd_filter_x3_workspace(ctypes.byref(d))
    ws = _wgrad_workspace(xs.device, nbytes, alloc_stream)
    if alloc_stream is None:
        dw = torch.empty(tuple(w_shape), device=xs.device, dtype=torch.float32)
    else:
        launching = torch.cuda.current_stream(xs.device)
        with torch.cuda.stream(alloc_stream):
            dw = torch.empty(tuple(w_shape), device=xs.device, dtype=torch.float32)
        dw.record_stream(launching)

    def launch():
        call("hkp_conv2d_bwd_filter_x3", ctypes.byref(d), _ptr(xs), _ptr(dys), _ptr(amax), _ptr(dw), _ptr(ws),
             nbytes, _stream())

    if _observer is None:
        launch()
    else:
        _observer(kernel_name(d, HKP_KOP_WGRAD_X3),
                  2.0 * n * ho * wo * d.k * d.r * d.s * d.c, 2.0 * (xs.numel() + dys.numel()) + 4.0 * dw.numel(),
                  launch)
    return dw


def conv2d_bwd_filter(x, dy, w_shape, stride=1, pad=0, dil=1, layout="nhwc", out=None, accumulate=False):
    """dL/dw in the weight's own layout (KRSC, or OIHW for the NCHW stem)."""
    _need(x, torch.float32, "conv2d_bwd_filter.x", 4)
    _need(dy, torch.float32, "conv2d_bwd_filter.dy", 4)
    w_shape = _shape4(w_shape, "conv2d_bwd_filter.w_shape")
    # the kernel writes k*r*s*C(x) floats: dw's Cin must be x's
    cw, c = (w_shape[3], x.shape[3]) if layout == "nhwc" else (w_shape[1], x.shape[1])
    if cw != c:
        raise HkpError("conv2d_bwd_filter: w_shape Cin %d != input C %d" % (cw, c))
    if out is not None:
        _need(out, torch.float32, "conv2d_bwd_filter.dw")
        if tuple(out.shape) != w_shape:
            raise HkpError("conv2d_bwd_filter: out shape %s != %s" % (tuple(out.shape), w_shape))
    elif accumulate:
        raise HkpError("conv2d_bwd_filter: accumulate=True needs out= (there is nothing to add to)")
    d = _fwd_desc(tuple(x.shape), w_shape, stride, pad, dil, layout)
    ho, wo = conv_out_hw(d.h, d.w, d.r, d.s, stride, pad, dil)
    if tuple(dy.shape) != (d.n, ho, wo, d.k):
        raise HkpError("conv2d_bwd_filter: dy shape %s != %s" % (tuple(dy.shape), (d.n, ho, wo, d.k)))
    from ._lib import lib
    nbytes = lib().hkp_conv_bwd_filter_workspace(ctypes.byref(d))
    ws = torch.empty(max(nbytes, 4) // 4, device=x.device, dtype=torch.float32)
    dw = out if out is not None else torch.empty(w_shape, device=x.device, dtype=torch.float32)
    call("hkp_conv2d_bwd_filter", ctypes.byref(d), _ptr(x), _ptr(dy), _ptr(dw), int(bool(accumulate)), _ptr(ws),
         nbytes, _stream())
    return dw


def bn_bwd_begin(g, out_mask, y, mean_invstd, gamma, want_dz=False, want_amax=False, split_only=False,
                 relu_ss=None):
    """First half of bn_bwd: validates and launches the reduce pass (per-tile
    channel sums; dz = g*mask when want_dz).  Returns the state bn_bwd_end /
    bn_bwd_local_stats take; state["dz"] is dz (written once the pass runs)."""
    _need(g, torch.float32, "bn_bwd.g")
    _need(y, torch.float32, "bn_bwd.y")
    if g.shape != y.shape or (out_mask is not None and out_mask.shape != y.shape):
        raise HkpError("bn_bwd: shape mismatch")
    c = y.shape[-1]
    if relu_ss is not None:
        if out_mask is not None:
            raise HkpError("bn_bwd: out_mask and relu_ss are exclusive")
        _need(relu_ss, torch.float32, "bn_bwd.relu_ss", 1)
        if relu_ss.numel() != 2 * c:
            raise HkpError("bn_bwd: relu_ss must be [2C]")
    m = y.numel() // c
    if split_only and c % 32:
        raise HkpError("bn_bwd: split_only needs C % 32 == 0")
    from ._lib import lib
    tiles = lib().hkp_bn_bwd_tiles(m)
    part = torch.empty((tiles, c, 2), device=y.device, dtype=torch.float32)
    maxima = torch.empty((tiles, c, 2), device=y.device, dtype=torch.float32) if split_only else None
    amax = torch.empty(1, device=y.device, dtype=torch.int32) if (want_amax or split_only) else None
    dz = torch.empty_like(y) if want_dz else None
    call("hkp_bn_bwd_reduce", m, c, _ptr(g), _ptr(out_mask), _ptr(relu_ss), _ptr(y), _ptr(mean_invstd), _ptr(dz),
         _ptr(part), _ptr(maxima), _ptr(amax if split_only else None), _stream())
    return dict(g=g, out_mask=out_mask, y=y, mi=mean_invstd, gamma=gamma, relu_ss=relu_ss, m=m, c=c, part=part,
                maxima=maxima, amax=amax, dz=dz, split_only=split_only, want_amax=want_amax)


def bn_bwd_local_stats(st):
    """SyncBN: this rank's [Σdz | Σdz·(y−mean) | max|dz| | max|y−mean| | m] fp64
    block (hkp_bn_bwd_stats) of a begun BN backward, to be all-gathered."""
    own = torch.empty(4 * st["c"] + 1, device=st["y"].device, dtype=torch.float64)
    call("hkp_bn_bwd_stats", st["c"], st["m"], _ptr(st["part"]), _ptr(st["maxima"]), _ptr(st["mi"]), _ptr(own),
         _stream())
    return own


def bn_bwd_end(st, ranks=None, own=None):
    """Second half of bn_bwd: coefficients (from this rank's sums, or — SyncBN —
    from `ranks` [R, 4C+1], every rank's bn_bwd_local_stats block in rank order,
    with `own` this rank's) and the apply pass → (dy, dgamma, dbeta, dz)."""
    y, c, m = st["y"], st["c"], st["m"]
    dgamma = torch.empty(c, device=y.device, dtype=torch.float32)
    dbeta = torch.empty(c, device=y.device, dtype=torch.float32)
    coef = torch.empty(3 * c, device=y.device, dtype=torch.float32)
    if ranks is None:
        call("hkp_bn_bwd_finalize", c, m, _ptr(st["part"]), _ptr(st["maxima"]), _ptr(st["mi"]), _ptr(st["gamma"]),
             _ptr(dgamma), _ptr(dbeta), _ptr(coef), _ptr(st["amax"]), _stream())
    else:
        _need(ranks, torch.float64, "bn_bwd_end.ranks")
        if ranks.dim() != 2 or ranks.shape[1] != 4 * c + 1 or own is None or own.numel() != 4 * c + 1:
            raise HkpError("bn_bwd_end: rank statistics must be [R, 4C+1] with this rank's block")
        call("hkp_bn_bwd_finalize_ranks", c, ranks.shape[0], _ptr(ranks.contiguous()), _ptr(own),
             1 if st["maxima"] is not None else 0, _ptr(st["mi"]), _ptr(st["gamma"]), _ptr(dgamma), _ptr(dbeta),
             _ptr(coef), _ptr(st["amax"]), _stream())
    if st["split_only"]:
        dy = _split_out(y.shape, y.device, 3)
        call("hkp_bn_bwd_apply", m, c, _ptr(st["g"]), _ptr(st["out_mask"]), _ptr(st["relu_ss"]), _ptr(y),
             _ptr(st["mi"]), _ptr(coef), None, _ptr(st["amax"]), _ptr(dy), _stream())
    else:
        dy = torch.empty_like(y)
        call("hkp_bn_bwd_apply", m, c, _ptr(st["g"]), _ptr(st["out_mask"]), _ptr(st["relu_ss"]), _ptr(y),
             _ptr(st["mi"]), _ptr(coef), _ptr(dy), _ptr(st["amax"]), None, _stream())
    if st["want_amax"] or st["split_only"]:
        dy._hkp_amax = st["amax"]
    return dy, dgamma, dbeta, st["dz"]


def bn_bwd(g, out_mask, y, mean_invstd, gamma, want_dz=False, want_amax=False, split_only=False, relu_ss=None,
           sync_group=None):
    """Train-mode BN(+ReLU mask) backward → (dy, dgamma, dbeta, dz or None).
    The ReLU mask is out_mask > 0, or (relu_ss = the forward's scale_shift) is
    recomputed from y bit-identically — no read of the fp32 activation.
    want_amax: max|dy| (uint32 IEEE bits, as absmax) is computed in the same pass
    and attached as dy._hkp_amax.  split_only: dy is returned as the packed f16x3
    split of dy * 2^e (the x3 backward convs' operand, _hkp_split_passes = 3) with
    2^e from an upper bound of max|dy| (attached as _hkp_amax, the scale's source);
    no fp32 dy is written.  sync_group = (group,): SyncBN — the dx coefficients
    from the channel sums of every rank of group (hkp.parallel.active_sync_group)."""
    st = bn_bwd_begin(g, out_mask, y, mean_invstd, gamma, want_dz, want_amax, split_only, relu_ss)
    if sync_group is None:
        return bn_bwd_end(st)
    from . import parallel
    own = bn_bwd_local_stats(st)
    return bn_bwd_end(st, parallel.gather_bn_stats(own, sync_group[0]), own)


def maxpool_bwd(dpool, route, in_shape):
    """Stem: dL/d(BN output) [in_shape] from dL/d(maxpool output) and the forward's
    route (bn_relu_maxpool(..., route=True)._hkp_route; ReLU mask included)."""
    _need(dpool, torch.float32, "maxpool_bwd.dpool", 4)
    _need(route, torch.uint8, "maxpool_bwd.route", 4)
    n, h, w, c = in_shape
    if tuple(dpool.shape) != (n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c) or route.shape != dpool.shape:
        raise HkpError("maxpool_bwd: dpool / route shape mismatch")
    dz = torch.empty(tuple(in_shape), device=dpool.device, dtype=torch.float32)
    call("hkp_maxpool_bwd", n, h, w, c, _ptr(dpool), _ptr(route), _ptr(dz), _stream())
    return dz


LOSS_KINDS = ("bce", "mse", "qfl")
NORM_MODES = ("elements", "instances")
ABSENT_MODES = ("zero", "ignore")


def _loss_choice(who, kind, norm, beta):
    """The names and beta of a loss call, checked before any tensor is looked at;
    returns beta as the float the kernel gets (2.0 when the kind has none)."""
    from ._lib import QFL_BETA_RANGE
    if kind not in LOSS_KINDS:
        raise HkpError("%s: unknown kind %r (known: %s)" % (who, kind, ", ".join(LOSS_KINDS)))
    if norm not in NORM_MODES:
        raise HkpError("%s: unknown norm %r (known: %s)" % (who, norm, ", ".join(NORM_MODES)))
    if kind != "qfl":
        return 2.0
    try:
        b = float(beta)
    except (TypeError, ValueError):
        raise HkpError("%s: beta must be a number, got %r" % (who, beta))
    if not QFL_BETA_RANGE[0] <= b <= QFL_BETA_RANGE[1]:          # NaN fails both
        raise HkpError("%s: beta %r outside [%g, %g]" % ((who, beta) + QFL_BETA_RANGE))
    return b


TOPK_MAX_K = 64                       # classes per image hkp_heat_loss_planes ranks


def _planes_choice(who, weights, topk, heat=None):
    """weights / topk of a loss call, checked before any kernel is called: their kinds,
    and against the shape and device of heat when it is given as [N,K,H,W]; returns topk
    as the int the kernel gets (0: off)."""
    if weights is not None and not isinstance(weights, torch.Tensor):
        raise HkpError("%s: weights must be a float32 tensor [N,K], got %s" % (who, type(weights).__name__))
    if topk is None:
        topk = 0
    elif isinstance(topk, bool) or not isinstance(topk, int):
        raise HkpError("%s: topk must be an int in 1..K or None, got %r" % (who, topk))
    elif topk < 1:
        raise HkpError("%s: topk %d outside 1..K" % (who, topk))
    if not isinstance(heat, torch.Tensor) or heat.dim() != 4:
        return topk
    n, k = heat.shape[:2]
    if topk and (topk > k or k > TOPK_MAX_K):
        raise HkpError("%s: topk %d outside 1..K (K = %d, at most %d with topk)" % (who, topk, k, TOPK_MAX_K))
    if weights is not None:
        if weights.dtype != torch.float32 or tuple(weights.shape) != (n, k) or weights.device != heat.device \
                or not weights.is_contiguous():
            raise HkpError("%s: weights must be contiguous float32 [%d,%d] on %s, got %s %s on %s"
                           % (who, n, k, heat.device, weights.dtype, tuple(weights.shape), weights.device))
    return topk


def _mask_choice(who, mask, heat=None):
    """The ignore mask of a loss call, checked before any kernel is called and without
    looking at a value: a contiguous uint8 tensor [N,H,W]; against heat, when that is given
    as [N,K,H,W]: its shape and device, and K <= 8 (a mask byte holds 8 class bits)."""
    from ._lib import MASK_MAX_K
    if mask is None:
        return
    if not isinstance(mask, torch.Tensor):
        raise HkpError("%s: mask must be a uint8 tensor [N,H,W], got %s" % (who, type(mask).__name__))
    if mask.dtype != torch.uint8 or mask.dim() != 3:
        raise HkpError("%s: mask must be uint8 [N,H,W], got %s %s" % (who, mask.dtype, tuple(mask.shape)))
    if not mask.is_contiguous():
        raise HkpError("%s: mask must be contiguous" % who)
    if not isinstance(heat, torch.Tensor) or heat.dim() != 4:
        return
    n, k, H, W = heat.shape
    if k > MASK_MAX_K:
        raise HkpError("%s: a mask holds %d class bits, heat has K = %d classes" % (who, MASK_MAX_K, k))
    if tuple(mask.shape) != (n, H, W) or mask.device != heat.device:
        raise HkpError("%s: mask must be uint8 [%d,%d,%d] on %s, got %s on %s"
                       % (who, n, H, W, heat.device, tuple(mask.shape), mask.device))


def _multi_loss_args(who, heat, pts, sigma, absent, planes=None, mask=None):
    """The checks heat_loss_multi and heat_loss_planes share, after _loss_choice and in this
    order: the absent mode; with planes = (weights, topk), _planes_choice; the mask
    (_mask_choice); heat, pts and that they go together; sigma.  Returns topk as
    _planes_choice does (0 without planes)."""
    if absent not in ABSENT_MODES:
        raise HkpError("%s: unknown absent %r (known: %s)" % (who, absent, ", ".join(ABSENT_MODES)))
    topk = _planes_choice(who, planes[0], planes[1], heat) if planes is not None else 0
    _mask_choice(who, mask, heat)
    _need(heat, torch.float32, who + ".heat", 4)
    _need_pts(pts, who + ".pts")
    if tuple(pts.shape[:2]) != tuple(heat.shape[:2]) or pts.device != heat.device:
        raise HkpError("%s: pts %s on %s does not go with heat %s on %s"
                       % (who, tuple(pts.shape), pts.device, tuple(heat.shape), heat.device))
    if heat.numel() == 0 or not float(sigma) > 0:
        raise HkpError("%s: empty heat or sigma %s" % (who, sigma))
    return topk


def _uv_as_pts(heat, uv):
    """uv [N,K,2] as pts [N,K,1,3]: each label one present instance."""
    _need(heat, torch.float32, "heat_loss.heat", 4)
    _need(uv, torch.float32, "heat_loss.uv", 3)
    n, k = heat.shape[:2]
    if tuple(uv.shape) != (n, k, 2):
        raise HkpError("heat_loss: uv must be [N,K,2]")
    return torch.cat([uv, torch.ones_like(uv[..., :1])], -1).reshape(n, k, 1, 3)


def heat_loss(heat, target=None, uv=None, sigma=8.0, kind="bce", want_grad=True, *, beta=2.0, norm="elements",
              weights=None, topk=None, mask=None):
    """fp64 BCE/MSE over [N,K,H,W] heatmaps → (loss 0-dim f64 tensor, dheat f32 or None).
    kind="qfl" (the quality focal loss of heat_loss_multi, with its beta and norm):
    from uv labels only, each taken as one present instance; a dense target raises.
    weights / topk (heat_loss_planes' plane weights and hard keypoint mining): from uv
    labels only, likewise; the same two values are returned.
    mask uint8 [N,H,W] (heat_loss_masked's per-pixel ignore mask of class bits, K <= 8): from
    uv labels only, likewise; a dense target raises."""
    from ._lib import HKP_LOSS_BCE, HKP_LOSS_MSE, lib
    if weights is not None or topk is not None or mask is not None:
        _loss_choice("heat_loss", kind, norm, beta)
        _planes_choice("heat_loss", weights, topk, heat)
        _mask_choice("heat_loss", mask, heat)
        if target is not None:
            raise HkpError("heat_loss: weights / topk / mask recompute the target from uv; a dense target is not "
                           "supported")
        pts = _uv_as_pts(heat, uv)
        if mask is not None:
            return heat_loss_masked(heat, pts, mask, sigma, kind, "zero", want_grad, beta=beta, norm=norm,
                                    weights=weights, topk=topk)[:2]
        return heat_loss_planes(heat, pts, sigma, kind, "zero", want_grad, beta=beta, norm=norm, weights=weights,
                                topk=topk)[:2]
    if kind == "qfl" or norm != "elements":
        _loss_choice("heat_loss", kind, norm, beta)
        if kind != "qfl":
            raise HkpError("heat_loss: norm %r needs kind 'qfl' or instance labels (heat_loss_multi)" % (norm,))
        if target is not None:
            raise HkpError("heat_loss: kind 'qfl' recomputes its target from uv; a dense target is not supported")
        return heat_loss_multi(heat, _uv_as_pts(heat, uv), sigma, kind, "zero", want_grad, beta=beta, norm=norm)
    _need(heat, torch.float32, "heat_loss.heat", 4)
    n, k, H, W = heat.shape
    if target is not None:
        _need(target, torch.float64, "heat_loss.target", 4)
        if target.shape != heat.shape:
            raise HkpError("heat_loss: target shape %s != %s" % (tuple(target.shape), tuple(heat.shape)))
    else:
        _need(uv, torch.float32, "heat_loss.uv", 3)
        if tuple(uv.shape) != (n, k, 2):
            raise HkpError("heat_loss: uv must be [N,K,2]")
    ws = torch.empty(lib().hkp_heat_loss_workspace() // 8, device=heat.device, dtype=torch.float64)
    loss = torch.empty((), device=heat.device, dtype=torch.float64)
    dheat = torch.empty_like(heat) if want_grad else None
    call("hkp_heat_loss", n, k, H, W, HKP_LOSS_BCE if kind == "bce" else HKP_LOSS_MSE, _ptr(heat), _ptr(target),
         _ptr(uv), float(sigma), _ptr(loss), _ptr(dheat), _ptr(ws), _stream())
    return loss, dheat


def heat_loss_planes(heat, pts, sigma=8.0, kind="bce", absent="zero", want_grad=True, *, beta=2.0, norm="elements",
                     weights=None, topk=None):
    """heat_loss_multi with a weight per (image, class) plane, the loss of every plane and
    hard keypoint mining, one entry (hkp_heat_loss_planes) → (loss 0-dim f64, dheat f32 or
    None, plane_loss f64 [N,K], plane_used int32 [N,K]); nothing is synchronised.
    weights float32 [N,K] on heat's device: a plane's loss and gradient are scaled by its
    weight; a weight that is not > 0 (0, negative, NaN) marks the plane as not labelled:
    it leaves the loss and the divisor, its dheat is +0 and its heat is never read.
    Weights scale, they never enter the divisor (torch's weight=).
    topk = T in 1..K (K <= 64): per image only the T eligible planes with the largest
    weight * summed loss are counted (OHKM); ties go to the lower class; the others keep
    their plane_loss and get dheat +0.
    plane_loss: the unweighted mean loss over a plane's pixels, -1 for a plane that is not
    eligible (absent under "ignore", or not labelled).  plane_used: 1 for a counted plane.
    The divisor: norm="elements": H*W times the counted planes; "instances": max(1, the
    present slots of the counted planes).  With weights=None, topk=None the loss and dheat
    are those of heat_loss_multi.  heat_loss_masked is this call with a per-pixel ignore
    mask."""
    from ._lib import (HKP_ABSENT_IGNORE, HKP_ABSENT_ZERO, HKP_LOSS_BCE, HKP_LOSS_MSE, HKP_LOSS_QFL,
                       HKP_NORM_ELEMENTS, HKP_NORM_INSTANCES, lib)
    beta = _loss_choice("heat_loss_planes", kind, norm, beta)
    topk = _multi_loss_args("heat_loss_planes", heat, pts, sigma, absent, (weights, topk))
    n, k, H, W = heat.shape
    ws = torch.empty(lib().hkp_heat_loss_planes_workspace(n, k, H, W) // 8, device=heat.device, dtype=torch.float64)
    loss = torch.empty((), device=heat.device, dtype=torch.float64)
    dheat = torch.empty_like(heat) if want_grad else None
    plane_loss = torch.empty((n, k), device=heat.device, dtype=torch.float64)
    plane_used = torch.empty((n, k), device=heat.device, dtype=torch.int32)
    kd = {"bce": HKP_LOSS_BCE, "mse": HKP_LOSS_MSE, "qfl": HKP_LOSS_QFL}[kind]
    call("hkp_heat_loss_planes", n, k, pts.shape[2], H, W, kd,
         HKP_ABSENT_ZERO if absent == "zero" else HKP_ABSENT_IGNORE,
         HKP_NORM_ELEMENTS if norm == "elements" else HKP_NORM_INSTANCES, beta, topk, _ptr(heat), _ptr(pts),
         _ptr(weights), float(sigma), _ptr(loss), _ptr(dheat), _ptr(plane_loss), _ptr(plane_used), _ptr(ws), _stream())
    return loss, dheat, plane_loss, plane_used


def heat_loss_masked(heat, pts, mask, sigma=8.0, kind="bce", absent="zero", want_grad=True, *, beta=2.0,
                     norm="elements", weights=None, topk=None):
    """heat_loss_planes with a per-pixel ignore mask, one entry (hkp_heat_loss_masked) → (loss
    0-dim f64, dheat f32 or None, plane_loss f64 [N,K], plane_used int32 [N,K], plane_pixels
    int32 [N,K]); nothing is synchronised.  heat_loss_planes keeps its own signature and its
    own entry; heat_loss_multi(mask=) and heat_loss(uv=, mask=) come here.
    mask uint8 [N,H,W] on heat's device, in the frame of heat and pts (K <= 8): bit c of a
    byte takes that pixel out for class c, 0xFF for every class.  A masked pixel adds
    nothing, gets dheat +0, and its heat is never read into a result (NaN there changes no
    output bit).  A plane's mean (plane_loss, and what topk ranks on, times the weight) runs
    over its kept pixels; a plane without a kept pixel is not labelled, as with a weight of
    0; norm="elements" divides by the kept pixels of the counted planes.  plane_pixels: the
    kept pixels of every eligible plane, 0 for the others.  With an all-zero mask the first
    four values have the bits of heat_loss_planes."""
    from ._lib import (HKP_ABSENT_IGNORE, HKP_ABSENT_ZERO, HKP_LOSS_BCE, HKP_LOSS_MSE, HKP_LOSS_QFL,
                       HKP_NORM_ELEMENTS, HKP_NORM_INSTANCES, lib)
    beta = _loss_choice("heat_loss_masked", kind, norm, beta)
    if mask is None:
        raise HkpError("heat_loss_masked: mask is required (heat_loss_planes is the call without one)")
    topk = _multi_loss_args("heat_loss_masked", heat, pts, sigma, absent, (weights, topk), mask)
    n, k, H, W = heat.shape
    ws = torch.empty(lib().hkp_heat_loss_masked_workspace(n, k, H, W) // 8, device=heat.device, dtype=torch.float64)
    loss = torch.empty((), device=heat.device, dtype=torch.float64)
    dheat = torch.empty_like(heat) if want_grad else None
    plane_loss = torch.empty((n, k), device=heat.device, dtype=torch.float64)
    plane_used = torch.empty((n, k), device=heat.device, dtype=torch.int32)
    plane_pixels = torch.empty((n, k), device=heat.device, dtype=torch.int32)
    kd = {"bce": HKP_LOSS_BCE, "mse": HKP_LOSS_MSE, "qfl": HKP_LOSS_QFL}[kind]
    call("hkp_heat_loss_masked", n, k, pts.shape[2], H, W, kd,
         HKP_ABSENT_ZERO if absent == "zero" else HKP_ABSENT_IGNORE,
         HKP_NORM_ELEMENTS if norm == "elements" else HKP_NORM_INSTANCES, beta, topk, _ptr(heat), _ptr(pts),
         _ptr(weights), _ptr(mask), float(sigma), _ptr(loss), _ptr(dheat), _ptr(plane_loss), _ptr(plane_used),
         _ptr(plane_pixels), _ptr(ws), _stream())
    return loss, dheat, plane_loss, plane_used, plane_pixels


def heat_loss_lines(heat, lines, sigma=8.0, kind="bce", absent="zero", want_grad=True, *, beta=2.0, norm="elements",
                    weights=None, topk=None, mask=None):
    """heat_loss_planes / heat_loss_masked against line labels, the target of line_target
    recomputed in registers, one entry (hkp_heat_loss_lines) → (loss 0-dim f64, dheat f32 or
    None, plane_loss f64 [N,K], plane_used int32 [N,K], plane_pixels int32 [N,K] or None
    without a mask); nothing is synchronised and no dense target is stored.
    lines float32 [N,K,S,5] (x0, y0, x1, y1, flag; flag > 0: present), 1 <= S <= 128, on
    heat's device: per pixel t = exp(-d2 / (2 sigma^2)) to the nearest present segment, 0 for
    a plane with none; a point is a zero-length segment (hkp.lines.from_points).
    kind, beta, absent, norm, weights, topk and mask mean what they mean in heat_loss_planes
    and heat_loss_masked, with one reading: the present slots that norm="instances" counts are
    segment slots, so a polyline of 12 pieces counts 12."""
    import math
    from ._lib import (HKP_ABSENT_IGNORE, HKP_ABSENT_ZERO, HKP_LOSS_BCE, HKP_LOSS_MSE, HKP_LOSS_QFL,
                       HKP_NORM_ELEMENTS, HKP_NORM_INSTANCES, lib)
    who = "heat_loss_lines"
    beta = _loss_choice(who, kind, norm, beta)
    if absent not in ABSENT_MODES:
        raise HkpError("%s: unknown absent %r (known: %s)" % (who, absent, ", ".join(ABSENT_MODES)))
    try:
        sg = float(sigma)
    except (TypeError, ValueError):
        raise HkpError("%s: sigma must be a number, got %r" % (who, sigma))
    if not (sg > 0 and math.isfinite(sg)):
        raise HkpError("%s: sigma %s must be finite and > 0" % (who, sigma))
    topk = _planes_choice(who, weights, topk, heat)
    _mask_choice(who, mask, heat)
    _lines_shape(lines, who + ".lines")
    if isinstance(heat, torch.Tensor) and heat.dim() == 4:
        if tuple(lines.shape[:2]) != tuple(heat.shape[:2]) or lines.device != heat.device:
            raise HkpError("%s: lines %s on %s does not go with heat %s on %s"
                           % (who, tuple(lines.shape), lines.device, tuple(heat.shape), heat.device))
        if heat.numel() == 0 or heat.shape[2] * heat.shape[3] > 1 << 30:
            raise HkpError("%s: bad heat size %s (no empty axis, H*W <= 2^30)" % (who, tuple(heat.shape)))
    _need(heat, torch.float32, who + ".heat", 4)
    _need_lines(lines, who + ".lines")
    n, k, H, W = heat.shape
    ws = torch.empty(lib().hkp_heat_loss_lines_workspace(n, k, H, W) // 8, device=heat.device, dtype=torch.float64)
    loss = torch.empty((), device=heat.device, dtype=torch.float64)
    dheat = torch.empty_like(heat) if want_grad else None
    plane_loss = torch.empty((n, k), device=heat.device, dtype=torch.float64)
    plane_used = torch.empty((n, k), device=heat.device, dtype=torch.int32)
    plane_pixels = torch.empty((n, k), device=heat.device, dtype=torch.int32) if mask is not None else None
    kd = {"bce": HKP_LOSS_BCE, "mse": HKP_LOSS_MSE, "qfl": HKP_LOSS_QFL}[kind]
    call("hkp_heat_loss_lines", n, k, lines.shape[2], H, W, kd,
         HKP_ABSENT_ZERO if absent == "zero" else HKP_ABSENT_IGNORE,
         HKP_NORM_ELEMENTS if norm == "elements" else HKP_NORM_INSTANCES, beta, topk, _ptr(heat), _ptr(lines),
         _ptr(weights), _ptr(mask), sg, _ptr(loss), _ptr(dheat), _ptr(plane_loss), _ptr(plane_used),
         _ptr(plane_pixels), _ptr(ws), _stream())
    return loss, dheat, plane_loss, plane_used, plane_pixels


def heat_loss_multi(heat, pts, sigma=8.0, kind="bce", absent="zero", want_grad=True, *, beta=2.0, norm="elements",
                    weights=None, topk=None, mask=None):
    """heat_loss against the multi-instance target of pts float32 [N,K,M,3] (u, v,
    flag), recomputed in registers → (loss 0-dim f64 tensor, dheat f32 or None).
    absent="zero": a plane without a present slot is trained against zeros;
    "ignore": it contributes nothing (dheat +0) and the mean runs over the other
    planes' elements (counted on the device; none: loss 0).
    kind="qfl": the quality focal loss, |t - p|^beta * BCE(p, t) per element (beta in
    [1, 8], as a float32; its minimum is at p == t in every pixel).
    norm="instances": the sum is divided by max(P, 1), P = the present slots of the
    batch (counted on the device), in place of the number of elements.
    The defaults reach hkp_heat_loss_multi; "qfl" or another norm hkp_heat_loss_multi_ex;
    weights or topk: the first two values of heat_loss_planes; mask (uint8 [N,H,W] class
    bits, K <= 8): the first two of heat_loss_masked."""
    from ._lib import (HKP_ABSENT_IGNORE, HKP_ABSENT_ZERO, HKP_LOSS_BCE, HKP_LOSS_MSE, HKP_LOSS_QFL,
                       HKP_NORM_ELEMENTS, HKP_NORM_INSTANCES, lib)
    if mask is not None:
        return heat_loss_masked(heat, pts, mask, sigma, kind, absent, want_grad, beta=beta, norm=norm, weights=weights,
                                topk=topk)[:2]
    if weights is not None or topk is not None:
        return heat_loss_planes(heat, pts, sigma, kind, absent, want_grad, beta=beta, norm=norm, weights=weights,
                                topk=topk)[:2]
    beta = _loss_choice("heat_loss_multi", kind, norm, beta)
    _multi_loss_args("heat_loss_multi", heat, pts, sigma, absent)
    n, k, H, W = heat.shape
    ws = torch.empty(lib().hkp_heat_loss_multi_workspace(n, k, H, W) // 8, device=heat.device, dtype=torch.float64)
    loss = torch.empty((), device=heat.device, dtype=torch.float64)
    dheat = torch.empty_like(heat) if want_grad else None
    kd = {"bce": HKP_LOSS_BCE, "mse": HKP_LOSS_MSE, "qfl": HKP_LOSS_QFL}[kind]
    ab = HKP_ABSENT_ZERO if absent == "zero" else HKP_ABSENT_IGNORE
    if kind == "qfl" or norm != "elements":
        call("hkp_heat_loss_multi_ex", n, k, pts.shape[2], H, W, kd, ab,
             HKP_NORM_ELEMENTS if norm == "elements" else HKP_NORM_INSTANCES, beta, _ptr(heat), _ptr(pts),
             float(sigma), _ptr(loss), _ptr(dheat), _ptr(ws), _stream())
    else:
        call("hkp_heat_loss_multi", n, k, pts.shape[2], H, W, kd, ab, _ptr(heat), _ptr(pts), float(sigma),
             _ptr(loss), _ptr(dheat), _ptr(ws), _stream())
    return loss, dheat


PEAKS_MATCH_MAX_T = 8                 # thresholds of one hkp_peaks_match launch
PEAKS_MATCH_MAX_BINS = 4096           # score bins


def match_thresholds(thresholds):
    """The thresholds of hkp_peaks_match as a tuple of floats, validated as the kernel
    validates them (on their fp32 values): 1 to 8, finite, > 0, strictly ascending."""
    try:
        th = tuple(float(v) for v in thresholds)
    except TypeError:
        raise ValueError("thresholds: expected a sequence of numbers, got %r" % (thresholds,))
    f32 = [ctypes.c_float(v).value for v in th]
    if not 1 <= len(th) <= PEAKS_MATCH_MAX_T:
        raise ValueError("thresholds: need 1 to %d of them, got %d" % (PEAKS_MATCH_MAX_T, len(th)))
    for q, v in enumerate(f32):
        if not (v > 0.0 and v != float("inf")) or (q and not v > f32[q - 1]):
            raise ValueError("thresholds: must be finite, > 0 and strictly ascending (as fp32), got %r" % (th,))
    return th


def peaks_match(peaks, counts, pts, thresholds, hist, totals, bins=1024, outputs=False):
    """Match decoded peaks to labels and ADD the outcome into the accumulators
    (hkp_peaks_match, include/hulkkp.h: COCO's greedy matching per plane and
    threshold on squared fp64 distances).  peaks float32 [N,K,P,3] (x, y, score)
    and counts int32 [N,K] as heat_peaks returns them; pts float32 [N,K,M,3] (u, v,
    flag), or [N,K,2] (one present instance per plane); thresholds: 1 to 8 pixel
    distances, ascending; hist int64 [K,T,2,bins] and totals int64 [K,8] on the
    same device, added to in place.  One launch, no synchronisation.
    outputs=True returns (peak_match int32 [N,K,T,P], gt_match int32 [N,K,M],
    gt_dist float32 [N,K,M]); otherwise None."""
    th = match_thresholds(thresholds)
    bins = int(bins)
    if not 1 <= bins <= PEAKS_MATCH_MAX_BINS:
        raise ValueError("peaks_match: need 1 <= bins <= %d, got %d" % (PEAKS_MATCH_MAX_BINS, bins))
    _need(peaks, torch.float32, "peaks_match.peaks", 4)
    n, k, p, _ = peaks.shape
    if peaks.shape[3] != 3 or not 1 <= p <= 16 or n < 1 or k < 1:
        raise HkpError("peaks_match: peaks must be [N,K,P,3] with 1 <= P <= 16, got %s" % (tuple(peaks.shape),))
    _need(counts, torch.int32, "peaks_match.counts", 2)
    if isinstance(pts, torch.Tensor) and pts.dim() == 3:
        _need(pts, torch.float32, "peaks_match.pts", 3)
        if pts.shape[2] != 2:
            raise HkpError("peaks_match: labels must be [N,K,2] or [N,K,M,3], got %s" % (tuple(pts.shape),))
        pts = torch.cat([pts, torch.ones_like(pts[..., :1])], dim=2).unsqueeze(2).contiguous()
    _need_pts(pts, "peaks_match.pts")
    m = pts.shape[2]
    t = len(th)
    _need(hist, torch.int64, "peaks_match.hist", 4)
    _need(totals, torch.int64, "peaks_match.totals", 2)
    if tuple(counts.shape) != (n, k) or tuple(pts.shape[:2]) != (n, k):
        raise HkpError("peaks_match: counts %s and pts %s do not go with peaks %s"
                       % (tuple(counts.shape), tuple(pts.shape), tuple(peaks.shape)))
    if tuple(hist.shape) != (k, t, 2, bins) or tuple(totals.shape) != (k, 8):
        raise HkpError("peaks_match: need hist %s and totals %s, got %s and %s"
                       % ((k, t, 2, bins), (k, 8), tuple(hist.shape), tuple(totals.shape)))
    for name, x in (("counts", counts), ("pts", pts), ("hist", hist), ("totals", totals)):
        if x.device != peaks.device:
            raise HkpError("peaks_match: %s is on %s, peaks on %s" % (name, x.device, peaks.device))
    pm = gm = gd = None
    if outputs:
        pm = torch.empty((n, k, t, p), device=peaks.device, dtype=torch.int32)
        gm = torch.empty((n, k, m), device=peaks.device, dtype=torch.int32)
        gd = torch.empty((n, k, m), device=peaks.device, dtype=torch.float32)
    call("hkp_peaks_match", n, k, p, m, t, bins, (ctypes.c_float * t)(*th), _ptr(peaks), _ptr(counts), _ptr(pts),
         _ptr(hist), _ptr(totals), _ptr(pm), _ptr(gm), _ptr(gd), _stream())
    return (pm, gm, gd) if outputs else None


TAGS_MAX_K = 8                        # tags are head rows K..2K-1 of at most 16
TAGS_MAX_GROUPS = 32                  # label group ids of hkp_tag_loss


def _tag_planes(who, low_all):
    """K and the lattice of low_all [N,2K,h,w] (heat logits, then the tag planes, which the
    kernels read in place from channel K on with the batch stride 2K*h*w)."""
    if not isinstance(low_all, torch.Tensor) or low_all.dim() != 4:
        raise HkpError("%s: low_all must be a float32 tensor [N,2K,h,w]" % who)
    n, k2, h, w = low_all.shape
    if k2 % 2 or not 1 <= k2 // 2 <= TAGS_MAX_K or min(n, h, w) < 1:
        raise HkpError("%s: low_all %s: need [N,2K,h,w] with 1 <= K <= %d (the tag map of class c is head row K + c "
                       "of at most 16) and non-empty planes" % (who, tuple(low_all.shape), TAGS_MAX_K))
    return n, k2 // 2, h, w


def _tag_weight(who, name, v):
    v = ctypes.c_float(float(v)).value
    if not (v >= 0.0 and v != float("inf")):
        raise HkpError("%s: %s must be finite and >= 0, got %r" % (who, name, v))
    return v


def _tags_ptr(low_all, k):
    return ctypes.c_void_p(low_all.data_ptr() + 4 * k * low_all.shape[2] * low_all.shape[3])


def tag_loss(low_all, pts, gid, H, W, scale, pull=1.0, push=1.0, want_grad=True, dtag=None):
    """Associative-embedding loss on the tag planes of low_all [N,2K,h,w] (channels K..2K-1,
    read in place) at the labelled points pts float32 [N,K,M,3] (u, v, flag) grouped by gid
    int32 [N,K,M] (a slot takes part when flag > 0 and 0 <= gid < 32; hkp.grouping.slot_groups
    builds the default) → (out3 float64 [3] = (total, mean pull, mean push) with total =
    mean over images of pull * pull_b + push * push_b, dtag float32 [N,K,h,w] =
    scale * d total / d tags or None).  dtag is written whole (a tensor given as dtag is
    filled in place).  The definition is hkp_tag_loss's (include/hulkkp.h); nothing is
    synchronised."""
    from ._lib import lib
    n, k, h, w = _tag_planes("tag_loss", low_all)
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise HkpError("tag_loss: bad picture size %dx%d" % (H, W))
    scale = _tag_weight("tag_loss", "scale", scale)
    pull = _tag_weight("tag_loss", "pull", pull)
    push = _tag_weight("tag_loss", "push", push)
    if not isinstance(pts, torch.Tensor) or pts.dim() != 4 or tuple(pts.shape[:2]) != (n, k) or pts.shape[3] != 3 \
            or not 1 <= pts.shape[2] <= 16:
        raise HkpError("tag_loss: pts must be [%d,%d,M,3] with 1 <= M <= 16, got %s"
                       % (n, k, tuple(pts.shape) if isinstance(pts, torch.Tensor) else type(pts).__name__))
    m = pts.shape[2]
    if not isinstance(gid, torch.Tensor) or tuple(gid.shape) != (n, k, m):
        raise HkpError("tag_loss: gid must be int32 [%d,%d,%d], got %s"
                       % (n, k, m, tuple(gid.shape) if isinstance(gid, torch.Tensor) else type(gid).__name__))
    if dtag is not None and (not want_grad or not isinstance(dtag, torch.Tensor) or tuple(dtag.shape) != (n, k, h, w)):
        raise HkpError("tag_loss: dtag must be float32 [%d,%d,%d,%d] and goes with want_grad" % (n, k, h, w))
    _need(low_all, torch.float32, "tag_loss.low_all", 4)
    _need(pts, torch.float32, "tag_loss.pts", 4)
    _need(gid, torch.int32, "tag_loss.gid", 3)
    if dtag is not None:
        _need(dtag, torch.float32, "tag_loss.dtag", 4)
    for name, t in (("pts", pts), ("gid", gid), ("dtag", dtag)):
        if t is not None and t.device != low_all.device:
            raise HkpError("tag_loss: %s is on %s, low_all on %s" % (name, t.device, low_all.device))
    out = torch.empty(3, device=low_all.device, dtype=torch.float64)
    ws = torch.empty(lib().hkp_tag_loss_workspace(n) // 8, device=low_all.device, dtype=torch.float64)
    if want_grad and dtag is None:
        dtag = torch.empty((n, k, h, w), device=low_all.device, dtype=torch.float32)
    call("hkp_tag_loss", n, k, m, h, w, H, W, _tags_ptr(low_all, k), 2 * k * h * w, _ptr(pts), _ptr(gid), scale, pull,
         push, _ptr(out), _ptr(dtag), _ptr(ws), _stream())
    return out, dtag


def group_order(order, k):
    """The class ids of peaks_group's `order` as a tuple of ints, validated as the kernel
    validates them: 1 to K of them, each in 0..K-1, none twice."""
    try:
        od = tuple(order)
    except TypeError:
        raise HkpError("peaks_group: order must be a sequence of class ids, got %r" % (order,))
    if not 1 <= len(od) <= k:
        raise HkpError("peaks_group: order needs 1 to %d class ids, got %d" % (k, len(od)))
    for c in od:
        if isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < k:
            raise HkpError("peaks_group: order %r: %r is no class of 0..%d" % (od, c, k - 1))
    if len(set(od)) != len(od):
        raise HkpError("peaks_group: order %r names a class twice" % (od,))
    return od


def peaks_group(peaks, counts, low_all, H, W, order, max_dist=1.0):
    """Group the decoded peaks of heat_peaks (peaks float32 [N,K,P,3], counts int32 [N,K]) by
    the tags of low_all [N,2K,h,w] (channels K..2K-1, read in place) → (group int32 [N,K,P],
    tag float32 [N,K,P], ngroups int32 [N]).  tag: the tag map's bilinear value at every used
    peak slot of every class (0 elsewhere).  group: per image the classes of `order` in turn
    and their peaks best first, each joining the group (without a member of its class yet)
    whose mean tag is nearest, if within max_dist, else opening a new one; -1 for unused
    slots and classes not in order.  A greedy rule (hkp_peaks_group, include/hulkkp.h), not
    a per-class Hungarian assignment.  One launch, nothing is synchronised."""
    n, k, h, w = _tag_planes("peaks_group", low_all)
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise HkpError("peaks_group: bad picture size %dx%d" % (H, W))
    od = group_order(order, k)
    md = ctypes.c_float(float(max_dist)).value
    if not (md > 0.0 and md != float("inf")):
        raise HkpError("peaks_group: max_dist must be finite and > 0, got %r" % (max_dist,))
    if not isinstance(peaks, torch.Tensor) or peaks.dim() != 4 or tuple(peaks.shape[:2]) != (n, k) \
            or peaks.shape[3] != 3 or not 1 <= peaks.shape[2] <= 16:
        raise HkpError("peaks_group: peaks must be [%d,%d,P,3] with 1 <= P <= 16, got %s"
                       % (n, k, tuple(peaks.shape) if isinstance(peaks, torch.Tensor) else type(peaks).__name__))
    p = peaks.shape[2]
    if not isinstance(counts, torch.Tensor) or tuple(counts.shape) != (n, k):
        raise HkpError("peaks_group: counts must be int32 [%d,%d]" % (n, k))
    _need(low_all, torch.float32, "peaks_group.low_all", 4)
    _need(peaks, torch.float32, "peaks_group.peaks", 4)
    _need(counts, torch.int32, "peaks_group.counts", 2)
    for name, t in (("peaks", peaks), ("counts", counts)):
        if t.device != low_all.device:
            raise HkpError("peaks_group: %s is on %s, low_all on %s" % (name, t.device, low_all.device))
    group = torch.empty((n, k, p), device=low_all.device, dtype=torch.int32)
    tag = torch.empty((n, k, p), device=low_all.device, dtype=torch.float32)
    ngroups = torch.empty(n, device=low_all.device, dtype=torch.int32)
    call("hkp_peaks_group", n, k, p, h, w, H, W, len(od), (ctypes.c_int32 * len(od))(*od), md, _ptr(peaks),
         _ptr(counts), _tags_ptr(low_all, k), 2 * k * h * w, _ptr(tag), _ptr(group), _ptr(ngroups), _stream())
    return group, tag, ngroups


def head_bwd(dheat, heat, h, w):
    """dlow [N,K,h,w] = upsample-adjoint(dheat * (1-heat) * heat)."""
    _need(dheat, torch.float32, "head_bwd.dheat", 4)
    n, k, H, W = dheat.shape
    if heat is not None and heat.shape != dheat.shape:
        raise HkpError("head_bwd: heat shape mismatch")
    from ._lib import lib
    dlow = torch.empty((n, k, h, w), device=dheat.device, dtype=torch.float32)
    nb = lib().hkp_head_bwd_workspace(n, k, w, H)
    ws = torch.empty(nb // 4, device=dheat.device, dtype=torch.float32)
    call("hkp_head_bwd", n, k, h, w, H, W, _ptr(dheat), _ptr(heat), _ptr(dlow), _ptr(ws), nb, _stream())
    return dlow


def head_fc_bwd(dlow, feat, w_kc):
    """→ (dfeat NHWC, dW [K,C], db [K])."""
    from ._lib import lib
    _need(dlow, torch.float32, "head_fc_bwd.dlow", 4)
    _need(feat, torch.float32, "head_fc_bwd.feat", 4)
    _need(w_kc, torch.float32, "head_fc_bwd.w", 2)
    n, h, w, c = feat.shape
    k = dlow.shape[1]
    if tuple(dlow.shape) != (n, k, h, w) or tuple(w_kc.shape) != (k, c):
        raise HkpError("head_fc_bwd: shape mismatch")
    nbytes = lib().hkp_head_fc_bwd_workspace(n, h * w, c, k)
    ws = torch.empty(nbytes // 4, device=feat.device, dtype=torch.float32)
    dfeat = torch.empty_like(feat)
    dw = torch.empty((k, c), device=feat.device, dtype=torch.float32)
    db = torch.empty(k, device=feat.device, dtype=torch.float32)
    call("hkp_head_fc_bwd", n, h * w, c, k, _ptr(dlow), _ptr(feat), _ptr(w_kc), _ptr(dfeat), _ptr(dw), _ptr(db),
         _ptr(ws), nbytes, _stream())
    return dfeat, dw, db
