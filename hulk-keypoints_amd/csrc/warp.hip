// Batched per-image affine warp of uint8 [n][hs][ws][3] batches into [n][h][w][3]:
// geometric augmentation (rotation, scale, translation, shear, flips) and resize
// are host-side matrix builders over this one kernel (hkp/geometry.py), one launch
// per batch.  A block owns one WARP_TH x WARP_TW tile of one output image; a thread
// makes 4 consecutive output pixels of one row and gathers their source taps
// straight from global memory (no LDS: see DESIGN "Affine warp").
//
// Arithmetic: integers only (include/hulkkp.h spells it out; tests/_warp_ref.py
// restates it in numpy int64).  Addresses are formed from clamped indices only, in
// every border mode: the int64 coordinate is clamped into [-2, dim + 1] before it
// is narrowed, each tap index is then clamped / reflected into [0, dim), and
// CONSTANT picks the fill value after the (in-bounds) load.
#include "common.h"

namespace hkp {

constexpr int WARP_TH = 16, WARP_TW = 64, WARP_PX = 4;       // tile, pixels per thread
static_assert(WARP_TH * WARP_TW == 256 * WARP_PX, "one tile per 256-thread block");

// tap index i in [-2, n + 2] → the row / column it reads in [0, n), and whether it
// lies outside the source
template <int BORDER>
__device__ __forceinline__ int warp_tap(int i, int n, bool& outside) {
    outside = i < 0 || i >= n;
    if (BORDER == HKP_WARP_BORDER_REFLECT101) i = i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i);
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

__device__ __forceinline__ int warp_clamp_coord(int64_t v, int n) {
    return (int)(v < -2 ? -2 : (v > (int64_t)n + 1 ? (int64_t)n + 1 : v));
}

// one output pixel from source coordinates (sx, sy), Q16
template <int INTERP, int BORDER>
__device__ __forceinline__ void warp_pixel(const uint8_t* __restrict__ src, int hs, int ws, int64_t sx, int64_t sy,
                                           int f0, int f1, int f2, int& b, int& g, int& r) {
    if (INTERP == HKP_WARP_NEAREST) {
        bool ox, oy;
        const int ix = warp_tap<BORDER>(warp_clamp_coord((sx + 32768) >> 16, ws), ws, ox);
        const int iy = warp_tap<BORDER>(warp_clamp_coord((sy + 32768) >> 16, hs), hs, oy);
        const uint8_t* p = src + ((size_t)iy * ws + ix) * 3;
        b = p[0], g = p[1], r = p[2];
        if (BORDER == HKP_WARP_BORDER_CONSTANT && (ox || oy)) b = f0, g = f1, r = f2;
    } else {
        const int64_t qx = (sx + 128) >> 8, qy = (sy + 128) >> 8;
        const int fx = (int)(qx & 255), fy = (int)(qy & 255);
        const int ix = warp_clamp_coord(qx >> 8, ws), iy = warp_clamp_coord(qy >> 8, hs);
        bool ox0, ox1, oy0, oy1;
        const int x0 = warp_tap<BORDER>(ix, ws, ox0), x1 = warp_tap<BORDER>(ix + 1, ws, ox1);
        const int y0 = warp_tap<BORDER>(iy, hs, oy0), y1 = warp_tap<BORDER>(iy + 1, hs, oy1);
        const uint8_t* r0 = src + (size_t)y0 * ws * 3;
        const uint8_t* r1 = src + (size_t)y1 * ws * 3;
        const uint8_t *p00 = r0 + x0 * 3, *p01 = r0 + x1 * 3, *p10 = r1 + x0 * 3, *p11 = r1 + x1 * 3;
        int v00[3] = {p00[0], p00[1], p00[2]}, v01[3] = {p01[0], p01[1], p01[2]};
        int v10[3] = {p10[0], p10[1], p10[2]}, v11[3] = {p11[0], p11[1], p11[2]};
        const int fill[3] = {f0, f1, f2};
        int o[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (BORDER == HKP_WARP_BORDER_CONSTANT) {
                if (ox0 || oy0) v00[c] = fill[c];
                if (ox1 || oy0) v01[c] = fill[c];
                if (ox0 || oy1) v10[c] = fill[c];
                if (ox1 || oy1) v11[c] = fill[c];
            }
            const int top = v00[c] * (256 - fx) + v01[c] * fx;
            const int bot = v10[c] * (256 - fx) + v11[c] * fx;
            o[c] = (top * (256 - fy) + bot * fy + 32768) >> 16;
        }
        b = o[0], g = o[1], r = o[2];
    }
}

template <int INTERP, int BORDER, bool DWORD>
__global__ __launch_bounds__(256) void warp_affine_u8_kernel(int hs, int ws, const uint8_t* __restrict__ in, int h,
                                                            int w, uint8_t* __restrict__ out,
                                                            const hkp_warp_xform* __restrict__ xforms) {
    const int tid = threadIdx.x, n = blockIdx.z;
    const int x = blockIdx.x * WARP_TW + (tid % (WARP_TW / WARP_PX)) * WARP_PX;
    const int y = blockIdx.y * WARP_TH + tid / (WARP_TW / WARP_PX);
    if (x >= w || y >= h) return;
    const hkp_warp_xform& xf = xforms[n];                    // block-uniform
    const int64_t m0 = xf.m[0], m3 = xf.m[3];
    int64_t sx = m0 * x + (int64_t)xf.m[1] * y + xf.m[2];
    int64_t sy = m3 * x + (int64_t)xf.m[4] * y + xf.m[5];
    const int f0 = xf.fill[0], f1 = xf.fill[1], f2 = xf.fill[2];
    const uint8_t* src = in + (size_t)n * hs * ws * 3;
    uint8_t* dst = out + (((size_t)n * h + y) * w + x) * 3;
    int px[WARP_PX * 3];
#pragma unroll
    for (int j = 0; j < WARP_PX; ++j) {
        // (past the row's end in the byte path: computed from clamped addresses, not stored)
        warp_pixel<INTERP, BORDER>(src, hs, ws, sx, sy, f0, f1, f2, px[3 * j], px[3 * j + 1], px[3 * j + 2]);
        sx += m0;
        sy += m3;
    }
    if (DWORD) {                                             // w % 4 == 0, out 4-byte aligned: x + 3 < w
        uint32_t d[3] = {0, 0, 0};
#pragma unroll
        for (int k = 0; k < WARP_PX * 3; ++k) d[k >> 2] |= (uint32_t)px[k] << (8 * (k & 3));
        uint32_t* o = (uint32_t*)dst;
        o[0] = d[0];
        o[1] = d[1];
        o[2] = d[2];
    } else {
#pragma unroll
        for (int j = 0; j < WARP_PX; ++j) {
            if (x + j < w) {
                dst[3 * j] = (uint8_t)px[3 * j];
                dst[3 * j + 1] = (uint8_t)px[3 * j + 1];
                dst[3 * j + 2] = (uint8_t)px[3 * j + 2];
            }
        }
    }
}

template <int INTERP, int BORDER>
static void warp_launch(bool dword, dim3 grid, hipStream_t s, int hs, int ws, const uint8_t* in, int h, int w,
                        uint8_t* out, const hkp_warp_xform* xf) {
    if (dword)
        hipLaunchKernelGGL((warp_affine_u8_kernel<INTERP, BORDER, true>), grid, dim3(256), 0, s, hs, ws, in, h, w, out, xf);
    else
        hipLaunchKernelGGL((warp_affine_u8_kernel<INTERP, BORDER, false>), grid, dim3(256), 0, s, hs, ws, in, h, w, out, xf);
}

// hkp_warp_mask_u8: one channel, warp_pixel's NEAREST rule (the same two helpers), the
// source byte through the image's table, the fill byte as given.  The block, tile and
// store paths are the image warp's.
template <int BORDER, bool DWORD>
__global__ __launch_bounds__(256) void warp_mask_u8_kernel(int hs, int ws, const uint8_t* __restrict__ in, int h, int w,
                                                          uint8_t* __restrict__ out,
                                                          const hkp_warp_xform* __restrict__ xforms, int fill,
                                                          const uint8_t* __restrict__ lut) {
    const int tid = threadIdx.x, n = blockIdx.z;
    const int x = blockIdx.x * WARP_TW + (tid % (WARP_TW / WARP_PX)) * WARP_PX;
    const int y = blockIdx.y * WARP_TH + tid / (WARP_TW / WARP_PX);
    if (x >= w || y >= h) return;
    const hkp_warp_xform& xf = xforms[n];                    // block-uniform
    const int64_t m0 = xf.m[0], m3 = xf.m[3];
    int64_t sx = m0 * x + (int64_t)xf.m[1] * y + xf.m[2];
    int64_t sy = m3 * x + (int64_t)xf.m[4] * y + xf.m[5];
    const uint8_t* src = in + (size_t)n * hs * ws;
    const uint8_t* tab = lut ? lut + (size_t)n * 256 : nullptr;
    uint8_t* dst = out + ((size_t)n * h + y) * w + x;
    int px[WARP_PX];
#pragma unroll
    for (int j = 0; j < WARP_PX; ++j) {
        bool ox, oy;
        const int ix = warp_tap<BORDER>(warp_clamp_coord((sx + 32768) >> 16, ws), ws, ox);
        const int iy = warp_tap<BORDER>(warp_clamp_coord((sy + 32768) >> 16, hs), hs, oy);
        int v = src[(size_t)iy * ws + ix];
        if (tab) v = tab[v];
        if (BORDER == HKP_WARP_BORDER_CONSTANT && (ox || oy)) v = fill;
        px[j] = v;
        sx += m0;
        sy += m3;
    }
    if (DWORD) {                                             // w % 4 == 0, out 4-byte aligned: x + 3 < w
        *(uint32_t*)dst = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16) | ((uint32_t)px[3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < WARP_PX; ++j)
            if (x + j < w) dst[j] = (uint8_t)px[j];
    }
}

}  // namespace hkp

using namespace hkp;

extern "C" int hkp_warp_affine_u8(int32_t n, int32_t hs, int32_t ws, const uint8_t* img_in, int32_t h, int32_t w,
                                  uint8_t* img_out, const hkp_warp_xform* xforms_host, const hkp_warp_xform* xforms,
                                  int32_t interp, int32_t border, hkp_stream_t stream) {
    static_assert(sizeof(hkp_warp_xform) == 32, "hkp_warp_xform layout");
    HKP_CHECK_ARG(n >= 1 && n <= 65535, "hkp_warp_affine_u8: bad batch size n=%d (1..65535)", n);
    HKP_CHECK_ARG(hs >= 1 && hs <= HKP_WARP_MAX_DIM && ws >= 1 && ws <= HKP_WARP_MAX_DIM,
                  "hkp_warp_affine_u8: source %dx%d outside 1..%d", hs, ws, HKP_WARP_MAX_DIM);
    HKP_CHECK_ARG(h >= 1 && h <= HKP_WARP_MAX_DIM && w >= 1 && w <= HKP_WARP_MAX_DIM,
                  "hkp_warp_affine_u8: output %dx%d outside 1..%d", h, w, HKP_WARP_MAX_DIM);
    HKP_CHECK_ARG(interp == HKP_WARP_BILINEAR || interp == HKP_WARP_NEAREST,
                  "hkp_warp_affine_u8: unknown interpolation %d", interp);
    HKP_CHECK_ARG(border >= HKP_WARP_BORDER_CONSTANT && border <= HKP_WARP_BORDER_REFLECT101,
                  "hkp_warp_affine_u8: unknown border mode %d", border);
    HKP_CHECK_ARG(border != HKP_WARP_BORDER_REFLECT101 || (hs >= 2 && ws >= 2),
                  "hkp_warp_affine_u8: REFLECT101 needs a source of at least 2x2, got %dx%d", hs, ws);
    HKP_CHECK_ARG(img_in && img_out && xforms_host && xforms, "hkp_warp_affine_u8: null pointer");
    HKP_CHECK_ARG(((uintptr_t)xforms & 3) == 0, "hkp_warp_affine_u8: xforms must be 4-byte aligned");
    const int64_t in_bytes = (int64_t)n * hs * ws * 3, out_bytes = (int64_t)n * h * w * 3;
    HKP_CHECK_ARG(img_out + out_bytes <= img_in || img_in + in_bytes <= img_out,
                  "hkp_warp_affine_u8: img_out must not overlap img_in (taps are gathered)");
    for (int32_t i = 0; i < n; ++i)
        HKP_CHECK_ARG(xforms_host[i].reserved == 0, "hkp_warp_affine_u8: transform %d has a non-zero reserved field", i);
    const bool dword = w % 4 == 0 && ((uintptr_t)img_out & 3) == 0;
    const dim3 grid((unsigned)((w + WARP_TW - 1) / WARP_TW), (unsigned)((h + WARP_TH - 1) / WARP_TH), (unsigned)n);
    const hipStream_t s = as_stream(stream);
#define HKP_WARP_CASE(I, B)                                                   \
    if (interp == I && border == B) warp_launch<I, B>(dword, grid, s, hs, ws, img_in, h, w, img_out, xforms)
    HKP_WARP_CASE(HKP_WARP_BILINEAR, HKP_WARP_BORDER_CONSTANT);
    HKP_WARP_CASE(HKP_WARP_BILINEAR, HKP_WARP_BORDER_REPLICATE);
    HKP_WARP_CASE(HKP_WARP_BILINEAR, HKP_WARP_BORDER_REFLECT101);
    HKP_WARP_CASE(HKP_WARP_NEAREST, HKP_WARP_BORDER_CONSTANT);
    HKP_WARP_CASE(HKP_WARP_NEAREST, HKP_WARP_BORDER_REPLICATE);
    HKP_WARP_CASE(HKP_WARP_NEAREST, HKP_WARP_BORDER_REFLECT101);
#undef HKP_WARP_CASE
    HKP_LAUNCH_CHECK("hkp_warp_affine_u8");
    return HKP_OK;
}

extern "C" int hkp_warp_mask_u8(int32_t n, int32_t hs, int32_t ws, const uint8_t* mask_in, int32_t h, int32_t w,
                                uint8_t* mask_out, const hkp_warp_xform* xforms_host, const hkp_warp_xform* xforms,
                                int32_t border, int32_t fill, const uint8_t* lut, hkp_stream_t stream) {
    HKP_CHECK_ARG(n >= 1 && n <= 65535, "hkp_warp_mask_u8: bad batch size n=%d (1..65535)", n);
    HKP_CHECK_ARG(hs >= 1 && hs <= HKP_WARP_MAX_DIM && ws >= 1 && ws <= HKP_WARP_MAX_DIM,
                  "hkp_warp_mask_u8: source %dx%d outside 1..%d", hs, ws, HKP_WARP_MAX_DIM);
    HKP_CHECK_ARG(h >= 1 && h <= HKP_WARP_MAX_DIM && w >= 1 && w <= HKP_WARP_MAX_DIM,
                  "hkp_warp_mask_u8: output %dx%d outside 1..%d", h, w, HKP_WARP_MAX_DIM);
    HKP_CHECK_ARG(border >= HKP_WARP_BORDER_CONSTANT && border <= HKP_WARP_BORDER_REFLECT101,
                  "hkp_warp_mask_u8: unknown border mode %d", border);
    HKP_CHECK_ARG(border != HKP_WARP_BORDER_REFLECT101 || (hs >= 2 && ws >= 2),
                  "hkp_warp_mask_u8: REFLECT101 needs a source of at least 2x2, got %dx%d", hs, ws);
    HKP_CHECK_ARG(fill >= 0 && fill <= 255, "hkp_warp_mask_u8: fill %d outside 0..255", fill);
    HKP_CHECK_ARG(mask_in && mask_out && xforms_host && xforms, "hkp_warp_mask_u8: null pointer");
    HKP_CHECK_ARG(((uintptr_t)xforms & 3) == 0, "hkp_warp_mask_u8: xforms must be 4-byte aligned");
    const int64_t in_bytes = (int64_t)n * hs * ws, out_bytes = (int64_t)n * h * w;
    HKP_CHECK_ARG(mask_out + out_bytes <= mask_in || mask_in + in_bytes <= mask_out,
                  "hkp_warp_mask_u8: mask_out must not overlap mask_in (taps are gathered)");
    for (int32_t i = 0; i < n; ++i)
        HKP_CHECK_ARG(xforms_host[i].reserved == 0, "hkp_warp_mask_u8: transform %d has a non-zero reserved field", i);
    const bool dword = w % 4 == 0 && ((uintptr_t)mask_out & 3) == 0;
    const dim3 grid((unsigned)((w + WARP_TW - 1) / WARP_TW), (unsigned)((h + WARP_TH - 1) / WARP_TH), (unsigned)n);
    const hipStream_t s = as_stream(stream);
#define HKP_WARP_MASK_CASE(B)                                                                                          \
    if (border == B) {                                                                                                 \
        if (dword)                                                                                                     \
            hipLaunchKernelGGL((warp_mask_u8_kernel<B, true>), grid, dim3(256), 0, s, hs, ws, mask_in, h, w, mask_out,  \
                               xforms, fill, lut);                                                                     \
        else                                                                                                           \
            hipLaunchKernelGGL((warp_mask_u8_kernel<B, false>), grid, dim3(256), 0, s, hs, ws, mask_in, h, w, mask_out, \
                               xforms, fill, lut);                                                                     \
    }
    HKP_WARP_MASK_CASE(HKP_WARP_BORDER_CONSTANT)
    HKP_WARP_MASK_CASE(HKP_WARP_BORDER_REPLICATE)
    HKP_WARP_MASK_CASE(HKP_WARP_BORDER_REFLECT101)
#undef HKP_WARP_MASK_CASE
    HKP_LAUNCH_CHECK("hkp_warp_mask_u8");
    return HKP_OK;
}
