// Line labels: the centreline target (include/hulkkp.h has the definition).
//
//  * hkp_line_target  d2 = the squared distance from every pixel to the nearest present
//                    segment of its plane, target = (double)expf(-d2 / den).  A zero-length
//                    segment is a point, in hkp_gauss_target's operation order.
//
// One launch.  A block works on one 32 x 32 tile of one plane (4 pixels of a row per
// thread).  The plane's records are read once per block, one slot per thread, and are
// compacted twice into LDS, both times by ballot, so slot order is kept and the loop
// over them has a wave-uniform trip count:
//   1. the present slots (flag > 0) get their per-segment constants dx, dy, inv and two
//      bounds on their distance d over the tile's pixels.  Distance to a segment is
//      convex, so ub = the largest distance at the tile's four corner pixels bounds d
//      from above; the distance from the tile's centre less the half diagonal bounds it
//      from below (triangle inequality).
//   2. a segment whose lower bound exceeds the smallest upper bound of the plane by more
//      than CULL_MARGIN pixels is farther than that other segment at every pixel of the
//      tile: it cannot hold the minimum, and it is dropped.  The margin is two pixels;
//      the fp32 rounding of a distance is below 0.05 px at the largest coordinates the
//      header allows (|.| <= 32768), so no dropped segment can win or tie after rounding.
// The survivors are evaluated by the definition, in slot order: the bits of the unculled
// minimum.  A bound that is NaN keeps its segment.
#include "common.h"
#include "lines_dev.h"

#pragma clang fp contract(off)

namespace hkp {

typedef double f64x2 __attribute__((ext_vector_type(2)));

// HAS_T / HAS_D: which outputs are written.  vec_t: target's base is 16-byte aligned and W
// is even (two doubles a store); vec_d: d2's base is 16-byte aligned and W % 4 == 0 (four
// floats a store); the scalar path otherwise.  grid = (tiles of a plane, planes or fewer).
template <bool HAS_T, bool HAS_D>
__global__ __launch_bounds__(256) void line_target_kernel(long planes, int s, int H, int W, int tiles_x, float den,
                                                         int vec_t, int vec_d, const float* __restrict__ lines,
                                                         double* __restrict__ target, float* __restrict__ d2out) {
    // (x0, y0, dx, dy) and inv of the segments kept, in slot order; inv = 0 stands for
    // l2 == 0 (dx = dy = 0: the product is 0 and t = 0 either way)
    __shared__ f32x4 sseg[HKP_LINE_MAX_S];
    __shared__ float sinv[HKP_LINE_MAX_S];
    __shared__ int swc[2];
    __shared__ float swub[2];
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int xa = tile_x * LINE_TW, ya = tile_y * LINE_TH;
    const int xb = min(xa + LINE_TW, W) - 1, yb = min(ya + LINE_TH, H) - 1;   // the tile's last pixel
    const float fxa = (float)xa, fya = (float)ya, fxb = (float)xb, fyb = (float)yb;
    const float mx = 0.5f * (fxa + fxb), my = 0.5f * (fya + fyb);
    const float ex = fxb - fxa, ey = fyb - fya;
    const float rad = 0.5f * sqrtf(ex * ex + ey * ey);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int x = xa + (threadIdx.x & 7) * 4, y = ya + (threadIdx.x >> 3);
    const int HW = H * W;

    for (long plane = blockIdx.y; plane < planes; plane += gridDim.y) {
        // ---- the present slots, their constants and bounds (waves 0 and 1: slot = thread)
        float x0 = 0.f, y0 = 0.f, dx = 0.f, dy = 0.f, inv = 0.f, lb = 0.f, ub = INFINITY;
        bool on = false;
        if (threadIdx.x < HKP_LINE_MAX_S) {
            const int j = threadIdx.x;
            if (j < s) {
                const float* rec = lines + (plane * s + j) * 5;
                on = rec[4] > 0.f;
                if (on) {
                    x0 = rec[0], y0 = rec[1];
                    dx = rec[2] - x0, dy = rec[3] - y0;
                    const float l2 = dx * dx + dy * dy;
                    inv = l2 > 0.f ? 1.0f / l2 : 0.f;
                    const float c = fmaxf(fmaxf(seg_d2(fxa, fya, x0, y0, dx, dy, inv), seg_d2(fxb, fya, x0, y0, dx, dy, inv)),
                                          fmaxf(seg_d2(fxa, fyb, x0, y0, dx, dy, inv), seg_d2(fxb, fyb, x0, y0, dx, dy, inv)));
                    ub = sqrtf(c);
                    lb = sqrtf(seg_d2(mx, my, x0, y0, dx, dy, inv)) - rad;
                }
            }
            float wub = ub;   // +inf where the slot is empty; fminf passes over a NaN
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) wub = fminf(wub, __shfl_xor(wub, o));
            if (lane == 0) swub[wid] = wub;
        }
        __syncthreads();
        // ---- drop what cannot be nearest anywhere in the tile; compact the rest
        unsigned long long mask = 0;
        if (threadIdx.x < HKP_LINE_MAX_S) {
            const float best = fminf(swub[0], swub[1]);
            on = on && !(lb > best + CULL_MARGIN);
            mask = __ballot(on);
            if (lane == 0) swc[wid] = __popcll(mask);
        }
        __syncthreads();
        if (threadIdx.x < HKP_LINE_MAX_S && on) {
            const int pos = (wid == 1 ? swc[0] : 0) + __popcll(mask & ((1ull << lane) - 1ull));
            sseg[pos] = f32x4{x0, y0, dx, dy};
            sinv[pos] = inv;
        }
        __syncthreads();
        const int cnt = __builtin_amdgcn_readfirstlane(swc[0] + swc[1]);

        // ---- 4 pixels of a row per thread, the survivors in slot order
        float d[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
        if (y < H && x < W) {
            const float fy = (float)y;
            for (int j = 0; j < cnt; ++j) {
                const f32x4 sg = sseg[j];
                const float iv = sinv[j];
                const float py = fy - sg[1];
                const float pydy = py * sg[3];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float px = (float)(x + e) - sg[0];
                    const float t = fminf(fmaxf((px * sg[2] + pydy) * iv, 0.f), 1.f);
                    const float cx = px - t * sg[2], cy = py - t * sg[3];
                    d[e] = fminf(d[e], cx * cx + cy * cy);
                }
            }
            const long at = plane * HW + (long)y * W + x;
            if constexpr (HAS_D) {
                float* o = d2out + at;
                if (vec_d) {   // W % 4 == 0: the four pixels are inside
                    *(f32x4*)o = f32x4{d[0], d[1], d[2], d[3]};
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (x + e < W) o[e] = d[e];
                }
            }
            if constexpr (HAS_T) {
                double tv[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) tv[e] = cnt > 0 ? (double)expf(-d[e] / den) : 0.0;
                double* o = target + at;
                if (vec_t) {   // W even: a pair is inside or outside whole
                    *(f64x2*)o = f64x2{tv[0], tv[1]};
                    if (x + 2 < W) *(f64x2*)(o + 2) = f64x2{tv[2], tv[3]};
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (x + e < W) o[e] = tv[e];
                }
            }
        }
        __syncthreads();   // the next plane restages sseg / swc
    }
}

}  // namespace hkp

using namespace hkp;

extern "C" int hkp_line_target(int32_t n, int32_t k, int32_t s, int32_t H, int32_t W, float sigma, const float* lines,
                               double* target, float* d2, hkp_stream_t stream) {
    HKP_CHECK_ARG(n >= 1 && k >= 1 && H >= 1 && W >= 1 && (long)H * W <= (1l << 30),
                  "hkp_line_target: bad sizes (n, k, H, W >= 1, H*W <= 2^30)");
    HKP_CHECK_ARG(s >= 1 && s <= HKP_LINE_MAX_S, "hkp_line_target: s = %d outside 1..%d", s, HKP_LINE_MAX_S);
    HKP_CHECK_ARG(sigma > 0.f && sigma < INFINITY, "hkp_line_target: sigma must be finite and > 0");
    HKP_CHECK_ARG(lines != nullptr, "hkp_line_target: null lines");
    HKP_CHECK_ARG(target != nullptr || d2 != nullptr, "hkp_line_target: both outputs are null");
    const long planes = (long)n * k;
    const float den = (float)(2.0 * (double)sigma * (double)sigma);
    const int tiles_x = cdiv(W, LINE_TW), tiles_y = cdiv(H, LINE_TH);
    const int vec_t = target && ((uintptr_t)target & 15) == 0 && W % 2 == 0;
    const int vec_d = d2 && ((uintptr_t)d2 & 15) == 0 && W % 4 == 0;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)(planes < 65535 ? planes : 65535));
    hipStream_t st = as_stream(stream);
#define HKP_LINE(T, D)                                                                                               \
    hipLaunchKernelGGL((line_target_kernel<T, D>), grid, dim3(256), 0, st, planes, s, H, W, tiles_x, den, vec_t, \
                       vec_d, lines, target, d2)
    if (target && d2) HKP_LINE(true, true);
    else if (target) HKP_LINE(true, false);
    else HKP_LINE(false, true);
#undef HKP_LINE
    HKP_LAUNCH_CHECK("hkp_line_target");
    return HKP_OK;
}
