// Test-time augmentation on the stride-8 lattice: the low-res logits of several
// views of one batch (flipped and / or rescaled inputs, each [n][k][h_v][w_v] fp32,
// packed one after the other) merged into logits [n][k][h][w] on the base view's
// lattice, in one launch.  Per output node and view: an axis-aligned map into the
// view's lattice (a*i + b per axis), a bilinear sample of the view's plane (channel
// perm[v][c]: the flip pairs), and a weighted sum over the views — of the logits,
// or of both tails of their sigmoids (HKP_MERGE_PROB).  hkp_heat_peaks reads the
// result as it reads a single forward's `low`.
//
// Arithmetic: fp64 throughout, no fused multiply-add, views in table order
// (include/hulkkp.h spells it out; tests/_tta_ref.py restates it in numpy float64).
// A tap of weight exactly 0 is not read, so a flip (a = -1, b = w - 1) is a copy.
// Addresses are formed from clamped indices only: the coordinate is clamped into
// [0, dim - 1] before the floor, the channel into [0, k - 1].
//
// One thread per output element (per 4 consecutive elements of a row where rows
// leave as 16-byte stores), grid-stride over a capped grid.  No LDS, no atomics; the
// view table is read from device memory (a by-value table indexed by the view loop
// would live in scratch).
#include "common.h"

namespace hkp {

constexpr int MERGE_THREADS = 256;
constexpr int MERGE_MAX_BLOCKS = 1024;     // 4 blocks per CU; larger outputs take more than one trip

// one axis: node i of the base lattice -> taps i0, i1 of a view's axis of n nodes and
// the weight f of i1 (0: i1 is not read)
__device__ __forceinline__ void merge_axis(double a, double b, int i, int n, int& i0, int& i1, double& f) {
    double c = a * (double)i + b;
    const double hi = (double)(n - 1);
    c = !(c >= 0.0) ? 0.0 : (c > hi ? hi : c);               // (a NaN from a broken table lands on 0: in range)
    const double fl = floor(c);
    i0 = (int)fl;
    f = c - fl;
    i1 = i0 + 1 < n - 1 ? i0 + 1 : n - 1;
}

// z_v of one node: rows r0 / r1 of the view's plane, columns x0 / x1
__device__ __forceinline__ double merge_sample(const float* __restrict__ r0, const float* __restrict__ r1, int x0,
                                               int x1, double fx, double fy) {
    double top = (double)r0[x0];
    if (fx != 0.0) top = top + fx * ((double)r0[x1] - top);
    if (fy == 0.0) return top;
    double bot = (double)r1[x0];
    if (fx != 0.0) bot = bot + fx * ((double)r1[x1] - bot);
    return top + fy * (bot - top);
}

template <int MODE, int VEC>
__global__ __launch_bounds__(MERGE_THREADS) void logits_merge_kernel(int k, int h, int w, int views, long items,
                                                                     const float* __restrict__ packed,
                                                                     const hkp_merge_view* __restrict__ table,
                                                                     const int32_t* __restrict__ perm,
                                                                     float* __restrict__ out) {
    const int wq = w / VEC;                                   // VEC == 4 only where w % 4 == 0
    const long stride = (long)gridDim.x * MERGE_THREADS;
    for (long t = (long)blockIdx.x * MERGE_THREADS + threadIdx.x; t < items; t += stride) {
        const int jq = (int)(t % wq);
        const long row = t / wq;                              // (b*k + c)*h + i
        const int i = (int)(row % h);
        const long plane = row / h;
        const int c = (int)(plane % k);
        const long b = plane / k;
        double acc[VEC], neg[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = 0.0, neg[e] = 0.0;
        for (int v = 0; v < views; ++v) {
            const hkp_merge_view& tv = table[v];
            const int hv = tv.h, wv = tv.w;
            const double wt = tv.weight, ax = tv.ax, bx = tv.bx;
            int pc = perm[v * k + c];
            pc = pc < 0 ? 0 : (pc >= k ? k - 1 : pc);
            int y0, y1;
            double fy;
            merge_axis(tv.ay, tv.by, i, hv, y0, y1, fy);
            const float* src = packed + tv.off + (b * k + pc) * ((long)hv * wv);
            const float* r0 = src + (long)y0 * wv;
            const float* r1 = src + (long)y1 * wv;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                int x0, x1;
                double fx;
                merge_axis(ax, bx, jq * VEC + e, wv, x0, x1, fx);
                const double z = merge_sample(r0, r1, x0, x1, fx, fy);
                if (MODE == HKP_MERGE_LOGIT) {
                    acc[e] = v == 0 ? wt * z : acc[e] + wt * z;           // the sum starts with view 0's term: -0 stays -0
                } else {
                    const double zc = z < -700.0 ? -700.0 : (z > 700.0 ? 700.0 : z);     // NaN stays NaN
                    acc[e] = acc[e] + wt / (1.0 + exp(-zc));
                    neg[e] = neg[e] + wt / (1.0 + exp(zc));
                }
            }
        }
        float o[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) o[e] = MODE == HKP_MERGE_LOGIT ? (float)acc[e] : (float)(log(acc[e]) - log(neg[e]));
        float* dst = out + row * w + (long)jq * VEC;
        if (VEC == 4) {
            f32x4 q;
            q[0] = o[0], q[1] = o[VEC > 1 ? 1 : 0], q[2] = o[VEC > 2 ? 2 : 0], q[3] = o[VEC > 3 ? 3 : 0];
            *(f32x4*)dst = q;
        } else {
            dst[0] = o[0];
        }
    }
}

}  // namespace hkp

using namespace hkp;

extern "C" int hkp_logits_merge(int32_t n, int32_t k, int32_t h, int32_t w, int32_t views, int32_t mode,
                                const float* packed, const void* table, const int32_t* perm, float* out,
                                hkp_stream_t stream) {
    static_assert(sizeof(hkp_merge_view) == 64, "hkp_merge_view layout");
    HKP_CHECK_ARG(n >= 1 && k >= 1 && h >= 1 && w >= 1, "hkp_logits_merge: bad output shape [%d,%d,%d,%d]", n, k, h, w);
    HKP_CHECK_ARG((int64_t)n * k * h * w <= ((int64_t)1 << 40), "hkp_logits_merge: output [%d,%d,%d,%d] too large", n,
                  k, h, w);
    HKP_CHECK_ARG(views >= 1 && views <= HKP_MERGE_MAX_VIEWS, "hkp_logits_merge: %d views outside 1..%d", views,
                  HKP_MERGE_MAX_VIEWS);
    HKP_CHECK_ARG(mode == HKP_MERGE_LOGIT || mode == HKP_MERGE_PROB, "hkp_logits_merge: unknown mode %d", mode);
    HKP_CHECK_ARG(packed && table && perm && out, "hkp_logits_merge: null pointer");
    HKP_CHECK_ARG(((uintptr_t)packed & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)perm & 3) == 0,
                  "hkp_logits_merge: packed, perm and out must be 4-byte aligned");
    HKP_CHECK_ARG(((uintptr_t)table & 7) == 0, "hkp_logits_merge: table must be 8-byte aligned");
    const bool vec = w % 4 == 0 && ((uintptr_t)out & 15) == 0;
    const long items = (long)n * k * h * (vec ? w / 4 : w);
    const long want = (items + MERGE_THREADS - 1) / MERGE_THREADS;
    const dim3 grid((unsigned)(want < MERGE_MAX_BLOCKS ? want : MERGE_MAX_BLOCKS));
    const hipStream_t s = as_stream(stream);
    const hkp_merge_view* tv = (const hkp_merge_view*)table;
#define HKP_MERGE_CASE(M, V)                                                                               \
    if (mode == M && vec == (V == 4))                                                                      \
    hipLaunchKernelGGL((logits_merge_kernel<M, V>), grid, dim3(MERGE_THREADS), 0, s, k, h, w, views, items, \
                       packed, tv, perm, out)
    HKP_MERGE_CASE(HKP_MERGE_LOGIT, 1);
    HKP_MERGE_CASE(HKP_MERGE_LOGIT, 4);
    HKP_MERGE_CASE(HKP_MERGE_PROB, 1);
    HKP_MERGE_CASE(HKP_MERGE_PROB, 4);
#undef HKP_MERGE_CASE
    HKP_LAUNCH_CHECK("hkp_logits_merge");
    return HKP_OK;
}
