// Multi-instance Gaussian target and loss (include/hulkkp.h has the definition).
//
//  * hkp_gauss_target_multi  dataset.py:36-44 with up to 16 instances per plane:
//                    t = max over the present slots of the single Gaussian of
//                    hkp_gauss_target (same fp32 operation order, so M = 1 gives
//                    its bits), 0 for a plane without a present slot.
//  * hkp_heat_loss_multi     train.py:21,25 (MSE train.py:13) against that target,
//                    recomputed in registers: heat_loss_kernel's per-element
//                    formulas, clamps and fp64 arithmetic.  Absent planes are
//                    negatives (HKP_ABSENT_ZERO) or leave the mean (HKP_ABSENT_IGNORE:
//                    dheat +0, divisor H*W*A with A counted on the device).
//  * hkp_heat_loss_multi_ex  the same launch scheme with two more choices: the
//                    quality focal kind HKP_LOSS_QFL (|t - p|^beta * BCE; beta = 2 is
//                    its own instantiation without pow) and the divisor
//                    HKP_NORM_INSTANCES (the present slots of the batch, counted by
//                    the pre-kernel that counts A).  Its kernels are its own: those
//                    of hkp_heat_loss_multi stay as they are.
//  * hkp_heat_loss_planes    hkp_heat_loss_multi_ex with a weight per plane, the loss of
//                    every plane and top-k planes per image (hard keypoint mining): a
//                    pre-kernel marks the eligible planes, the pass (two with top-k: sums,
//                    then dheat) skips the others, and a one-block kernel sums each
//                    plane's partials, ranks, fixes the divisor and forms the loss.  Its
//                    kernels are its own too.
//
// A block works on one chunk of one plane (block = plane * chunks + chunk), so
// the plane's records are read once per block: wave 0 compacts the present
// ones into LDS, and the loop over them has a wave-uniform trip count.  Each
// block writes one partial; the finalize sums them in index order.
#include "common.h"

#pragma clang fp contract(off)

namespace hkp {

constexpr int MULTI_MAX_M = 16;
constexpr int MULTI_CHUNKS = 64;   // blocks per plane at most (C3 shard tail: 32 planes -> 1920 blocks)

// blocks per plane for `items` work items of one plane: at most MULTI_CHUNKS, and as
// few as give every block the same number of 256-item trips
static inline int multi_chunks(long items) {
    const long want = (items + 255) / 256;
    if (want <= MULTI_CHUNKS) return (int)(want < 1 ? 1 : want);
    const long trips = (want + MULTI_CHUNKS - 1) / MULTI_CHUNKS;
    return (int)((want + trips - 1) / trips);
}

// the present records of a plane, compacted in slot order; returns their number
// (the same in every lane, in a scalar register).  Selected on the flag: what an
// empty slot holds is never read into the result.
__device__ __forceinline__ int stage_instances(const float* __restrict__ rec, int m, float* su, float* sv, int* scnt) {
    if (threadIdx.x < 64) {   // wave 0: lane j reads record j (one load latency), a ballot compacts
        const int j = threadIdx.x;
        float u = 0.f, v = 0.f;
        bool on = false;
        if (j < m) {
            u = rec[3 * j];
            v = rec[3 * j + 1];
            on = rec[3 * j + 2] > 0.f;
        }
        const unsigned long long mask = __ballot(on);
        if (on) {
            const int pos = __popcll(mask & ((1ull << j) - 1ull));
            su[pos] = u;
            sv[pos] = v;
        }
        if (j == 0) *scnt = __popcll(mask);
    }
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(*scnt);
}

__device__ __forceinline__ double multi_block_sum_d(double v, double* red) {
    v = wave_sum_d(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) red[wid] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
    return t;
}

template <int KIND>
__device__ __forceinline__ double loss_elem(double x, double y, double inv_n, float* g_out) {
    double l, g;
    if constexpr (KIND == HKP_LOSS_BCE) {
        l = (y - 1.0) * fmax(log1p(-x), -100.0) - y * fmax(log(x), -100.0);
        g = (x - y) / fmax((1.0 - x) * x, (double)1e-12f) * inv_n;
    } else {
        l = (x - y) * (x - y);
        g = 2.0 * inv_n * (x - y);
    }
    *g_out = (float)g;
    return l;
}

__global__ __launch_bounds__(256) void gauss_target_multi_kernel(int m, int H, int W, int chunks, float den,
                                                                const float* __restrict__ pts,
                                                                double* __restrict__ out) {
    __shared__ float su[MULTI_MAX_M], sv[MULTI_MAX_M];
    __shared__ int scnt;
    const long plane = blockIdx.x / chunks;
    const int chunk = blockIdx.x - (int)plane * chunks;
    const int cnt = stage_instances(pts + plane * 3 * m, m, su, sv, &scnt);
    const int HW = H * W;
    double* o = out + plane * (long)HW;
    for (int i = chunk * 256 + threadIdx.x; i < HW; i += chunks * 256) {
        const int yy = i / W, xx = i - yy * W;
        float t = 0.f;
        for (int j = 0; j < cnt; ++j) {
            const float dx = (float)xx - su[j], dy = (float)yy - sv[j];
            t = fmaxf(t, expf(-(dx * dx + dy * dy) / den));
        }
        o[i] = (double)t;
    }
}

// HKP_NORM_ELEMENTS: inv[0] = 1 / (H*W*A), A = planes with a present slot; 0 when there
// is none.  HKP_NORM_INSTANCES: inv[0] = 1 / max(P, 1), P = present slots of all planes.
__global__ __launch_bounds__(256) void multi_active_kernel(int planes, int m, double hw, int norm_mode,
                                                          const float* __restrict__ pts, double* __restrict__ inv) {
    __shared__ int red[4], redp[4];
    int c = 0, np = 0;
    for (int p = threadIdx.x; p < planes; p += 256) {
        const float* rec = pts + (long)p * 3 * m;
        int on = 0;
        for (int j = 0; j < m; ++j) on += rec[3 * j + 2] > 0.f ? 1 : 0;
        c += on > 0 ? 1 : 0;
        np += on;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        c += __shfl_xor(c, o);
        np += __shfl_xor(np, o);
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = c;
        redp[threadIdx.x >> 6] = np;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int a = red[0] + red[1] + red[2] + red[3];
        const int pres = redp[0] + redp[1] + redp[2] + redp[3];
        if (norm_mode == HKP_NORM_INSTANCES)
            inv[0] = 1.0 / (double)(pres > 1 ? pres : 1);
        else
            inv[0] = a > 0 ? 1.0 / (hw * (double)a) : 0.0;
    }
}

// VEC4: W % 4 == 0 and 16-byte aligned bases: an item is 4 pixels of one row
template <int KIND, bool VEC4>
__global__ __launch_bounds__(256) void heat_loss_multi_kernel(int m, int H, int W, int chunks, float den,
                                                             double inv_n_host, const double* __restrict__ inv_n_dev,
                                                             const float* __restrict__ p,
                                                             const float* __restrict__ pts, float* __restrict__ dheat,
                                                             double* __restrict__ part) {
    __shared__ float su[MULTI_MAX_M], sv[MULTI_MAX_M];
    __shared__ int scnt;
    __shared__ double red[4];
    const long plane = blockIdx.x / chunks;
    const int chunk = blockIdx.x - (int)plane * chunks;
    const int cnt = stage_instances(pts + plane * 3 * m, m, su, sv, &scnt);
    const int HW = H * W;
    const float* pp = p + plane * (long)HW;
    float* dp = dheat ? dheat + plane * (long)HW : nullptr;
    const int first = chunk * 256 + threadIdx.x, step = chunks * 256;
    // HKP_ABSENT_IGNORE (inv_n_dev set): a plane without a present slot leaves the loss
    if (inv_n_dev != nullptr && cnt == 0) {
        if (dp) {
            if constexpr (VEC4) {
                for (int q = first; q < (HW >> 2); q += step) ((f32x4*)dp)[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
                for (int i = first; i < HW; i += step) dp[i] = 0.f;
            }
        }
        if (threadIdx.x == 0) part[blockIdx.x] = 0.0;
        return;
    }
    const double inv_n = inv_n_dev ? inv_n_dev[0] : inv_n_host;
    double acc = 0.0;
    if constexpr (VEC4) {
        const int W4 = W >> 2;
        for (int q = first; q < (HW >> 2); q += step) {
            const int yy = q / W4, x0 = (q - yy * W4) * 4;
            const f32x4 xv = ((const f32x4*)pp)[q];
            float t[4] = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < cnt; ++j) {
                const float u = su[j];
                const float dy = (float)yy - sv[j];
                const float dy2 = dy * dy;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float dx = (float)(x0 + e) - u;
                    t[e] = fmaxf(t[e], expf(-(dx * dx + dy2) / den));
                }
            }
            f32x4 gv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float g;
                acc += loss_elem<KIND>((double)xv[e], (double)t[e], inv_n, &g);
                gv[e] = g;
            }
            if (dp) ((f32x4*)dp)[q] = gv;
        }
    } else {
        for (int i = first; i < HW; i += step) {
            const int yy = i / W, xx = i - yy * W;
            float t = 0.f;
            for (int j = 0; j < cnt; ++j) {
                const float dx = (float)xx - su[j], dy = (float)yy - sv[j];
                t = fmaxf(t, expf(-(dx * dx + dy * dy) / den));
            }
            float g;
            acc += loss_elem<KIND>((double)pp[i], (double)t, inv_n, &g);
            if (dp) dp[i] = g;
        }
    }
    const double s = multi_block_sum_d(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void loss_multi_finalize_kernel(int nparts, double inv_n_host,
                                                                 const double* __restrict__ inv_n_dev,
                                                                 const double* __restrict__ part, double* loss) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) s += part[i];
    const double t = multi_block_sum_d(s, red);
    if (threadIdx.x == 0) loss[0] = t * (inv_n_dev ? inv_n_dev[0] : inv_n_host);
}

// ---- hkp_heat_loss_multi_ex: the kinds of loss_elem plus the quality focal loss ----
// QFL2: beta == 2 (d*d, no pow); QFLG: any beta in [1, 8], bm1 = beta - 1.
constexpr int EX_BCE = 0, EX_MSE = 1, EX_QFL2 = 2, EX_QFLG = 3;

template <int EK>
__device__ __forceinline__ double loss_elem_ex(double x, double y, double inv_n, double beta, double bm1,
                                               float* g_out) {
    if constexpr (EK == EX_BCE) {
        return loss_elem<HKP_LOSS_BCE>(x, y, inv_n, g_out);
    } else if constexpr (EK == EX_MSE) {
        return loss_elem<HKP_LOSS_MSE>(x, y, inv_n, g_out);
    } else {
        // float64 autograd of binary_cross_entropy(x, y, 'none') * |x - y|^beta (ATen's clamps)
        const double bce = (y - 1.0) * fmax(log1p(-x), -100.0) - y * fmax(log(x), -100.0);
        const double d = x - y;
        const double den = fmax((1.0 - x) * x, (double)1e-12f);
        double l, g;
        if constexpr (EK == EX_QFL2) {
            const double dd = d * d;
            l = dd * bce;
            g = (2.0 * d * bce + dd * d / den) * inv_n;
        } else {
            const double ad = fabs(d);
            const double pm1 = pow(ad, bm1);      // |d|^(beta-1); beta = 1: exactly 1
            const double pw = pm1 * ad;
            l = pw * bce;
            g = (beta * pm1 * copysign(1.0, d) * bce + pw * d / den) * inv_n;
        }
        // p == t: the minimum, exactly (0^0 at beta = 1, the clamped logs at 0 and 1)
        if (d == 0.0) {
            l = 0.0;
            g = 0.0;
        }
        *g_out = (float)g;
        return l;
    }
}

// heat_loss_multi_kernel with the kind EK, leaving absent planes out on `ignore` and
// reading the divisor from inv_n_dev whenever it is set (either may come without the other)
template <int EK, bool VEC4>
__global__ __launch_bounds__(256) void heat_loss_multi_ex_kernel(int m, int H, int W, int chunks, float den, int ignore,
                                                                float betaf, double inv_n_host,
                                                                const double* __restrict__ inv_n_dev,
                                                                const float* __restrict__ p,
                                                                const float* __restrict__ pts,
                                                                float* __restrict__ dheat, double* __restrict__ part) {
    __shared__ float su[MULTI_MAX_M], sv[MULTI_MAX_M];
    __shared__ int scnt;
    __shared__ double red[4];
    const long plane = blockIdx.x / chunks;
    const int chunk = blockIdx.x - (int)plane * chunks;
    const int cnt = stage_instances(pts + plane * 3 * m, m, su, sv, &scnt);
    const int HW = H * W;
    const float* pp = p + plane * (long)HW;
    float* dp = dheat ? dheat + plane * (long)HW : nullptr;
    const int first = chunk * 256 + threadIdx.x, step = chunks * 256;
    if (ignore && cnt == 0) {
        if (dp) {
            if constexpr (VEC4) {
                for (int q = first; q < (HW >> 2); q += step) ((f32x4*)dp)[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
                for (int i = first; i < HW; i += step) dp[i] = 0.f;
            }
        }
        if (threadIdx.x == 0) part[blockIdx.x] = 0.0;
        return;
    }
    const double inv_n = inv_n_dev ? inv_n_dev[0] : inv_n_host;
    const double beta = (double)betaf, bm1 = beta - 1.0;
    double acc = 0.0;
    if constexpr (VEC4) {
        const int W4 = W >> 2;
        for (int q = first; q < (HW >> 2); q += step) {
            const int yy = q / W4, x0 = (q - yy * W4) * 4;
            const f32x4 xv = ((const f32x4*)pp)[q];
            float t[4] = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < cnt; ++j) {
                const float u = su[j];
                const float dy = (float)yy - sv[j];
                const float dy2 = dy * dy;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float dx = (float)(x0 + e) - u;
                    t[e] = fmaxf(t[e], expf(-(dx * dx + dy2) / den));
                }
            }
            f32x4 gv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float g;
                acc += loss_elem_ex<EK>((double)xv[e], (double)t[e], inv_n, beta, bm1, &g);
                gv[e] = g;
            }
            if (dp) ((f32x4*)dp)[q] = gv;
        }
    } else {
        for (int i = first; i < HW; i += step) {
            const int yy = i / W, xx = i - yy * W;
            float t = 0.f;
            for (int j = 0; j < cnt; ++j) {
                const float dx = (float)xx - su[j], dy = (float)yy - sv[j];
                t = fmaxf(t, expf(-(dx * dx + dy * dy) / den));
            }
            float g;
            acc += loss_elem_ex<EK>((double)pp[i], (double)t, inv_n, beta, bm1, &g);
            if (dp) dp[i] = g;
        }
    }
    const double s = multi_block_sum_d(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// ---- hkp_heat_loss_planes: plane weights, per-plane values, hard keypoint mining ----
// Its kernels are its own: those above stay as they are.  Per plane the workspace holds
// info (bit 0: eligible; the present slots from bit 8 up), used (1: counted) and S.
constexpr int PL_ALL = 0, PL_SUMS = 1, PL_GRAD = 2;   // one pass; top-k pass 1; top-k pass 2

// loss_elem_ex with the gradient kept in fp64 (the caller scales it by the plane's weight)
template <int EK>
__device__ __forceinline__ double loss_elem_pl(double x, double y, double inv_n, double beta, double bm1,
                                               double* g_out) {
    double l, g;
    if constexpr (EK == EX_BCE) {
        l = (y - 1.0) * fmax(log1p(-x), -100.0) - y * fmax(log(x), -100.0);
        g = (x - y) / fmax((1.0 - x) * x, (double)1e-12f) * inv_n;
    } else if constexpr (EK == EX_MSE) {
        l = (x - y) * (x - y);
        g = 2.0 * inv_n * (x - y);
    } else {
        const double bce = (y - 1.0) * fmax(log1p(-x), -100.0) - y * fmax(log(x), -100.0);
        const double d = x - y;
        const double den = fmax((1.0 - x) * x, (double)1e-12f);
        if constexpr (EK == EX_QFL2) {
            const double dd = d * d;
            l = dd * bce;
            g = (2.0 * d * bce + dd * d / den) * inv_n;
        } else {
            const double ad = fabs(d);
            const double pm1 = pow(ad, bm1);
            const double pw = pm1 * ad;
            l = pw * bce;
            g = (beta * pm1 * copysign(1.0, d) * bce + pw * d / den) * inv_n;
        }
        if (d == 0.0) {
            l = 0.0;
            g = 0.0;
        }
    }
    *g_out = g;
    return l;
}

// eligibility and present slots of every plane; used = eligible and inv[0] from the
// eligible planes: what holds without top-k (with it, planes_finish_kernel decides both)
__global__ __launch_bounds__(256) void planes_prepare_kernel(int planes, int m, double hw, int ignore, int norm_mode,
                                                            const float* __restrict__ pts,
                                                            const float* __restrict__ weights, int* __restrict__ info,
                                                            int* __restrict__ used, double* __restrict__ inv) {
    __shared__ int red[4], redp[4];
    int c = 0, np = 0;
    for (int p = threadIdx.x; p < planes; p += 256) {
        const float* rec = pts + (long)p * 3 * m;
        int on = 0;
        for (int j = 0; j < m; ++j) on += rec[3 * j + 2] > 0.f ? 1 : 0;
        bool el = !(ignore && on == 0);
        if (weights != nullptr && !(weights[p] > 0.f)) el = false;
        info[p] = (el ? 1 : 0) | (on << 8);
        used[p] = el ? 1 : 0;
        c += el ? 1 : 0;
        np += el ? on : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        c += __shfl_xor(c, o);
        np += __shfl_xor(np, o);
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = c;
        redp[threadIdx.x >> 6] = np;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int a = red[0] + red[1] + red[2] + red[3];
        const int pres = redp[0] + redp[1] + redp[2] + redp[3];
        if (norm_mode == HKP_NORM_INSTANCES)
            inv[0] = 1.0 / (double)(pres > 1 ? pres : 1);
        else
            inv[0] = a > 0 ? 1.0 / (hw * (double)a) : 0.0;
    }
}

// heat_loss_multi_ex_kernel on the planes that take part.  PL_ALL: the counted planes,
// partial and dheat; PL_SUMS: the eligible planes, the partial alone; PL_GRAD: the counted
// planes, dheat alone.  A plane that takes no part gets dheat +0 and none of its heat or
// labels is read.
template <int EK, bool VEC4, int MODE>
__global__ __launch_bounds__(256) void heat_loss_planes_kernel(int m, int H, int W, int chunks, float den, float betaf,
                                                              const double* __restrict__ inv_n_dev,
                                                              const int* __restrict__ info,
                                                              const int* __restrict__ used,
                                                              const float* __restrict__ weights,
                                                              const float* __restrict__ p,
                                                              const float* __restrict__ pts, float* __restrict__ dheat,
                                                              double* __restrict__ part) {
    __shared__ float su[MULTI_MAX_M], sv[MULTI_MAX_M];
    __shared__ int scnt;
    __shared__ double red[4];
    const long plane = blockIdx.x / chunks;
    const int chunk = blockIdx.x - (int)plane * chunks;
    const int HW = H * W;
    const float* pp = p + plane * (long)HW;
    float* dp = (MODE != PL_SUMS && dheat) ? dheat + plane * (long)HW : nullptr;
    const int first = chunk * 256 + threadIdx.x, step = chunks * 256;
    const int takes = __builtin_amdgcn_readfirstlane(MODE == PL_SUMS ? (info[plane] & 1) : used[plane]);
    if (!takes) {
        if (dp) {
            if constexpr (VEC4) {
                for (int q = first; q < (HW >> 2); q += step) ((f32x4*)dp)[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
                for (int i = first; i < HW; i += step) dp[i] = 0.f;
            }
        }
        return;
    }
    const int cnt = stage_instances(pts + plane * 3 * m, m, su, sv, &scnt);
    const double inv_n = MODE == PL_SUMS ? 0.0 : inv_n_dev[0];
    const double wd = weights ? (double)weights[plane] : 1.0;
    const double beta = (double)betaf, bm1 = beta - 1.0;
    double acc = 0.0;
    if constexpr (VEC4) {
        const int W4 = W >> 2;
        for (int q = first; q < (HW >> 2); q += step) {
            const int yy = q / W4, x0 = (q - yy * W4) * 4;
            const f32x4 xv = ((const f32x4*)pp)[q];
            float t[4] = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < cnt; ++j) {
                const float u = su[j];
                const float dy = (float)yy - sv[j];
                const float dy2 = dy * dy;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float dx = (float)(x0 + e) - u;
                    t[e] = fmaxf(t[e], expf(-(dx * dx + dy2) / den));
                }
            }
            f32x4 gv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                double g;
                acc += loss_elem_pl<EK>((double)xv[e], (double)t[e], inv_n, beta, bm1, &g);
                gv[e] = (float)(g * wd);
            }
            if (dp) ((f32x4*)dp)[q] = gv;
        }
    } else {
        for (int i = first; i < HW; i += step) {
            const int yy = i / W, xx = i - yy * W;
            float t = 0.f;
            for (int j = 0; j < cnt; ++j) {
                const float dx = (float)xx - su[j], dy = (float)yy - sv[j];
                t = fmaxf(t, expf(-(dx * dx + dy * dy) / den));
            }
            double g;
            acc += loss_elem_pl<EK>((double)pp[i], (double)t, inv_n, beta, bm1, &g);
            if (dp) dp[i] = (float)(g * wd);
        }
    }
    if constexpr (MODE != PL_GRAD) {
        const double s = multi_block_sum_d(acc, red);
        if (threadIdx.x == 0) part[blockIdx.x] = s;
    }
}

// r' of plane q ranks ahead of r of plane p (q != p, both of one image): the larger
// value, a NaN above every number, equal values (and two NaN) to the lower class
__device__ __forceinline__ bool planes_ahead(double rq, int cq, double rp, int cp) {
    const bool nq = rq != rq, np = rp != rp;
    if (nq || np) return nq && (!np || cq < cp);
    return rq > rp || (rq == rp && cq < cp);
}

// One block.  S of every eligible plane (its partials in chunk order); with topk > 0 the
// ranking per image, which decides `used`; the divisor from the counted planes; the two
// plane outputs; and the loss, the counted planes' w * S added in plane order.  The
// partials and the loss terms pass through LDS, PLANES_STAGE doubles at a time, so that
// the two sequential sums wait for one global load each, not one per term.
constexpr int PLANES_STAGE = 4096;   // at least MULTI_CHUNKS planes' partials

__global__ __launch_bounds__(256) void planes_finish_kernel(int planes, int k, int chunks, int topk, double hw,
                                                           int norm_mode, const float* __restrict__ weights,
                                                           const int* __restrict__ info, int* used,
                                                           const double* __restrict__ part, double* S, double* inv,
                                                           double* loss, double* __restrict__ plane_loss,
                                                           int32_t* __restrict__ plane_used) {
    __shared__ int red[4], redp[4];
    __shared__ double stage[PLANES_STAGE];
    const int tile = PLANES_STAGE / chunks;          // planes per trip, >= 64
    for (int p0 = 0; p0 < planes; p0 += tile) {
        const int np0 = planes - p0 < tile ? planes - p0 : tile;
        const double* pa0 = part + (long)p0 * chunks;
        for (int i = threadIdx.x; i < np0 * chunks; i += 256) stage[i] = pa0[i];
        __syncthreads();
        for (int p = threadIdx.x; p < np0; p += 256) {
            double s = 0.0;
            if (info[p0 + p] & 1) {
                const double* pa = stage + p * chunks;
                for (int c = 0; c < chunks; ++c) s += pa[c];
            }
            S[p0 + p] = s;
        }
        __syncthreads();
    }
    if (topk > 0) {
        for (int p = threadIdx.x; p < planes; p += 256) {
            int u = 0;
            if (info[p] & 1) {
                const int b = p / k, c = p - b * k;
                const double r = (weights ? (double)weights[p] : 1.0) * S[p];
                int ahead = 0;
                for (int cq = 0; cq < k; ++cq) {
                    const int q = b * k + cq;
                    if (cq == c || !(info[q] & 1)) continue;
                    const double rq = (weights ? (double)weights[q] : 1.0) * S[q];
                    ahead += planes_ahead(rq, cq, r, c) ? 1 : 0;
                }
                u = ahead < topk ? 1 : 0;
            }
            used[p] = u;
        }
        __syncthreads();
    }
    int cn = 0, np = 0;
    for (int p = threadIdx.x; p < planes; p += 256) {
        const int el = info[p] & 1, u = used[p];
        cn += u;
        np += u ? (info[p] >> 8) : 0;
        if (plane_loss) plane_loss[p] = el ? S[p] / hw : -1.0;
        if (plane_used) plane_used[p] = u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cn += __shfl_xor(cn, o);
        np += __shfl_xor(np, o);
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = cn;
        redp[threadIdx.x >> 6] = np;
    }
    // a plane that is not counted adds +0.0, which leaves a sum of terms >= 0 (or NaN) as it is
    double t = 0.0;
    for (int p0 = 0; p0 < planes; p0 += 256) {
        const int p = p0 + threadIdx.x;
        __syncthreads();
        stage[threadIdx.x] = (p < planes && used[p]) ? (weights ? (double)weights[p] : 1.0) * S[p] : 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int np0 = planes - p0 < 256 ? planes - p0 : 256;
            for (int i = 0; i < np0; ++i) t += stage[i];
        }
    }
    if (threadIdx.x == 0) {
        const int a = red[0] + red[1] + red[2] + red[3];
        const int pres = redp[0] + redp[1] + redp[2] + redp[3];
        double d;
        if (norm_mode == HKP_NORM_INSTANCES)
            d = 1.0 / (double)(pres > 1 ? pres : 1);
        else
            d = a > 0 ? 1.0 / (hw * (double)a) : 0.0;
        inv[0] = d;
        loss[0] = t * d;
    }
}

static inline bool multi_sizes_ok(int32_t n, int32_t k, int32_t m, int32_t H, int32_t W) {
    // a plane is indexed with 32-bit integers, the block index too
    return n > 0 && k > 0 && m >= 1 && m <= MULTI_MAX_M && H > 0 && W > 0 && (long)H * W <= (1L << 30) &&
           (long)n * k * MULTI_CHUNKS <= (1L << 30);
}

}  // namespace hkp

using namespace hkp;

extern "C" int hkp_gauss_target_multi(int32_t n, int32_t k, int32_t m, int32_t H, int32_t W, float sigma,
                                      const float* pts, double* out, hkp_stream_t stream) {
    HKP_CHECK_ARG(multi_sizes_ok(n, k, m, H, W) && sigma > 0.f,
                  "hkp_gauss_target_multi: bad sizes (1 <= m <= 16, H*W <= 2^30)");
    HKP_CHECK_ARG(pts && out, "hkp_gauss_target_multi: null tensor");
    const float den = (float)(2.0 * (double)sigma * (double)sigma);
    const int chunks = multi_chunks((long)H * W);
    hipLaunchKernelGGL(gauss_target_multi_kernel, dim3((unsigned)(n * k * chunks)), dim3(256), 0, as_stream(stream), m,
                       H, W, chunks, den, pts, out);
    HKP_LAUNCH_CHECK("hkp_gauss_target_multi");
    return HKP_OK;
}

// one double for 1 / (H*W*A), then a partial per block (at most MULTI_CHUNKS a plane)
extern "C" int64_t hkp_heat_loss_multi_workspace(int32_t n, int32_t k, int32_t H, int32_t W) {
    if (n <= 0 || k <= 0 || H <= 0 || W <= 0) return -1;
    return (int64_t)(1 + (int64_t)n * k * MULTI_CHUNKS) * (int64_t)sizeof(double);
}

extern "C" int hkp_heat_loss_multi(int32_t n, int32_t k, int32_t m, int32_t H, int32_t W, int32_t loss_kind,
                                   int32_t absent_mode, const float* heat, const float* pts, float sigma,
                                   double* loss, float* dheat, void* workspace, hkp_stream_t stream) {
    HKP_CHECK_ARG(multi_sizes_ok(n, k, m, H, W) && sigma > 0.f,
                  "hkp_heat_loss_multi: bad sizes (1 <= m <= 16, H*W <= 2^30)");
    HKP_CHECK_ARG(heat && pts && loss && workspace, "hkp_heat_loss_multi: null tensor");
    HKP_CHECK_ARG(loss_kind == HKP_LOSS_BCE || loss_kind == HKP_LOSS_MSE, "hkp_heat_loss_multi: bad loss kind");
    HKP_CHECK_ARG(absent_mode == HKP_ABSENT_ZERO || absent_mode == HKP_ABSENT_IGNORE,
                  "hkp_heat_loss_multi: bad absent mode");
    const int planes = n * k;
    const long HW = (long)H * W;
    const float den = (float)(2.0 * (double)sigma * (double)sigma);
    const bool vec4 = W % 4 == 0 && ((uintptr_t)heat & 15) == 0 && ((uintptr_t)dheat & 15) == 0;
    const int chunks = multi_chunks(vec4 ? HW / 4 : HW);
    double* inv_dev = absent_mode == HKP_ABSENT_IGNORE ? (double*)workspace : nullptr;
    double* part = (double*)workspace + 1;
    const double inv_n = 1.0 / (double)((long)planes * HW);
    const int nblocks = planes * chunks;
    hipStream_t st = as_stream(stream);
    if (inv_dev) {
        hipLaunchKernelGGL(multi_active_kernel, dim3(1), dim3(256), 0, st, planes, m, (double)HW,
                           HKP_NORM_ELEMENTS, pts, inv_dev);
        HKP_LAUNCH_CHECK("hkp_heat_loss_multi(active)");
    }
#define HKP_LOSS_M(KD, V4)                                                                                         \
    hipLaunchKernelGGL((heat_loss_multi_kernel<KD, V4>), dim3((unsigned)nblocks), dim3(256), 0, st, m, H, W, chunks, \
                       den, inv_n, inv_dev, heat, pts, dheat, part)
    if (loss_kind == HKP_LOSS_BCE) {
        if (vec4) HKP_LOSS_M(HKP_LOSS_BCE, true); else HKP_LOSS_M(HKP_LOSS_BCE, false);
    } else {
        if (vec4) HKP_LOSS_M(HKP_LOSS_MSE, true); else HKP_LOSS_M(HKP_LOSS_MSE, false);
    }
#undef HKP_LOSS_M
    HKP_LAUNCH_CHECK("hkp_heat_loss_multi");
    hipLaunchKernelGGL(loss_multi_finalize_kernel, dim3(1), dim3(256), 0, st, nblocks, inv_n, inv_dev, part, loss);
    HKP_LAUNCH_CHECK("hkp_heat_loss_multi(finalize)");
    return HKP_OK;
}

extern "C" int hkp_heat_loss_multi_ex(int32_t n, int32_t k, int32_t m, int32_t H, int32_t W, int32_t loss_kind,
                                      int32_t absent_mode, int32_t norm_mode, float beta, const float* heat,
                                      const float* pts, float sigma, double* loss, float* dheat, void* workspace,
                                      hkp_stream_t stream) {
    HKP_CHECK_ARG(multi_sizes_ok(n, k, m, H, W) && sigma > 0.f,
                  "hkp_heat_loss_multi_ex: bad sizes (1 <= m <= 16, H*W <= 2^30)");
    HKP_CHECK_ARG(heat && pts && loss && workspace, "hkp_heat_loss_multi_ex: null tensor");
    HKP_CHECK_ARG(loss_kind == HKP_LOSS_BCE || loss_kind == HKP_LOSS_MSE || loss_kind == HKP_LOSS_QFL,
                  "hkp_heat_loss_multi_ex: bad loss kind");
    HKP_CHECK_ARG(absent_mode == HKP_ABSENT_ZERO || absent_mode == HKP_ABSENT_IGNORE,
                  "hkp_heat_loss_multi_ex: bad absent mode");
    HKP_CHECK_ARG(norm_mode == HKP_NORM_ELEMENTS || norm_mode == HKP_NORM_INSTANCES,
                  "hkp_heat_loss_multi_ex: bad norm mode");
    // NaN fails both comparisons
    HKP_CHECK_ARG(loss_kind != HKP_LOSS_QFL || (beta >= 1.f && beta <= 8.f),
                  "hkp_heat_loss_multi_ex: beta %g outside [1, 8]", (double)beta);
    const int planes = n * k;
    const long HW = (long)H * W;
    const float den = (float)(2.0 * (double)sigma * (double)sigma);
    const bool vec4 = W % 4 == 0 && ((uintptr_t)heat & 15) == 0 && ((uintptr_t)dheat & 15) == 0;
    const int chunks = multi_chunks(vec4 ? HW / 4 : HW);
    const int ignore = absent_mode == HKP_ABSENT_IGNORE ? 1 : 0;
    // the divisor comes from the device unless it is the plain n*k*H*W
    double* inv_dev = (ignore || norm_mode == HKP_NORM_INSTANCES) ? (double*)workspace : nullptr;
    double* part = (double*)workspace + 1;
    const double inv_n = 1.0 / (double)((long)planes * HW);
    const int nblocks = planes * chunks;
    hipStream_t st = as_stream(stream);
    if (inv_dev) {
        hipLaunchKernelGGL(multi_active_kernel, dim3(1), dim3(256), 0, st, planes, m, (double)HW, norm_mode, pts,
                           inv_dev);
        HKP_LAUNCH_CHECK("hkp_heat_loss_multi_ex(active)");
    }
    const int ek = loss_kind == HKP_LOSS_BCE ? EX_BCE : loss_kind == HKP_LOSS_MSE ? EX_MSE
                 : beta == 2.f ? EX_QFL2 : EX_QFLG;
#define HKP_LOSS_EX(EK, V4)                                                                                     \
    hipLaunchKernelGGL((heat_loss_multi_ex_kernel<EK, V4>), dim3((unsigned)nblocks), dim3(256), 0, st, m, H, W, \
                       chunks, den, ignore, beta, inv_n, inv_dev, heat, pts, dheat, part)
#define HKP_LOSS_EX_V(EK) \
    if (vec4) HKP_LOSS_EX(EK, true); else HKP_LOSS_EX(EK, false)
    switch (ek) {
        case EX_BCE: HKP_LOSS_EX_V(EX_BCE); break;
        case EX_MSE: HKP_LOSS_EX_V(EX_MSE); break;
        case EX_QFL2: HKP_LOSS_EX_V(EX_QFL2); break;
        default: HKP_LOSS_EX_V(EX_QFLG); break;
    }
#undef HKP_LOSS_EX_V
#undef HKP_LOSS_EX
    HKP_LAUNCH_CHECK("hkp_heat_loss_multi_ex");
    hipLaunchKernelGGL(loss_multi_finalize_kernel, dim3(1), dim3(256), 0, st, nblocks, inv_n, inv_dev, part, loss);
    HKP_LAUNCH_CHECK("hkp_heat_loss_multi_ex(finalize)");
    return HKP_OK;
}

// inv, the block partials, S per plane (doubles); then info and used per plane (int32)
extern "C" int64_t hkp_heat_loss_planes_workspace(int32_t n, int32_t k, int32_t H, int32_t W) {
    if (n <= 0 || k <= 0 || H <= 0 || W <= 0) return -1;
    const int64_t planes = (int64_t)n * k;
    return (1 + planes * MULTI_CHUNKS + planes + (2 * planes + 1) / 2) * (int64_t)sizeof(double);
}

extern "C" int hkp_heat_loss_planes(int32_t n, int32_t k, int32_t m, int32_t H, int32_t W, int32_t loss_kind,
                                    int32_t absent_mode, int32_t norm_mode, float beta, int32_t topk,
                                    const float* heat, const float* pts, const float* weights, float sigma,
                                    double* loss, float* dheat, double* plane_loss, int32_t* plane_used,
                                    void* workspace, hkp_stream_t stream) {
    HKP_CHECK_ARG(multi_sizes_ok(n, k, m, H, W) && sigma > 0.f,
                  "hkp_heat_loss_planes: bad sizes (1 <= m <= 16, H*W <= 2^30)");
    HKP_CHECK_ARG(heat && pts && loss && workspace, "hkp_heat_loss_planes: null tensor");
    HKP_CHECK_ARG(loss_kind == HKP_LOSS_BCE || loss_kind == HKP_LOSS_MSE || loss_kind == HKP_LOSS_QFL,
                  "hkp_heat_loss_planes: bad loss kind");
    HKP_CHECK_ARG(absent_mode == HKP_ABSENT_ZERO || absent_mode == HKP_ABSENT_IGNORE,
                  "hkp_heat_loss_planes: bad absent mode");
    HKP_CHECK_ARG(norm_mode == HKP_NORM_ELEMENTS || norm_mode == HKP_NORM_INSTANCES,
                  "hkp_heat_loss_planes: bad norm mode");
    // NaN fails both comparisons
    HKP_CHECK_ARG(loss_kind != HKP_LOSS_QFL || (beta >= 1.f && beta <= 8.f),
                  "hkp_heat_loss_planes: beta %g outside [1, 8]", (double)beta);
    HKP_CHECK_ARG(topk >= 0 && topk <= k && (topk == 0 || k <= 64),
                  "hkp_heat_loss_planes: topk %d outside 0..k (k = %d; at most 64 classes with top-k)", topk, k);
    const int planes = n * k;
    const long HW = (long)H * W;
    const float den = (float)(2.0 * (double)sigma * (double)sigma);
    const bool vec4 = W % 4 == 0 && ((uintptr_t)heat & 15) == 0 && ((uintptr_t)dheat & 15) == 0;
    const int chunks = multi_chunks(vec4 ? HW / 4 : HW);
    const int ignore = absent_mode == HKP_ABSENT_IGNORE ? 1 : 0;
    double* inv_dev = (double*)workspace;
    double* part = inv_dev + 1;
    double* S = part + (long)planes * MULTI_CHUNKS;
    int* info = (int*)(S + planes);
    int* used = info + planes;
    const int nblocks = planes * chunks;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(planes_prepare_kernel, dim3(1), dim3(256), 0, st, planes, m, (double)HW, ignore, norm_mode, pts,
                       weights, info, used, inv_dev);
    HKP_LAUNCH_CHECK("hkp_heat_loss_planes(prepare)");
    const int ek = loss_kind == HKP_LOSS_BCE ? EX_BCE : loss_kind == HKP_LOSS_MSE ? EX_MSE
                 : beta == 2.f ? EX_QFL2 : EX_QFLG;
#define HKP_LOSS_PL(EK, V4, MODE)                                                                                  \
    hipLaunchKernelGGL((heat_loss_planes_kernel<EK, V4, MODE>), dim3((unsigned)nblocks), dim3(256), 0, st, m, H, W, \
                       chunks, den, beta, inv_dev, info, used, weights, heat, pts, dheat, part)
#define HKP_LOSS_PL_V(EK, MODE) \
    if (vec4) HKP_LOSS_PL(EK, true, MODE); else HKP_LOSS_PL(EK, false, MODE)
#define HKP_LOSS_PL_K(MODE)                               \
    switch (ek) {                                         \
        case EX_BCE: HKP_LOSS_PL_V(EX_BCE, MODE); break;  \
        case EX_MSE: HKP_LOSS_PL_V(EX_MSE, MODE); break;  \
        case EX_QFL2: HKP_LOSS_PL_V(EX_QFL2, MODE); break; \
        default: HKP_LOSS_PL_V(EX_QFLG, MODE); break;     \
    }
    if (topk == 0) {
        HKP_LOSS_PL_K(PL_ALL)
    } else {
        HKP_LOSS_PL_K(PL_SUMS)
    }
    HKP_LAUNCH_CHECK("hkp_heat_loss_planes");
    hipLaunchKernelGGL(planes_finish_kernel, dim3(1), dim3(256), 0, st, planes, k, chunks, topk, (double)HW, norm_mode,
                       weights, info, used, part, S, inv_dev, loss, plane_loss, plane_used);
    HKP_LAUNCH_CHECK("hkp_heat_loss_planes(finish)");
    if (topk > 0 && dheat != nullptr) {
        HKP_LOSS_PL_K(PL_GRAD)
        HKP_LAUNCH_CHECK("hkp_heat_loss_planes(dheat)");
    }
#undef HKP_LOSS_PL_K
#undef HKP_LOSS_PL_V
#undef HKP_LOSS_PL
    return HKP_OK;
}
