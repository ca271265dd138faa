// Multi-instance Gaussian target and loss (include/hulkkp.h has the definition).
//
//  * hkp_gauss_target_multi  dataset.py:36-44 with up to 16 instances per plane:
//                    t = max over the present slots of the single Gaussian of
//                    hkp_gauss_target (same fp32 operation order, so M = 1 gives
//                    its bits), 0 for a plane without a present slot.
//  * hkp_heat_loss_multi     train.py:21,25 (MSE train.py:13) against that target,
//                    recomputed in registers, with loss.hip's per-element formulas,
//                    clamps and fp64 arithmetic (loss_elem.h).  Absent planes are
//                    negatives (HKP_ABSENT_ZERO) or leave the mean (HKP_ABSENT_IGNORE:
//                    dheat +0, divisor H*W*A with A counted on the device).
//  * hkp_heat_loss_multi_ex  two more choices: the quality focal kind HKP_LOSS_QFL
//                    (|t - p|^beta * BCE; beta = 2 is its own instantiation without
//                    pow) and the divisor HKP_NORM_INSTANCES (the present slots of the
//                    batch).  hkp_heat_loss_multi is this entry at BCE / MSE and
//                    HKP_NORM_ELEMENTS, under its own name.
//  * hkp_heat_loss_planes    with a weight per plane, the loss of every plane and top-k
//                    planes per image (hard keypoint mining): the pass (two with top-k:
//                    sums, then dheat) skips the planes that take no part, and a
//                    one-block kernel sums each plane's partials, ranks, fixes the
//                    divisor and forms the loss.
//  * hkp_heat_loss_masked    hkp_heat_loss_planes with a per-pixel ignore mask, uint8 [n][H][W]
//                    of class bits: a count pass over the mask (the kept pixels of every
//                    plane), then the planes entry's launches with the mask flag set: a
//                    masked pixel is selected out of the sum and of dheat, a plane's mean
//                    and the elements divisor run over the kept pixels.
//  * hkp_heat_loss_lines     the planes / masked entries over line labels [n][k][s][5]: the
//                    same pre-, count- and finish-kernels around line_loss_walk_kernel,
//                    which walks a plane's 32 x 32 tiles with lines.hip's staging and cull.
//
// All three losses are one body, heat_loss_walk_kernel, a template over (kind, 16-byte
// path, mode); the mode says which planes take part and what a block leaves behind:
//   WALK_EX   hkp_heat_loss_multi(_ex): a plane without a present slot is left out under
//             `ignore`; its blocks write a partial of 0; the divisor is the host's, or
//             the device's when inv_n_dev is set.
//   PL_ALL    hkp_heat_loss_planes in one pass: the counted planes (`used`), partial and
//             dheat.  PL_SUMS (top-k, pass 1): the eligible planes (`info`), the partial
//             alone.  PL_GRAD (top-k, pass 2): the counted planes, dheat alone.  A plane
//             that takes no part writes no partial and none of its heat or labels is read.
// A block works on one chunk of one plane (block = plane * chunks + chunk), so the
// plane's records are read once per block: wave 0 compacts the present ones into LDS,
// and the loop over them has a wave-uniform trip count.  Each block writes one partial;
// the finalize / finish kernel sums them in index order.
#include <string>

#include "common.h"
#include "lines_dev.h"
#include "loss_elem.h"

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

// the target at pixel (xx, yy): the largest of the cnt staged instances' Gaussians
__device__ __forceinline__ float target_at(int xx, int yy, int cnt, const float* su, const float* sv, float den) {
    float t = 0.f;
    for (int j = 0; j < cnt; ++j) {
        const float dx = (float)xx - su[j], dy = (float)yy - sv[j];
        t = fmaxf(t, expf(-(dx * dx + dy * dy) / den));
    }
    return t;
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
        const int yy = i / W;
        o[i] = (double)target_at(i - yy * W, yy, cnt, su, sv, den);
    }
}

// HKP_NORM_ELEMENTS: 1 / (H*W*a), a = the planes that count; 0 when there is none.
// HKP_NORM_INSTANCES: 1 / max(pres, 1), pres = their present slots.
__device__ __forceinline__ double loss_divisor(int norm_mode, int a, int pres, double hw) {
    if (norm_mode == HKP_NORM_INSTANCES) return 1.0 / (double)(pres > 1 ? pres : 1);
    return a > 0 ? 1.0 / (hw * (double)a) : 0.0;
}

// hkp_heat_loss_masked's divisor.  HKP_NORM_ELEMENTS: 1 / the kept pixels of the planes that
// count (an exact integer), 0 when there is none; HKP_NORM_INSTANCES as loss_divisor.
__device__ __forceinline__ double masked_divisor(int norm_mode, long long kept, int pres) {
    if (norm_mode == HKP_NORM_INSTANCES) return 1.0 / (double)(pres > 1 ? pres : 1);
    return kept > 0 ? 1.0 / (double)kept : 0.0;
}

// One block, before the pass.  A plane is eligible unless it has no present slot under
// `ignore`, or weights is given and its weight is not > 0.  inv[0]: the divisor over the
// eligible planes.  With info / used (hkp_heat_loss_planes; both or neither), per plane:
// info = bit 0: eligible, the present slots from bit 8 up; used = eligible, which is what
// holds without top-k (with it, planes_finish_kernel decides `used` and the divisor).
// MASKED (hkp_heat_loss_masked): npix[p] = the plane's kept pixels, H*W less the set bits
// of its class that mask_count_kernel counted (cnt [n][mchunks][8], added here: integers,
// any order); a plane without a kept pixel is not eligible, and HKP_NORM_ELEMENTS divides
// by the eligible planes' kept pixels.
// RS, FO: the floats of a label record and where its flag is: (u, v, flag) for points,
// (x0, y0, x1, y1, flag) for hkp_heat_loss_lines' segments.
template <bool MASKED, int RS = 3, int FO = 2>
__global__ __launch_bounds__(256) void planes_count_kernel(int planes, int m, double hw, int ignore, int norm_mode,
                                                          const float* __restrict__ pts,
                                                          const float* __restrict__ weights, int* __restrict__ info,
                                                          int* __restrict__ used, double* __restrict__ inv, int k,
                                                          int mchunks, const int* __restrict__ cnt,
                                                          int* __restrict__ npix) {
    __shared__ int red[4], redp[4];
    __shared__ long long redn[4];
    int c = 0, np = 0;
    long long ne = 0;
    for (int p = threadIdx.x; p < planes; p += 256) {
        const float* rec = pts + (long)p * RS * m;
        int on = 0;
        for (int j = 0; j < m; ++j) on += rec[RS * j + FO] > 0.f ? 1 : 0;
        bool el = !(ignore && on == 0);
        if (weights != nullptr && !(weights[p] > 0.f)) el = false;
        if constexpr (MASKED) {
            const int b = p / k, cl = p - b * k;
            const int* cb = cnt + (long)b * mchunks * 8 + cl;
            int set = 0;
            for (int j = 0; j < mchunks; ++j) set += cb[8 * j];
            const int kept = (int)hw - set;
            npix[p] = kept;
            if (kept <= 0) el = false;
            ne += el ? kept : 0;
        }
        if (info != nullptr) {
            info[p] = (el ? 1 : 0) | (on << 8);
            used[p] = el ? 1 : 0;
        }
        c += el ? 1 : 0;
        np += el ? on : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        c += __shfl_xor(c, o);
        np += __shfl_xor(np, o);
        if constexpr (MASKED) ne += __shfl_xor(ne, o);
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = c;
        redp[threadIdx.x >> 6] = np;
        if constexpr (MASKED) redn[threadIdx.x >> 6] = ne;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if constexpr (MASKED)
            inv[0] = masked_divisor(norm_mode, redn[0] + redn[1] + redn[2] + redn[3],
                                    redp[0] + redp[1] + redp[2] + redp[3]);
        else
            inv[0] = loss_divisor(norm_mode, red[0] + red[1] + red[2] + red[3], redp[0] + redp[1] + redp[2] + redp[3], hw);
    }
}

// The set bits of every class in a slice of one image's mask: block (image, chunk) leaves
// cnt[image][chunk][8].  An item is 4 bytes, one 32-bit load when the image's bytes are
// 4-byte aligned (WORD), 4 bounded byte loads otherwise.
constexpr int MASK_MAX_K = 8;
template <bool WORD>
__global__ __launch_bounds__(256) void mask_count_kernel(int HW, int mchunks, const uint8_t* __restrict__ mask,
                                                        int* __restrict__ cnt) {
    __shared__ int red[4][8];
    const int b = blockIdx.x / mchunks, chunk = blockIdx.x - b * mchunks;
    const uint8_t* mi = mask + (long)b * HW;
    const int items = (HW + 3) >> 2;
    int s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int q = chunk * 256 + threadIdx.x; q < items; q += mchunks * 256) {
        uint32_t w;
        if constexpr (WORD) {
            w = ((const uint32_t*)mi)[q];
        } else {
            w = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * q + e < HW) w |= (uint32_t)mi[4 * q + e] << (8 * e);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] += __popc(w & (0x01010101u << j));
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[j] += __shfl_xor(s[j], o);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) red[threadIdx.x >> 6][j] = s[j];
    }
    __syncthreads();
    if (threadIdx.x < 8)
        cnt[(long)blockIdx.x * 8 + threadIdx.x] =
            red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

constexpr int WALK_EX = 0, PL_ALL = 1, PL_SUMS = 2, PL_GRAD = 3;   // the header has what each means

// The plane walk.  VEC4: W % 4 == 0 and 16-byte aligned bases: an item is 4 pixels of one
// row.  ignore and inv_n_host are read by WALK_EX alone (inv_n_dev, when set, goes before
// inv_n_host); info, used and weights by the PL_ modes alone, and they come last so that
// WALK_EX keeps the argument offsets it was measured with ("One body").
// MASKED (PL_ modes, hkp_heat_loss_masked): bit (plane % k) of mask[image][pixel] takes the
// pixel out: its term and its dheat are +0 by a select, whatever its heat holds.  Under
// VEC4 the 4 mask bytes of an item are one 32-bit load when the mask base is 4-byte
// aligned (W % 4 == 0 holds), 4 byte loads otherwise.  mask and k are the last arguments.
template <int EK, bool VEC4, int MODE, bool MASKED = false>
__global__ __launch_bounds__(256) void heat_loss_walk_kernel(int m, int H, int W, int chunks, float den, int ignore,
                                                            float betaf, double inv_n_host,
                                                            const double* __restrict__ inv_n_dev,
                                                            const float* __restrict__ p,
                                                            const float* __restrict__ pts, float* __restrict__ dheat,
                                                            double* __restrict__ part, const int* __restrict__ info,
                                                            const int* __restrict__ used,
                                                            const float* __restrict__ weights,
                                                            const uint8_t* __restrict__ mask, int k) {
    static_assert(!MASKED || MODE != WALK_EX, "the mask goes with the planes modes");
    __shared__ float su[MULTI_MAX_M], sv[MULTI_MAX_M];
    __shared__ int scnt;
    __shared__ double red[4];
    const long plane = blockIdx.x / chunks;
    const int chunk = blockIdx.x - (int)plane * chunks;
    const int HW = H * W;
    const float* pp = p + plane * (long)HW;
    float* dp = (MODE != PL_SUMS && dheat) ? dheat + plane * (long)HW : nullptr;
    const int first = chunk * 256 + threadIdx.x, step = chunks * 256;
    const float* rec = pts + plane * 3 * m;
    int cnt = 0, takes;
    if constexpr (MODE == WALK_EX) {
        cnt = stage_instances(rec, m, su, sv, &scnt);
        takes = !(ignore && cnt == 0);
    } else {
        takes = __builtin_amdgcn_readfirstlane(MODE == PL_SUMS ? (info[plane] & 1) : used[plane]);
    }
    if (__builtin_expect(!takes, 0)) {   // the plane leaves the loss: dheat +0 (unlikely: kept behind the loops)
        if (dp) {
            if constexpr (VEC4) {
                for (int q = first; q < (HW >> 2); q += step) ((f32x4*)dp)[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
                for (int i = first; i < HW; i += step) dp[i] = 0.f;
            }
        }
        if (MODE == WALK_EX && threadIdx.x == 0) part[blockIdx.x] = 0.0;
        return;
    }
    if constexpr (MODE != WALK_EX) cnt = stage_instances(rec, m, su, sv, &scnt);
    double inv_n;
    if constexpr (MODE == WALK_EX) inv_n = inv_n_dev ? inv_n_dev[0] : inv_n_host;
    else inv_n = MODE == PL_SUMS ? 0.0 : inv_n_dev[0];
    // the planes entry scales the fp64 gradient by the plane's weight before the cast
    const double wd = (MODE != WALK_EX && weights) ? (double)weights[plane] : 1.0;
    const double beta = (double)betaf, bm1 = beta - 1.0;
    double acc = 0.0;
    const uint8_t* mi = nullptr;
    int cbit = 0;
    bool mword = false;
    if constexpr (MASKED) {
        const long img = plane / k;
        cbit = (int)(plane - img * k);
        mi = mask + img * (long)HW;
        mword = ((uintptr_t)mi & 3) == 0;
    }
    if constexpr (VEC4) {
        const int W4 = W >> 2;
        for (int q = first; q < (HW >> 2); q += step) {
            const int yy = q / W4, x0 = (q - yy * W4) * 4;
            const f32x4 xv = ((const f32x4*)pp)[q];
            uint32_t mw = 0;
            if constexpr (MASKED) {
                if (mword) {
                    mw = ((const uint32_t*)mi)[q];
                } else {
                    const uint8_t* mb = mi + 4 * (long)q;
                    mw = (uint32_t)mb[0] | ((uint32_t)mb[1] << 8) | ((uint32_t)mb[2] << 16) | ((uint32_t)mb[3] << 24);
                }
                mw >>= cbit;
            }
            float t[4] = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < cnt; ++j) {   // target_at for 4 pixels of a row: dy once
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
                const double l = loss_elem<EK>((double)xv[e], (double)t[e], inv_n, beta, bm1, &g);
                if constexpr (MASKED) {
                    const bool keep = !((mw >> (8 * e)) & 1u);
                    acc += keep ? l : 0.0;
                    gv[e] = keep ? (float)(g * wd) : 0.f;
                } else {
                    acc += l;
                    gv[e] = MODE == WALK_EX ? (float)g : (float)(g * wd);
                }
            }
            if (dp) ((f32x4*)dp)[q] = gv;
        }
    } else {
        for (int i = first; i < HW; i += step) {
            const int yy = i / W;
            const float t = target_at(i - yy * W, yy, cnt, su, sv, den);
            double g;
            const double l = loss_elem<EK>((double)pp[i], (double)t, inv_n, beta, bm1, &g);
            if constexpr (MASKED) {
                const bool keep = !((mi[i] >> cbit) & 1);
                acc += keep ? l : 0.0;
                if (dp) dp[i] = keep ? (float)(g * wd) : 0.f;
            } else {
                acc += l;
                if (dp) dp[i] = MODE == WALK_EX ? (float)g : (float)(g * wd);
            }
        }
    }
    if constexpr (MODE != PL_GRAD) {
        const double s = block_sum_d(acc, red);
        if (threadIdx.x == 0) part[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(256) void loss_multi_finalize_kernel(int nparts, double inv_n_host,
                                                                 const double* __restrict__ inv_n_dev,
                                                                 const double* __restrict__ part, double* loss) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) s += part[i];
    const double t = block_sum_d(s, red);
    if (threadIdx.x == 0) loss[0] = t * (inv_n_dev ? inv_n_dev[0] : inv_n_host);
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

// MASKED: a plane's mean, in plane_loss and in the ranking, is S over its kept pixels
// (npix), the divisor of HKP_NORM_ELEMENTS the counted planes' kept pixels, and
// plane_pixels gets npix (0 for a plane that is not eligible).
template <bool MASKED>
__global__ __launch_bounds__(256) void planes_finish_kernel(int planes, int k, int chunks, int topk, double hw,
                                                           int norm_mode, const float* __restrict__ weights,
                                                           const int* __restrict__ info, int* used,
                                                           const double* __restrict__ part, double* S, double* inv,
                                                           double* loss, double* __restrict__ plane_loss,
                                                           int32_t* __restrict__ plane_used,
                                                           const int* __restrict__ npix,
                                                           int32_t* __restrict__ plane_pixels) {
    __shared__ int red[4], redp[4];
    __shared__ long long redn[4];
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
                const double r = (weights ? (double)weights[p] : 1.0) * (MASKED ? S[p] / (double)npix[p] : S[p]);
                int ahead = 0;
                for (int cq = 0; cq < k; ++cq) {
                    const int q = b * k + cq;
                    if (cq == c || !(info[q] & 1)) continue;
                    const double rq =
                        (weights ? (double)weights[q] : 1.0) * (MASKED ? S[q] / (double)npix[q] : S[q]);
                    ahead += planes_ahead(rq, cq, r, c) ? 1 : 0;
                }
                u = ahead < topk ? 1 : 0;
            }
            used[p] = u;
        }
        __syncthreads();
    }
    int cn = 0, np = 0;
    long long ne = 0;
    for (int p = threadIdx.x; p < planes; p += 256) {
        const int el = info[p] & 1, u = used[p];
        cn += u;
        np += u ? (info[p] >> 8) : 0;
        if constexpr (MASKED) {
            ne += u ? npix[p] : 0;
            if (plane_loss) plane_loss[p] = el ? S[p] / (double)npix[p] : -1.0;
            if (plane_pixels) plane_pixels[p] = el ? npix[p] : 0;
        } else {
            if (plane_loss) plane_loss[p] = el ? S[p] / hw : -1.0;
        }
        if (plane_used) plane_used[p] = u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cn += __shfl_xor(cn, o);
        np += __shfl_xor(np, o);
        if constexpr (MASKED) ne += __shfl_xor(ne, o);
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = cn;
        redp[threadIdx.x >> 6] = np;
        if constexpr (MASKED) redn[threadIdx.x >> 6] = ne;
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
        double d;
        if constexpr (MASKED)
            d = masked_divisor(norm_mode, redn[0] + redn[1] + redn[2] + redn[3],
                               redp[0] + redp[1] + redp[2] + redp[3]);
        else
            d = loss_divisor(norm_mode, red[0] + red[1] + red[2] + red[3], redp[0] + redp[1] + redp[2] + redp[3], hw);
        inv[0] = d;
        loss[0] = t * d;
    }
}

// blocks per plane for a plane of `tiles` 32 x 32 tiles: multi_chunks' rule on tiles (one
// tile a trip)
static inline int line_chunks(int tiles) {
    if (tiles <= MULTI_CHUNKS) return tiles;
    const int trips = (tiles + MULTI_CHUNKS - 1) / MULTI_CHUNKS;
    return (tiles + trips - 1) / trips;
}

// hkp_heat_loss_lines' walk: the PL_ modes of heat_loss_walk_kernel over line labels.  A
// block owns one chunk of one plane (block = plane * chunks + chunk) and walks the plane's
// LINE_TW x LINE_TH tiles chunk, chunk + chunks, ...; a thread has 4 pixels of a row in each.
// The plane's records are read once per block, one slot per thread (waves 0 and 1); per
// tile they are bounded, culled and compacted into LDS exactly as line_target_kernel does
// it (lines.hip's header and DESIGN "Line labels" have the argument), so d2 and the target
// have hkp_line_target's bits.  VEC4: W % 4 == 0 and 16-byte aligned heat and dheat: the 4
// pixels are one load and one store; mword: W % 4 == 0 and a 4-byte aligned mask: the 4
// mask bytes are one load.  Every thread adds its elements into one accumulator over all
// its tiles; the block leaves one partial.
template <int EK, bool VEC4, int MODE, bool MASKED>
__global__ __launch_bounds__(256) void line_loss_walk_kernel(int s, int H, int W, int tiles_x, int tiles, int chunks,
                                                            float den, float betaf, int mword,
                                                            const double* __restrict__ inv_n_dev,
                                                            const float* __restrict__ p,
                                                            const float* __restrict__ lines,
                                                            float* __restrict__ dheat, double* __restrict__ part,
                                                            const int* __restrict__ info,
                                                            const int* __restrict__ used,
                                                            const float* __restrict__ weights,
                                                            const uint8_t* __restrict__ mask, int k) {
    static_assert(MODE == PL_ALL || MODE == PL_SUMS || MODE == PL_GRAD, "the planes modes");
    __shared__ f32x4 sseg[HKP_LINE_MAX_S];
    __shared__ float sinv[HKP_LINE_MAX_S];
    __shared__ int swc[2];
    __shared__ float swub[2];
    __shared__ double red[4];
    const long plane = blockIdx.x / chunks;
    const int chunk = blockIdx.x - (int)plane * chunks;
    const int HW = H * W;
    const float* pp = p + plane * (long)HW;
    float* dp = (MODE != PL_SUMS && dheat) ? dheat + plane * (long)HW : nullptr;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int tx = (threadIdx.x & 7) * 4, ty = threadIdx.x >> 3;
    const int takes = __builtin_amdgcn_readfirstlane(MODE == PL_SUMS ? (info[plane] & 1) : used[plane]);
    if (__builtin_expect(!takes, 0)) {   // the plane leaves the loss: dheat +0 over this block's tiles
        if (dp) {
            for (int tile = chunk; tile < tiles; tile += chunks) {
                const int tile_y = tile / tiles_x;
                const int x = (tile - tile_y * tiles_x) * LINE_TW + tx, y = tile_y * LINE_TH + ty;
                if (y < H && x < W) {
                    float* o = dp + (long)y * W + x;
                    if constexpr (VEC4) {
                        *(f32x4*)o = f32x4{0.f, 0.f, 0.f, 0.f};
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (x + e < W) o[e] = 0.f;
                    }
                }
            }
        }
        return;
    }
    // ---- the plane's present slots and their constants, once (waves 0 and 1: slot = thread)
    float x0 = 0.f, y0 = 0.f, dx = 0.f, dy = 0.f, inv = 0.f;
    bool present = false;
    if (threadIdx.x < s) {
        const float* rec = lines + (plane * s + threadIdx.x) * 5;
        present = rec[4] > 0.f;
        if (present) {
            x0 = rec[0], y0 = rec[1];
            dx = rec[2] - x0, dy = rec[3] - y0;
            const float l2 = dx * dx + dy * dy;
            inv = l2 > 0.f ? 1.0f / l2 : 0.f;
        }
    }
    const double inv_n = MODE == PL_SUMS ? 0.0 : inv_n_dev[0];
    const double wd = weights ? (double)weights[plane] : 1.0;
    const double beta = (double)betaf, bm1 = beta - 1.0;
    const uint8_t* mi = nullptr;
    int cbit = 0;
    if constexpr (MASKED) {
        const long img = plane / k;
        cbit = (int)(plane - img * k);
        mi = mask + img * (long)HW;
    }
    double acc = 0.0;
    for (int tile = chunk; tile < tiles; tile += chunks) {   // block-uniform
        const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
        const int xa = tile_x * LINE_TW, ya = tile_y * LINE_TH;
        const int xb = min(xa + LINE_TW, W) - 1, yb = min(ya + LINE_TH, H) - 1;   // the tile's last pixel
        const float fxa = (float)xa, fya = (float)ya, fxb = (float)xb, fyb = (float)yb;
        const float mx = 0.5f * (fxa + fxb), my = 0.5f * (fya + fyb);
        const float ex = fxb - fxa, ey = fyb - fya;
        const float rad = 0.5f * sqrtf(ex * ex + ey * ey);
        // ---- the bounds of every present segment over this tile
        float lb = 0.f, ub = INFINITY;
        bool on = present;
        if (threadIdx.x < HKP_LINE_MAX_S) {
            if (on) {
                const float c = fmaxf(fmaxf(seg_d2(fxa, fya, x0, y0, dx, dy, inv), seg_d2(fxb, fya, x0, y0, dx, dy, inv)),
                                      fmaxf(seg_d2(fxa, fyb, x0, y0, dx, dy, inv), seg_d2(fxb, fyb, x0, y0, dx, dy, inv)));
                ub = sqrtf(c);
                lb = sqrtf(seg_d2(mx, my, x0, y0, dx, dy, inv)) - rad;
            }
            float wub = ub;   // +inf where the slot is empty; fminf passes over a NaN
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) wub = fminf(wub, __shfl_xor(wub, o));
            if (lane == 0) swub[wid] = wub;
        }
        __syncthreads();
        // ---- drop what cannot be nearest anywhere in the tile; compact the rest
        unsigned long long bal = 0;
        if (threadIdx.x < HKP_LINE_MAX_S) {
            const float best = fminf(swub[0], swub[1]);
            on = on && !(lb > best + CULL_MARGIN);
            bal = __ballot(on);
            if (lane == 0) swc[wid] = __popcll(bal);
        }
        __syncthreads();
        if (threadIdx.x < HKP_LINE_MAX_S && on) {
            const int pos = (wid == 1 ? swc[0] : 0) + __popcll(bal & ((1ull << lane) - 1ull));
            sseg[pos] = f32x4{x0, y0, dx, dy};
            sinv[pos] = inv;
        }
        __syncthreads();
        const int cnt = __builtin_amdgcn_readfirstlane(swc[0] + swc[1]);

        // ---- 4 pixels of a row per thread, the survivors in slot order
        const int x = xa + tx, y = ya + ty;
        if (y < H && x < W) {
            float d[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
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
            const long at = (long)y * W + x;
            float hv[4] = {0.5f, 0.5f, 0.5f, 0.5f};   // a pixel past the row's end is selected out below
            if constexpr (VEC4) {
                const f32x4 xv = *(const f32x4*)(pp + at);
#pragma unroll
                for (int e = 0; e < 4; ++e) hv[e] = xv[e];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (x + e < W) hv[e] = pp[at + e];
            }
            uint32_t mw = 0;
            if constexpr (MASKED) {
                if (mword) {
                    mw = *(const uint32_t*)(mi + at);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (x + e < W) mw |= (uint32_t)mi[at + e] << (8 * e);
                }
                mw >>= cbit;
            }
            float gv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float t = cnt > 0 ? expf(-d[e] / den) : 0.f;
                double g;
                const double l = loss_elem<EK>((double)hv[e], (double)t, inv_n, beta, bm1, &g);
                const bool keep = (VEC4 || x + e < W) && !(MASKED && ((mw >> (8 * e)) & 1u));
                if constexpr (MODE != PL_GRAD) acc += keep ? l : 0.0;
                gv[e] = keep ? (float)(g * wd) : 0.f;
            }
            if (dp) {
                float* o = dp + at;
                if constexpr (VEC4) {
                    *(f32x4*)o = f32x4{gv[0], gv[1], gv[2], gv[3]};
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (x + e < W) o[e] = gv[e];
                }
            }
        }
        __syncthreads();   // the next tile restages sseg / swc
    }
    if constexpr (MODE != PL_GRAD) {
        const double sum = block_sum_d(acc, red);
        if (threadIdx.x == 0) part[blockIdx.x] = sum;
    }
}

static inline bool multi_sizes_ok(int32_t n, int32_t k, int32_t m, int32_t H, int32_t W) {
    // a plane is indexed with 32-bit integers, the block index too
    return n > 0 && k > 0 && m >= 1 && m <= MULTI_MAX_M && H > 0 && W > 0 && (long)H * W <= (1L << 30) &&
           (long)n * k * MULTI_CHUNKS <= (1L << 30);
}

// What the three loss entries check and derive alike.  The workspace starts with the
// device's divisor and the block partials (at most MULTI_CHUNKS a plane); weights, info
// and used are hkp_heat_loss_planes' own and stay null for the others.
struct LossPlan {
    int planes, m, H, W, chunks, nblocks, ek, ignore, norm_mode;
    bool vec4;
    float den, beta;
    double hw, inv_n;   // H*W; 1 / (n*k*H*W), the divisor the host knows
    const float *heat, *pts, *weights;
    float* dheat;
    double *inv_dev, *part;
    int *info, *used;
    // hkp_heat_loss_masked's own: the mask, its classes, the count pass's chunks and partial
    // counts, the kept pixels per plane
    const uint8_t* mask;
    int k, mchunks;
    int *cnt, *npix;
};

// `who` is the entry's name in the error texts, qfl_ok whether it knows HKP_LOSS_QFL
static int loss_plan(const char* who, bool qfl_ok, int32_t n, int32_t k, int32_t m, int32_t H, int32_t W,
                     int32_t loss_kind, int32_t absent_mode, int32_t norm_mode, float beta, const float* heat,
                     const float* pts, float sigma, double* loss, float* dheat, void* workspace, LossPlan* lp) {
    HKP_CHECK_ARG(multi_sizes_ok(n, k, m, H, W) && sigma > 0.f, "%s: bad sizes (1 <= m <= 16, H*W <= 2^30)", who);
    HKP_CHECK_ARG(heat && pts && loss && workspace, "%s: null tensor", who);
    HKP_CHECK_ARG(loss_kind == HKP_LOSS_BCE || loss_kind == HKP_LOSS_MSE || (qfl_ok && loss_kind == HKP_LOSS_QFL),
                  "%s: bad loss kind", who);
    HKP_CHECK_ARG(absent_mode == HKP_ABSENT_ZERO || absent_mode == HKP_ABSENT_IGNORE, "%s: bad absent mode", who);
    HKP_CHECK_ARG(norm_mode == HKP_NORM_ELEMENTS || norm_mode == HKP_NORM_INSTANCES, "%s: bad norm mode", who);
    // NaN fails both comparisons
    HKP_CHECK_ARG(loss_kind != HKP_LOSS_QFL || (beta >= 1.f && beta <= 8.f), "%s: beta %g outside [1, 8]", who,
                  (double)beta);
    *lp = LossPlan{};
    const long HW = (long)H * W;
    lp->planes = n * k;
    lp->m = m, lp->H = H, lp->W = W;
    lp->vec4 = W % 4 == 0 && ((uintptr_t)heat & 15) == 0 && ((uintptr_t)dheat & 15) == 0;
    lp->chunks = multi_chunks(lp->vec4 ? HW / 4 : HW);
    lp->nblocks = lp->planes * lp->chunks;
    lp->ek = loss_kind == HKP_LOSS_BCE ? EK_BCE : loss_kind == HKP_LOSS_MSE ? EK_MSE : beta == 2.f ? EK_QFL2 : EK_QFLG;
    lp->ignore = absent_mode == HKP_ABSENT_IGNORE ? 1 : 0;
    lp->norm_mode = norm_mode;
    lp->den = (float)(2.0 * (double)sigma * (double)sigma);
    lp->beta = beta;
    lp->hw = (double)HW;
    lp->inv_n = 1.0 / (double)((long)lp->planes * HW);
    lp->heat = heat, lp->pts = pts, lp->dheat = dheat;
    lp->inv_dev = (double*)workspace;
    lp->part = lp->inv_dev + 1;
    return HKP_OK;
}

static void launch_count(const LossPlan& lp, hipStream_t st) {
    if (lp.mask)
        hipLaunchKernelGGL(planes_count_kernel<true>, dim3(1), dim3(256), 0, st, lp.planes, lp.m, lp.hw, lp.ignore,
                           lp.norm_mode, lp.pts, lp.weights, lp.info, lp.used, lp.inv_dev, lp.k, lp.mchunks, lp.cnt,
                           lp.npix);
    else
        hipLaunchKernelGGL(planes_count_kernel<false>, dim3(1), dim3(256), 0, st, lp.planes, lp.m, lp.hw, lp.ignore,
                           lp.norm_mode, lp.pts, lp.weights, lp.info, lp.used, lp.inv_dev, 0, 0, nullptr, nullptr);
}

// the one (kind x 16-byte path x mode) dispatch; inv_n_dev: where the pass reads its
// divisor (WALK_EX: null for the host's)
static void launch_walk(const LossPlan& lp, int mode, const double* inv_n_dev, hipStream_t st) {
#define HKP_WALK(EK, V4, MD, MK)                                                                                   \
    hipLaunchKernelGGL((heat_loss_walk_kernel<EK, V4, MD, MK>), dim3((unsigned)lp.nblocks), dim3(256), 0, st, lp.m,  \
                       lp.H, lp.W, lp.chunks, lp.den, lp.ignore, lp.beta, lp.inv_n, inv_n_dev, lp.heat, lp.pts,      \
                       lp.dheat, lp.part, lp.info, lp.used, lp.weights, lp.mask, lp.k)
#define HKP_WALK_M(EK, V4, MD)                             \
    if constexpr (MD != WALK_EX) {                         \
        if (lp.mask) HKP_WALK(EK, V4, MD, true);           \
        else HKP_WALK(EK, V4, MD, false);                  \
    } else HKP_WALK(EK, V4, MD, false)
#define HKP_WALK_V(EK, MD) \
    if (lp.vec4) { HKP_WALK_M(EK, true, MD); } else { HKP_WALK_M(EK, false, MD); }
#define HKP_WALK_K(MD)                                \
    switch (lp.ek) {                                  \
        case EK_BCE: HKP_WALK_V(EK_BCE, MD); break;   \
        case EK_MSE: HKP_WALK_V(EK_MSE, MD); break;   \
        case EK_QFL2: HKP_WALK_V(EK_QFL2, MD); break; \
        default: HKP_WALK_V(EK_QFLG, MD); break;      \
    }
    switch (mode) {
        case WALK_EX: HKP_WALK_K(WALK_EX) break;
        case PL_ALL: HKP_WALK_K(PL_ALL) break;
        case PL_SUMS: HKP_WALK_K(PL_SUMS) break;
        default: HKP_WALK_K(PL_GRAD) break;
    }
#undef HKP_WALK_K
#undef HKP_WALK_V
#undef HKP_WALK_M
#undef HKP_WALK
}

// hkp_heat_loss_multi_ex, and hkp_heat_loss_multi as its BCE / MSE, HKP_NORM_ELEMENTS case
static int heat_loss_multi_run(const char* who, bool qfl_ok, int32_t n, int32_t k, int32_t m, int32_t H, int32_t W,
                               int32_t loss_kind, int32_t absent_mode, int32_t norm_mode, float beta,
                               const float* heat, const float* pts, float sigma, double* loss, float* dheat,
                               void* workspace, hkp_stream_t stream) {
    LossPlan lp;
    const int rc = loss_plan(who, qfl_ok, n, k, m, H, W, loss_kind, absent_mode, norm_mode, beta, heat, pts, sigma, loss,
                             dheat, workspace, &lp);
    if (rc != HKP_OK) return rc;
    hipStream_t st = as_stream(stream);
    // the divisor comes from the device unless it is the plain n*k*H*W
    const double* inv_dev = (lp.ignore || norm_mode == HKP_NORM_INSTANCES) ? lp.inv_dev : nullptr;
    if (inv_dev) {
        launch_count(lp, st);
        HKP_LAUNCH_CHECK((std::string(who) + "(active)").c_str());
    }
    launch_walk(lp, WALK_EX, inv_dev, st);
    HKP_LAUNCH_CHECK(who);
    hipLaunchKernelGGL(loss_multi_finalize_kernel, dim3(1), dim3(256), 0, st, lp.nblocks, lp.inv_n, inv_dev, lp.part,
                       loss);
    HKP_LAUNCH_CHECK((std::string(who) + "(finalize)").c_str());
    return HKP_OK;
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

// one double for the device's divisor, then a partial per block (at most MULTI_CHUNKS a plane)
extern "C" int64_t hkp_heat_loss_multi_workspace(int32_t n, int32_t k, int32_t H, int32_t W) {
    if (n <= 0 || k <= 0 || H <= 0 || W <= 0) return -1;
    return (int64_t)(1 + (int64_t)n * k * MULTI_CHUNKS) * (int64_t)sizeof(double);
}

extern "C" int hkp_heat_loss_multi(int32_t n, int32_t k, int32_t m, int32_t H, int32_t W, int32_t loss_kind,
                                   int32_t absent_mode, const float* heat, const float* pts, float sigma,
                                   double* loss, float* dheat, void* workspace, hkp_stream_t stream) {
    return heat_loss_multi_run("hkp_heat_loss_multi", false, n, k, m, H, W, loss_kind, absent_mode, HKP_NORM_ELEMENTS,
                               2.f, heat, pts, sigma, loss, dheat, workspace, stream);
}

extern "C" int hkp_heat_loss_multi_ex(int32_t n, int32_t k, int32_t m, int32_t H, int32_t W, int32_t loss_kind,
                                      int32_t absent_mode, int32_t norm_mode, float beta, const float* heat,
                                      const float* pts, float sigma, double* loss, float* dheat, void* workspace,
                                      hkp_stream_t stream) {
    return heat_loss_multi_run("hkp_heat_loss_multi_ex", true, n, k, m, H, W, loss_kind, absent_mode, norm_mode, beta,
                               heat, pts, sigma, loss, dheat, workspace, stream);
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
    LossPlan lp;
    const int rc = loss_plan("hkp_heat_loss_planes", true, n, k, m, H, W, loss_kind, absent_mode, norm_mode, beta, heat,
                             pts, sigma, loss, dheat, workspace, &lp);
    if (rc != HKP_OK) return rc;
    HKP_CHECK_ARG(topk >= 0 && topk <= k && (topk == 0 || k <= 64),
                  "hkp_heat_loss_planes: topk %d outside 0..k (k = %d; at most 64 classes with top-k)", topk, k);
    double* S = lp.part + (long)lp.planes * MULTI_CHUNKS;
    lp.weights = weights;
    lp.info = (int*)(S + lp.planes);
    lp.used = lp.info + lp.planes;
    hipStream_t st = as_stream(stream);
    launch_count(lp, st);
    HKP_LAUNCH_CHECK("hkp_heat_loss_planes(prepare)");
    launch_walk(lp, topk == 0 ? PL_ALL : PL_SUMS, lp.inv_dev, st);
    HKP_LAUNCH_CHECK("hkp_heat_loss_planes");
    hipLaunchKernelGGL(planes_finish_kernel<false>, dim3(1), dim3(256), 0, st, lp.planes, k, lp.chunks, topk, lp.hw,
                       norm_mode, weights, lp.info, lp.used, lp.part, S, lp.inv_dev, loss, plane_loss, plane_used,
                       nullptr, nullptr);
    HKP_LAUNCH_CHECK("hkp_heat_loss_planes(finish)");
    if (topk > 0 && dheat != nullptr) {
        launch_walk(lp, PL_GRAD, lp.inv_dev, st);
        HKP_LAUNCH_CHECK("hkp_heat_loss_planes(dheat)");
    }
    return HKP_OK;
}

// the planes entry's workspace, then npix per plane and the count pass's partial counts
// [n][MULTI_CHUNKS][8] (int32)
extern "C" int64_t hkp_heat_loss_masked_workspace(int32_t n, int32_t k, int32_t H, int32_t W) {
    const int64_t base = hkp_heat_loss_planes_workspace(n, k, H, W);
    if (base < 0) return -1;
    const int64_t ints = (int64_t)n * k + (int64_t)n * MULTI_CHUNKS * 8;
    return base + (ints + 1) / 2 * (int64_t)sizeof(double);
}

extern "C" int hkp_heat_loss_masked(int32_t n, int32_t k, int32_t m, int32_t H, int32_t W, int32_t loss_kind,
                                    int32_t absent_mode, int32_t norm_mode, float beta, int32_t topk,
                                    const float* heat, const float* pts, const float* weights, const uint8_t* mask,
                                    float sigma, double* loss, float* dheat, double* plane_loss, int32_t* plane_used,
                                    int32_t* plane_pixels, void* workspace, hkp_stream_t stream) {
    HKP_CHECK_ARG(mask != nullptr, "hkp_heat_loss_masked: null mask (hkp_heat_loss_planes is the entry without one)");
    HKP_CHECK_ARG(k <= MASK_MAX_K, "hkp_heat_loss_masked: k = %d classes, a mask byte holds %d", k, MASK_MAX_K);
    LossPlan lp;
    const int rc = loss_plan("hkp_heat_loss_masked", true, n, k, m, H, W, loss_kind, absent_mode, norm_mode, beta, heat,
                             pts, sigma, loss, dheat, workspace, &lp);
    if (rc != HKP_OK) return rc;
    HKP_CHECK_ARG(topk >= 0 && topk <= k, "hkp_heat_loss_masked: topk %d outside 0..k (k = %d)", topk, k);
    double* S = lp.part + (long)lp.planes * MULTI_CHUNKS;
    lp.weights = weights;
    lp.info = (int*)(S + lp.planes);
    lp.used = lp.info + lp.planes;
    // (past the planes entry's workspace, which ends on a multiple of 8 bytes)
    lp.npix = (int*)((char*)workspace + hkp_heat_loss_planes_workspace(n, k, H, W));
    lp.cnt = lp.npix + lp.planes;
    lp.mask = mask, lp.k = k;
    const int HW = H * W;
    lp.mchunks = multi_chunks(((long)HW + 3) / 4);
    hipStream_t st = as_stream(stream);
    if (HW % 4 == 0 && ((uintptr_t)mask & 3) == 0)
        hipLaunchKernelGGL(mask_count_kernel<true>, dim3((unsigned)(n * lp.mchunks)), dim3(256), 0, st, HW, lp.mchunks,
                           mask, lp.cnt);
    else
        hipLaunchKernelGGL(mask_count_kernel<false>, dim3((unsigned)(n * lp.mchunks)), dim3(256), 0, st, HW, lp.mchunks,
                           mask, lp.cnt);
    HKP_LAUNCH_CHECK("hkp_heat_loss_masked(count)");
    launch_count(lp, st);
    HKP_LAUNCH_CHECK("hkp_heat_loss_masked(prepare)");
    launch_walk(lp, topk == 0 ? PL_ALL : PL_SUMS, lp.inv_dev, st);
    HKP_LAUNCH_CHECK("hkp_heat_loss_masked");
    hipLaunchKernelGGL(planes_finish_kernel<true>, dim3(1), dim3(256), 0, st, lp.planes, k, lp.chunks, topk, lp.hw,
                       norm_mode, weights, lp.info, lp.used, lp.part, S, lp.inv_dev, loss, plane_loss, plane_used,
                       lp.npix, plane_pixels);
    HKP_LAUNCH_CHECK("hkp_heat_loss_masked(finish)");
    if (topk > 0 && dheat != nullptr) {
        launch_walk(lp, PL_GRAD, lp.inv_dev, st);
        HKP_LAUNCH_CHECK("hkp_heat_loss_masked(dheat)");
    }
    return HKP_OK;
}

// the masked entry's workspace, whatever mask is given: the planes entry's, then npix per
// plane and the count pass's partial counts
extern "C" int64_t hkp_heat_loss_lines_workspace(int32_t n, int32_t k, int32_t H, int32_t W) {
    return hkp_heat_loss_masked_workspace(n, k, H, W);
}

extern "C" int hkp_heat_loss_lines(int32_t n, int32_t k, int32_t s, int32_t H, int32_t W, int32_t loss_kind,
                                   int32_t absent_mode, int32_t norm_mode, float beta, int32_t topk, const float* heat,
                                   const float* lines, const float* weights, const uint8_t* mask, float sigma,
                                   double* loss, float* dheat, double* plane_loss, int32_t* plane_used,
                                   int32_t* plane_pixels, void* workspace, hkp_stream_t stream) {
    const char* who = "hkp_heat_loss_lines";
    HKP_CHECK_ARG(n >= 1 && k >= 1 && H >= 1 && W >= 1 && (long)H * W <= (1L << 30) &&
                      (long)n * k * MULTI_CHUNKS <= (1L << 30),
                  "%s: bad sizes (n, k, H, W >= 1, H*W <= 2^30)", who);
    HKP_CHECK_ARG(s >= 1 && s <= HKP_LINE_MAX_S, "%s: s = %d outside 1..%d", who, s, HKP_LINE_MAX_S);
    HKP_CHECK_ARG(sigma > 0.f && sigma < INFINITY, "%s: sigma must be finite and > 0", who);
    HKP_CHECK_ARG(heat && lines && loss && workspace, "%s: null tensor", who);
    HKP_CHECK_ARG(loss_kind == HKP_LOSS_BCE || loss_kind == HKP_LOSS_MSE || loss_kind == HKP_LOSS_QFL,
                  "%s: bad loss kind", who);
    HKP_CHECK_ARG(absent_mode == HKP_ABSENT_ZERO || absent_mode == HKP_ABSENT_IGNORE, "%s: bad absent mode", who);
    HKP_CHECK_ARG(norm_mode == HKP_NORM_ELEMENTS || norm_mode == HKP_NORM_INSTANCES, "%s: bad norm mode", who);
    // NaN fails both comparisons
    HKP_CHECK_ARG(loss_kind != HKP_LOSS_QFL || (beta >= 1.f && beta <= 8.f), "%s: beta %g outside [1, 8]", who,
                  (double)beta);
    HKP_CHECK_ARG(topk >= 0 && topk <= k && (topk == 0 || k <= 64),
                  "%s: topk %d outside 0..k (k = %d; at most 64 classes with top-k)", who, topk, k);
    HKP_CHECK_ARG(mask == nullptr || k <= MASK_MAX_K, "%s: k = %d classes, a mask byte holds %d", who, k, MASK_MAX_K);
    const int planes = n * k, HW = H * W;
    const int tiles_x = cdiv(W, LINE_TW), tiles = tiles_x * cdiv(H, LINE_TH);
    const int chunks = line_chunks(tiles), nblocks = planes * chunks;
    const bool vec4 = W % 4 == 0 && ((uintptr_t)heat & 15) == 0 && ((uintptr_t)dheat & 15) == 0;
    const int mword = mask && W % 4 == 0 && ((uintptr_t)mask & 3) == 0;
    const int ek = loss_kind == HKP_LOSS_BCE ? EK_BCE : loss_kind == HKP_LOSS_MSE ? EK_MSE : beta == 2.f ? EK_QFL2 : EK_QFLG;
    const int ignore = absent_mode == HKP_ABSENT_IGNORE ? 1 : 0;
    const float den = (float)(2.0 * (double)sigma * (double)sigma);
    const double hw = (double)HW;
    // the masked entry's layout: inv, the partials, S; info, used; npix, the mask counts
    double* inv_dev = (double*)workspace;
    double* part = inv_dev + 1;
    double* S = part + (long)planes * MULTI_CHUNKS;
    int* info = (int*)(S + planes);
    int* used = info + planes;
    int* npix = (int*)((char*)workspace + hkp_heat_loss_planes_workspace(n, k, H, W));
    int* cnt = npix + planes;
    hipStream_t st = as_stream(stream);
    if (mask) {
        const int mchunks = multi_chunks(((long)HW + 3) / 4);
        if (HW % 4 == 0 && ((uintptr_t)mask & 3) == 0)
            hipLaunchKernelGGL(mask_count_kernel<true>, dim3((unsigned)(n * mchunks)), dim3(256), 0, st, HW, mchunks,
                               mask, cnt);
        else
            hipLaunchKernelGGL(mask_count_kernel<false>, dim3((unsigned)(n * mchunks)), dim3(256), 0, st, HW, mchunks,
                               mask, cnt);
        HKP_LAUNCH_CHECK("hkp_heat_loss_lines(count)");
        hipLaunchKernelGGL((planes_count_kernel<true, 5, 4>), dim3(1), dim3(256), 0, st, planes, s, hw, ignore, norm_mode,
                           lines, weights, info, used, inv_dev, k, mchunks, cnt, npix);
    } else {
        hipLaunchKernelGGL((planes_count_kernel<false, 5, 4>), dim3(1), dim3(256), 0, st, planes, s, hw, ignore, norm_mode,
                           lines, weights, info, used, inv_dev, 0, 0, nullptr, nullptr);
    }
    HKP_LAUNCH_CHECK("hkp_heat_loss_lines(prepare)");
    // the one (kind x 16-byte path x mode x masked) dispatch of the line walk
    auto walk = [&](int mode) {
#define HKP_LWALK(EK, V4, MD, MK)                                                                                   \
    hipLaunchKernelGGL((line_loss_walk_kernel<EK, V4, MD, MK>), dim3((unsigned)nblocks), dim3(256), 0, st, s, H, W,  \
                       tiles_x, tiles, chunks, den, beta, mword, inv_dev, heat, lines, dheat, part, info, used,      \
                       weights, mask, k)
#define HKP_LWALK_M(EK, V4, MD)            \
    if (mask) HKP_LWALK(EK, V4, MD, true); \
    else HKP_LWALK(EK, V4, MD, false)
#define HKP_LWALK_V(EK, MD) \
    if (vec4) { HKP_LWALK_M(EK, true, MD); } else { HKP_LWALK_M(EK, false, MD); }
#define HKP_LWALK_K(MD)                                \
    switch (ek) {                                      \
        case EK_BCE: HKP_LWALK_V(EK_BCE, MD); break;   \
        case EK_MSE: HKP_LWALK_V(EK_MSE, MD); break;   \
        case EK_QFL2: HKP_LWALK_V(EK_QFL2, MD); break; \
        default: HKP_LWALK_V(EK_QFLG, MD); break;      \
    }
        switch (mode) {
            case PL_ALL: HKP_LWALK_K(PL_ALL) break;
            case PL_SUMS: HKP_LWALK_K(PL_SUMS) break;
            default: HKP_LWALK_K(PL_GRAD) break;
        }
#undef HKP_LWALK_K
#undef HKP_LWALK_V
#undef HKP_LWALK_M
#undef HKP_LWALK
    };
    walk(topk == 0 ? PL_ALL : PL_SUMS);
    HKP_LAUNCH_CHECK("hkp_heat_loss_lines");
    if (mask)
        hipLaunchKernelGGL(planes_finish_kernel<true>, dim3(1), dim3(256), 0, st, planes, k, chunks, topk, hw, norm_mode,
                           weights, info, used, part, S, inv_dev, loss, plane_loss, plane_used, npix, plane_pixels);
    else
        hipLaunchKernelGGL(planes_finish_kernel<false>, dim3(1), dim3(256), 0, st, planes, k, chunks, topk, hw,
                           norm_mode, weights, info, used, part, S, inv_dev, loss, plane_loss, plane_used, nullptr,
                           nullptr);
    HKP_LAUNCH_CHECK("hkp_heat_loss_lines(finish)");
    if (topk > 0 && dheat != nullptr) {
        walk(PL_GRAD);
        HKP_LAUNCH_CHECK("hkp_heat_loss_lines(dheat)");
    }
    return HKP_OK;
}
