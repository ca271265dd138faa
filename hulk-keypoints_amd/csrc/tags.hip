// Associative-embedding tags (include/hulkkp.h has the definitions): one scalar tag
// map per keypoint class on the stride-8 lattice, the tag planes read in place from
// the head's [n][2k][h][w] output (a base pointer and a batch stride).
//
//  * hkp_tag_loss     the pull / push loss of Newell et al. (2017) on the tags
//                     sampled at the labelled points, and its closed-form gradient
//                     on the lattice.  One 256-thread block per (image, plane): the
//                     block samples the image's <= 128 points in fp64, forms the
//                     <= 32 group means (8 lanes per group, a fixed shuffle order),
//                     the 32 x 32 push terms (4 per thread) and every point's
//                     gradient coefficient in LDS, then gathers its own plane: each
//                     node loops over the plane's m slots and adds the taps that
//                     fall on it, so dtag is written whole, without atomics and
//                     without a memset.  The plane-0 block of an image leaves the
//                     image's (pull, push) in the workspace; a one-wave launch sums
//                     them over the batch in a fixed order.
//  * hkp_peaks_group  greedy grouping of the peaks of hkp_heat_peaks by tag: one
//                     wavefront per image, the sampled tags in LDS, the state of
//                     group g (fp64 sum, count, mean, last class) in the registers
//                     of lane g % 64 (two groups per lane: at most 8 x 16 groups),
//                     the nearest open group found by a wave minimum with the tie
//                     going to the lower id.
//
// Per-lane state is scalars only (no indexed arrays: no scratch).  Every tap index
// comes from a coordinate clamped to the lattice first (a NaN goes to 0), so no
// address leaves the plane.
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace hkp {

constexpr int TAG_MAX_K = 8;
constexpr int TAG_MAX_M = 16;                      // label slots / peak slots per plane
constexpr int TAG_MAX_PTS = TAG_MAX_K * TAG_MAX_M;
constexpr int TAG_MAX_GROUPS = 32;                 // label group ids
constexpr int TAG_MAX_DIM = 32767;                 // h, w (a tap's (y0, x0) packs into one int)
constexpr int TAG_NO_TAP = 0x7FFF7FFF;             // (32767, 32767): no node is at or right below it

// the lattice frame of hkp_heat_peaks along one axis: pixel u of a W-wide picture on a
// w-node lattice -> first tap x0 and its fraction fx; the second tap is min(x0 + 1, w - 1)
__device__ __forceinline__ void lattice_tap(float u, int w, int W, int* x0, double* fx) {
    double x = (W > 1 && w > 1) ? (double)u * (double)(w - 1) / (double)(W - 1) : 0.0;
    const double hi = (double)(w - 1);
    x = x > 0.0 ? x : 0.0;                         // NaN -> 0
    x = x < hi ? x : hi;
    const int f = w > 1 ? min((int)floor(x), w - 2) : 0;
    *x0 = f;
    *fx = x - (double)f;
}

// fp64 bilinear value of an fp32 plane
__device__ __forceinline__ double lattice_sample(const float* __restrict__ plane, int h, int w, int x0, int y0,
                                                 double fx, double fy) {
    const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
    const double t00 = (double)plane[(long)y0 * w + x0], t01 = (double)plane[(long)y0 * w + x1];
    const double t10 = (double)plane[(long)y1 * w + x0], t11 = (double)plane[(long)y1 * w + x1];
    const double top = (1.0 - fx) * t00 + fx * t01;
    const double bot = (1.0 - fx) * t10 + fx * t11;
    return (1.0 - fy) * top + fy * bot;
}

// sum over the 8 consecutive lanes of a group; every lane ends with the same bits
__device__ __forceinline__ double lanes8_sum_d(double v) {
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(256) void tag_loss_kernel(int K, int M, int h, int w, int H, int W, long bstride,
                                                      int planes, double cscale, double pull_w, double push_w,
                                                      const float* __restrict__ tags, const float* __restrict__ pts,
                                                      const int32_t* __restrict__ gid, float* __restrict__ dtag,
                                                      double* __restrict__ ws) {
    __shared__ double s_t[TAG_MAX_PTS], s_fx[TAG_MAX_PTS], s_fy[TAG_MAX_PTS], s_coef[TAG_MAX_PTS];
    __shared__ int s_g[TAG_MAX_PTS], s_xy[TAG_MAX_PTS];
    __shared__ double s_mu[TAG_MAX_GROUPS], s_dmu[TAG_MAX_GROUPS], s_ps[TAG_MAX_GROUPS];
    __shared__ int s_n[TAG_MAX_GROUPS];
    __shared__ double s_red[2];

    const int tid = threadIdx.x;
    const int b = blockIdx.x / planes, c = blockIdx.x - b * planes;
    const int KM = K * M;                                       // <= TAG_MAX_PTS (host-checked)
    const long hw = (long)h * w;
    const float* timg = tags + (long)b * bstride;

    // 1. the image's points: thread i samples point i = class * M + slot
    if (tid < TAG_MAX_PTS) {
        int g = -1, xy = TAG_NO_TAP;
        double t = 0.0, fx = 0.0, fy = 0.0;
        if (tid < KM) {
            const long rec = (long)b * KM + tid;
            const int gg = gid[rec];
            if (pts[rec * 3 + 2] > 0.f && gg >= 0 && gg < TAG_MAX_GROUPS) {
                int x0, y0;
                lattice_tap(pts[rec * 3 + 0], w, W, &x0, &fx);
                lattice_tap(pts[rec * 3 + 1], h, H, &y0, &fy);
                t = lattice_sample(timg + (long)(tid / M) * hw, h, w, x0, y0, fx, fy);
                g = gg;
                xy = (y0 << 16) | x0;
            }
        }
        s_g[tid] = g;
        s_xy[tid] = xy;
        s_t[tid] = t;
        s_fx[tid] = fx;
        s_fy[tid] = fy;
    }
    __syncthreads();

    // 2. group g = tid / 8: its members' sum and count, 8 lanes taking every 8th point
    const int g8 = tid >> 3, l8 = tid & 7;
    {
        double s = 0.0;
        int cn = 0;
        for (int i = l8; i < KM; i += 8) {
            const bool in = s_g[i] == g8;
            s += in ? s_t[i] : 0.0;
            cn += in ? 1 : 0;
        }
        s = lanes8_sum_d(s);
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) cn += __shfl_xor(cn, o);
        if (l8 == 0) {
            s_n[g8] = cn;
            s_mu[g8] = cn > 0 ? s / (double)cn : 0.0;
        }
    }
    __syncthreads();

    // 3. the push terms of group g8 against the 4 groups l8, l8 + 8, ...
    int G = 0;
    for (int q = 0; q < TAG_MAX_GROUPS; ++q) G += s_n[q] > 0 ? 1 : 0;
    const double pairs = (double)G * (double)(G - 1);
    {
        double ps = 0.0, dm = 0.0;
        const bool mine = s_n[g8] > 0;
        const double mu = s_mu[g8];
#pragma unroll
        for (int j = 0; j < TAG_MAX_GROUPS / 8; ++j) {
            const int g2 = l8 + 8 * j;
            if (mine && g2 != g8 && s_n[g2] > 0) {
                const double d = mu - s_mu[g2];
                const double e = exp(-(d * d) * 0.5);
                ps += e;
                dm += d * e;
            }
        }
        ps = lanes8_sum_d(ps);
        dm = lanes8_sum_d(dm);
        if (l8 == 0) {
            s_ps[g8] = ps;
            s_dmu[g8] = G >= 2 ? -(2.0 / pairs) * dm : 0.0;      // d push_b / d mu_g
        }
    }
    __syncthreads();

    // 4. every point's share of the pull and its gradient coefficient
    double pl = 0.0;
    if (tid < TAG_MAX_PTS) {
        const int g = s_g[tid];
        double coef = 0.0;
        if (g >= 0) {
            const double ng = (double)s_n[g];
            const double dev = s_t[tid] - s_mu[g];
            pl = dev * dev / ng;
            coef = cscale * (pull_w * (2.0 * dev / ((double)G * ng)) + push_w * (s_dmu[g] / ng));
        }
        s_coef[tid] = coef;
    }
    if (tid < TAG_MAX_PTS) {                                    // waves 0 and 1, whole
        pl = wave_sum_d(pl);
        if ((tid & 63) == 0) s_red[tid >> 6] = pl;
    }
    __syncthreads();
    if (c == 0 && tid == 0) {                                   // the image's two values, once
        double push = 0.0;
        for (int q = 0; q < TAG_MAX_GROUPS; ++q) push += s_n[q] > 0 ? s_ps[q] : 0.0;
        ws[2 * (long)b + 0] = G > 0 ? (s_red[0] + s_red[1]) / (double)G : 0.0;
        ws[2 * (long)b + 1] = G >= 2 ? push / pairs : 0.0;
    }
    if (dtag == nullptr) return;

    // 5. the plane's gradient, gathered: slot order, then the taps 00, 01, 10, 11
    float* out = dtag + ((long)b * K + c) * hw;
    const int base = c * M;
    for (long node = tid; node < hw; node += 256) {
        const int yy = (int)(node / w), xx = (int)(node - (long)yy * w);
        double acc = 0.0;
        for (int mi = 0; mi < M; ++mi) {
            const int xy = s_xy[base + mi];
            const int x0 = xy & 0xFFFF, y0 = xy >> 16;
            if ((unsigned)(xx - x0) <= 1u && (unsigned)(yy - y0) <= 1u) {
                const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
                const double fx = s_fx[base + mi], fy = s_fy[base + mi], cf = s_coef[base + mi];
                if (yy == y0 && xx == x0) acc += cf * ((1.0 - fy) * (1.0 - fx));
                if (yy == y0 && xx == x1) acc += cf * ((1.0 - fy) * fx);
                if (yy == y1 && xx == x0) acc += cf * (fy * (1.0 - fx));
                if (yy == y1 && xx == x1) acc += cf * (fy * fx);
            }
        }
        out[node] = (float)acc;
    }
}

// out[3] = (total, mean pull, mean push) over the batch: lane l sums images l, l + 64, ...
__global__ __launch_bounds__(64) void tag_loss_finalize_kernel(int n, double pull_w, double push_w,
                                                              const double* __restrict__ ws,
                                                              double* __restrict__ out) {
    double p = 0.0, q = 0.0, t = 0.0;
    for (int b = threadIdx.x; b < n; b += 64) {
        const double pl = ws[2 * (long)b], ps = ws[2 * (long)b + 1];
        p += pl;
        q += ps;
        t += pull_w * pl + push_w * ps;
    }
    p = wave_sum_d(p);
    q = wave_sum_d(q);
    t = wave_sum_d(t);
    if (threadIdx.x == 0) {
        out[0] = t / (double)n;
        out[1] = p / (double)n;
        out[2] = q / (double)n;
    }
}

struct group_order {
    int v[TAG_MAX_K];
};

constexpr int GROUP_NONE = 1 << 30;

__global__ __launch_bounds__(64) void peaks_group_kernel(int K, int P, int h, int w, int H, int W, int Q,
                                                        group_order ord, double max_dist, long bstride,
                                                        const float* __restrict__ peaks,
                                                        const int32_t* __restrict__ counts,
                                                        const float* __restrict__ tags, float* __restrict__ tag,
                                                        int32_t* __restrict__ group, int32_t* __restrict__ ngroups) {
    __shared__ float s_tag[TAG_MAX_PTS];
    __shared__ int s_grp[TAG_MAX_PTS];
    __shared__ int s_cnt[TAG_MAX_K], s_ord[TAG_MAX_K];
    const int lane = threadIdx.x;
    const long b = blockIdx.x;
    const int KP = K * P;                                       // <= TAG_MAX_PTS (host-checked)
    const long hw = (long)h * w;
#pragma unroll
    for (int q = 0; q < TAG_MAX_K; ++q)
        if (lane == q) s_ord[q] = ord.v[q];
    if (lane < K) {
        const int cnt = counts[b * K + lane];
        s_cnt[lane] = cnt < 0 ? 0 : (cnt > P ? P : cnt);
    }
    __syncthreads();

    // the tag of every used peak slot, of every class
    for (int e = lane; e < KP; e += 64) {
        const int c = e / P, j = e - c * P;
        float tv = 0.f;
        if (j < s_cnt[c]) {
            const float* pk = peaks + (b * KP + e) * 3;
            int x0, y0;
            double fx, fy;
            lattice_tap(pk[0], w, W, &x0, &fx);
            lattice_tap(pk[1], h, H, &y0, &fy);
            tv = (float)lattice_sample(tags + b * bstride + (long)c * hw, h, w, x0, y0, fx, fy);
        }
        s_tag[e] = tv;
        s_grp[e] = -1;
        tag[b * KP + e] = tv;
    }
    __syncthreads();

    // greedy: lane l holds groups l and l + 64
    int ng = 0;
    double sum0 = 0.0, sum1 = 0.0, mean0 = 0.0, mean1 = 0.0;
    int n0 = 0, n1 = 0, last0 = -1, last1 = -1;                 // last: the order index of the newest member
    for (int qi = 0; qi < Q; ++qi) {
        const int c = min(max(s_ord[qi], 0), K - 1);            // (host-checked; clamped where it indexes)
        const int cnt = s_cnt[c];
        for (int j = 0; j < cnt; ++j) {
            const double t = (double)s_tag[c * P + j];
            const double d0 = fabs(t - mean0), d1 = fabs(t - mean1);
            const bool e0 = lane < ng && last0 != qi && d0 <= max_dist;          // a NaN is never eligible
            const bool e1 = lane + 64 < ng && last1 != qi && d1 <= max_dist;
            double bd = (double)INFINITY;
            int bi = GROUP_NONE;
            if (e0) {
                bd = d0;
                bi = lane;
            }
            if (e1 && d1 < bd) {
                bd = d1;
                bi = lane + 64;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double od = __shfl_xor(bd, o);
                const int oi = __shfl_xor(bi, o);
                const bool better = od < bd || (od == bd && oi < bi);
                bd = better ? od : bd;
                bi = better ? oi : bi;
            }
            const bool opens = bi == GROUP_NONE;                // wave-uniform
            const int id = opens ? ng : bi;
            if (lane == (id & 63)) {
                if (id < 64) {
                    sum0 = opens ? t : sum0 + t;
                    n0 = opens ? 1 : n0 + 1;
                    mean0 = sum0 / (double)n0;
                    last0 = qi;
                } else {
                    sum1 = opens ? t : sum1 + t;
                    n1 = opens ? 1 : n1 + 1;
                    mean1 = sum1 / (double)n1;
                    last1 = qi;
                }
            }
            if (lane == 0) s_grp[c * P + j] = id;
            ng += opens ? 1 : 0;
        }
    }
    __syncthreads();
    for (int e = lane; e < KP; e += 64) group[b * KP + e] = s_grp[e];
    if (lane == 0) ngroups[b] = ng;
}

}  // namespace hkp

using namespace hkp;

static bool tag_weight_ok(float v) { return isfinite(v) && v >= 0.f; }

extern "C" int64_t hkp_tag_loss_workspace(int32_t n) { return n > 0 ? (int64_t)n * 2 * (int64_t)sizeof(double) : 0; }

extern "C" int hkp_tag_loss(int32_t n, int32_t k, int32_t m, int32_t h, int32_t w, int32_t H, int32_t W,
                            const float* tags, int64_t batch_stride, const float* pts, const int32_t* gid,
                            float scale, float pull_w, float push_w, double* out, float* dtag, void* workspace,
                            hkp_stream_t stream) {
    HKP_CHECK_ARG(n >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "hkp_tag_loss: bad sizes (n=%d h=%d w=%d H=%d W=%d)", n,
                  h, w, H, W);
    HKP_CHECK_ARG(k >= 1 && 2 * k <= 16, "hkp_tag_loss: tags are head rows k..2k-1 of at most 16: need 1 <= k <= %d "
                  "(got %d)", TAG_MAX_K, k);
    HKP_CHECK_ARG(m >= 1 && m <= TAG_MAX_M, "hkp_tag_loss: need 1 <= m <= %d (got %d)", TAG_MAX_M, m);
    HKP_CHECK_ARG(h <= TAG_MAX_DIM && w <= TAG_MAX_DIM, "hkp_tag_loss: lattice %d x %d exceeds %d nodes a side", h, w,
                  TAG_MAX_DIM);
    HKP_CHECK_ARG(tags && pts && gid && out && workspace, "hkp_tag_loss: null tensor");
    HKP_CHECK_ARG(batch_stride >= (int64_t)k * h * w, "hkp_tag_loss: batch stride %lld is less than k*h*w",
                  (long long)batch_stride);
    HKP_CHECK_ARG(tag_weight_ok(scale) && tag_weight_ok(pull_w) && tag_weight_ok(push_w),
                  "hkp_tag_loss: scale, pull and push must be finite and >= 0 (got %g, %g, %g)", (double)scale,
                  (double)pull_w, (double)push_w);
    HKP_CHECK_ARG((long)n * k <= 0x7FFFFFFFL, "hkp_tag_loss: too many planes");
    const int planes = dtag ? k : 1;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(tag_loss_kernel, dim3((unsigned)((long)n * planes)), dim3(256), 0, st, k, m, h, w, H, W,
                       (long)batch_stride, planes, (double)scale / (double)n, (double)pull_w, (double)push_w, tags, pts,
                       gid, dtag, (double*)workspace);
    HKP_LAUNCH_CHECK("hkp_tag_loss");
    hipLaunchKernelGGL(tag_loss_finalize_kernel, dim3(1), dim3(64), 0, st, n, (double)pull_w, (double)push_w,
                       (const double*)workspace, out);
    HKP_LAUNCH_CHECK("hkp_tag_loss(finalize)");
    return HKP_OK;
}

extern "C" int hkp_peaks_group(int32_t n, int32_t k, int32_t p, int32_t h, int32_t w, int32_t H, int32_t W, int32_t q,
                               const int32_t* order_host, float max_dist, const float* peaks, const int32_t* counts,
                               const float* tags, int64_t batch_stride, float* tag, int32_t* group, int32_t* ngroups,
                               hkp_stream_t stream) {
    HKP_CHECK_ARG(n >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "hkp_peaks_group: bad sizes (n=%d h=%d w=%d H=%d W=%d)",
                  n, h, w, H, W);
    HKP_CHECK_ARG(k >= 1 && 2 * k <= 16, "hkp_peaks_group: tags are head rows k..2k-1 of at most 16: need 1 <= k <= %d "
                  "(got %d)", TAG_MAX_K, k);
    HKP_CHECK_ARG(p >= 1 && p <= TAG_MAX_M, "hkp_peaks_group: need 1 <= p <= %d (got %d)", TAG_MAX_M, p);
    HKP_CHECK_ARG(h <= TAG_MAX_DIM && w <= TAG_MAX_DIM, "hkp_peaks_group: lattice %d x %d exceeds %d nodes a side", h, w,
                  TAG_MAX_DIM);
    HKP_CHECK_ARG(q >= 1 && q <= k, "hkp_peaks_group: need 1 <= q <= k classes in order (got %d, k=%d)", q, k);
    HKP_CHECK_ARG(order_host && peaks && counts && tags && tag && group && ngroups, "hkp_peaks_group: null tensor");
    HKP_CHECK_ARG(batch_stride >= (int64_t)k * h * w, "hkp_peaks_group: batch stride %lld is less than k*h*w",
                  (long long)batch_stride);
    HKP_CHECK_ARG(isfinite(max_dist) && max_dist > 0.f, "hkp_peaks_group: max_dist must be finite and > 0 (got %g)",
                  (double)max_dist);
    group_order ord;
    for (int i = 0; i < TAG_MAX_K; ++i) ord.v[i] = 0;
    unsigned seen = 0u;
    for (int i = 0; i < q; ++i) {
        const int c = order_host[i];
        HKP_CHECK_ARG(c >= 0 && c < k, "hkp_peaks_group: order[%d] = %d is no class of 0..%d", i, c, k - 1);
        HKP_CHECK_ARG(!((seen >> c) & 1u), "hkp_peaks_group: class %d is in order twice", c);
        seen |= 1u << c;
        ord.v[i] = c;
    }
    hipLaunchKernelGGL(peaks_group_kernel, dim3((unsigned)n), dim3(64), 0, as_stream(stream), k, p, h, w, H, W, q, ord,
                       (double)max_dist, (long)batch_stride, peaks, counts, tags, tag, group, ngroups);
    HKP_LAUNCH_CHECK("hkp_peaks_group");
    return HKP_OK;
}
