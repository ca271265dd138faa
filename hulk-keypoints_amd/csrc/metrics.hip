// Keypoint evaluation on the device (include/hulkkp.h has the definition).
//
//  * hkp_peaks_match  the decoded peaks of hkp_heat_peaks against the instance
//                    labels of hkp_heat_loss_multi: COCO's greedy matching per plane
//                    at up to 8 distance thresholds at once, added into int64
//                    accumulators (score histograms of true / false positives and
//                    per-class totals) that stay on the device for a whole pass.
//
// One launch, one wavefront per plane, four planes of ONE class per block.  The
// 16 x 16 table of squared distances (fp64) lies in LDS; the selection runs on
// lane = (threshold % 4) * 16 + label slot, so four thresholds advance together
// and a round's minimum is four xor-shuffles inside a 16-lane group.  Everything
// accumulated is an integer, so the order of the atomic adds cannot show: the
// histogram takes one 64-bit add per peak and threshold (its bins are sparse);
// the totals are summed over the block's waves in LDS and take seven adds per
// block.  Per-lane state is scalars only (no indexed arrays: no scratch).
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace hkp {

constexpr int MATCH_MAX = 16;      // peak slots and label slots per plane
constexpr int MATCH_MAX_T = 8;     // thresholds
constexpr int MATCH_MAX_BINS = 4096;
constexpr int MATCH_WAVES = 4;     // planes per block

struct match_thresholds {
    float v[MATCH_MAX_T];
};

__device__ __forceinline__ int score_bin(float s, int bins) {
    if (s >= 1.f) return bins - 1;
    if (!(s > 0.f)) return 0;      // <= 0, -0 and NaN
    const int b = (int)(s * (float)bins);
    return b < bins - 1 ? b : bins - 1;
}

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(MATCH_WAVES * 64) void peaks_match_kernel(
    int n, int k, int p, int m, int t, int bins, int chunks, match_thresholds th, const float* __restrict__ peaks,
    const int32_t* __restrict__ counts, const float* __restrict__ pts, unsigned long long* __restrict__ hist,
    unsigned long long* __restrict__ totals, int32_t* __restrict__ peak_match, int32_t* __restrict__ gt_match,
    float* __restrict__ gt_dist) {
    __shared__ double tab[MATCH_WAVES][MATCH_MAX * MATCH_MAX];   // d2[j][i], NaN where no pair
    __shared__ float spx[MATCH_WAVES][MATCH_MAX], spy[MATCH_WAVES][MATCH_MAX];
    __shared__ float slu[MATCH_WAVES][MATCH_MAX], slv[MATCH_WAVES][MATCH_MAX];
    __shared__ int sbin[MATCH_WAVES][MATCH_MAX];
    __shared__ int sres[MATCH_WAVES][MATCH_MAX_T * MATCH_MAX];    // label slot a peak took, -1: none
    __shared__ double stau2[MATCH_MAX_T];
    __shared__ long long stot[MATCH_WAVES][8];

    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int c = blockIdx.x / chunks;
    const int b = (blockIdx.x - c * chunks) * MATCH_WAVES + wid;
    const bool active = b < n;                        // wave-uniform
    const long plane = active ? (long)b * k + c : 0;

    if (threadIdx.x < MATCH_MAX_T) {
        float tv = 0.f;
#pragma unroll
        for (int q = 0; q < MATCH_MAX_T; ++q) tv = lane == q ? th.v[q] : tv;
        stau2[lane] = (double)tv * (double)tv;
    }

    // stage the plane: lane j < cnt holds peak j, lane i < m label slot i
    int cnt = 0;
    if (active) {
        cnt = counts[plane];
        cnt = cnt < 0 ? 0 : (cnt > p ? p : cnt);
    }
    cnt = __builtin_amdgcn_readfirstlane(cnt);
    if (lane < cnt) {
        const float* pk = peaks + (plane * p + lane) * 3;
        spx[wid][lane] = pk[0];
        spy[wid][lane] = pk[1];
        sbin[wid][lane] = score_bin(pk[2], bins);
    }
    bool on = false;
    if (active && lane < m) {
        const float* rec = pts + (plane * m + lane) * 3;
        on = rec[2] > 0.f;
        if (on) {
            slu[wid][lane] = rec[0];
            slv[wid][lane] = rec[1];
        }
    }
    const unsigned long long present = __ballot(on);
    __syncthreads();

#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int e = r * 64 + lane, j = e >> 4, i = e & 15;
        double d2 = __builtin_nan("");
        if (j < cnt && ((present >> i) & 1ull)) {
            const double dx = (double)spx[wid][j] - (double)slu[wid][i];
            const double dy = (double)spy[wid][j] - (double)slv[wid][i];
            d2 = dx * dx + dy * dy;
        }
        tab[wid][e] = d2;
    }
    __syncthreads();

    // greedy selection: group g = lane / 16 runs threshold t0 + g, lane % 16 is the label slot
    const int i = lane & 15, g = lane >> 4;
    const int loose = t - 1;
    int took_me = -1;          // at the loosest threshold: the peak slot that took instance i
    double took_d2 = 0.0;
    for (int t0 = 0; t0 < t; t0 += 4) {
        const int ti = t0 + g;
        const bool ton = ti < t;
        const double tau2 = ton ? stau2[ti] : -1.0;
        bool taken = false;
        for (int j = 0; j < cnt; ++j) {
            const double d = tab[wid][j * 16 + i];
            const bool el = !taken && d <= tau2;      // NaN (no pair, NaN coordinate) is never eligible
            double bd = el ? d : (double)INFINITY;
            int bi = el ? i : MATCH_MAX;
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) {
                const double od = __shfl_xor(bd, o);
                const int oi = __shfl_xor(bi, o);
                const bool better = od < bd || (od == bd && oi < bi);
                bd = better ? od : bd;
                bi = better ? oi : bi;
            }
            if (el && bi == i) {
                taken = true;
                if (ti == loose) {
                    took_me = j;
                    took_d2 = d;
                }
            }
            if (i == 0 && ton) sres[wid][ti * 16 + j] = bi < MATCH_MAX ? bi : -1;
        }
    }
    __syncthreads();

    // per peak and threshold: peak_match and one histogram add
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int e = r * 64 + lane, ti = e >> 4, j = e & 15;
        if (active && ti < t && j < p) {
            const int res = j < cnt ? sres[wid][e] : -2;
            if (peak_match) peak_match[(plane * t + ti) * p + j] = res;
            if (j < cnt) {
                const long slot = ((long)c * t + ti) * 2 + (res >= 0 ? 0 : 1);
                atomicAdd(hist + slot * bins + sbin[wid][j], 1ull);
            }
        }
    }

    // the loosest threshold's view of the labels, held by group loose % 4
    const bool mine = active && g == (loose & 3) && i < m;
    const bool here = mine && ((present >> i) & 1ull);
    const bool hit = here && took_me >= 0;
    long long q = 0;
    if (mine) {
        const float dist = hit ? (float)sqrt(took_d2) : -1.f;
        if (hit) q = (long long)floor((double)dist * 65536.0 + 0.5);
        if (gt_match) gt_match[plane * m + i] = here ? took_me : -2;
        if (gt_dist) gt_dist[plane * m + i] = dist;
    }
    const int n_present = __popcll(present);
    const int n_hit = __popcll(__ballot(hit));
    q = wave_sum_ll(q);
    if (lane < 8) {
        long long v = 0;
        v = lane == 0 ? (active ? 1 : 0) : v;
        v = lane == 1 ? (active && n_present == 0 ? 1 : 0) : v;
        v = lane == 2 ? n_present : v;
        v = lane == 3 ? cnt : v;
        v = lane == 4 ? n_hit : v;
        v = lane == 5 ? q : v;
        v = lane == 6 ? (n_present == 0 ? cnt : 0) : v;
        stot[wid][lane] = v;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        long long s = 0;
#pragma unroll
        for (int w = 0; w < MATCH_WAVES; ++w) s += stot[w][threadIdx.x];
        if (s != 0) atomicAdd(totals + (long)c * 8 + threadIdx.x, (unsigned long long)s);
    }
}

}  // namespace hkp

using namespace hkp;

extern "C" int hkp_peaks_match(int32_t n, int32_t k, int32_t p, int32_t m, int32_t t, int32_t bins,
                               const float* thresholds_host, const float* peaks, const int32_t* counts,
                               const float* pts, int64_t* hist, int64_t* totals, int32_t* peak_match,
                               int32_t* gt_match, float* gt_dist, hkp_stream_t stream) {
    HKP_CHECK_ARG(n >= 1 && k >= 1, "hkp_peaks_match: bad sizes (n=%d k=%d)", n, k);
    HKP_CHECK_ARG(p >= 1 && p <= MATCH_MAX && m >= 1 && m <= MATCH_MAX,
                  "hkp_peaks_match: need 1 <= p, m <= %d (got p=%d m=%d)", MATCH_MAX, p, m);
    HKP_CHECK_ARG(t >= 1 && t <= MATCH_MAX_T, "hkp_peaks_match: need 1 <= t <= %d thresholds (got %d)", MATCH_MAX_T,
                  t);
    HKP_CHECK_ARG(bins >= 1 && bins <= MATCH_MAX_BINS, "hkp_peaks_match: need 1 <= bins <= %d (got %d)",
                  MATCH_MAX_BINS, bins);
    HKP_CHECK_ARG(thresholds_host && peaks && counts && pts && hist && totals, "hkp_peaks_match: null tensor");
    match_thresholds th;
    for (int q = 0; q < MATCH_MAX_T; ++q) th.v[q] = 0.f;
    for (int q = 0; q < t; ++q) {
        const float v = thresholds_host[q];
        HKP_CHECK_ARG(isfinite(v) && v > 0.f && (q == 0 || v > thresholds_host[q - 1]),
                      "hkp_peaks_match: thresholds must be finite, > 0 and strictly ascending (threshold %d is %g)", q,
                      (double)v);
        th.v[q] = v;
    }
    const long chunks = ((long)n + MATCH_WAVES - 1) / MATCH_WAVES;
    HKP_CHECK_ARG((long)n * k <= 0x7FFFFFFFL && chunks * k <= 0x7FFFFFFFL, "hkp_peaks_match: too many planes");
    hipLaunchKernelGGL(peaks_match_kernel, dim3((unsigned)(chunks * k)), dim3(MATCH_WAVES * 64), 0, as_stream(stream),
                       n, k, p, m, t, bins, (int)chunks, th, peaks, counts, pts, (unsigned long long*)hist,
                       (unsigned long long*)totals, peak_match, gt_match, gt_dist);
    HKP_LAUNCH_CHECK("hkp_peaks_match");
    return HKP_OK;
}
