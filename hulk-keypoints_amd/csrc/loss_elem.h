// What the heatmap losses share (loss.hip, loss_multi.hip): the per-element formulas
// and the block sum.  Every clamp and constant of the losses is here and nowhere else.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace hkp {

// BCE and MSE carry the values of HKP_LOSS_BCE / HKP_LOSS_MSE.  HKP_LOSS_QFL is one of
// two: QFL2 for beta == 2 (d*d, no pow), QFLG for any beta in [1, 8] (bm1 = beta - 1).
constexpr int EK_BCE = 0, EK_MSE = 1, EK_QFL2 = 2, EK_QFLG = 3;
static_assert(EK_BCE == HKP_LOSS_BCE && EK_MSE == HKP_LOSS_MSE, "the kinds of loss_elem");

// One element's loss term (returned) and its fp64 gradient, already divided by N
// (inv_n = 1 / N); the caller scales the gradient, if it does, and casts it to fp32:
//   BCE  l = (y-1)*max(log1p(-x),-100) - y*max(log x,-100),  g = (x-y) / max((1-x)*x, EPS) / N
//   MSE  l = (x-y)^2,  g = 2 (x-y) / N
//   QFL  l = |x-y|^beta * BCE: the float64 autograd of binary_cross_entropy(x, y, 'none')
//        * |x - y|^beta with ATen's clamps
// EPS is ATen's binary_cross_entropy_backward constant, a float widened to double
// (loss.hip's header).  beta and bm1 are read by QFLG alone.
template <int EK>
__device__ __forceinline__ double loss_elem(double x, double y, double inv_n, double beta, double bm1,
                                            double* g_out) {
    if constexpr (EK == EK_MSE) {
        *g_out = 2.0 * inv_n * (x - y);
        return (x - y) * (x - y);
    } else {
        const double bce = (y - 1.0) * fmax(log1p(-x), -100.0) - y * fmax(log(x), -100.0);
        const double d = x - y;
        const double den = fmax((1.0 - x) * x, (double)1e-12f);
        if constexpr (EK == EK_BCE) {
            *g_out = d / den * inv_n;
            return bce;
        } else {
            double l, g;
            if constexpr (EK == EK_QFL2) {
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
            // x == y: the minimum, exactly (0^0 at beta = 1, the clamped logs at 0 and 1)
            if (d == 0.0) {
                l = 0.0;
                g = 0.0;
            }
            *g_out = g;
            return l;
        }
    }
}

// the block's values through the wave butterfly, then the waves in index order; the
// result is valid in thread 0 (red: one double per wave)
__device__ __forceinline__ double block_sum_d(double v, double* red) {
    v = wave_sum_d(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) red[wid] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
    return t;
}

}  // namespace hkp
