// Fused multi-tensor Adam (L2 weight decay) — SURVEY §8(f2): the optimizer step of
// train.py:36 (optim.Adam(lr=1e-4, weight_decay=1e-4), train.py:79) as one pass
// over every parameter: read p, g, m, v; write p, m, v (28 B per element, HBM-bound)
// in a handful of launches instead of torch's ~10 foreach kernels per tensor group.
//
// Per element, the operation sequence of torch.optim.Adam's multi-tensor path
// (torch/optim/adam.py _multi_tensor_adam, amsgrad=False, maximize=False):
//     g  = g + wd * p                      _foreach_add(grads, params, alpha=wd)
//     m  = m + (1 - b1) * (g - m)          _foreach_lerp_(exp_avgs, grads, 1 - b1)
//     v  = v * b2 + (1 - b2) * g * g       _foreach_mul_ / _foreach_addcmul_
//     d  = sqrt(v) / sqrt(bc2) + eps       _foreach_sqrt / _foreach_div_ / _foreach_add_
//     p  = p + (-lr / bc1) * m / d         _foreach_addcdiv_
// with 1 - b1, 1 - b2, bc1 = 1 - b1^step, bc2 = 1 - b2^step computed on the host
// in double (as torch does: its scalars are Python floats) and passed as fp32.
//
// Optional extras of the same pass (hkp_adam_step_ex), both off in hkp_adam_step:
//   * gradient clipping by the global L2 norm (torch/nn/utils/clip_grad.py,
//     clip_grad_norm_: _foreach_norm, stack, norm, _foreach_mul_(grads, coef)):
//     hkp_grad_norm leaves norm and coef = min(max_norm / (norm + 1e-6), 1) on the
//     device (fp64 sums in a fixed order, no atomics: the same bits on every run),
//     and the Adam pass reads g * coef instead of g (g itself is not written: 4 B
//     per element more for the norm's read, 32 B in all);
//   * an exponential moving average of the weights (torch/optim/swa_utils.py,
//     get_ema_multi_avg_fn: _foreach_lerp_(ema, params, 1 - decay)) updated from
//     the new p in the same read: e = e + (1 - decay) * (p - e), 8 B per element
//     more (40 B in all) instead of a separate 12 B pass.
#include "common.h"

namespace hkp {

constexpr int ADAM_MAXT = 48;
constexpr int ADAM_UNIT = 4096;   // elements per block (256 threads x 4 float4)

struct AdamT {
    float* p;
    const float* g;
    float* m;
    float* v;
    long n;
};

struct AdamTable {
    AdamT t[ADAM_MAXT];
    int ubeg[ADAM_MAXT + 1];
    int n;
    float b2, omb1, omb2, eps, wd, neg_step, bc2_sqrt;   // omb = 1 - beta (host double → fp32)
};

// a + s*b as one rounding where ATen's CUDA functors contract (a + scalar*x →
// fma): the weight-decay add, the lerp, addcmul and addcdiv
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamTable& a) {
    g = __fmaf_rn(a.wd, p, g);
    m = __fmaf_rn(a.omb1, __fsub_rn(g, m), m);
    v = __fmaf_rn(a.omb2, __fmul_rn(g, g), __fmul_rn(v, a.b2));
    const float d = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), a.bc2_sqrt), a.eps);
    p = __fmaf_rn(a.neg_step, __fdiv_rn(m, d), p);
}

// the extras of hkp_adam_step_ex: the EMA tensor of each table entry, the clip
// coefficient on the device
struct AdamExtra {
    float* e[ADAM_MAXT];
    const float* coef;
    float omd;                    // 1 - decay
};

// one 4096-element unit of one tensor; COEF: g = g * *coef before adam_elem
// (_foreach_mul_(grads, coef), g not written back); EMA: e = lerp(e, p_new, omd)
template <bool COEF, bool EMA>
__device__ __forceinline__ void adam_unit(const AdamTable& a, const AdamExtra* x) {
    int j = 0;
    while (j + 1 < a.n && (int)blockIdx.x >= a.ubeg[j + 1]) ++j;
    const AdamT& T = a.t[j];
    float* const E = EMA ? x->e[j] : nullptr;
    const float coef = COEF ? *x->coef : 1.f;         // uniform: one scalar load per block
    const float omd = EMA ? x->omd : 0.f;
    const long base = (long)(blockIdx.x - a.ubeg[j]) * ADAM_UNIT;
    const bool vec = ((T.n & 3) == 0) &&
                     ((((uintptr_t)T.p | (uintptr_t)T.g | (uintptr_t)T.m | (uintptr_t)T.v | (uintptr_t)E) & 15) == 0);
    if (vec) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long i = base + 4L * (threadIdx.x + 256 * q);
            if (i >= T.n) break;
            f32x4 p = *(const f32x4*)(T.p + i), g = *(const f32x4*)(T.g + i);
            f32x4 m = *(const f32x4*)(T.m + i), v = *(const f32x4*)(T.v + i);
            f32x4 ema;
            if (EMA) ema = *(const f32x4*)(E + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = p[e], me = m[e], ve = v[e];
                adam_elem(pe, COEF ? __fmul_rn(g[e], coef) : g[e], me, ve, a);
                p[e] = pe;
                m[e] = me;
                v[e] = ve;
                if (EMA) ema[e] = __fmaf_rn(omd, __fsub_rn(pe, ema[e]), ema[e]);
            }
            *(f32x4*)(T.p + i) = p;
            *(f32x4*)(T.m + i) = m;
            *(f32x4*)(T.v + i) = v;
            if (EMA) *(f32x4*)(E + i) = ema;
        }
    } else {
        for (long i = base + threadIdx.x; i < base + ADAM_UNIT && i < T.n; i += 256) {
            float p = T.p[i], m = T.m[i], v = T.v[i];
            adam_elem(p, COEF ? __fmul_rn(T.g[i], coef) : T.g[i], m, v, a);
            T.p[i] = p;
            T.m[i] = m;
            T.v[i] = v;
            if (EMA) {
                const float e = E[i];
                E[i] = __fmaf_rn(omd, __fsub_rn(p, e), e);
            }
        }
    }
}

__global__ __launch_bounds__(256) void adam_kernel(const AdamTable a) { adam_unit<false, false>(a, nullptr); }

template <bool COEF, bool EMA>
__global__ __launch_bounds__(256) void adam_ex_kernel(const AdamTable a, const AdamExtra x) {
    adam_unit<COEF, EMA>(a, &x);
}

// ---- global L2 norm of the gradients and the clip coefficient (hkp_grad_norm)

struct NormT {
    const float* g;
    long n;
};

struct NormTable {
    NormT t[ADAM_MAXT];
    int ubeg[ADAM_MAXT + 1];
    int n;
};

// the block's 256 values in a fixed order: the wave's xor butterfly, then the four
// waves through LDS as (w0 + w1) + (w2 + w3); the result is valid in thread 0
__device__ __forceinline__ double block_sum_d(double v, double* red) {
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// one block per 4096-element unit (the Adam kernel's units): the squares in fp64
// (exact for fp32 inputs), summed per thread in element order, then over the block;
// one fp64 partial per block
__global__ __launch_bounds__(256) void grad_norm_kernel(const NormTable a, double* __restrict__ partials) {
    __shared__ double red[4];
    int j = 0;
    while (j + 1 < a.n && (int)blockIdx.x >= a.ubeg[j + 1]) ++j;
    const NormT& T = a.t[j];
    const long base = (long)(blockIdx.x - a.ubeg[j]) * ADAM_UNIT;
    const bool vec = ((T.n & 3) == 0) && (((uintptr_t)T.g & 15) == 0);
    double s = 0.0;
    if (vec) {
        f32x4 g[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {                 // the four loads in flight together
            const long i = base + 4L * (threadIdx.x + 256 * q);
            g[q] = i < T.n ? *(const f32x4*)(T.g + i) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = (double)g[q][e];
                s += d * d;
            }
    } else {
        for (long i = base + threadIdx.x; i < base + ADAM_UNIT && i < T.n; i += 256) {
            const double d = (double)T.g[i];
            s += d * d;
        }
    }
    s = block_sum_d(s, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// one block: the partials in a fixed order (thread t takes t, t + 256, ...), the
// norm and the coefficient of clip_grad_norm_ in fp32: c = max_norm / (norm + 1e-6),
// clamped to at most 1 with NaN kept (torch.clamp(c, max=1.0))
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ partials, long np,
                                                               float max_norm, float* __restrict__ out) {
    __shared__ double red[4];
    double s = 0.0;
    for (long i = threadIdx.x; i < np; i += 256) s += partials[i];
    s = block_sum_d(s, red);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(s);
        const float c = __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f));
        out[0] = norm;
        out[1] = c < 1.f ? c : (c != c ? c : 1.f);
    }
}

}  // namespace hkp

using namespace hkp;

extern "C" int hkp_adam_step(int32_t ntensors, const hkp_adam_tensor* tensors, float beta2, float one_minus_beta1,
                             float one_minus_beta2, float eps, float weight_decay, float neg_step_size,
                             float bias_correction2_sqrt, hkp_stream_t stream) {
    HKP_CHECK_ARG(ntensors >= 0 && (ntensors == 0 || tensors), "hkp_adam_step: bad tensor list");
    HKP_CHECK_ARG(bias_correction2_sqrt > 0.f, "hkp_adam_step: bias_correction2_sqrt must be > 0");
    for (int i = 0; i < ntensors; ++i) {
        const hkp_adam_tensor& t = tensors[i];
        HKP_CHECK_ARG(t.n >= 0 && (t.n == 0 || (t.param && t.grad && t.exp_avg && t.exp_avg_sq)),
                      "hkp_adam_step: tensor %d: null pointer", i);
        HKP_CHECK_ARG((t.n + ADAM_UNIT - 1) / ADAM_UNIT < (1L << 30), "hkp_adam_step: tensor %d too large", i);
    }
    hipStream_t st = as_stream(stream);
    for (int i0 = 0; i0 < ntensors; i0 += ADAM_MAXT) {
        AdamTable a;
        a.n = 0;
        a.b2 = beta2; a.omb1 = one_minus_beta1; a.omb2 = one_minus_beta2; a.eps = eps; a.wd = weight_decay;
        a.neg_step = neg_step_size; a.bc2_sqrt = bias_correction2_sqrt;
        long units = 0;
        for (int i = i0; i < ntensors && i < i0 + ADAM_MAXT; ++i) {
            const hkp_adam_tensor& s = tensors[i];
            if (s.n == 0) continue;
            AdamT& d = a.t[a.n];
            d.p = s.param; d.g = s.grad; d.m = s.exp_avg; d.v = s.exp_avg_sq; d.n = s.n;
            a.ubeg[a.n++] = (int)units;
            units += (s.n + ADAM_UNIT - 1) / ADAM_UNIT;
        }
        if (units == 0) continue;
        HKP_CHECK_ARG(units < (1L << 31), "hkp_adam_step: too many elements in one launch");
        a.ubeg[a.n] = (int)units;
        hipLaunchKernelGGL(adam_kernel, dim3((unsigned)units), dim3(256), 0, st, a);
        HKP_LAUNCH_CHECK("hkp_adam_step");
    }
    return HKP_OK;
}

// ---- hkp_adam_step_ex: the same pass with a clip coefficient and / or an EMA

extern "C" int hkp_adam_step_ex(int32_t ntensors, const hkp_adam_tensor* tensors, float* const* ema,
                                float one_minus_decay, const float* coef, float beta2, float one_minus_beta1,
                                float one_minus_beta2, float eps, float weight_decay, float neg_step_size,
                                float bias_correction2_sqrt, hkp_stream_t stream) {
    if (!ema && !coef)
        return hkp_adam_step(ntensors, tensors, beta2, one_minus_beta1, one_minus_beta2, eps, weight_decay,
                             neg_step_size, bias_correction2_sqrt, stream);
    HKP_CHECK_ARG(ntensors >= 0 && (ntensors == 0 || tensors), "hkp_adam_step_ex: bad tensor list");
    HKP_CHECK_ARG(bias_correction2_sqrt > 0.f, "hkp_adam_step_ex: bias_correction2_sqrt must be > 0");
    HKP_CHECK_ARG(!ema || (one_minus_decay > 0.f && one_minus_decay < 0.5f),
                  "hkp_adam_step_ex: one_minus_decay must lie in (0, 0.5)");
    for (int i = 0; i < ntensors; ++i) {
        const hkp_adam_tensor& t = tensors[i];
        HKP_CHECK_ARG(t.n >= 0 && (t.n == 0 || (t.param && t.grad && t.exp_avg && t.exp_avg_sq)),
                      "hkp_adam_step_ex: tensor %d: null pointer", i);
        HKP_CHECK_ARG(!ema || t.n == 0 || ema[i], "hkp_adam_step_ex: tensor %d: null ema pointer", i);
        HKP_CHECK_ARG((t.n + ADAM_UNIT - 1) / ADAM_UNIT < (1L << 30), "hkp_adam_step_ex: tensor %d too large", i);
    }
    hipStream_t st = as_stream(stream);
    for (int i0 = 0; i0 < ntensors; i0 += ADAM_MAXT) {
        AdamTable a;
        AdamExtra x;
        a.n = 0;
        a.b2 = beta2; a.omb1 = one_minus_beta1; a.omb2 = one_minus_beta2; a.eps = eps; a.wd = weight_decay;
        a.neg_step = neg_step_size; a.bc2_sqrt = bias_correction2_sqrt;
        x.coef = coef;
        x.omd = one_minus_decay;
        long units = 0;
        for (int i = i0; i < ntensors && i < i0 + ADAM_MAXT; ++i) {
            const hkp_adam_tensor& s = tensors[i];
            if (s.n == 0) continue;
            AdamT& d = a.t[a.n];
            d.p = s.param; d.g = s.grad; d.m = s.exp_avg; d.v = s.exp_avg_sq; d.n = s.n;
            x.e[a.n] = ema ? ema[i] : nullptr;
            a.ubeg[a.n++] = (int)units;
            units += (s.n + ADAM_UNIT - 1) / ADAM_UNIT;
        }
        if (units == 0) continue;
        HKP_CHECK_ARG(units < (1L << 31), "hkp_adam_step_ex: too many elements in one launch");
        a.ubeg[a.n] = (int)units;
        const dim3 grid((unsigned)units), block(256);
        if (coef && ema)
            hipLaunchKernelGGL((adam_ex_kernel<true, true>), grid, block, 0, st, a, x);
        else if (coef)
            hipLaunchKernelGGL((adam_ex_kernel<true, false>), grid, block, 0, st, a, x);
        else
            hipLaunchKernelGGL((adam_ex_kernel<false, true>), grid, block, 0, st, a, x);
        HKP_LAUNCH_CHECK("hkp_adam_step_ex");
    }
    return HKP_OK;
}

extern "C" int64_t hkp_grad_norm_partials(int32_t ntensors, const hkp_adam_tensor* tensors) {
    if (ntensors < 0 || (ntensors > 0 && !tensors)) return -1;
    int64_t units = 0;
    for (int i = 0; i < ntensors; ++i) {
        if (tensors[i].n < 0) return -1;
        units += (tensors[i].n + ADAM_UNIT - 1) / ADAM_UNIT;
    }
    return units;
}

extern "C" int hkp_grad_norm(int32_t ntensors, const hkp_adam_tensor* tensors, float max_norm, double* partials,
                             int64_t partials_len, float* out, hkp_stream_t stream) {
    HKP_CHECK_ARG(ntensors >= 0 && (ntensors == 0 || tensors), "hkp_grad_norm: bad tensor list");
    HKP_CHECK_ARG(max_norm > 0.f, "hkp_grad_norm: max_norm must be > 0 (inf: the norm only)");
    HKP_CHECK_ARG(out, "hkp_grad_norm: null output");
    for (int i = 0; i < ntensors; ++i) {
        const hkp_adam_tensor& t = tensors[i];
        HKP_CHECK_ARG(t.n >= 0 && (t.n == 0 || t.grad), "hkp_grad_norm: tensor %d: null pointer", i);
        HKP_CHECK_ARG((t.n + ADAM_UNIT - 1) / ADAM_UNIT < (1L << 30), "hkp_grad_norm: tensor %d too large", i);
    }
    const int64_t need = hkp_grad_norm_partials(ntensors, tensors);
    HKP_CHECK_ARG(need == 0 || (partials && partials_len >= need),
                  "hkp_grad_norm: scratch buffer too small (%lld doubles, need %lld)", (long long)partials_len,
                  (long long)need);
    hipStream_t st = as_stream(stream);
    int64_t done = 0;
    for (int i0 = 0; i0 < ntensors; i0 += ADAM_MAXT) {
        NormTable a;
        a.n = 0;
        long units = 0;
        for (int i = i0; i < ntensors && i < i0 + ADAM_MAXT; ++i) {
            const hkp_adam_tensor& s = tensors[i];
            if (s.n == 0) continue;
            a.t[a.n].g = s.grad;
            a.t[a.n].n = s.n;
            a.ubeg[a.n++] = (int)units;
            units += (s.n + ADAM_UNIT - 1) / ADAM_UNIT;
        }
        if (units == 0) continue;
        HKP_CHECK_ARG(units < (1L << 31), "hkp_grad_norm: too many elements in one launch");
        a.ubeg[a.n] = (int)units;
        hipLaunchKernelGGL(grad_norm_kernel, dim3((unsigned)units), dim3(256), 0, st, a, partials + done);
        HKP_LAUNCH_CHECK("hkp_grad_norm");
        done += units;
    }
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)partials, (long)done,
                       max_norm, out);
    HKP_LAUNCH_CHECK("hkp_grad_norm");
    return HKP_OK;
}
