// Operand packing for the f16x3 convs (conv_x3.hip, wgrad_x3.hip): fp32 tensors into
// the packed split layout  [line][ hi(32 ch) | lo(32 ch) ]  fp16, 128 B per line
// (hi = f16(v), lo = f16(v - hi)), weights scaled per output channel by a power of
// two; the plain-fp16 weight pack; and the 7x7/s2 stem's image planes and weights.
// (weight_pack.hip is the batched form of the weight packers.)
#include "common.h"
#include "x3_plan.h"

namespace hkp {

// 2^e putting max|x| in [2^13, 2^14) (1 for 0 / non-finite): exact scaling
__device__ __forceinline__ float pow2_scale_of(float m) {
    if (!(m > 0.f) || !(m < INFINITY)) return 1.f;
    int e;
    frexpf(m, &e);
    e = 14 - e;
    e = e < -100 ? -100 : (e > 100 ? 100 : e);
    return ldexpf(1.f, e);
}

// ---------------------------------------------------------------------------
// operand packing

__device__ __forceinline__ void split_store(float v, _Float16* hi_p) {   // hi at p, lo at p + 32
    const _Float16 h = (_Float16)v;
    hi_p[0] = h;
    hi_p[32] = (_Float16)(v - (float)h);
}

// block max |x| over a row of n elements addressed by idx(i); result broadcast
template <typename F>
__device__ __forceinline__ float block_absmax(int n, F&& val) {
    __shared__ float red[8];
    float m = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) m = fmaxf(m, fabsf(val(i)));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    float r = 0.f;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) r = fmaxf(r, red[i]);
    __syncthreads();
    return r;
}

// w[k][tap][c] fp32 (KRSC) * 2^e_k → ws[k][tap][c/32][hi32|lo32]; one block per k.
// Element e → 2e - (c&31) (lo 32 halves later); wscale[k] = 2^-e_k.
__global__ __launch_bounds__(256) void weight_pack_x3_kernel(int rsc, const float* __restrict__ w,
                                                            _Float16* __restrict__ ws, float* __restrict__ wscale) {
    const int k = blockIdx.x;
    const float* row = w + (long)k * rsc;
    const float sc = pow2_scale_of(block_absmax(rsc, [&](int i) { return row[i]; }));
    for (int i = threadIdx.x; i < rsc; i += blockDim.x) {
        const long e = (long)k * rsc + i;
        split_store(row[i] * sc, ws + 2 * e - (e & 31));
    }
    if (threadIdx.x == 0) wscale[k] = 1.f / sc;
}

// w[k][tap][c] fp32 (KRSC) * 2^e_k → fp16 KRSC (the plain-fp16 conv's operand:
// 64-channel 128-B lines); one block per k, wscale[k] = 2^-e_k
__global__ __launch_bounds__(256) void weight_pack_f16_kernel(int rsc, const float* __restrict__ w,
                                                             _Float16* __restrict__ out, float* __restrict__ wscale) {
    const int k = blockIdx.x;
    const float* row = w + (long)k * rsc;
    const float sc = pow2_scale_of(block_absmax(rsc, [&](int i) { return row[i]; }));
    for (int i = threadIdx.x; i < rsc; i += blockDim.x) out[(long)k * rsc + i] = (_Float16)(row[i] * sc);
    if (threadIdx.x == 0) wscale[k] = 1.f / sc;
}

// flipped dgrad weight, packed: row c (forward input channel) holds element
// (r', s', k) = w[k][R-1-r'][S-1-s'][c] * 2^e_c; one block per c
__global__ __launch_bounds__(256) void weight_flip_pack_x3_kernel(int K, int R, int S, int C,
                                                                 const float* __restrict__ w,
                                                                 _Float16* __restrict__ out,
                                                                 float* __restrict__ wscale) {
    const int c = blockIdx.x;
    const int n = R * S * K;
    auto val = [&](int i) {
        const int k = i % K, t = i / K, sp = t % S, rp = t / S;
        return w[(((long)k * R + (R - 1 - rp)) * S + (S - 1 - sp)) * C + c];
    };
    const float sc = pow2_scale_of(block_absmax(n, val));
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const long e = (long)c * n + i;
        split_store(val(i) * sc, out + 2 * e - (e & 31));
    }
    if (threadIdx.x == 0) wscale[c] = 1.f / sc;
}

// x * 2^e (e from amax; 1 without) → packed split [P][C/32][hi32|lo32]
__global__ __launch_bounds__(256) void split_pack_x3_kernel(long n4, const f32x4* __restrict__ x,
                                                           const unsigned* __restrict__ amax,
                                                           _Float16* __restrict__ out) {
    const float sc = pow2_scale_for(amax);
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        f32x4 v = x[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] *= sc;
        store_split4(v, i, out, 3);
    }
}

// Stem operand: the image → zero-padded NHWC4 planes [2][N][Hp][Wp][4] (hi, then
// lo = f16(x-hi)); padded pixel (hp, wp) = input (hp-3, wp-3).  U8: the image is
// the uint8 HWC batch cv2.imread gives ([N][H][W][C], BGR) and x = u8 / 255 in
// fp32 — ToTensor (dataset.py:16) fused into the stem's operand pack.
template <bool U8>
__global__ __launch_bounds__(256) void stem_pack_x3_kernel(int N, int C, int H, int W, int Hp, int Wp,
                                                          const void* __restrict__ src, _Float16* __restrict__ out) {
    const long total = (long)N * Hp * Wp;
    const long plane = total * 4;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += stride) {
        const int wp = (int)(p % Wp);
        const long t = p / Wp;
        const int hp = (int)(t % Hp);
        const int n = (int)(t / Hp);
        const int h = hp - 3, w = wp - 3;
        const bool in = (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;
        f32x4 v;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (!(in && c < C)) {
                v[c] = 0.f;
            } else if constexpr (U8) {
                const uint8_t u = ((const uint8_t*)src)[(((long)n * H + h) * W + w) * C + c];
                v[c] = __fdiv_rn((float)u, 255.f);
            } else {
                v[c] = ((const float*)src)[(((long)n * C + c) * H + h) * W + w];
            }
        }
        h16x4 hv, lv;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const _Float16 hh = (_Float16)v[c];
            hv[c] = hh;
            lv[c] = (_Float16)(v[c] - (float)hh);
        }
        *(h16x4*)(out + p * 4) = hv;
        *(h16x4*)(out + plane + p * 4) = lv;
    }
}

// Stem weight OIHW [K][C][7][7] * 2^e_k → [K][r][hi32|lo32], 32 = 8 taps (s; 7 = 0)
// x 4 channels (C..3 = 0); one block per k, wscale[k] = 2^-e_k
__global__ __launch_bounds__(256) void stem_weight_pack_x3_kernel(int C, const float* __restrict__ w,
                                                                 _Float16* __restrict__ out,
                                                                 float* __restrict__ wscale) {
    const int k = blockIdx.x;
    const float* wk = w + (long)k * C * 49;
    const float sc = pow2_scale_of(block_absmax(C * 49, [&](int i) { return wk[i]; }));
    for (int e = threadIdx.x; e < 7 * 32; e += blockDim.x) {
        const int c = e & 3, s = (e >> 2) & 7, r = e >> 5;
        const float v = (s < 7 && c < C) ? wk[(c * 7 + r) * 7 + s] * sc : 0.f;
        split_store(v, out + ((long)k * 7 + r) * 64 + s * 4 + c);
    }
    if (threadIdx.x == 0) wscale[k] = 1.f / sc;
}

}  // namespace hkp

using namespace hkp;

extern "C" int hkp_weight_pack_x3(int32_t k, int32_t rsc, int32_t c, const float* w, uint16_t* w_split,
                                  float* w_inv_scale, hkp_stream_t stream) {
    HKP_CHECK_ARG(k > 0 && c > 0 && c % 32 == 0 && rsc > 0 && rsc % c == 0 && w && w_split && w_inv_scale,
                  "hkp_weight_pack_x3: bad args");
    hipLaunchKernelGGL(weight_pack_x3_kernel, dim3(k), dim3(256), 0, as_stream(stream), rsc, w, (_Float16*)w_split,
                       w_inv_scale);
    HKP_LAUNCH_CHECK("hkp_weight_pack_x3");
    return HKP_OK;
}

extern "C" int hkp_weight_pack_f16(int32_t k, int32_t rsc, const float* w, uint16_t* w_f16, float* w_inv_scale,
                                   hkp_stream_t stream) {
    HKP_CHECK_ARG(k > 0 && rsc > 0 && w && w_f16 && w_inv_scale, "hkp_weight_pack_f16: bad args");
    hipLaunchKernelGGL(weight_pack_f16_kernel, dim3(k), dim3(256), 0, as_stream(stream), rsc, w, (_Float16*)w_f16,
                       w_inv_scale);
    HKP_LAUNCH_CHECK("hkp_weight_pack_f16");
    return HKP_OK;
}

extern "C" int hkp_split_pack_x3(int64_t n, int32_t c, const float* x, const uint32_t* amax_bits,
                                 uint16_t* x_split, hkp_stream_t stream) {
    HKP_CHECK_ARG(n > 0 && c > 0 && c % 32 == 0 && n % c == 0 && x && x_split, "hkp_split_pack_x3: bad args");
    long g = (n / 4 + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(split_pack_x3_kernel, dim3((unsigned)g), dim3(256), 0, as_stream(stream), (long)(n / 4),
                       (const f32x4*)x, (const unsigned*)amax_bits, (_Float16*)x_split);
    HKP_LAUNCH_CHECK("hkp_split_pack_x3");
    return HKP_OK;
}

extern "C" int hkp_weight_flip_pack_x3(const hkp_conv_desc* d, const float* w, uint16_t* wf_split,
                                       float* wf_inv_scale, hkp_stream_t stream) {
    HKP_CHECK_ARG(d && w && wf_split && wf_inv_scale, "hkp_weight_flip_pack_x3: null argument");
    HKP_CHECK_ARG(d->k % 32 == 0, "hkp_weight_flip_pack_x3: need Cout%%32==0 (k=%d)", d->k);
    hipLaunchKernelGGL(weight_flip_pack_x3_kernel, dim3(d->c), dim3(256), 0, as_stream(stream), d->k, d->r, d->s,
                       d->c, w, (_Float16*)wf_split, wf_inv_scale);
    HKP_LAUNCH_CHECK("hkp_weight_flip_pack_x3");
    return HKP_OK;
}

extern "C" int64_t hkp_stem_pack_x3_elems(const hkp_conv_desc* d) {
    int ho, wo;
    if (!stem_x3_shape(d) || hkp_conv_out_hw(d, &ho, &wo) != HKP_OK) return -1;
    return 2L * d->n * (2L * ho + 6) * (2L * wo + 6) * 4;
}

static int stem_pack(const hkp_conv_desc* d, const void* src, bool u8, uint16_t* x_split, hkp_stream_t stream,
                     const char* who) {
    int ho, wo;
    int rc = hkp_conv_out_hw(d, &ho, &wo);
    if (rc) return rc;
    HKP_CHECK_ARG(stem_x3_shape(d), "%s: needs the 7x7/s2/p3 NCHW stem with C<=4, Cout%%64==0", who);
    HKP_CHECK_ARG(src && x_split, "%s: null tensor", who);
    const int hp = 2 * ho + 6, wp = 2 * wo + 6;
    long g = ((long)d->n * hp * wp + 255) / 256;
    if (g > 8192) g = 8192;
    if (u8)
        hipLaunchKernelGGL(stem_pack_x3_kernel<true>, dim3((unsigned)g), dim3(256), 0, as_stream(stream), d->n, d->c,
                           d->h, d->w, hp, wp, src, (_Float16*)x_split);
    else
        hipLaunchKernelGGL(stem_pack_x3_kernel<false>, dim3((unsigned)g), dim3(256), 0, as_stream(stream), d->n, d->c,
                           d->h, d->w, hp, wp, src, (_Float16*)x_split);
    HKP_LAUNCH_CHECK(who);
    return HKP_OK;
}

extern "C" int hkp_stem_pack_x3(const hkp_conv_desc* d, const float* x_nchw, uint16_t* x_split, hkp_stream_t stream) {
    return stem_pack(d, x_nchw, false, x_split, stream, "hkp_stem_pack_x3");
}

extern "C" int hkp_stem_pack_x3_u8(const hkp_conv_desc* d, const uint8_t* img_nhwc, uint16_t* x_split,
                                   hkp_stream_t stream) {
    return stem_pack(d, img_nhwc, true, x_split, stream, "hkp_stem_pack_x3_u8");
}

extern "C" int hkp_stem_weight_pack_x3(int32_t k, int32_t c, const float* w_oihw, uint16_t* w_split,
                                       float* w_inv_scale, hkp_stream_t stream) {
    HKP_CHECK_ARG(k > 0 && c >= 1 && c <= 4 && w_oihw && w_split && w_inv_scale, "hkp_stem_weight_pack_x3: bad args");
    hipLaunchKernelGGL(stem_weight_pack_x3_kernel, dim3(k), dim3(256), 0, as_stream(stream), c, w_oihw,
                       (_Float16*)w_split, w_inv_scale);
    HKP_LAUNCH_CHECK("hkp_stem_weight_pack_x3");
    return HKP_OK;
}
