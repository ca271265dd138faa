// Domain randomisation on uint8 [B,H,W,3] BGR batches: the reference's
// commented-out imgaug pipeline (dataset.py:18-31) as one launch per batch.
// A block owns one HKP_AUG_TILE_H x HKP_AUG_TILE_W tile of one image and runs
// that image's program (include/hulkkp.h: hkp_aug_program), so the stage loop and
// its switch are uniform across the block.
//
//   load    the tile plus a 2-pixel halo (a program without BLUR: the tile's rows
//           only) goes into LDS as bytes.  An LDS row keeps its global row's
//           address modulo 4, so the body of a row is whole aligned dwords on both
//           sides and only its first / last < 4 bytes move as bytes; nothing
//           outside [row start, row end) of the tensor is read.  Rows above /
//           below the image are the reflected rows (reflect-101), loaded under
//           their own coordinates.
//   pre     the stages before the BLUR run in place over every in-image pixel of
//           tile + halo, each under its own image coordinates (the LUT of its
//           image, the noise counter y*W + x of the pixel it is) — so what a halo
//           pixel becomes does not depend on which tile loads it.  Columns left /
//           right of the image are then copied from their reflected columns.
//   blur    horizontal pass bytes → fp32 LDS; vertical pass, rint + clamp and the
//           stages after the BLUR in registers (channels in named registers: no
//           indexed local array, no scratch).
//   store   results go through a byte LDS tile laid out on the output rows'
//           address modulo 4 and leave as aligned dwords (+ < 4 head / tail bytes).
//
// Arithmetic: fp32, every operation rounded on its own (-ffp-contract=off and the
// __f*_rn intrinsics), no transcendental on the device; after every stage the
// pixel is uint8 again: q8(v) = clamp(rint(v), 0, 255), rint half to even.
#include "common.h"

namespace hkp {

constexpr int AUG_TH = HKP_AUG_TILE_H, AUG_TW = HKP_AUG_TILE_W, AUG_HALO = 2;
constexpr int AUG_IN_ROWS = AUG_TH + 2 * AUG_HALO;                         // rows of tile + halo
constexpr int AUG_IN_COLS = AUG_TW + 2 * AUG_HALO;                         // columns of tile + halo
constexpr int AUG_IN_STRIDE = (AUG_IN_COLS * 3 + 3 + 3) & ~3;              // row bytes + alignment shift, dword multiple
constexpr int AUG_OUT_STRIDE = (AUG_TW * 3 + 3 + 3) & ~3;
constexpr int AUG_HB_STRIDE = AUG_TW * 3;                                  // fp32 per row of the horizontal pass
constexpr int AUG_LUT_BYTES = 3 * 256;

__device__ __forceinline__ int aug_q8(float v) { return (int)fminf(fmaxf(rintf(v), 0.f), 255.f); }

// reflect-101 (-1 → 1, -2 → 2, n → n-2, n+1 → n-3); rows / columns further out are
// never needed by a stored pixel and only have to stay inside the image
__device__ __forceinline__ int aug_reflect(int i, int n) {
    i = i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i);
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// first output word of Philox4x32-10 at counter (c0, 0, 0, 0)
__device__ __forceinline__ uint32_t aug_philox_x0(uint32_t c0, uint32_t k0, uint32_t k1) {
    uint32_t c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// The HSV stage: one round trip, nothing quantised inside.  Order of operations
// (fp32, each one rounded; tests/_augment_ref.py follows it line for line), with
// r, g, b the channel values as floats:
//   mx = max(max(r, g), b);  mn = min(min(r, g), b);  d = mx - mn;  V = mx
//   S  = mx > 0 ? (255 * d) / mx : 0
//   h  = 0                      if d == 0
//        (g - b) / d, + 6 if < 0  if mx == r
//        2 + (b - r) / d          if mx == g
//        4 + (r - g) / d          otherwise                (ties in that order)
//   h  = h + dh;  if h < 0: h = h + 6;  if h >= 6: h = h - 6
//        (the second test also takes a tiny negative h that h + 6 rounded up to 6)
//   S  = min(max(S * mul + add, 0), 255)
//   c  = (V * S) / 255;  i = floor(h);  f = h - i
//   p  = V - c;  q = V - c * f;  t = V - c * (1 - f)
//   (r, g, b) = i == 0: (V, t, p)  1: (q, V, p)  2: (p, V, t)  3: (p, q, V)  4: (t, p, V)  else: (V, p, q)
//   each of r, g, b: rint, clamp to [0, 255]
__device__ __forceinline__ void aug_hsv(float dh, float add, float mul, int& bi, int& gi, int& ri) {
    const float r = (float)ri, g = (float)gi, b = (float)bi;
    const float mx = fmaxf(fmaxf(r, g), b), mn = fminf(fminf(r, g), b);
    const float d = __fsub_rn(mx, mn);
    float S = mx > 0.f ? __fdiv_rn(__fmul_rn(255.f, d), mx) : 0.f;
    float h;
    if (d == 0.f) {
        h = 0.f;
    } else if (mx == r) {
        h = __fdiv_rn(__fsub_rn(g, b), d);
        if (h < 0.f) h = __fadd_rn(h, 6.f);
    } else if (mx == g) {
        h = __fadd_rn(2.f, __fdiv_rn(__fsub_rn(b, r), d));
    } else {
        h = __fadd_rn(4.f, __fdiv_rn(__fsub_rn(r, g), d));
    }
    h = __fadd_rn(h, dh);
    if (h < 0.f) h = __fadd_rn(h, 6.f);
    if (h >= 6.f) h = __fsub_rn(h, 6.f);
    S = fminf(fmaxf(__fadd_rn(__fmul_rn(S, mul), add), 0.f), 255.f);
    const float c = __fdiv_rn(__fmul_rn(mx, S), 255.f);
    const float fl = floorf(h);
    const float f = __fsub_rn(h, fl);
    const float p = __fsub_rn(mx, c);
    const float q = __fsub_rn(mx, __fmul_rn(c, f));
    const float t = __fsub_rn(mx, __fmul_rn(c, __fsub_rn(1.f, f)));
    float ro, go, bo;
    if (fl == 0.f) {
        ro = mx, go = t, bo = p;
    } else if (fl == 1.f) {
        ro = q, go = mx, bo = p;
    } else if (fl == 2.f) {
        ro = p, go = mx, bo = t;
    } else if (fl == 3.f) {
        ro = p, go = q, bo = mx;
    } else if (fl == 4.f) {
        ro = t, go = p, bo = mx;
    } else {
        ro = mx, go = p, bo = q;
    }
    ri = aug_q8(ro);
    gi = aug_q8(go);
    bi = aug_q8(bo);
}

// stages [first, last) of the block's program on one pixel (ctr = y*W + x in the
// image's own coordinates); the BLUR stage is the caller's
__device__ __forceinline__ void aug_apply(const hkp_aug_program* prog, const uint8_t* s_lut, int first, int last,
                                          const float* __restrict__ gauss, uint32_t ctr, int& b, int& g, int& r) {
    for (int i = first; i < last; ++i) {
        const hkp_aug_stage* st = &prog->stages[i];
        switch (st->kind) {
            case HKP_AUG_LUT: {
                const uint8_t* lut = s_lut + i * AUG_LUT_BYTES;
                b = lut[b];
                g = lut[256 + g];
                r = lut[512 + r];
                break;
            }
            case HKP_AUG_HSV:
                aug_hsv(st->f[0], st->f[1], st->f[2], b, g, r);
                break;
            case HKP_AUG_NOISE: {
                const uint32_t x0 = aug_philox_x0(ctr, st->key[0], st->key[1]);
                const float nz = __fmul_rn(gauss[x0 >> 20], st->f[0]);
                b = aug_q8(__fadd_rn((float)b, nz));
                g = aug_q8(__fadd_rn((float)g, nz));
                r = aug_q8(__fadd_rn((float)r, nz));
                break;
            }
            default:
                break;
        }
    }
}

// lds[g - g0 ...] → bytes [g0, g1) of global memory, lds placed so that
// (lds address) % 4 == g0 % 4: aligned dwords in the middle, < 4 bytes at either
// end; one wave per call, at most 64 dwords (the load side does the same split
// inline, with its loads hoisted)
__device__ __forceinline__ void aug_row_store(uintptr_t g0, uintptr_t g1, const uint8_t* lds, int lane) {
    const uintptr_t a0 = (g0 + 3) & ~(uintptr_t)3, a1 = g1 & ~(uintptr_t)3;
    const uintptr_t hend = a0 < g1 ? a0 : g1;
    const uintptr_t tbeg = a1 > hend ? a1 : hend;
    const uintptr_t a = a0 + 4 * (uintptr_t)lane;
    if (a + 4 <= a1) *(uint32_t*)a = *(const uint32_t*)(lds + (a - g0));
    if (lane < 3 && g0 + lane < hend) *(uint8_t*)(g0 + lane) = lds[lane];
    if (lane >= 4 && lane < 7 && tbeg + (lane - 4) < g1) *(uint8_t*)(tbeg + (lane - 4)) = lds[tbeg + (lane - 4) - g0];
}

// LDS image (dynamic, sized by the host: AUG_LDS_BLUR when any program of the batch
// has a BLUR, else AUG_LDS_PLAIN, which more blocks per CU fit):
//   s_in | s_lut | s_prog | s_sh | BLUR: s_hb (the store tile then reuses s_in, dead
//                                  after the horizontal pass)  /  else: the store tile
constexpr int AUG_OFF_LUT = AUG_IN_ROWS * AUG_IN_STRIDE;
constexpr int AUG_OFF_PROG = AUG_OFF_LUT + HKP_AUG_MAX_STAGES * AUG_LUT_BYTES;
constexpr int AUG_OFF_SH = AUG_OFF_PROG + (int)sizeof(hkp_aug_program);
constexpr int AUG_OFF_X = (AUG_OFF_SH + AUG_IN_ROWS * 4 + 15) & ~15;
constexpr int AUG_LDS_BLUR = AUG_OFF_X + AUG_IN_ROWS * AUG_HB_STRIDE * 4;
constexpr int AUG_LDS_PLAIN = AUG_OFF_X + AUG_TH * AUG_OUT_STRIDE;
static_assert(AUG_TH * AUG_OUT_STRIDE <= AUG_IN_ROWS * AUG_IN_STRIDE, "the store tile reuses s_in");
constexpr int AUG_ROWS_PER_WAVE = AUG_IN_ROWS / 4;                       // 4 waves, one row each per round
constexpr int AUG_LUT_DW_PER_THREAD = HKP_AUG_MAX_STAGES * AUG_LUT_BYTES / 4 / 256;
static_assert(AUG_IN_ROWS % 4 == 0 && HKP_AUG_MAX_STAGES * AUG_LUT_BYTES % 1024 == 0, "load loops");

__global__ __launch_bounds__(256) void augment_u8_kernel(int H, int W, int lds_blur, const uint8_t* __restrict__ in,
                                                        uint8_t* __restrict__ out,
                                                        const hkp_aug_program* __restrict__ progs,
                                                        const uint8_t* __restrict__ luts,
                                                        const float* __restrict__ gauss) {
    extern __shared__ __attribute__((aligned(16))) uint8_t aug_smem[];
    uint8_t* const s_in = aug_smem;
    uint8_t* const s_lut = aug_smem + AUG_OFF_LUT;
    hkp_aug_program& s_prog = *(hkp_aug_program*)(aug_smem + AUG_OFF_PROG);
    int* const s_sh = (int*)(aug_smem + AUG_OFF_SH);       // per LDS row: its global row's address % 4
    float* const s_hb = (float*)(aug_smem + AUG_OFF_X);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.z, x0 = blockIdx.x * AUG_TW, y0 = blockIdx.y * AUG_TH;

    if (tid < (int)(sizeof(hkp_aug_program) / 4)) ((uint32_t*)&s_prog)[tid] = ((const uint32_t*)(progs + n))[tid];
    __syncthreads();
    int nst = s_prog.nstages;
    nst = nst < 0 ? 0 : (nst > HKP_AUG_MAX_STAGES ? HKP_AUG_MAX_STAGES : nst);
    int bi = -1;
    for (int i = 0; i < nst; ++i)
        if (s_prog.stages[i].kind == HKP_AUG_BLUR && bi < 0) bi = i;
    const bool blur = bi >= 0;
    if (blur && !lds_blur) return;      // (block-uniform) the host sized the LDS from another program than this
    uint8_t* const s_out = blur ? s_in : aug_smem + AUG_OFF_X;

    // ---- load: the LUTs of the LUT stages, and the in-image columns [cx0, cx1) of rows
    // [r_lo, r_hi), one wave per row.  Every global load is issued before the first
    // LDS write waits for one (registers with static indices), so the block pays one
    // memory latency here, not one per row.
    uint32_t lut_dw[AUG_LUT_DW_PER_THREAD];
#pragma unroll
    for (int k = 0; k < AUG_LUT_DW_PER_THREAD; ++k) {
        const int idx = tid + 256 * k, slot = idx / (AUG_LUT_BYTES / 4);
        lut_dw[k] = 0;
        if (slot < nst && s_prog.stages[slot].kind == HKP_AUG_LUT)
            lut_dw[k] = ((const uint32_t*)(luts + (long)n * HKP_AUG_MAX_STAGES * AUG_LUT_BYTES))[idx];
    }
    const int r_lo = blur ? 0 : AUG_HALO, r_hi = blur ? AUG_IN_ROWS : AUG_HALO + AUG_TH;
    const int xl = x0 - AUG_HALO;                                  // image column of LDS column 0
    const int cx0 = xl < 0 ? 0 : xl, cx1 = x0 + AUG_TW + AUG_HALO < W ? x0 + AUG_TW + AUG_HALO : W;
    uint32_t ld_dw[AUG_ROWS_PER_WAVE];
    uint8_t ld_hb[AUG_ROWS_PER_WAVE], ld_tb[AUG_ROWS_PER_WAVE];
    int o_dw[AUG_ROWS_PER_WAVE], o_hb[AUG_ROWS_PER_WAVE], o_tb[AUG_ROWS_PER_WAVE];    // LDS offsets, -1: none
#pragma unroll
    for (int k = 0; k < AUG_ROWS_PER_WAVE; ++k) {
        const int r = wave + 4 * k;
        o_dw[k] = o_hb[k] = o_tb[k] = -1;
        ld_dw[k] = 0;
        ld_hb[k] = ld_tb[k] = 0;
        if (r < r_lo || r >= r_hi) continue;
        const int sy = aug_reflect(y0 - AUG_HALO + r, H);
        // address LDS column 0 would have (left of the row at x0 == 0: arithmetic only)
        const intptr_t v0 = (intptr_t)in + (((long)n * H + sy) * W + xl) * 3;
        const int sh = (int)(v0 & 3);
        if (lane == 0) s_sh[r] = sh;
        // bytes [g0, g1) of the row; LDS byte of global byte g: row0 + (g - v0), the same modulo 4
        const uintptr_t g0 = (uintptr_t)(v0 + (long)(cx0 - xl) * 3), g1 = (uintptr_t)(v0 + (long)(cx1 - xl) * 3);
        const int row0 = r * AUG_IN_STRIDE + sh;
        const uintptr_t a0 = (g0 + 3) & ~(uintptr_t)3, a1 = g1 & ~(uintptr_t)3;
        const uintptr_t hend = a0 < g1 ? a0 : g1;
        const uintptr_t tbeg = a1 > hend ? a1 : hend;
        const uintptr_t a = a0 + 4 * (uintptr_t)lane;
        if (a + 4 <= a1) {
            o_dw[k] = row0 + (int)(a - (uintptr_t)v0);
            ld_dw[k] = *(const uint32_t*)a;
        }
        if (lane < 3 && g0 + lane < hend) {
            o_hb[k] = row0 + (int)(g0 + lane - (uintptr_t)v0);
            ld_hb[k] = *(const uint8_t*)(g0 + lane);
        }
        if (lane >= 4 && lane < 7 && tbeg + (lane - 4) < g1) {
            o_tb[k] = row0 + (int)(tbeg + (lane - 4) - (uintptr_t)v0);
            ld_tb[k] = *(const uint8_t*)(tbeg + (lane - 4));
        }
    }
#pragma unroll
    for (int k = 0; k < AUG_LUT_DW_PER_THREAD; ++k) ((uint32_t*)s_lut)[tid + 256 * k] = lut_dw[k];
#pragma unroll
    for (int k = 0; k < AUG_ROWS_PER_WAVE; ++k) {
        if (o_dw[k] >= 0) *(uint32_t*)(s_in + o_dw[k]) = ld_dw[k];
        if (o_hb[k] >= 0) s_in[o_hb[k]] = ld_hb[k];
        if (o_tb[k] >= 0) s_in[o_tb[k]] = ld_tb[k];
    }
    __syncthreads();

    if (blur) {
        const float w0 = s_prog.stages[bi].f[0], w1 = s_prog.stages[bi].f[1], w2 = s_prog.stages[bi].f[2];
        if (bi > 0) {
            // ---- stages before the BLUR, in place over tile + halo
            for (int i = tid; i < AUG_IN_ROWS * AUG_IN_COLS; i += 256) {
                const int r = i / AUG_IN_COLS, c = i % AUG_IN_COLS;
                const int x = xl + c;
                if (x < 0 || x >= W) continue;
                const int sy = aug_reflect(y0 - AUG_HALO + r, H);
                uint8_t* p = s_in + r * AUG_IN_STRIDE + s_sh[r] + c * 3;
                int b = p[0], g = p[1], rr = p[2];
                aug_apply(&s_prog, s_lut, 0, bi, gauss, (uint32_t)sy * (uint32_t)W + (uint32_t)x, b, g, rr);
                p[0] = (uint8_t)b;
                p[1] = (uint8_t)g;
                p[2] = (uint8_t)rr;
            }
            __syncthreads();
        }
        // ---- columns -2, -1, W, W+1 from their reflections
        if (tid < AUG_IN_ROWS * 4) {
            const int r = tid >> 2, j = tid & 3;
            const int x = j < 2 ? j - 2 : W + j - 2;
            const int c = x - xl, sc = aug_reflect(x, W) - xl;
            if (c >= 0 && c < AUG_IN_COLS && sc >= 0 && sc < AUG_IN_COLS) {
                uint8_t* row = s_in + r * AUG_IN_STRIDE + s_sh[r];
                row[c * 3] = row[sc * 3];
                row[c * 3 + 1] = row[sc * 3 + 1];
                row[c * 3 + 2] = row[sc * 3 + 2];
            }
        }
        __syncthreads();
        // ---- horizontal pass: s_hb[r][3x + ch], taps at bytes j, j+3, .., j+12
        for (int i = tid; i < AUG_IN_ROWS * AUG_HB_STRIDE; i += 256) {
            const int r = i / AUG_HB_STRIDE, j = i % AUG_HB_STRIDE;
            const uint8_t* p = s_in + r * AUG_IN_STRIDE + s_sh[r] + j;
            float a = __fadd_rn(__fmul_rn(w2, (float)p[0]), __fmul_rn(w1, (float)p[3]));
            a = __fadd_rn(a, __fmul_rn(w0, (float)p[6]));
            a = __fadd_rn(a, __fmul_rn(w1, (float)p[9]));
            a = __fadd_rn(a, __fmul_rn(w2, (float)p[12]));
            s_hb[i] = a;
        }
        __syncthreads();
    }

    // ---- vertical pass (or the plain pixel), remaining stages, into the store tile
    const float w0 = blur ? s_prog.stages[bi].f[0] : 0.f, w1 = blur ? s_prog.stages[bi].f[1] : 0.f,
                w2 = blur ? s_prog.stages[bi].f[2] : 0.f;
    const int x = lane, gx = x0 + x;
    const uintptr_t out_tile = (uintptr_t)out + (((long)n * H + y0) * W + x0) * 3;     // row y: + y * 3W
#pragma unroll 2
    for (int k = 0; k < AUG_TH / 4; ++k) {
        const int y = wave + 4 * k, gy = y0 + y;
        if (gy >= H || gx >= W) continue;
        int b, g, r;
        if (blur) {
            const float* hb = s_hb + y * AUG_HB_STRIDE + 3 * x;
            float v[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float a = __fadd_rn(__fmul_rn(w2, hb[ch]), __fmul_rn(w1, hb[AUG_HB_STRIDE + ch]));
                a = __fadd_rn(a, __fmul_rn(w0, hb[2 * AUG_HB_STRIDE + ch]));
                a = __fadd_rn(a, __fmul_rn(w1, hb[3 * AUG_HB_STRIDE + ch]));
                a = __fadd_rn(a, __fmul_rn(w2, hb[4 * AUG_HB_STRIDE + ch]));
                v[ch] = a;
            }
            b = aug_q8(v[0]);
            g = aug_q8(v[1]);
            r = aug_q8(v[2]);
        } else {
            const uint8_t* p = s_in + (y + AUG_HALO) * AUG_IN_STRIDE + s_sh[y + AUG_HALO] + (x + AUG_HALO) * 3;
            b = p[0], g = p[1], r = p[2];
        }
        aug_apply(&s_prog, s_lut, blur ? bi + 1 : 0, nst, gauss, (uint32_t)gy * (uint32_t)W + (uint32_t)gx, b, g, r);
        const int osh = (int)((out_tile + (uintptr_t)(y * W) * 3) & 3);
        uint8_t* o = s_out + y * AUG_OUT_STRIDE + osh + 3 * x;
        o[0] = (uint8_t)b;
        o[1] = (uint8_t)g;
        o[2] = (uint8_t)r;
    }
    __syncthreads();

    // ---- store: one wave per output row
    const int tw = W - x0 < AUG_TW ? W - x0 : AUG_TW;
    for (int y = wave; y < AUG_TH && y0 + y < H; y += 4) {
        const uintptr_t g0 = out_tile + (uintptr_t)(y * W) * 3;
        aug_row_store(g0, g0 + (uintptr_t)tw * 3, s_out + y * AUG_OUT_STRIDE + (int)(g0 & 3), lane);
    }
}

}  // namespace hkp

using namespace hkp;

extern "C" int hkp_augment_u8(int32_t n, int32_t h, int32_t w, const uint8_t* img_in, uint8_t* img_out,
                              const hkp_aug_program* programs_host, const hkp_aug_program* programs,
                              const uint8_t* luts, const float* gauss_table, hkp_stream_t stream) {
    static_assert(sizeof(hkp_aug_stage) == 32 && sizeof(hkp_aug_program) == 288, "hkp_aug_program layout");
    HKP_CHECK_ARG(n > 0 && n <= 65535, "hkp_augment_u8: bad batch size n=%d (1..65535)", n);
    HKP_CHECK_ARG(h >= 3 && w >= 3, "hkp_augment_u8: h and w must be at least 3 (reflect-101 borders), got %dx%d", h, w);
    HKP_CHECK_ARG((int64_t)h * w <= INT32_MAX && (h + AUG_TH - 1) / AUG_TH <= 65535,
                  "hkp_augment_u8: image %dx%d too large", h, w);
    HKP_CHECK_ARG(img_in && img_out && programs_host && programs && luts && gauss_table,
                  "hkp_augment_u8: null pointer");
    const int64_t total = (int64_t)n * h * w * 3;
    HKP_CHECK_ARG(img_out + total <= img_in || img_in + total <= img_out,
                  "hkp_augment_u8: img_out must not overlap img_in (the blur reads neighbours)");
    HKP_CHECK_ARG(((uintptr_t)programs & 3) == 0 && ((uintptr_t)luts & 3) == 0 && ((uintptr_t)gauss_table & 3) == 0,
                  "hkp_augment_u8: programs, luts and gauss_table must be 4-byte aligned");
    int any_blur = 0;
    for (int32_t i = 0; i < n; ++i) {
        const hkp_aug_program& p = programs_host[i];
        HKP_CHECK_ARG(p.nstages >= 0 && p.nstages <= HKP_AUG_MAX_STAGES,
                      "hkp_augment_u8: program %d has a bad stage count %d (0..%d)", i, p.nstages, HKP_AUG_MAX_STAGES);
        int blurs = 0;
        for (int32_t s = 0; s < p.nstages; ++s) {
            const int32_t kind = p.stages[s].kind;
            HKP_CHECK_ARG(kind >= HKP_AUG_LUT && kind <= HKP_AUG_NOISE,
                          "hkp_augment_u8: program %d stage %d has an unknown stage kind %d", i, s, kind);
            blurs += kind == HKP_AUG_BLUR;
        }
        HKP_CHECK_ARG(blurs <= 1, "hkp_augment_u8: program %d has more than one BLUR stage (%d)", i, blurs);
        any_blur |= blurs;
    }
    const dim3 grid((unsigned)((w + AUG_TW - 1) / AUG_TW), (unsigned)((h + AUG_TH - 1) / AUG_TH), (unsigned)n);
    hipLaunchKernelGGL(augment_u8_kernel, grid, dim3(256), any_blur ? AUG_LDS_BLUR : AUG_LDS_PLAIN, as_stream(stream),
                       h, w, any_blur, img_in, img_out, programs, luts, gauss_table);
    HKP_LAUNCH_CHECK("hkp_augment_u8");
    return HKP_OK;
}
