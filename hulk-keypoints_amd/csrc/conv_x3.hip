// f16x3 implicit-GEMM convolution (the main-path conv arithmetic), deep-pipelined:
// forward, stride-1 backward-data (the same kernel on the gradient with flipped
// weights) and the 7x7/s2 stem.  Backward-filter: wgrad_x3.hip; the operand
// packers: pack_x3.hip; what both share with this file: x3_dev.h.
//
// f16x3 arithmetic: every operand v is split as hi = f16(v), lo = f16(v - hi) and
//     v_a * v_b ≈ hi_a*hi_b + hi_a*lo_b + lo_a*hi_b
// (3 fp16 MFMAs, fp32 accumulation, the dropped lo*lo and lo's own rounding cost
// ~2^-22 relative per product).  All three products go into ONE fp32
// accumulator — fp32-class with the same rounding as separate ones, and half the
// accumulator registers, which is what pays for the 256x256 tiles below.  lo is
// stored unscaled, so it is exact only while v - hi is an fp16 normal
// (|v| >= 2^-3): operands with no natural scale are scaled by a power of two —
// weights per output channel (max|w| -> [2^13, 2^14), inverse applied in the
// epilogue), gradients per tensor from max|dy| — and activations keep an
// absolute error floor of 2^-25 below 2^-3, negligible next to fp32 rounding of
// the sums they feed.
//
// Operands arrive PRE-SPLIT in the "packed split" layout written by their
// producers (bn_apply / bn_relu_maxpool with split_passes=3, hkp_split_pack_x3,
// hkp_weight_pack_x3):
//     xs[pixel][C/32][ hi(32 ch) | lo(32 ch) ]        fp16, 128 B per (pixel, group)
//     ws[k][tap][C/32][ hi(32 ch) | lo(32 ch) ]       (+ ws_scale[k]: 2^-e_k)
// so the 32 channels of one filter tap of one GEMM row are one 128-B cache line
// holding both planes — the same bytes as the fp32 tensor.
//
// Forward kernel (conv_x3_kernel<BN, STEM, PAIR, MFD, SK, P>): tile 256 pixels x
// BN output channels, 8 waves as 4x2 (wave tile 64 x BN/2).  A K-step stages one
// 128-B line per GEMM row (32 channels hi|lo; P = 1: 64 plain fp16 channels) into
// a 2- or 3-stage LDS ring by LDS-DMA (global_load_lds_dwordx4: no VGPR round
// trip, no ds_write), NST-1 K-steps in flight ahead of the compute, retired by a
// counted s_waitcnt vmcnt + raw s_barrier (never __syncthreads inside the loop:
// its fence would drain the DMA queue).  LDS rows are unpadded (the DMA writes
// lane-linear 1 KiB pieces); an XOR swizzle of the 16-B chunk index with
// (row>>1)&7, applied to the per-lane DMA SOURCE address and to the ds_read
// address, makes the fragment reads conflict-free (0 conflicts measured).  K
// order: channel group outer, filter tap inner (a pixel line is re-read by the
// next taps while in L2).  Out-of-image taps / rows past M load a zero line.
// MFMA bodies: 16x16x32 (MFD 16) or 32x32x16 (MFD 32), software-pipelined (next
// fragments read during the current MFMAs, one ds_read per MFMA gap, one barrier
// per K-step).  Epilogue: NHWC fp32 (or fp16) store (x weight scale, x gradient
// scale, + addend) + BN tile partials per 128-row tile.
//
// Operand layouts (P): 3 = the packed f16x3 split above (fp32-accurate, the
// default arithmetic); 1 = plain fp16 NHWC activations and KRSC weights (each
// output channel scaled by a power of two) — BASELINE config C4's "fp16 with
// MFMA", the same kernel with 2 MFMAs per 64 channels instead of 3 per 32.
// Intermediate precisions on the packed layout (inference; DESIGN "precision
// modes"), 2 MFMAs per 32 channels: P = 2 keeps hi_x*hi_w + lo_x*hi_w (the
// weights rounded to fp16 after their per-channel power-of-two scale, the
// activation exact to ~2^-22), P = 4 keeps hi_x*hi_w + hi_x*lo_w (the activation
// rounded to fp16, the weights exact).
//
// Replaces the cuDNN convs of src/resnet.py:20-37,77,86,137,184-188 and their
// backward under loss.backward() (train.py:35).
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "x3_plan.h"
#include "x3_dev.h"

namespace hkp {

// LDS ring depth of a conv_x3 tile config (32-channel / 128-B stages): 256x256
// tiles 2 (B fragments refilled per column instead), two blocks per CU (PAIR:
// 256x64 tiles and the stem) 2, otherwise 3.  The whole 160 KiB at most (the
// stream-K flag reuses the drained ring).
constexpr int x3_nst(int BN, bool PAIR) { return (BN == 256 || PAIR) ? 2 : 3; }

// the ring, or (P = 1) the staged fp16 output tile if that is larger (256x256: 132 KiB)
constexpr int x3_lds_bytes(int BN, bool PAIR, int P) {
    return P == 1 && 256 * (BN + 8) * 2 > x3_nst(BN, PAIR) * (256 + BN) * 128 ? 256 * (BN + 8) * 2
                                                                              : x3_nst(BN, PAIR) * (256 + BN) * 128;
}
// A3 (conv_x3_a3_kernel): the 256x256 16x16x32 body with separate A and B rings —
// A (the activation lines) 3 stages deep, so a stage's DMA has two K-steps to
// land instead of one (the 1x1 convs of config C4 stream every A line from HBM),
// B (the weights, L2-resident) 2 stages: 5 x 32 KiB = the whole 160 KiB; the
// epilogue's scratch and column scales reuse the drained ring.
constexpr int X3_A3_LDS = 5 * 256 * 128;
// ... with BM-row A stages (A3_192: 192-row tiles, 136 KiB; A3_160: 125 KiB, with a
// 1 KiB sink for the A DMA pieces past row 160 — 20 pieces over 8 waves, 3 each)
constexpr int x3_a3_lds(int BM, int BN = 256) { return 3 * BM * 128 + 2 * BN * 128 + (BM % 64 ? 1024 : 0); }
// waves in M of a BM-row tile (8 waves): 4 (64- / 48-row wave tiles), 2 for 160 rows
// (40-row wave tiles do not split into 16-row MFMA tiles; 80 x 64 instead)
constexpr int x3_wm(int BM) { return BM == 160 ? 2 : 4; }

// BN-partials scratch (x3_bn_partials_w: [2][WM][BN] floats) past the ring, so
// the epilogue needs no barrier before it, then the tile's BN column scales
// (loaded during the pipeline fill: a global load in the epilogue waited ~4 us
// behind the other CUs' output writes); the two-blocks-per-CU tiles (PAIR) have
// no LDS to spare: they reuse the ring after a barrier and load scales late
constexpr int x3_red_bytes(int BN, bool PAIR) { return PAIR ? 0 : 2 * 4 * BN * 4 + BN * 4; }

// ---- stream-K bookkeeping (X3Args::sk_units) ----
__device__ __forceinline__ long sk_start(long b, long U, int G) { return b * U / G; }
// the block whose unit range holds unit u: the largest b with sk_start(b) <= u
__device__ __forceinline__ int sk_block_of(long u, long U, int G) { return (int)(((u + 1) * G + U - 1) / U) - 1; }

typedef f32x4 __attribute__((address_space(1))) gf32x4;
typedef unsigned __attribute__((address_space(1))) gu32;

// A partial tile segment: publish this block's accumulators as an fp32 slab,
// count the arrival; the last-arriving segment's block reads every slab of the
// tile in segment order (fixed summation order: the result does not depend on
// which block arrives last) and returns true with the sum in its accumulators.
// Stream-K is column-grouped: the grid is NG groups of n_tiles blocks; group g
// runs units [g*U/NG, (g+1)*U/NG) of the (m-tile, K-step) sequence, block
// g*n_tiles + nt of it for column tile nt — the n_tiles blocks of a group are
// adjacent after the XCD remap and read the same A lines at the same time (one
// L2 fetch), as the data-parallel grid's neighbouring tiles do.
// Slab of group gg's block for tile (mt, nt): slot 2*(gg*n_tiles + nt) + (0: mt
// is the group's first m-tile, 1: its last).  Hand-off per
// cdna_hip_programming.md §6 Guideline 16 (split-K counter form): every wave
// drains its stores, barrier, one lane releases at agent scope and adds to the
// counter; the last arriver acquires at agent scope before any wave reads a
// slab, and re-zeroes the counter.
template <int NV4, typename Get, typename Set>
__device__ __forceinline__ bool sk_combine(const X3Args& a, int T, int tid, char* flag_lds, Get&& get, Set&& set) {
    const long U = a.sk_units;
    const int NT = a.n_tiles, NG = (a.sk_grid ? a.sk_grid : (int)gridDim.x) / NT;
    const int mt = T / NT, nt = T - mt * NT;
    const long t0 = (long)mt * a.nks;
    const int b0 = sk_block_of(t0, U, NG), nseg = sk_block_of(t0 + a.nks - 1, U, NG) - b0 + 1;
    auto slab = [&](int gg) {
        const int which = sk_start(gg, U, NG) >= t0 ? 0 : 1;
        return (gf32x4*)a.sk_ws + (long)(a.sk_one ? gg * NT + nt : 2 * (gg * NT + nt) + which) * NV4 * 512;
    };
    gf32x4* mine = slab((a.sk_grid ? a.sk_b : xcd_remap(blockIdx.x, gridDim.x)) / NT);
#pragma unroll
    for (int v = 0; v < NV4; ++v) mine[v * 512 + tid] = get(v);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        gu32* cnt = (gu32*)a.sk_cnt + T;
        const unsigned prev = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = prev == (unsigned)(nseg - 1);
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        *(volatile int*)flag_lds = last;
    }
    __syncthreads();
    if (!*(volatile int*)flag_lds) return false;
    // 8 loads in flight per chunk (the accumulators leave few free registers;
    // double-buffered chunks, or a chunk index computed at run time, put the
    // 256x256 accumulators into scratch)
    static_assert(NV4 % 8 == 0 || NV4 < 8, "sk_combine chunks");
    constexpr int CW = NV4 < 8 ? NV4 : 8;
    for (int sg = 0; sg < nseg; ++sg) {
        const gf32x4* p = slab(b0 + sg);
#pragma unroll
        for (int v0 = 0; v0 < NV4; v0 += CW) {
            f32x4 x[CW];
#pragma unroll
            for (int v = 0; v < CW; ++v) x[v] = p[(v0 + v) * 512 + tid];
#pragma unroll
            for (int v = 0; v < CW; ++v) set(v0 + v, sg == 0 ? x[v] : get(v0 + v) + x[v]);
        }
    }
    return true;
}

// NHWC offset of output (row m, channel n) of a launch (-1: row past M); strided
// dgrad writes one output phase per launch
__device__ __forceinline__ long x3_out_off(const X3Args& a, int m, int n) {
    if (m >= a.M) return -1;
    long pix = m;
    if (a.ost) {
        const int hw = a.Ho * a.Wo, ni = m / hw, rem = m - ni * hw;
        const int ho = rem / a.Wo, wo = rem - ho * a.Wo;
        pix = ((long)ni * a.OH + ho * a.ost + a.oy) * a.OW + wo * a.ost + a.ox;
    }
    return pix * a.K + n;
}

// One output element: y (fp32) or y16 (fp16, the plain-fp16 path), scaled, +
// the addend (dgrad's residual-branch gradient)
__device__ __forceinline__ void x3_store(const X3Args& a, long off, float v, float av) {
    if (off < 0) return;
    v = a.add ? v + av : v;
    if (a.y16) a.y16[off] = (_Float16)v;
    else a.y[off] = v;
}

// The MFMAs of one 128-B stage row pair (A fragment a0/a1, B fragment b0/b1 =
// the row's chunks 0-3 / 4-7) for operand layout P:
//   P = 3 (packed f16x3 split, chunks = hi32 | lo32):  hi*hi + hi*lo + lo*hi
//   P = 2 / 4 (packed split): two of those three products (see the header)
//   P = 1 (plain fp16, chunks = channels 0-31 | 32-63): two k-slices
// fp16 MFMAs per 128-B stage row pair
constexpr int x3_nprod(int P) { return P == 3 ? 3 : 2; }

template <int P, typename V, typename Acc, typename Mfma>
__device__ __forceinline__ void x3_products(Acc& acc, const V& a0, const V& a1, const V& b0, const V& b1, Mfma&& mfma) {
    if constexpr (P == 3) {
        acc = mfma(a0, b0, acc);
        acc = mfma(a0, b1, acc);
        acc = mfma(a1, b0, acc);
    } else if constexpr (P == 2) {         // weights at fp16: (hi_x + lo_x) * hi_w
        acc = mfma(a0, b0, acc);
        acc = mfma(a1, b0, acc);
    } else if constexpr (P == 4) {         // activation at fp16: hi_x * (hi_w + lo_w)
        acc = mfma(a0, b0, acc);
        acc = mfma(a0, b1, acc);
    } else {
        acc = mfma(a0, b0, acc);
        acc = mfma(a1, b1, acc);
    }
}

// BN tile partials of the tile in the accumulators: per 128-row half, the
// column sum and the sum of squares about the half's mean (Chan-mergeable in
// bn_finalize).  VAL(i, j, r) / ROW(i, r) address the accumulator element and
// its output row; COLS per wave column block, LGRP lanes per column group.
template <int BN, int NI, int NJ, int NR, int CW, int SHF, typename Val, typename Row>
__device__ __forceinline__ void x3_bn_partials(const X3Args& a, char* smem, int m0, int n0, int wm, int wn, int lane,
                                               int tid, Val&& val, Row&& row) {
    constexpr int WM = 4;
    __syncthreads();                       // every wave done reading the ring
    float* red = (float*)smem;             // [WM][BN] column sums, then [2][BN] half-tile means
    float* tmean = red + WM * BN;
    float colsum[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int r = 0; r < NR; ++r) s += (row(i, r) < a.M) ? val(i, j, r) : 0.f;
        for (int o = SHF; o < 64; o <<= 1) s += __shfl_xor(s, o);
        colsum[j] = s;
    }
    if (lane < CW) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) red[wm * BN + wn * NJ * CW + j * CW + lane] = colsum[j];
    }
    __syncthreads();
    const long tile128 = (long)a.part_base + ((m0 - a.m_base) >> 7);
    for (int e = tid; e < 2 * BN; e += 512) {
        const int h = e / BN, c = e - h * BN;
        const int cnt = min(128, a.M - (m0 + 128 * h));
        if (cnt > 0) {
            const float s = red[(2 * h) * BN + c] + red[(2 * h + 1) * BN + c];
            tmean[h * BN + c] = s / (float)cnt;
            a.part[((tile128 + h) * a.K + n0 + c) * 2 + 0] = s;
        }
    }
    __syncthreads();
    const float* mu_h = tmean + (wm >> 1) * BN;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const float mu = mu_h[wn * NJ * CW + j * CW + (lane % CW)];
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const float d = val(i, j, r) - mu;
                q += (row(i, r) < a.M) ? d * d : 0.f;
            }
        for (int o = SHF; o < 64; o <<= 1) q += __shfl_xor(q, o);
        colsum[j] = q;
    }
    __syncthreads();
    if (lane < CW) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) red[wm * BN + wn * NJ * CW + j * CW + lane] = colsum[j];
    }
    __syncthreads();
    for (int e = tid; e < 2 * BN; e += 512) {
        const int h = e / BN, c = e - h * BN;
        if (a.M - (m0 + 128 * h) > 0)
            a.part[((tile128 + h) * a.K + n0 + c) * 2 + 1] = red[(2 * h) * BN + c] + red[(2 * h + 1) * BN + c];
    }
}

// BN tile partials, one barrier, VALU-lean (a wave64 VALU op costs 4 cycles;
// the first version's ~1700 per wave, mostly row masks and selects, took ~6 us
// per tile): each lane reduces its own NI*NR rows of a column to (sum, M2 about
// its own mean) in registers — on f32x4 vectors (packed fp32 ops), without row
// masks when all 64 rows of the wave are valid (every tile but the last) — the
// lane groups of a column merge pairwise by Chan's formula over log2(64/CW)
// shuffle steps (sums and M2s are symmetric in the pair, so both lanes get the
// same bits), and the two waves of a 128-row half merge through a small LDS
// scratch (red: [2][WM][BN] floats, outside anything still being read):
//   n = na + nb,  sum = sa + sb,  M2 = M2a + M2b + (mb - ma)^2 * na*nb / n.
// Same quantities as x3_bn_partials (sum, M2 about the half-tile mean).
// A wave covers 16 * NI rows (WM = 4 waves: NI = 4 for the 256-row tiles, 3 for the
// 192-row A3 tiles), so a partial tile (a half tile) holds 32 * NI rows: 128 / 96.
// WMP = 2 (the 160-row A3 tiles, NI = 5): a wave's 80 rows are a whole partial tile,
// written from its lanes after the shuffle merge (no LDS, no WIDE form).
// VEC(i, j): the f32x4 of accumulator rows ROW(i, 0..3) of column block j.
// SC(j): the column's output scale (a power of two: sums scale by it, M2 by its
// square, exactly) when VEC is the unscaled accumulator.
//
// WIDE (full 256-row tiles; scratch of 33 * BN floats that is free once every
// wave is past its last fragment read, e.g. the drained ring): the lanes' (sum,
// M2) go to LDS as they are, and one thread per (128-row half, column) merges
// the four row groups of each wave and then the half's two waves — the order
// and the formulas of the shuffle tree below (equal counts: Chan's factor is
// the constant n/2, the 1/n scalings powers of two), so the partials are the
// same bits, without its 34 dependent lane shuffles and per-merge divisions.
__device__ __forceinline__ void x3_chan_merge(float& s, float& q, float s2, float q2, float inv_n, float f) {
    const float d = s2 * inv_n - s * inv_n;
    s = s + s2;
    q = (q + q2) + d * d * f;
}

template <int BN, int NI, int NJ, int CW, int SHF, int WMP = 4, typename Vec, typename Row, typename Sc>
__device__ __forceinline__ void x3_bn_partials_w(const X3Args& a, float* red, int m0, int n0, int wm, int wn,
                                                 int lane, Vec&& vec, Row&& row, Sc&& sc_of,
                                                 float* wide = nullptr) {
    constexpr int WROWS = 16 * NI;                                   // rows per wave
    if constexpr (CW == 16 && SHF == 16 && WMP == 4 && (NI == 4 || NI == 3)) {
        if (wide != nullptr && m0 + 4 * WROWS <= a.M) {              // block-uniform
            const int q = lane >> 4, r16 = lane & 15;
            constexpr float inv = 1.f / (NI * 4);
            float ls[NJ], lq[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                f32x4 s4 = vec(0, j);
#pragma unroll
                for (int i = 1; i < NI; ++i) s4 += vec(i, j);
                const float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
                const f32x4 mu = {s * inv, s * inv, s * inv, s * inv};
                f32x4 q4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    const f32x4 d = vec(i, j) - mu;
                    q4 += d * d;
                }
                ls[j] = s;
                lq[j] = (q4[0] + q4[1]) + (q4[2] + q4[3]);
            }
            lds_sync();                                              // the scratch is free
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int c = wn * NJ * CW + j * CW + r16;
                wide[(wm * 4 + q) * BN + c] = ls[j];
                wide[16 * BN + (wm * 4 + q) * BN + c] = lq[j];
                if (wm == 0 && q == 0) wide[32 * BN + c] = sc_of(j);
            }
            lds_sync();
            for (int t = threadIdx.x; t < 2 * BN; t += blockDim.x) {
                const int h = t / BN, c = t - h * BN;
                float S[2], Q[2];
#pragma unroll
                for (int v = 0; v < 2; ++v) {
                    const int w4 = (2 * h + v) * 4;
                    float s[4], qq[4];
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        s[g] = wide[(w4 + g) * BN + c];
                        qq[g] = wide[16 * BN + (w4 + g) * BN + c];
                    }
                    // groups of n1 = 4 * NI rows: Chan's factor n_a n_b / n = n1 / 2, ...
                    constexpr float n1 = 4.f * NI;
                    x3_chan_merge(s[0], qq[0], s[1], qq[1], 1.f / n1, n1 / 2);   // lane pairs l, l ^ 16
                    x3_chan_merge(s[2], qq[2], s[3], qq[3], 1.f / n1, n1 / 2);
                    x3_chan_merge(s[0], qq[0], s[2], qq[2], 1.f / (2 * n1), n1); // then l, l ^ 32
                    S[v] = s[0];
                    Q[v] = qq[0];
                }
                x3_chan_merge(S[0], Q[0], S[1], Q[1], 1.f / (16 * NI), 8.f * NI);   // even wave, odd wave
                const float sc = wide[32 * BN + c];
                const long tile128 = (long)a.part_base + (m0 - a.m_base) / (2 * WROWS) + h;
                a.part[(tile128 * a.K + n0 + c) * 2 + 0] = S[0] * sc;
                a.part[(tile128 * a.K + n0 + c) * 2 + 1] = Q[0] * (sc * sc);
            }
            return;
        }
    }
    float* rs = red;                                                 // [WM][BN] wave sums
    float* rq = red + 4 * BN;                                        // [WM][BN] wave M2
    const int nw = min(WROWS, max(0, a.M - (m0 + WROWS * wm)));    // valid rows of this wave (a prefix)
    float ls[NJ], lq[NJ], ln;
    if (nw == WROWS) {                                               // every row valid: no masks
        ln = (float)(NI * 4);
        constexpr float inv = 1.f / (NI * 4);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            f32x4 s4 = vec(0, j);
#pragma unroll
            for (int i = 1; i < NI; ++i) s4 += vec(i, j);
            const float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
            const f32x4 mu = {s * inv, s * inv, s * inv, s * inv};
            f32x4 q4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const f32x4 d = vec(i, j) - mu;
                q4 += d * d;
            }
            ls[j] = s;
            lq[j] = (q4[0] + q4[1]) + (q4[2] + q4[3]);
        }
    } else {
        ln = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) ln += (row(i, r) < a.M) ? 1.f : 0.f;
        const float linv = ln > 0.f ? 1.f / ln : 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) s += (row(i, r) < a.M) ? vec(i, j)[r] : 0.f;
            const float mu = s * linv;
            float q = 0.f;
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float d = vec(i, j)[r] - mu;
                    q += (row(i, r) < a.M) ? d * d : 0.f;
                }
            ls[j] = s;
            lq[j] = q;
        }
    }
    // pairwise Chan merge across the lane groups of a column (counts ride along)
    for (int o = SHF; o < 64; o <<= 1) {
        const float nb = __shfl_xor(ln, o);
        const float nt = ln + nb;
        const float f = nt > 0.f ? ln * nb / nt : 0.f;
        const float ia = ln > 0.f ? 1.f / ln : 0.f, ib = nb > 0.f ? 1.f / nb : 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const float sb = __shfl_xor(ls[j], o), qb = __shfl_xor(lq[j], o);
            const float d = sb * ib - ls[j] * ia;
            ls[j] = ls[j] + sb;
            lq[j] = (lq[j] + qb) + d * d * f;
        }
        ln = nt;
    }
    if constexpr (WMP == 2) {              // 2 waves in M (160-row tiles): a wave IS a partial tile
        if (nw == 0 || lane >= CW) return;
        const long pt = (long)a.part_base + (m0 - a.m_base) / WROWS + wm;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = wn * NJ * CW + j * CW + lane;
            const float sc = sc_of(j);
            a.part[(pt * a.K + n0 + c) * 2 + 0] = ls[j] * sc;
            a.part[(pt * a.K + n0 + c) * 2 + 1] = lq[j] * (sc * sc);
        }
        return;
    }
    if (lane < CW) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = wn * NJ * CW + j * CW + lane;
            rs[wm * BN + c] = ls[j];
            rq[wm * BN + c] = lq[j];
        }
    }
    lds_sync();
    const int nb = min(WROWS, max(0, a.M - (m0 + WROWS * (wm | 1))));   // valid rows of the odd wave of the half
    if ((wm & 1) || nw == 0 || lane >= CW) return;
    const long tile128 = (long)a.part_base + (m0 - a.m_base) / (2 * WROWS) + (wm >> 1);
    const float ia = 1.f / (float)nw, ib = nb > 0 ? 1.f / (float)nb : 0.f;
    const float f = (float)nw * (float)nb / (float)(nw + nb);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = wn * NJ * CW + j * CW + lane;
        const float sa = rs[wm * BN + c], qa = rq[wm * BN + c];
        const float sb = rs[(wm + 1) * BN + c], qb = rq[(wm + 1) * BN + c];
        const float d = sb * ib - sa * ia;
        const float sum = nb > 0 ? sa + sb : sa;
        const float m2 = nb > 0 ? (qa + qb) + d * d * f : qa;
        const float sc = sc_of(j);
        a.part[(tile128 * a.K + n0 + c) * 2 + 0] = sum * sc;
        a.part[(tile128 * a.K + n0 + c) * 2 + 1] = m2 * (sc * sc);
    }
}

// fp16 output tile staged in LDS ([256][BN + 8] halves: the 16-B row pad makes
// the fragment-layout ds_write_b16s conflict-free) and written as whole 16-B
// row chunks: 8x fewer store instructions than per-element fp16 stores, full
// 128-B lines — the epilogue of the short-K 1x1 convs of config C4 is most of
// their time.
template <int BN>
__device__ __forceinline__ void x3_store_tile_f16(const X3Args& a, const char* smem, int m0, int n0, int tid) {
    constexpr int CH = BN / 8, PITCH = BN + 8;
#pragma unroll 4
    for (int e = tid; e < 256 * CH; e += 512) {
        const int row = e / CH, cc = e - row * CH;
        const int m = m0 + row;
        if (m < a.M)
            x3_st16((uint4*)(a.y16 + (long)m * a.K + n0 + cc * 8), *(const uint4*)(smem + (row * PITCH + cc * 8) * 2), a.st_kind, 1);
    }
}

// BN-apply epilogue of the fp16 tile (hkp_conv2d_fwd_f16_bn): the staged fp16 y
// chunk, x scale + shift, + the residual chunk (raw or scaled + shifted), ReLU —
// bn_apply_f16's arithmetic on the same fp16 y, so the fused path returns what
// conv + hkp_bn_apply_f16 would with the same scale/shift.  ssl: LDS [4][BN]
// (scale, shift, residual scale, residual shift of the tile's columns).  A
// thread always handles the same 8 channels (512 % (BN/8) == 0).
template <int BN>
struct X3Res {
    static constexpr int NPT = 256 * (BN / 8) / 512;     // 16-B chunks per thread
    f16x8 r[NPT];
};
// the residual chunks this thread's store loop will use, loaded before the tile
// is staged (the loads of a whole tile in flight at once: a per-chunk load in
// the store loop exposed its HBM latency ~4 times per tile)
template <int BN>
__device__ __forceinline__ X3Res<BN> x3_ep_res_load(const X3Args& a, int m0, int n0, int tid) {
    constexpr int CH = BN / 8;
    X3Res<BN> res;
    const int cc = tid % CH;
#pragma unroll
    for (int u = 0; u < X3Res<BN>::NPT; ++u) {
        const int row = (tid + 512 * u) / CH, m = m0 + row;
        res.r[u] = f16x8{};
        if (a.ep_res && m < a.M)
            res.r[u] = __builtin_nontemporal_load((const f16x8*)(a.ep_res + (long)m * a.K + n0 + cc * 8));
    }
    return res;
}

template <int BN>
__device__ __forceinline__ void x3_store_tile_f16_bn(const X3Args& a, const char* smem, const float* ssl,
                                                     const X3Res<BN>& res, int m0, int n0, int tid) {
    constexpr int CH = BN / 8, PITCH = BN + 8;
    static_assert(512 % CH == 0, "fixed channels per thread");
    const int cc = tid % CH;
    float sa[8], sb[8], ra[8], rb[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        sa[e] = ssl[cc * 8 + e];
        sb[e] = ssl[BN + cc * 8 + e];
        ra[e] = ssl[2 * BN + cc * 8 + e];
        rb[e] = ssl[3 * BN + cc * 8 + e];
    }
    const bool hres = a.ep_res != nullptr, rsc = a.ep_rss != nullptr, relu = a.ep_relu != 0;
#pragma unroll
    for (int u = 0; u < X3Res<BN>::NPT; ++u) {
        const int row = (tid + 512 * u) / CH;
        const int m = m0 + row;
        if (m >= a.M) continue;
        const long off = (long)m * a.K + n0 + cc * 8;
        const f16x8 v = *(const f16x8*)(smem + (row * PITCH + cc * 8) * 2);
        const f16x8 r = res.r[u];
        f16x8 h;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float o = __fadd_rn(__fmul_rn((float)v[k], sa[k]), sb[k]);
            if (hres) o = rsc ? __fadd_rn(o, __fadd_rn(__fmul_rn((float)r[k], ra[k]), rb[k])) : __fadd_rn(o, (float)r[k]);
            if (relu) o = o > 0.f ? o : 0.f;
            h[k] = (_Float16)o;
        }
        x3_st16((f16x8*)(a.y16 + off), h, a.st_kind, 2);
    }
}

// the fused epilogue's per-column parameters: thread tid < 2*BN holds scale (tid
// < BN) or shift of column tid % BN, and the residual's; loaded before the tile
// is staged (their latency hides behind it), written to LDS after
struct X3EpSS {
    float v0 = 0.f, v1 = 0.f;
};
template <int BN>
__device__ __forceinline__ X3EpSS x3_ep_load(const X3Args& a, int n0, int tid) {
    X3EpSS r;
    if (a.ep_ss && tid < 2 * BN) {
        const int h = tid / BN, c = tid - h * BN;
        r.v0 = a.ep_ss[h * a.K + n0 + c];
        r.v1 = a.ep_rss ? a.ep_rss[h * a.K + n0 + c] : 0.f;
    }
    return r;
}
template <int BN>
__device__ __forceinline__ void x3_ep_store(float* ssl, const X3EpSS& r, int tid) {
    if (tid < 2 * BN) {
        ssl[tid] = r.v0;
        ssl[2 * BN + tid] = r.v1;
    }
}

// Mainloop + epilogue of the 16x16x32-MFMA bodies: one k32 step per half of a
// 128-B stage row (LDS ring, DMA issue and the swizzled rows exactly as the
// 32x32 path).  Wave tile 64 x BN/2 = UM x UN 16x16 tiles.
// Fragment read: lane reads row (lane & 15) of a 16-row tile, 16-B chunk
// (lane >> 4) (first half) / 4 + (lane >> 4) (second half): with the
// (row >> 1) & 7 chunk swizzle every ds_read_b128 lane group covers the 64 banks
// once.  Output fragment: lane holds column (lane & 15), rows 4 * (lane >> 4) + 0..3.
// Pipeline per K-step t (NST 3): [issue DMA t+NST-1] wait own DMA of t+1 (+ this
// wave's reads of t), barrier, [read A frags of t+1] then per column block j:
// [MFMAs of t with B_j] [refill B_j with t+1's].  NST 2 (256x256; 256x64 pairs):
// A single-buffered, t+2's DMA issued right after the barrier into t's buffer.
template <int BN, int NST, int STAGE, int GL, int P, bool A3, int GA, int BM, typename Issue, typename IssueA,
          typename IssueB>
__device__ __forceinline__ void conv_x3_mf16_body(const X3Args& a, char* smem, int tile, int ks, int nks, bool partial,
                                                  int m0, int n0, int wm, int wn, int lane, int tid,
                                                  Issue& issue_next, IssueA& issue_a, IssueB& issue_b) {
    constexpr int WM = x3_wm(BM), WN = 8 / WM, ROW = 128;
    constexpr int UM = BM / (WM * 16), UN = BN / (WN * 16);
    constexpr int NMC = x3_nprod(P) * UM;           // MFMAs per column block per K-step
    static_assert(BM == 256 || (A3 && (BM == 192 || BM == 160) && P != 1),
                  "192- / 160-row tiles: the A3 body, packed operands");
    constexpr bool PAIRB = BN == 64 && NST == 2;    // the 256x64 two-blocks-per-CU tiles
    static_assert(!A3 || (BN == 256 && NST == 2) || (BN == 128 && BM == 160), "A3: 256-wide tiles (128: 160 rows)");
    // PAIRB and A3 have no LDS past the ring: the epilogue's scratch is the drained
    // ring and the column scales are loaded in the epilogue
    constexpr bool RINGSCR = PAIRB || A3;
    constexpr int RED_OFF = RINGSCR ? 0 : x3_lds_bytes(BN, PAIRB, P);
    constexpr int LDS_ALL = A3 ? x3_a3_lds(BM, BN) : x3_lds_bytes(BN, PAIRB, P) + x3_red_bytes(BN, PAIRB);
    float* const scl = (float*)(smem + RED_OFF + 2 * 4 * BN * 4);   // [BN] column scales (!RINGSCR)
    float sclv = 1.f;                              // issued before the fill, stored after it
    if constexpr (!RINGSCR) {
        if (tid < BN) sclv = (a.wscale ? a.wscale[n0 + tid] : 1.f) * (a.amax ? 1.f / pow2_scale_for(a.amax) : 1.f);
    }
    auto store_scl = [&]() {
        if constexpr (!RINGSCR) {
            if (tid < BN) scl[tid] = sclv;
        }
    };
    const int r16 = lane & 15, q = lane >> 4;
    const int sw = (r16 >> 1) & 7;                 // the DMA's swizzle of every row ≡ r16 (mod 16)
    const int fo_h = r16 * ROW + ((q ^ sw) << 4), fo_l = r16 * ROW + (((4 + q) ^ sw) << 4);
    // A3: A stages at [0, 3*BM*ROW), B stages past them, each its own ring
    const int a_base = (wm * UM * 16) * ROW, b_base = ((A3 ? 0 : BM) + wn * UN * 16) * ROW;

    f32x4 acc[UM][UN];
#pragma unroll
    for (int i = 0; i < UM; ++i)
#pragma unroll
        for (int j = 0; j < UN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    struct FA {
        f16x8 h[UM], l[UM];
    };
    f16x8 bh[UN], bl[UN];
    auto read_a = [&](FA& f, const char* st) {
#pragma unroll
        for (int i = 0; i < UM; ++i) {
            f.h[i] = *(const f16x8*)(st + a_base + i * 16 * ROW + fo_h);
            f.l[i] = *(const f16x8*)(st + a_base + i * 16 * ROW + fo_l);
        }
    };
    auto read_b = [&](int j, const char* st) {
        bh[j] = *(const f16x8*)(st + b_base + j * 16 * ROW + fo_h);
        bl[j] = *(const f16x8*)(st + b_base + j * 16 * ROW + fo_l);
    };
    auto mfma = [](const f16x8& x, const f16x8& y, const f32x4& c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(x, y, c, 0, 0, 0);
    };
    auto mma_col = [&](const FA& f, int j) {
#pragma unroll
        for (int i = 0; i < UM; ++i) x3_products<P>(acc[i][j], f.h[i], f.l[i], bh[j], bl[j], mfma);
    };

    // The next stage's DMA (GL pieces per wave) is issued inside the K-step's
    // MFMA stream, one piece per column block, instead of as a burst after the
    // barrier (a piece costs ~60 issue cycles, MI355X_MICROARCH.md; the burst
    // left every SIMD without an MFMA to issue right after each barrier).  The
    // last K-steps issue nothing (peeled: no branch inside the scheduled region).
    auto sched_kstep = [&](const bool dma) {
#pragma unroll
        for (int j = 0; j < UN; ++j) {
            __builtin_amdgcn_sched_group_barrier(0x008, NMC, 0);     // column j's MFMAs
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);       // refill B_j
            if (dma && j * ((GL + UN - 1) / UN) < GL)
                __builtin_amdgcn_sched_group_barrier(0x020, (GL + UN - 1) / UN, 0);   // DMA pieces
        }
    };
    // the same with NP DMA pieces in the step (A3: B only, or A and B)
    auto sched_kstep_n = [&](auto np) {
        constexpr int NP = decltype(np)::value;
#pragma unroll
        for (int j = 0; j < UN; ++j) {
            __builtin_amdgcn_sched_group_barrier(0x008, NMC, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            if (NP > 0 && j * ((NP + UN - 1) / UN) < NP)
                __builtin_amdgcn_sched_group_barrier(0x020, (NP + UN - 1) / UN, 0);
        }
    };
    if constexpr (A3) {
        // A3: the NST 2 schedule below with A one stage further ahead.  Issue order
        // per K-step t (after its barrier): B(t+2) into B's slot of t, then A(t+3)
        // into A's slot of t (both read into registers during step t-1); so at step
        // t's top, waiting until only A(t+2) is in flight (vmcnt GA) retires A(t+1)
        // and B(t+1).  Prologue order A0 B0 A1 B1 A2.
        constexpr int GB = GL - GA;
        const char* const bring = smem + 3 * BM * ROW;
        issue_a();
        issue_b();
        if (nks > 1) {
            issue_a();
            issue_b();
        }
        if (nks > 2) issue_a();
        if (nks > 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GL + GA) : "memory");
        else if (nks > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GL) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        lds_barrier();
        x3_stamp(a, 1);
        const int wv = wm * 2 + wn;
        if (a.prio == 1 && wv >= 4) __builtin_amdgcn_s_setprio(1);
        if (a.prio == 2 && wv < 4) __builtin_amdgcn_s_setprio(1);
        FA fa;
        read_a(fa, smem);
#pragma unroll
        for (int j = 0; j < UN; ++j) read_b(j, bring);
        int ca = 0, cb = 0;
        // one K-step: NP DMA pieces issued (GL: B(t+2) and A(t+3); GB: B only; 0),
        // WA: A(t+2) may stay in flight at the top
        auto kstep = [&](auto np, auto wa) {
            constexpr int NP = decltype(np)::value;
            if constexpr (decltype(wa)::value) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(GA) : "memory");
            else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            lds_barrier();
            ca = ca == 2 ? 0 : ca + 1;
            cb ^= 1;
            const char* sta = smem + ca * (BM * ROW);
            const char* stb = bring + cb * (BN * ROW);
            if constexpr (NP > 0) issue_b();
            if constexpr (NP == GL) issue_a();
#pragma unroll
            for (int j = 0; j < UN; ++j) {
                mma_col(fa, j);
                read_b(j, stb);
            }
            read_a(fa, sta);
            sched_kstep_n(np);
            __builtin_amdgcn_sched_group_barrier(0x100, 2 * UM, 0);      // next A frags
            __builtin_amdgcn_sched_barrier(0);
        };
        using IGL = std::integral_constant<int, GL>;
        using IGB = std::integral_constant<int, GB>;
        using I0 = std::integral_constant<int, 0>;
        int t = 0;
        for (; t + 3 < nks; ++t) kstep(IGL{}, std::true_type{});
        if (t + 2 < nks) {
            kstep(IGB{}, std::true_type{});
            ++t;
        }
        if (t + 1 < nks) kstep(I0{}, std::false_type{});
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int j = 0; j < UN; ++j) mma_col(fa, j);
        if (a.prio) __builtin_amdgcn_s_setprio(0);
    } else if constexpr (NST == 2) {
        // 2-stage ring (256x256 tiles; 256x64 at two blocks per CU), A single-buffered
        // (registers: 128 acc + 32 A + 64 B): per K-step t — wait own DMA of t+1,
        // barrier, then per column j [MFMAs of t with B_j] [refill B_j with t+1's]
        // [a DMA piece of t+2 into t's buffer, read before the barrier], then A of
        // t+1 (its latency covered by the SIMD's other wave)
        issue_next();
        if (nks > 1) issue_next();
        store_scl();
        if (nks > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GL) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        lds_barrier();
        x3_stamp(a, 1);
        FA fa;
        read_a(fa, smem);
#pragma unroll
        for (int j = 0; j < UN; ++j) read_b(j, smem);
        int cur = 0;
        auto kstep = [&](const bool dma) {
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            lds_barrier();
            cur ^= 1;
            const char* st = smem + cur * STAGE;
            if (dma) issue_next();
#pragma unroll
            for (int j = 0; j < UN; ++j) {
                mma_col(fa, j);
                read_b(j, st);
            }
            read_a(fa, st);
            sched_kstep(dma);
            __builtin_amdgcn_sched_group_barrier(0x100, 2 * UM, 0);      // next A frags
            __builtin_amdgcn_sched_barrier(0);
        };
        int t = 0;
        for (; t + 2 < nks; ++t) kstep(true);
        if (t + 1 < nks) kstep(false);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int j = 0; j < UN; ++j) mma_col(fa, j);
    } else {
        // 3-stage ring (256x128 tiles), the 2-stage body's schedule with two
        // stages of DMA lead: A single-buffered, per K-step t — wait own DMA of
        // t+1 (t+2 stays in flight), barrier, then per column j [MFMAs of t with
        // B_j] [refill B_j with t+1's] [a DMA piece of t+3 into t's buffer: t's
        // fragments were all read during step t-1], then A of t+1.  (The burst
        // of t+2's DMA before the barrier, with A double-buffered, left every SIMD
        // without an MFMA to issue after each barrier.)
        static_assert(NST == 3, "stage t+3 goes into stage t's buffer");
        for (int s = 0; s < NST; ++s)
            if (s < nks) issue_next();
        store_scl();
        {
            const int after = std::min(nks, NST) - 1;         // stages in flight past stage 0
            if (after >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * GL) : "memory");
            else if (after == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GL) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        lds_barrier();
        x3_stamp(a, 1);
        FA fa;
        read_a(fa, smem);
#pragma unroll
        for (int j = 0; j < UN; ++j) read_b(j, smem);
        int cur = 0;
        auto kstep = [&](const int t, const bool dma) {
            if (t + 2 < nks) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(GL) : "memory");
            else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            lds_barrier();
            cur = cur == NST - 1 ? 0 : cur + 1;
            const char* st = smem + cur * STAGE;
            if (dma) issue_next();
#pragma unroll
            for (int j = 0; j < UN; ++j) {
                mma_col(fa, j);
                read_b(j, st);
            }
            read_a(fa, st);
            sched_kstep(dma);
            __builtin_amdgcn_sched_group_barrier(0x100, 2 * UM, 0);      // next A frags
            __builtin_amdgcn_sched_barrier(0);
        };
        int t = 0;
        for (; t + 3 < nks; ++t) kstep(t, true);
        for (; t + 1 < nks; ++t) kstep(t, false);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int j = 0; j < UN; ++j) mma_col(fa, j);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // no DMA in flight into the ring past here
    x3_stamp(a, 2);

    if constexpr (BM == 256) {             // (the 192- / 160-row grids run whole tiles)
        if (partial) {                     // stream-K: fold the tile's segments
            auto get = [&](int v) -> f32x4 { return acc[v / UN][v % UN]; };
            auto set = [&](int v, f32x4 y) { acc[v / UN][v % UN] = y; };
            if (!sk_combine<UM * UN>(a, tile, tid, smem, get, set)) return;
        }
    }
    const int rbase = m0 + wm * UM * 16 + 4 * q;
    // column scale (weight scale x gradient scale): the prefetched LDS copy, or
    // (PAIRB, A3) loaded now
    auto col_scale = [&](int c) -> float {
        if constexpr (RINGSCR) return (a.wscale ? a.wscale[n0 + c] : 1.f) * (a.amax ? 1.f / pow2_scale_for(a.amax) : 1.f);
        else return scl[c];
    };
    if constexpr (P == 1) {                // fp16 output: partials, scale, LDS-staged store
        float sc[UN];
#pragma unroll
        for (int j = 0; j < UN; ++j) sc[j] = col_scale(wn * UN * 16 + j * 16 + r16);
        if (a.part) {
            if constexpr (RINGSCR) lds_sync();         // the scratch is the ring
            x3_bn_partials_w<BN, UM, UN, 16, 16, WM>(
                a, (float*)(smem + RED_OFF), m0, n0, wm, wn, lane, [&](int i, int j) { return acc[i][j]; },
                [&](int i, int r) { return rbase + i * 16 + r; }, [&](int j) { return sc[j]; }, (float*)smem);
        }
        const X3EpSS eps = x3_ep_load<BN>(a, n0, tid);
        X3Res<BN> eres;
        if (a.ep_ss) eres = x3_ep_res_load<BN>(a, m0, n0, tid);
        lds_sync();                        // the ring is free
        x3_stamp(a, 3);
        _Float16* t = (_Float16*)smem;
        constexpr int PITCH = BN + 8;
        constexpr int SS_OFF = 256 * PITCH * 2;
        static_assert(SS_OFF + 4 * BN * 4 <= LDS_ALL, "epilogue LDS");
#pragma unroll
        for (int i = 0; i < UM; ++i)
#pragma unroll
            for (int j = 0; j < UN; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    t[(wm * UM * 16 + i * 16 + 4 * q + r) * PITCH + wn * UN * 16 + j * 16 + r16] =
                        (_Float16)(acc[i][j][r] * sc[j]);
        if (a.ep_ss) x3_ep_store<BN>((float*)(smem + SS_OFF), eps, tid);
        lds_sync();
        x3_stamp(a, 4);
        if (a.ep_ss) x3_store_tile_f16_bn<BN>(a, smem, (const float*)(smem + SS_OFF), eres, m0, n0, tid);
        else x3_store_tile_f16<BN>(a, smem, m0, n0, tid);
        x3_stamp(a, 5);
        return;
    }
    // ---- epilogue (fp32 output): BN partials, then the scaled tile ----
    float sc[UN];
#pragma unroll
    for (int j = 0; j < UN; ++j) sc[j] = col_scale(wn * UN * 16 + j * 16 + r16);
    if (a.part) {
        if constexpr (RINGSCR) lds_sync();             // the scratch is the ring
        x3_bn_partials_w<BN, UM, UN, 16, 16, WM>(
            a, (float*)(smem + RED_OFF), m0, n0, wm, wn, lane, [&](int i, int j) { return acc[i][j]; },
            [&](int i, int r) { return rbase + i * 16 + r; }, [&](int j) { return sc[j]; }, (float*)smem);
    }
    x3_stamp(a, 3);
    {
        // The output tile is staged through the (drained) ring as fp32 rows and
        // written as whole 16-B row chunks — 32 store instructions per thread,
        // full 128-B lines (a phase output row of the strided dgrad is still 4
        // contiguous channels per chunk; the addend is read the same way).  The
        // fragment-layout stores (128 4-B stores per thread, 64-B pieces) of
        // every CU at once took ~34 us per C2 layer4 tile (10 %): more than a
        // wave's 63 outstanding memory ops, so the waves stalled on their
        // completion instead of ending and letting the next block start.
        // 256-wide tiles stage half the rows per pass (128 KiB).
        constexpr int PASSES = BN == 256 ? 2 : 1, RPP = BM / PASSES, PITCH = BN + 4, C4 = BN / 4;
        static_assert(RPP * PITCH * 4 <= LDS_ALL, "staging");
        float* t = (float*)smem;
        lds_sync();                                    // every wave done with the ring and the partials' scratch
#pragma unroll
        for (int h = 0; h < PASSES; ++h) {
            if (PASSES == 1 || (wm * UM * 16) / RPP == h) {          // the pass holding this wave's rows
#pragma unroll
                for (int i = 0; i < UM; ++i)
#pragma unroll
                    for (int j = 0; j < UN; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            t[(wm * UM * 16 + i * 16 + 4 * q + r - h * RPP) * PITCH + wn * UN * 16 + j * 16 + r16] =
                                acc[i][j][r] * sc[j];
            }
            lds_sync();
            if (!a.add && !a.ost) {
#pragma unroll 4
                for (int e = tid; e < RPP * C4; e += 512) {
                    const int row = e / C4, c4 = e - row * C4;
                    const int m = m0 + h * RPP + row;
                    if (m < a.M)
                        // nontemporal (in-process A/B, profiles/r05_store_ab.log: C2 1825.7 ->
                        // 1841.1 img/s; C3 training 464.6 both)
                        x3_st16((f32x4*)(a.y + (long)m * a.K + n0 + c4 * 4), *(const f32x4*)(t + row * PITCH + c4 * 4),
                                a.st_kind, 2);
                }
            } else {
#pragma unroll 2
                for (int e = tid; e < RPP * C4; e += 512) {
                    const int row = e / C4, c4 = e - row * C4;
                    const long off = x3_out_off(a, m0 + h * RPP + row, n0 + c4 * 4);
                    if (off >= 0) {
                        f32x4 v = *(const f32x4*)(t + row * PITCH + c4 * 4);
                        if (a.add) {
                            const f32x4 ad = *(const f32x4*)(a.add + off);
#pragma unroll
                            for (int k = 0; k < 4; ++k) v[k] = v[k] + ad[k];
                        }
                        *(f32x4*)(a.y + off) = v;
                    }
                }
            }
            if (h + 1 < PASSES) lds_sync();            // the next pass overwrites the rows just read
        }
    }
    x3_stamp(a, 4);
    x3_stamp(a, 5);
}

// STEM: the 7x7/s2 stem on the zero-padded NHWC4 image planes of
// hkp_stem_pack_x3 (a.H/a.W = padded size, stride 2, pad 0, R = 7, S = 1: one
// K-step per filter row = 8 taps x 4 channels; logical chunk j of a row holds
// padded pixels 2wo+2j, 2wo+2j+1 from the hi plane (j < 4) or the lo plane).
// MFD: MFMA shape, 32 = v_mfma_f32_32x32x16_f16 (two k16 slices per 128-B
// stage), 16 = v_mfma_f32_16x16x32_f16 (one k32 step per stage half; same cycles
// per FLOP, lower power per FLOP, so the chip holds a higher clock under load —
// MI355X_MICROARCH.md "DVFS give-back" item 7).
// P: operand layout and products (x3_products) — 3 packed f16x3 split, 2 / 4
// packed split with two of its three products, 1 plain fp16.
template <int BN, bool STEM, bool PAIR, int MFD, int P, bool A3 = false, int BM = 256>
__device__ __forceinline__ void conv_x3_tile(const X3Args& a, char* smem, int tile, int ks, int nks, bool partial) {
    constexpr int WM = x3_wm(BM), WN = 8 / WM;
    constexpr int TM = BM / (WM * 32), TN = BN / (WN * 32);
    constexpr int ROW = 128;                       // bytes per LDS row (one packed line)
    constexpr int CPR = ROW / 16;                  // 16-B chunks per row
    constexpr int RPI = 1024 / ROW;                // rows per DMA wave-instruction
    constexpr int NST = x3_nst(BN, PAIR);          // LDS ring depth
    constexpr int STAGE = (BM + BN) * ROW;
    constexpr int GA = (BM / RPI + 7) / 8;         // A DMA instructions per wave per stage (rounded up)
    constexpr bool A_SINK = BM / RPI % 8 != 0;    // pieces past row BM load the zero line into a sink
    constexpr int GBT = BN / RPI;                  // B DMA instructions per stage (all waves)
    constexpr int GB = GBT >= 8 ? GBT / 8 : 1;     // per wave (GBT < 8: waves duplicate, same bytes)
    constexpr int GL = GA + GB;                    // DMA instructions per wave per stage
    static_assert(MFD == 16 || MFD == 32, "bad conv_x3 MFMA shape");
    static_assert(P == 3 || ((P == 1 || P == 2 || P == 4) && !STEM), "bad conv_x3 operand layout");
    static_assert(!(MFD == 32 && BN == 256), "256x256 tiles run the 16x16x32 body");
    static_assert(NST * STAGE <= 160 * 1024, "LDS");
    static_assert(!A3 || ((BN == 256 || (BN == 128 && BM == 160)) && !STEM && !PAIR && MFD == 16),
                  "A3: the 16x16x32 body on 256-wide tiles (128-wide: 160 rows)");
    static_assert(BM == 256 || (A3 && (BM == 192 || BM == 160) && x3_packed(P)), "192- / 160-row tiles: A3, packed");
    static_assert(!A_SINK || A3, "the A sink is the A3 body's");

    const int mt = tile / a.n_tiles, nt = tile - mt * a.n_tiles;
    const int m0 = a.m_base + (mt + a.mt0) * BM, n0 = nt * BN;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = w / WN, wn = w % WN;

    // swizzled physical chunk of a logical chunk in row r
    auto swz = [](int row) { return (row >> 1) & 7; };
    // halves offset, inside a packed line, of logical chunk L
    auto lofs = [&](int L) -> long {
        if constexpr (STEM) return (L >> 2) * a.plane + (L & 3) * 8;
        else return L * 8;
    };

    // ---- DMA source bookkeeping (rows this lane feeds) ----
    // Per row: the image-space origin (hb, wb) of its receptive field packed as
    // two int16, and the unsigned 32-bit element offset of that (possibly
    // padded-out) origin pixel from xbase = a.xs - pad*(W+1)*cstride (the
    // furthest a padded-out origin reaches before a.xs); a tap adds a
    // wave-uniform offset.  Rows past M get an origin that is never in-bounds.  B
    // rows: 32-bit offsets from a.ws.  (64-bit pointers here pushed the 256x256
    // kernels past 256 VGPRs; the spill reload inside the DMA issue waited
    // vmcnt(0) on every K-step.  The host checks the operand sizes fit.)
    const int cstride = STEM ? 4 : a.cch * 64;     // halves per pixel
    const long xbias = (long)a.pad * (a.W + 1) * cstride;
    const _Float16* xbase = a.xs - xbias;
    int a_org[GA];
    unsigned a_off[GA];
#pragma unroll
    for (int i = 0; i < GA; ++i) {
        const int row = RPI * (w * GA + i) + lane / CPR;
        const int Lc = (lane % CPR) ^ swz(row);
        const long L = lofs(Lc);
#ifdef HKP_AB_KNOBS
        const int m = a.a_wrap ? (m0 + row) % a.a_wrap : m0 + row;
#else
        const int m = m0 + row;
#endif
        int hb = -16384, wb = -16384;
        long off = 0;
        if (m < a.M && (!A_SINK || RPI * (w * GA + i) < BM)) {
            const int hw = a.Ho * a.Wo;
            const int n = m / hw, rem = m - n * hw;
            const int ho = rem / a.Wo, wo = rem - ho * a.Wo;
            hb = ho * a.stride - a.pad;
            wb = wo * a.stride - a.pad;
            off = (((long)n * a.H + hb) * a.W + wb) * cstride + L;
        }
        a_org[i] = (int)(((unsigned)hb << 16) | ((unsigned)wb & 0xFFFFu));
        a_off[i] = (unsigned)(off + xbias);
    }
    const int bline = a.RS * a.cch * 64;           // halves per weight row (output channel)
    int b_off[GB], b_dst[GB];
#pragma unroll
    for (int j = 0; j < GB; ++j) {
        const int bi = (w * GB + j) % GBT;
        const int row = RPI * bi + lane / CPR;
        const int Lc = (lane % CPR) ^ swz(row);
        b_off[j] = (n0 + row) * bline + (STEM ? Lc * 8 : (int)lofs(Lc));
        b_dst[j] = (BM + RPI * bi) * ROW;
    }
    const _Float16* zero = (const _Float16*)g_x3_zero_line;

    // staging state of the next K-step to issue (wave-uniform, advanced per issue)
    // (a stream-K segment starts at K-step ks: channel group outer, tap inner)
    int q_buf = 0;
    int q_cc = ks / a.RS;
    int q_tap = ks - q_cc * a.RS;
    int q_rr = q_tap / a.S, q_ss = q_tap - q_rr * a.S;
    auto issue_next = [&]() {
        char* st = smem + q_buf * STAGE;
        const int dh = q_rr * a.dil, dw = q_ss * a.dil;
        const long toff = ((long)dh * a.W + dw) * cstride + q_cc * 64;
#pragma unroll
        for (int i = 0; i < GA; ++i) {
            const int hb = a_org[i] >> 16, wb = (int)(short)(a_org[i] & 0xFFFF);
            const bool in = (unsigned)(hb + dh) < (unsigned)a.H && (unsigned)(wb + dw) < (unsigned)a.W;
            glds16(in ? xbase + ((unsigned long)a_off[i] + toff) : zero, st + (RPI * (w * GA + i)) * ROW);
        }
        const int boff = (q_tap * a.cch + q_cc) * 64;
#pragma unroll
        for (int j = 0; j < GB; ++j) glds16(a.ws + (unsigned)(b_off[j] + boff), st + b_dst[j]);
        q_buf = q_buf == NST - 1 ? 0 : q_buf + 1;
        if (++q_ss == a.S) {
            q_ss = 0;
            ++q_rr;
        }
        if (++q_tap == a.RS) {
            q_tap = 0;
            q_rr = 0;
            ++q_cc;
        }
    };

    // A3: A and B stages in rings of their own (3 and 2 deep), A issued one K-step
    // ahead of B — each with its own (channel group, tap) position
    int qa_buf = 0, qa_cc = q_cc, qa_tap = q_tap, qa_rr = q_rr, qa_ss = q_ss;
    int qb_buf = 0, qb_cc = q_cc, qb_tap = q_tap;
    // issue_a(): the next A stage, then the advance to the stage after it
    auto issue_a = [&]() {
        {
            char* st = smem + qa_buf * (BM * ROW);
            const int dh = qa_rr * a.dil, dw = qa_ss * a.dil;
            const long toff = ((long)dh * a.W + dw) * cstride + qa_cc * 64;
#pragma unroll
            for (int i = 0; i < GA; ++i) {
                const int hb = a_org[i] >> 16, wb = (int)(short)(a_org[i] & 0xFFFF);
                const bool in = (unsigned)(hb + dh) < (unsigned)a.H && (unsigned)(wb + dw) < (unsigned)a.W;
                const int prow = RPI * (w * GA + i);
                char* dst = st + prow * ROW;
                if constexpr (A_SINK) dst = prow < BM ? dst : smem + (3 * BM + 2 * BN) * ROW;   // wave-uniform
                glds16(in ? xbase + ((unsigned long)a_off[i] + toff) : zero, dst);
            }
        }
        qa_buf = qa_buf == 2 ? 0 : qa_buf + 1;
        if (++qa_ss == a.S) {
            qa_ss = 0;
            ++qa_rr;
        }
        if (++qa_tap == a.RS) {
            qa_tap = 0;
            qa_rr = 0;
            ++qa_cc;
        }
    };
    auto issue_b = [&]() {
        char* st = smem + 3 * (BM * ROW) + qb_buf * (BN * ROW) - BM * ROW;   // b_dst counts from row BM
        const int boff = (qb_tap * a.cch + qb_cc) * 64;
#pragma unroll
        for (int j = 0; j < GB; ++j) glds16(a.ws + (unsigned)(b_off[j] + boff), st + b_dst[j]);
        qb_buf ^= 1;
        if (++qb_tap == a.RS) {
            qb_tap = 0;
            ++qb_cc;
        }
    };

    if constexpr (MFD == 16) {
        conv_x3_mf16_body<BN, NST, STAGE, GL, P, A3, GA, BM>(a, smem, tile, ks, nks, partial, m0, n0, wm, wn, lane,
                                                             tid, issue_next, issue_a, issue_b);
        return;
    } else {
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // fragment reads: lane reads row (lane&31) of each 32-row tile; logical chunk
    // of k16 slice u (of 2 per row half): 2u + kh (first half) / 4 + 2u + kh
    const int frow = lane & 31, kh = lane >> 5;
    int foff[2][2];
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
#pragma unroll
        for (int u = 0; u < 2; ++u) foff[pl][u] = frow * ROW + ((((CPR / 2) * pl + 2 * u + kh) ^ swz(frow)) << 4);
    const int a_base = (wm * TM * 32) * ROW, b_base = (BM + wn * TN * 32) * ROW;

    struct Frag {
        f16x8 ah[TM], al[TM], bh[TN], bl[TN];
    };
    auto read_frag = [&](Frag& f, const char* st, int u) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            f.ah[i] = *(const f16x8*)(st + a_base + i * 32 * ROW + foff[0][u]);
            f.al[i] = *(const f16x8*)(st + a_base + i * 32 * ROW + foff[1][u]);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            f.bh[j] = *(const f16x8*)(st + b_base + j * 32 * ROW + foff[0][u]);
            f.bl[j] = *(const f16x8*)(st + b_base + j * 32 * ROW + foff[1][u]);
        }
    };
    auto mfma = [](const f16x8& x, const f16x8& y, const f32x16& c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(x, y, c, 0, 0, 0);
    };
    auto mma = [&](const Frag& f) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) x3_products<P>(acc[i][j], f.ah[i], f.al[i], f.bh[j], f.bl[j], mfma);
    };
    constexpr int NR = 2 * (TM + TN), NM = x3_nprod(P) * TM * TN;   // ds_reads / MFMAs per k16 slice

    // prologue: NST-1 stages in flight, stage 0 landed everywhere
    issue_next();
    for (int s = 1; s < NST - 1; ++s)
        if (s < nks) issue_next();
    {
        const int after = std::min(nks - 1, NST - 2);   // stages issued after stage 0
        if (after >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GL) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    lds_barrier();
    Frag f0, f1;
    int cur = 0;
    read_frag(f0, smem, 0);

    // wait for this wave's DMA of stage t+1, given that the stages up to
    // min(nks-1, t+NST-1) have been issued; lgkmcnt(0) retires this wave's
    // fragment reads of the buffer the next DMA will overwrite
    auto wait_next = [&](int t) {
        const int after = std::min(nks - 1, t + NST - 1) - (t + 1);
        if (after >= 1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(GL) : "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    };

    // one barrier per K-step, placed between its two k16 halves:
    //   [issue DMA t+NST-1] [read frags u=1 of t] [MFMA u=0 of t]
    //   wait own DMA of t+1, barrier (t+1 landed everywhere; t-1 fully read)
    //   [read frags u=0 of t+1] [MFMA u=1 of t]
    // DMA t+NST-1 overwrites the buffer of t-1, whose reads retired before the
    // previous barrier.  Each half is one basic block so the ds_reads can be
    // interleaved one per MFMA gap.  The last K-step is peeled so the loop body
    // has no branch around the MFMAs (a join of two differently scheduled acc
    // writers costs a full accumulator copy).
    for (int t = 0; t + 1 < nks; ++t) {
        const char* st = smem + cur * STAGE;
        if (t + NST - 1 < nks) issue_next();
        read_frag(f1, st, 1);
        mma(f0);
        interleave<NM, NR>();
        __builtin_amdgcn_sched_barrier(0);       // every MFMA of this half ahead of the wait
        wait_next(t);
        lds_barrier();
        cur = cur == NST - 1 ? 0 : cur + 1;
        mma(f1);
        read_frag(f0, smem + cur * STAGE, 0);
        interleave<NM, NR>();
        __builtin_amdgcn_sched_barrier(0);
    }
    read_frag(f1, smem + cur * STAGE, 1);
    mma(f0);
    mma(f1);

    if (!STEM && partial) {                // stream-K: fold the tile's segments
        auto get = [&](int v) -> f32x4 {
            const f32x16& x = acc[(v >> 2) / TN][(v >> 2) % TN];
            const int q4 = (v & 3) * 4;
            return f32x4{x[q4], x[q4 + 1], x[q4 + 2], x[q4 + 3]};
        };
        auto set = [&](int v, f32x4 y) {
            f32x16& x = acc[(v >> 2) / TN][(v >> 2) % TN];
            const int q4 = (v & 3) * 4;
            x[q4] = y[0]; x[q4 + 1] = y[1]; x[q4 + 2] = y[2]; x[q4 + 3] = y[3];
        };
        if (!sk_combine<TM * TN * 4>(a, tile, tid, smem, get, set)) return;
    }
    const float ginv = a.amax ? 1.f / pow2_scale_for(a.amax) : 1.f;   // exact (power of two)
    const int rbase = m0 + wm * TM * 32 + 4 * kh;
    if constexpr (P == 1) {                // fp16 output: scale, partials, LDS-staged store
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const float sc = (a.wscale ? a.wscale[n0 + wn * TN * 32 + j * 32 + frow] : 1.f) * ginv;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] *= sc;
        }
        if (a.part)
            x3_bn_partials<BN, TM, TN, 16, 32, 32>(
                a, smem, m0, n0, wm, wn, lane, tid, [&](int i, int j, int r) { return acc[i][j][r]; },
                [&](int i, int r) { return rbase + i * 32 + (r & 3) + 8 * (r >> 2); });
        const X3EpSS eps = x3_ep_load<BN>(a, n0, tid);
        X3Res<BN> eres;
        if (a.ep_ss) eres = x3_ep_res_load<BN>(a, m0, n0, tid);
        __syncthreads();
        _Float16* t = (_Float16*)smem;
        constexpr int PITCH = BN + 8;
        constexpr int SS_OFF = 256 * PITCH * 2;
        static_assert(SS_OFF + 4 * BN * 4 <= x3_lds_bytes(BN, PAIR, P) + x3_red_bytes(BN, PAIR), "epilogue LDS");
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    t[(wm * TM * 32 + i * 32 + 4 * kh + (r & 3) + 8 * (r >> 2)) * PITCH + wn * TN * 32 + j * 32 +
                      frow] = (_Float16)acc[i][j][r];
        if (a.ep_ss) x3_ep_store<BN>((float*)(smem + SS_OFF), eps, tid);
        __syncthreads();
        if (a.ep_ss) x3_store_tile_f16_bn<BN>(a, smem, (const float*)(smem + SS_OFF), eres, m0, n0, tid);
        else x3_store_tile_f16<BN>(a, smem, m0, n0, tid);
        return;
    }

    // ---- epilogue: NHWC store (x scales, + addend) + BN partials per 128-row tile ----
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * TN * 32 + j * 32 + frow;
        const float sc = (a.wscale ? a.wscale[n] : 1.f) * ginv;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            // output offsets of the fragment's 16 rows (-1: past M), then all its
            // addend loads in flight at once (one exposed latency per fragment)
            long off[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) off[r] = x3_out_off(a, rbase + i * 32 + (r & 3) + 8 * (r >> 2), n);
            float av[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) av[r] = (a.add && off[r] >= 0) ? a.add[off[r]] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[i][j][r] *= sc;
                x3_store(a, off[r], acc[i][j][r], av[r]);
            }
        }
    }
    if (a.part == nullptr) return;
    x3_bn_partials<BN, TM, TN, 16, 32, 32>(
        a, smem, m0, n0, wm, wn, lane, tid, [&](int i, int j, int r) { return acc[i][j][r]; },
        [&](int i, int r) { return rbase + i * 32 + (r & 3) + 8 * (r >> 2); });
    }
}

// One tile per block (blocks remapped XCD-aware), or (SK) column-grouped
// stream-K: group g runs units [g*U/NG, (g+1)*U/NG) of the m-tile-major
// (m-tile, K-step) sequence, one tile segment after another (sk_combine).
// Separate instantiations (SK): the stream-K loop's live state would otherwise
// raise the register allocation of the one-tile kernels.  PAIR = two blocks per
// CU (256x64 tiles, the stem: 80 KiB each): one block's prologue / epilogue
// overlaps the other's main loop.
// the first-round stagger of X3Args (one wave-uniform wait at block start)
__device__ __forceinline__ void x3_stagger(const X3Args& a) {
    const int b = blockIdx.x;
    if (a.stagger_ticks > 0 && b < a.stagger_blocks && ((b >> 3) & 1)) {
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__builtin_amdgcn_s_memrealtime() - t0 < (unsigned long long)a.stagger_ticks) __builtin_amdgcn_s_sleep(2);
    }
}

template <int BN, bool STEM, bool PAIR, int MFD, bool SK, int P>
__global__ __launch_bounds__(512, PAIR ? 2 : 1) void conv_x3_kernel(X3Args a) {
    __shared__ __attribute__((aligned(1024))) char smem[x3_lds_bytes(BN, PAIR, P) + x3_red_bytes(BN, PAIR)];
    if constexpr (!SK) x3_stagger(a);
    x3_stamp(a, 0);
    const int G = gridDim.x, b = xcd_remap(blockIdx.x, G);
    if constexpr (!SK) {
        conv_x3_tile<BN, STEM, PAIR, MFD, P>(a, smem, b, 0, a.nks, false);
        return;
    }
    // column-grouped stream-K (sk_combine): group g = b / n_tiles, column tile b % n_tiles
    const int NT = a.n_tiles, NG = G / NT, g = b / NT, nt = b - g * NT;
    if (g >= NG) return;                   // grid is NG * n_tiles; never taken
    const long U = a.sk_units, u0 = sk_start(g, U, NG), u1 = sk_start(g + 1, U, NG);
    for (long u = u0; u < u1;) {
        const int mt = (int)(u / a.nks);
        const long t0 = (long)mt * a.nks;
        const int ks = (int)(u - t0), ke = (int)min((long)a.nks, u1 - t0);
        if (u != u0) __syncthreads();      // the previous segment is done with the LDS ring
        conv_x3_tile<BN, STEM, PAIR, MFD, P>(a, smem, mt * NT + nt, ks, ke - ks, ks != 0 || ke != a.nks);
        u = t0 + ke;
    }
}

// One 256x256 tile per block on the A3 body (3-stage A ring, 2-stage B ring);
// with a.main_blocks > 0 the blocks past it run the grid's split-K tail (the
// segments of conv_x3_tail_kernel) in the same launch: they are dispatched as the
// full rounds' tiles finish, without the second launch's gap — and, in training,
// ahead of a side-stream wgrad that would otherwise take the freed CUs first.
template <int P>
__device__ __forceinline__ void conv_x3_a3_grid(const X3Args& a, char* smem) {
    x3_stagger(a);
    x3_stamp(a, 0);
    const int b = blockIdx.x;
    if (a.tail_groups == 0 || b < a.main_blocks) {
        conv_x3_tile<256, false, false, 16, P, true>(
            a, smem, xcd_remap(b, a.tail_groups ? a.main_blocks : gridDim.x), 0, a.nks, false);
        return;
    }
    X3Args t = a;
    const int NT = a.n_tiles, G = a.tail_groups * NT;
    t.mt0 = a.tail_mt0;
    t.sk_units = a.tail_units;
    t.sk_grid = G;
    t.sk_b = xcd_remap(b - a.main_blocks, G);
    const int g = t.sk_b / NT, nt = t.sk_b - g * NT;
    const long U = t.sk_units, u0 = sk_start(g, U, a.tail_groups), u1 = sk_start(g + 1, U, a.tail_groups);
    const int mt = (int)(u0 / a.nks);
    const int ks = (int)(u0 - (long)mt * a.nks), ke = (int)(u1 - (long)mt * a.nks);
    conv_x3_tile<256, false, false, 16, P, true>(t, smem, mt * NT + nt, ks, ke - ks, true);
}

template <int P>
__global__ __launch_bounds__(512, 1) void conv_x3_a3_kernel(X3Args a) {
    __shared__ __attribute__((aligned(1024))) char smem[X3_A3_LDS];
    conv_x3_a3_grid<P>(a, smem);
}

// The A3 body on 192 x 256 tiles (HKP_TILE_192_A3, packed operands): a grid whose
// 256-row tiles leave most CUs idle in a single partial round — the B=8 shard's
// layer3, 150 m-tiles on 256 CUs — runs ceil(M / 192) blocks in the same one
// round, each 3/4 of a tile (200 m-tiles: 0.78 of the CUs instead of 0.59).
// Waves 4 x 2 as in A3 (48 x 128 each, 96 accumulators), the A ring 3 stages of
// 192 lines; BN partials per 96-row half tile (hkp_bn_finalize tile_rows 96).
template <int P>
__global__ __launch_bounds__(512, 1) void conv_x3_a3_192_kernel(X3Args a) {
    __shared__ __attribute__((aligned(1024))) char smem[x3_a3_lds(192)];
    x3_stamp(a, 0);
    conv_x3_tile<256, false, false, 16, P, true, 192>(a, smem, xcd_remap(blockIdx.x, gridDim.x), 0, a.nks, false);
}

// ... on 160 x 256 tiles (HKP_TILE_160_A3): 240 m-tiles for the B=8 shard's layer3,
// 0.94 of the CUs, each 5/8 of a 256-row tile.  Waves 2 x 4 (80 x 64 each, 80
// accumulators); a wave's rows are one 80-row BN partial tile.
template <int P>
__global__ __launch_bounds__(512, 1) void conv_x3_a3_160_kernel(X3Args a) {
    __shared__ __attribute__((aligned(1024))) char smem[x3_a3_lds(160)];
    x3_stamp(a, 0);
    conv_x3_tile<256, false, false, 16, P, true, 160>(a, smem, xcd_remap(blockIdx.x, gridDim.x), 0, a.nks, false);
}

// ... on 160 x 128 tiles (HKP_TILE_160_A3 with Cout % 256 != 0, Cout % 128 == 0): the
// B=8 shard's layer2 (128 channels: 150 256x128 tiles -> 240 160x128); waves 2 x 4
// of 80 x 32, a 2-stage ring of 128 weight rows
template <int P>
__global__ __launch_bounds__(512, 1) void conv_x3_a3_160x128_kernel(X3Args a) {
    __shared__ __attribute__((aligned(1024))) char smem[x3_a3_lds(160, 128)];
    x3_stamp(a, 0);
    conv_x3_tile<128, false, false, 16, P, true, 160>(a, smem, xcd_remap(blockIdx.x, gridDim.x), 0, a.nks, false);
}

// Mixed tile heights in one launch (HKP_TILE_MIX_A3, packed operands, Cout % 256
// == 0, more than one round of tiles): a 256-row grid charges its last, partly
// filled round as a whole one.  The three A3 bodies give the same bits per output
// element and cost the same per row, so every CU gets 256-row tiles first and one
// shorter tile last (x3_mix_plan: C2 layer3, 600 row-units per CU, runs 256 + 192 +
// 160 = 38 sixteen-row blocks per CU instead of 2 rounds + a split-K tail; layer4
// 4 x 256 + 192 = 76 instead of 5 x 256 = 80) — no slab, no combine, no workspace.
// The block index picks the region (block-uniform); tall tiles first, since blocks
// are dispatched in index order as CUs free up.  Every region but the last is whole
// full tiles; only the last region's last tile is cut by M.  The XCD remap runs
// inside each region, as in the in-launch tail of conv_x3_a3_kernel.
template <int P>
__global__ __launch_bounds__(512, 1) void conv_x3_a3_mix_kernel(X3Args a) {
    __shared__ __attribute__((aligned(1024))) char smem[X3_A3_LDS];
    x3_stagger(a);
    x3_stamp(a, 0);
    const int b = blockIdx.x;
    if (b < a.mix_b1) {
        conv_x3_tile<256, false, false, 16, P, true, 256>(a, smem, xcd_remap(b, a.mix_b1), 0, a.nks, false);
        return;
    }
    X3Args t = a;
    if (b < a.mix_b2) {
        t.m_base = a.mix_m1;
        t.part_base = a.mix_p1;
        conv_x3_tile<256, false, false, 16, P, true, 192>(t, smem, xcd_remap(b - a.mix_b1, a.mix_b2 - a.mix_b1), 0,
                                                          a.nks, false);
        return;
    }
    t.m_base = a.mix_m2;
    t.part_base = a.mix_p2;
    conv_x3_tile<256, false, false, 16, P, true, 160>(t, smem, xcd_remap(b - a.mix_b2, (int)gridDim.x - a.mix_b2), 0,
                                                      a.nks, false);
}

// Split-K tail: the m-tiles of the last, partly filled round of a one-tile grid,
// each cut into S equal K segments — one block per segment, a single round —
// summed by the tile's last-arriving segment in segment order (sk_combine; the
// launch is laid out as a column-grouped stream-K grid of NG = tiles x S groups,
// so every group's unit range lies inside one tile).  The stream-K kernel's
// segment loop is what made the 256x256 stream-K body spill; a block here runs
// exactly one segment (a two-segment form that balanced C2 layer4's 176 tail
// tiles over all 256 CUs spilled outside the K loop and measured no faster than
// the plain partial round, whose CUs run at a higher clock).  C2 layer3 on
// 256x256 tiles: 600 tiles = 2 rounds + 88 tiles, which run as 176 half tiles.
template <int BN, int P>
__global__ __launch_bounds__(512, 1) void conv_x3_tail_kernel(X3Args a) {
    __shared__ __attribute__((aligned(1024))) char smem[x3_lds_bytes(BN, false, P) + x3_red_bytes(BN, false)];
    const int G = gridDim.x, b = xcd_remap(blockIdx.x, G);
    const int NT = a.n_tiles, NG = G / NT, g = b / NT, nt = b - g * NT;
    const long U = a.sk_units, u0 = sk_start(g, U, NG), u1 = sk_start(g + 1, U, NG);
    const int mt = (int)(u0 / a.nks);
    const int ks = (int)(u0 - (long)mt * a.nks), ke = (int)(u1 - (long)mt * a.nks);
    conv_x3_tile<BN, false, false, 16, P>(a, smem, mt * NT + nt, ks, ke - ks, true);
}

}  // namespace hkp

// the halo, stem patch and DUO bodies: this translation unit's, in the order
// they have always stood here (x3_start launches all of them from one switch)
#include "x3_halo.h"
#include "x3_stem.h"
#include "x3_duo.h"

namespace hkp {

// Compute units (one 512-thread conv block per CU at a time); cached per process.
static int x3_cus() {
    static int n = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) !=
                                                      hipSuccess || v <= 0)
            v = 256;
        return v;
    }();
    return n;
}

HKP_AB_KNOB(int, g_x3_split_tail, 0);                 // hkp_debug_x3_split_tail
HKP_AB_KNOB(int, g_x3_pair128, 1);                    // hkp_debug_x3_pair128
HKP_AB_KNOB(unsigned long long*, g_x3_stamps, nullptr);   // hkp_debug_x3_stamps
HKP_AB_KNOB(int, g_x3_stagger_ns, 0);                 // hkp_debug_x3_stagger
HKP_AB_KNOB(int, g_x3_store, 0);                      // hkp_debug_x3_store
HKP_AB_KNOB(int, g_duo_stagger_ns, -1);               // hkp_debug_duo_stagger
HKP_AB_KNOB(int, g_x3_prio, 0);                       // hkp_debug_x3_prio
HKP_AB_KNOB(int, g_x3_a_wrap, 0);                     // hkp_debug_x3_a_wrap

// run f with std::integral_constant<int, P> for a runtime operand layout P
template <typename F>
static void x3_dispatch_p(int P, F&& f) {
    switch (P) {
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        default: break;
    }
}

// the planner's A/B knobs (x3_plan.h) as this build has them
static X3Knobs x3_knobs() {
    X3Knobs kn;
    kn.pair128 = g_x3_pair128 != 0;
    kn.split_tail = g_x3_split_tail != 0;
    kn.stem_pair = g_stem_pair != 0;
    kn.duo_stagger_ns = g_duo_stagger_ns;
    return kn;
}

// the plan of a launch with the caller's stream-K workspace (ws, ws_bytes; nullable) on this device
static X3LaunchPlan x3_plan_of(const X3Problem& p, int policy, const void* ws, int64_t ws_bytes) {
    return x3_launch_plan(p, policy, ws ? ws_bytes : 0, x3_cus(), x3_knobs());
}

// the problem's geometry in the kernels' argument block
static void x3_set_geometry(X3Args& a, const X3Problem& p) {
    a.N = p.N; a.H = p.H; a.W = p.W; a.C = p.C; a.K = p.K; a.R = p.R; a.S = p.S;
    a.stride = p.stride; a.pad = p.pad; a.dil = p.dil; a.Ho = p.Ho; a.Wo = p.Wo;
    a.M = (int)p.M; a.cch = p.cch; a.RS = p.RS;
    a.ost = p.ost; a.OH = p.OH; a.OW = p.OW; a.oy = p.oy; a.ox = p.ox;
}

// start the kernel of one planned launch on operand layout P (3 packed f16x3 split, 2 / 4
// its two-product sets, 1 plain fp16).  The cases stand in the order in which the kernels
// have always been instantiated, which is the order of the device code: keep it, append
static void x3_start(const X3Launch& l, int P, hipStream_t st, const X3Args& a) {
    const dim3 g((unsigned)l.blocks), b((unsigned)l.threads);
    switch (l.kernel) {
        case HKP_X3K_DUO:
            hipLaunchKernelGGL(conv_x3_duo_kernel<1>, g, b, 0, st, a);
            break;
        case HKP_X3K_HALO_BNIN:
            if (P == 3) hipLaunchKernelGGL(conv_x3_halo_bnin_kernel<3>, g, b, 0, st, a);
            else hipLaunchKernelGGL(conv_x3_halo_bnin_kernel<1>, g, b, 0, st, a);
            break;
        case HKP_X3K_HALO:
            x3_dispatch_p(P, [&](auto pc) { hipLaunchKernelGGL(conv_x3_halo_kernel<pc.value>, g, b, 0, st, a); });
            break;
        case HKP_X3K_A3_MIX:                   // mixed and shorter A3 tiles: packed operands only (x3_choose)
            x3_dispatch_p(P, [&](auto pc) {
                if constexpr (x3_packed(pc.value)) hipLaunchKernelGGL(conv_x3_a3_mix_kernel<pc.value>, g, b, 0, st, a);
            });
            break;
        case HKP_X3K_A3_192:
        case HKP_X3K_A3_160X128:
        case HKP_X3K_A3_160:
            x3_dispatch_p(P, [&](auto pc) {
                if constexpr (x3_packed(pc.value)) {
                    constexpr int Q = pc.value;
                    if (l.kernel == HKP_X3K_A3_192) hipLaunchKernelGGL(conv_x3_a3_192_kernel<Q>, g, b, 0, st, a);
                    else if (l.kernel == HKP_X3K_A3_160X128) hipLaunchKernelGGL(conv_x3_a3_160x128_kernel<Q>, g, b, 0, st, a);
                    else hipLaunchKernelGGL(conv_x3_a3_160_kernel<Q>, g, b, 0, st, a);
                }
            });
            break;
        case HKP_X3K_A3:
            x3_dispatch_p(P, [&](auto pc) { hipLaunchKernelGGL(conv_x3_a3_kernel<pc.value>, g, b, 0, st, a); });
            break;
        case HKP_X3K_SK_128:                   // conv_x3_kernel's stream-K and one-tile forms
        case HKP_X3K_SK_64:
        case HKP_X3K_TILE_256:
        case HKP_X3K_TILE_128_MF16:
        case HKP_X3K_TILE_128_MF32:
        case HKP_X3K_PAIR_64:
            x3_dispatch_p(P, [&](auto pc) {
                constexpr int Q = pc.value;
                if (l.kernel == HKP_X3K_SK_128)
                    hipLaunchKernelGGL((conv_x3_kernel<128, false, false, 16, true, Q>), g, b, 0, st, a);
                else if (l.kernel == HKP_X3K_SK_64)
                    hipLaunchKernelGGL((conv_x3_kernel<64, false, false, 32, true, Q>), g, b, 0, st, a);
                else if (l.kernel == HKP_X3K_TILE_256)
                    hipLaunchKernelGGL((conv_x3_kernel<256, false, false, 16, false, Q>), g, b, 0, st, a);
                else if (l.kernel == HKP_X3K_TILE_128_MF16)
                    hipLaunchKernelGGL((conv_x3_kernel<128, false, false, 16, false, Q>), g, b, 0, st, a);
                else if (l.kernel == HKP_X3K_TILE_128_MF32)
                    hipLaunchKernelGGL((conv_x3_kernel<128, false, false, 32, false, Q>), g, b, 0, st, a);
                else
                    hipLaunchKernelGGL((conv_x3_kernel<64, false, true, 16, false, Q>), g, b, 0, st, a);
            });
            break;
        case HKP_X3K_TAIL:
            x3_dispatch_p(P, [&](auto pc) { hipLaunchKernelGGL((conv_x3_tail_kernel<256, pc.value>), g, b, 0, st, a); });
            break;
        default:
            break;
    }
}

// Run plan pl of problem p: a holds the caller's pointers and epilogue; the geometry is the
// problem's, every launch's grid and tile arithmetic the plan's (x3_plan.h)
static void launch_x3(const X3Problem& p, const X3LaunchPlan& pl, hipStream_t st, X3Args& a, void* ws) {
    x3_set_geometry(a, p);
    a.stamps = g_x3_stamps;
    a.st_kind = g_x3_store;
    a.prio = g_x3_prio;
#ifdef HKP_AB_KNOBS
    a.a_wrap = g_x3_a_wrap;
#endif
    for (int i = 0; i < pl.n_launches; ++i) {
        const X3Launch& l = pl.launch[i];
        if (l.blocks == 0) continue;       // a tail-only grid's full rounds
        X3Args t = a;
        t.n_tiles = l.n_tiles; t.nks = l.nks; t.sk_units = l.sk_units; t.sk_one = l.sk_one; t.mt0 = l.mt0;
        t.main_blocks = l.main_blocks; t.tail_groups = l.tail_groups; t.tail_mt0 = l.tail_mt0; t.tail_units = l.tail_units;
        t.mix_b1 = l.mix_b1; t.mix_b2 = l.mix_b2; t.mix_m1 = l.mix_m1; t.mix_m2 = l.mix_m2;
        t.mix_p1 = l.mix_p1; t.mix_p2 = l.mix_p2;
        t.stagger_blocks = l.stagger_blocks;
        t.stagger_ticks = (l.stagger_ns < 0 ? g_x3_stagger_ns : l.stagger_ns) / 10;
        if (l.uses_ws) {
            t.sk_cnt = (unsigned*)ws;
            t.sk_ws = (float*)((char*)ws + X3_SK_CNT_BYTES);
        }
        x3_start(l, p.P, st, t);
    }
}

}  // namespace hkp

using namespace hkp;

extern "C" int64_t hkp_conv_x3_sk_workspace_bytes(void) { return x3_sk_ws_bytes(256, x3_cus()); }

static int check_tile(const hkp_conv_desc* d, const char* who) {
    HKP_CHECK_ARG(d->tile >= HKP_TILE_AUTO && d->tile <= HKP_TILE_MIX_A3, "%s: unknown tile policy %d", who,
                  d->tile);
    HKP_CHECK_ARG(d->tile != HKP_TILE_RESERVED_7 && d->tile != HKP_TILE_RESERVED_8 && d->tile != HKP_TILE_RESERVED_14,
                  "%s: tile policy %d is retired (a persistent conv body, measured slower)", who, d->tile);
    return HKP_OK;
}

// forward launch shared by the f16x3 (P 3) and plain-fp16 (P 1) entry points
static int conv_fwd_x3_common(const hkp_conv_desc* d, const uint16_t* xs, const uint16_t* ws, const float* wsc,
                              float* y, uint16_t* y16, float* part, void* sk_ws, int64_t sk_bytes, int P,
                              hkp_stream_t stream, const char* who, const X3Args* ep = nullptr) {
    int ho, wo;
    int rc = hkp_conv_out_hw(d, &ho, &wo);
    if (rc) return rc;
    rc = check_tile(d, who);
    if (rc) return rc;
    HKP_CHECK_ARG(xs && ws && (x3_packed(P) ? y != nullptr && y16 == nullptr : y == nullptr && y16 != nullptr),
                  "%s: null tensor (the packed split writes fp32 y, P 1 fp16 y)", who);
    HKP_CHECK_ARG(d->in_layout == HKP_LAYOUT_NHWC, "%s: NHWC only", who);
    const int cg = x3_packed(P) ? 32 : 64;
    HKP_CHECK_ARG(d->c % cg == 0 && d->k % 64 == 0, "%s: need Cin%%%d==0, Cout%%64==0 (c=%d k=%d)", who, cg, d->c,
                  d->k);
    const long M = (long)d->n * ho * wo;
    HKP_CHECK_ARG(M < (1L << 31) && x3_offsets_fit(d->n, d->h, d->w, d->c / cg * 64, d->k, d->r * d->s), "%s: too large",
                  who);
    X3Args a;
    a.xs = (const _Float16*)xs; a.ws = (const _Float16*)ws; a.wscale = wsc;
    a.y = y; a.y16 = (_Float16*)y16; a.part = part; a.amax = nullptr; a.add = nullptr; a.plane = 0;
    X3Problem p = x3_problem_fwd(d, ho, wo, P);
    if (ep) {
        a.ep_ss = ep->ep_ss; a.ep_res = ep->ep_res; a.ep_rss = ep->ep_rss; a.ep_relu = ep->ep_relu;
        a.in_ss = ep->in_ss;
        p.out_bn = ep->ep_ss != nullptr;
        p.in_bn = ep->in_ss != nullptr;
    }
    const X3LaunchPlan pl = x3_plan_of(p, d->tile, sk_ws, sk_bytes);
    if (p.in_bn) {
        // the fused input BN runs where the unfused conv would run the halo-tile body,
        // so its output is the unfused path's, bit for bit
        HKP_CHECK_ARG(P == 3 || P == 1, "%s: fused input BN needs f16x3 or plain fp16", who);
        HKP_CHECK_ARG(pl.c.halo,
                      "%s: the fused input BN needs a launch on the halo-tile body (stride-1 3x3, pad = dil = 1, "
                      "Ho %% 8 == 0, Wo %% 32 == 0)", who);
    }
    launch_x3(p, pl, as_stream(stream), a, sk_ws);
    HKP_LAUNCH_CHECK(who);
    return HKP_OK;
}

extern "C" int hkp_conv2d_fwd_x3(const hkp_conv_desc* d, const uint16_t* x_split, const uint16_t* w_split,
                                 const float* w_inv_scale, float* y, float* stat_partials, void* sk_workspace,
                                 int64_t sk_ws_bytes, hkp_stream_t stream) {
    HKP_CHECK_ARG(d && y, "hkp_conv2d_fwd_x3: null argument");
    return conv_fwd_x3_common(d, x_split, w_split, w_inv_scale, y, nullptr, stat_partials, sk_workspace, sk_ws_bytes,
                              3, stream, "hkp_conv2d_fwd_x3");
}

extern "C" int hkp_conv2d_fwd_x3_bnin(const hkp_conv_desc* d, const float* x_raw, const float* in_scale_shift,
                                      const uint16_t* w_split, const float* w_inv_scale, float* y, float* stat_partials,
                                      void* sk_workspace, int64_t sk_ws_bytes, hkp_stream_t stream) {
    HKP_CHECK_ARG(d && y && x_raw && in_scale_shift, "hkp_conv2d_fwd_x3_bnin: null argument");
    X3Args ep;
    ep.in_ss = in_scale_shift;
    return conv_fwd_x3_common(d, (const uint16_t*)x_raw, w_split, w_inv_scale, y, nullptr, stat_partials, sk_workspace,
                              sk_ws_bytes, 3, stream, "hkp_conv2d_fwd_x3_bnin", &ep);
}

extern "C" int hkp_conv2d_fwd_f16_bnin(const hkp_conv_desc* d, const uint16_t* x_raw_f16, const float* in_scale_shift,
                                       const uint16_t* w_f16, const float* w_inv_scale, uint16_t* y_f16,
                                       float* stat_partials, void* sk_workspace, int64_t sk_ws_bytes,
                                       hkp_stream_t stream) {
    HKP_CHECK_ARG(d && y_f16 && x_raw_f16 && in_scale_shift, "hkp_conv2d_fwd_f16_bnin: null argument");
    X3Args ep;
    ep.in_ss = in_scale_shift;
    return conv_fwd_x3_common(d, x_raw_f16, w_f16, w_inv_scale, nullptr, y_f16, stat_partials, sk_workspace,
                              sk_ws_bytes, 1, stream, "hkp_conv2d_fwd_f16_bnin", &ep);
}

extern "C" int hkp_conv2d_fwd_x3_products(const hkp_conv_desc* d, const uint16_t* x_split, const uint16_t* w_split,
                                          const float* w_inv_scale, int32_t products, float* y, float* stat_partials,
                                          void* sk_workspace, int64_t sk_ws_bytes, hkp_stream_t stream) {
    HKP_CHECK_ARG(d && y, "hkp_conv2d_fwd_x3_products: null argument");
    HKP_CHECK_ARG(products == HKP_X3_ALL || products == HKP_X3_W16 || products == HKP_X3_X16,
                  "hkp_conv2d_fwd_x3_products: unknown product set %d", products);
    const int P = products == HKP_X3_ALL ? 3 : products == HKP_X3_W16 ? 2 : 4;
    return conv_fwd_x3_common(d, x_split, w_split, w_inv_scale, y, nullptr, stat_partials, sk_workspace, sk_ws_bytes,
                              P, stream, "hkp_conv2d_fwd_x3_products");
}

extern "C" int hkp_conv2d_fwd_f16(const hkp_conv_desc* d, const uint16_t* x_f16, const uint16_t* w_f16,
                                  const float* w_inv_scale, uint16_t* y_f16, float* stat_partials,
                                  void* sk_workspace, int64_t sk_ws_bytes, hkp_stream_t stream) {
    HKP_CHECK_ARG(d && y_f16, "hkp_conv2d_fwd_f16: null argument");
    return conv_fwd_x3_common(d, x_f16, w_f16, w_inv_scale, nullptr, y_f16, stat_partials, sk_workspace, sk_ws_bytes,
                              1, stream, "hkp_conv2d_fwd_f16");
}

extern "C" int hkp_conv2d_fwd_f16_bn(const hkp_conv_desc* d, const uint16_t* x_f16, const uint16_t* w_f16,
                                     const float* w_inv_scale, const float* scale_shift, const uint16_t* res_f16,
                                     const float* res_scale_shift, int32_t relu, uint16_t* out_f16,
                                     void* sk_workspace, int64_t sk_ws_bytes, hkp_stream_t stream) {
    HKP_CHECK_ARG(d && out_f16 && scale_shift, "hkp_conv2d_fwd_f16_bn: null argument");
    HKP_CHECK_ARG(!res_scale_shift || res_f16, "hkp_conv2d_fwd_f16_bn: res_scale_shift needs a residual");
    X3Args ep;
    ep.ep_ss = scale_shift;
    ep.ep_res = (const _Float16*)res_f16;
    ep.ep_rss = res_scale_shift;
    ep.ep_relu = relu ? 1 : 0;
    return conv_fwd_x3_common(d, x_f16, w_f16, w_inv_scale, nullptr, out_f16, nullptr, sk_workspace, sk_ws_bytes, 1,
                              stream, "hkp_conv2d_fwd_f16_bn", &ep);
}

extern "C" int hkp_conv2d_bwd_data_x3(const hkp_conv_desc* d, const uint16_t* dy_split, const uint16_t* wf_split,
                                      const float* wf_inv_scale, const uint32_t* dy_amax_bits, const float* add,
                                      float* dx, void* sk_workspace, int64_t sk_ws_bytes, hkp_stream_t stream) {
    int ho, wo;
    int rc = hkp_conv_out_hw(d, &ho, &wo);
    if (rc) return rc;
    HKP_CHECK_ARG(dy_split && wf_split && dx, "hkp_conv2d_bwd_data_x3: null tensor");
    HKP_CHECK_ARG(d->in_layout == HKP_LAYOUT_NHWC && d->stride == 1,
                  "hkp_conv2d_bwd_data_x3: stride-1 NHWC convs only (strided ones use hkp_conv2d_bwd_data)");
    HKP_CHECK_ARG(d->c % 64 == 0 && d->k % 32 == 0, "hkp_conv2d_bwd_data_x3: need Cin%%64==0, Cout%%32==0");
    const int padp = d->dilation * (d->r - 1) - d->pad;
    HKP_CHECK_ARG(padp >= 0 && d->dilation * (d->s - 1) - d->pad == padp, "hkp_conv2d_bwd_data_x3: padding");
    const long M = (long)d->n * d->h * d->w;
    HKP_CHECK_ARG(M < (1L << 31) && x3_offsets_fit(d->n, ho, wo, d->k / 32 * 64, d->c, d->r * d->s),
                  "hkp_conv2d_bwd_data_x3: too large");
    X3Args a;
    a.xs = (const _Float16*)dy_split; a.ws = (const _Float16*)wf_split; a.wscale = wf_inv_scale;
    a.y = dx; a.part = nullptr; a.amax = (const unsigned*)dy_amax_bits; a.add = add; a.plane = 0;
    const X3Problem p = x3_problem_dgrad(d, ho, wo);
    launch_x3(p, x3_plan_of(p, d->tile, sk_workspace, sk_ws_bytes), as_stream(stream), a, sk_workspace);
    HKP_LAUNCH_CHECK("hkp_conv2d_bwd_data_x3");
    return HKP_OK;
}

// (strided dgrad as stride-1 convs, one per output phase: phase_taps, x3_plan.h)
__global__ __launch_bounds__(256) void phase_fill_kernel(long total, int C4, int Ha, int Wa, int OH, int OW, int ost,
                                                        int oy, int ox, const f32x4* __restrict__ add,
                                                        f32x4* __restrict__ dx) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int c4 = (int)(i % C4);
        long p = i / C4;
        const int b = (int)(p % Wa);
        p /= Wa;
        const int a = (int)(p % Ha);
        const long n = p / Ha;
        const long off = ((n * OH + (long)a * ost + oy) * OW + (long)b * ost + ox) * C4 + c4;
        dx[off] = add ? add[off] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

extern "C" int hkp_phase_taps(int32_t r, int32_t pad, int32_t stride, int32_t phase) {
    int rm, om;
    if (r <= 0 || stride <= 0 || phase < 0 || phase >= stride) return -1;
    return phase_taps(r, pad, stride, phase, &rm, &om);
}

extern "C" int hkp_conv2d_bwd_data_x3_strided(const hkp_conv_desc* d, const uint16_t* dy_split,
                                              const uint16_t* const* phase_split, const float* const* phase_inv_scale,
                                              const uint32_t* dy_amax_bits, const float* add, float* dx,
                                              void* sk_workspace, int64_t sk_ws_bytes, hkp_stream_t stream) {
    int ho, wo;
    int rc = hkp_conv_out_hw(d, &ho, &wo);
    if (rc) return rc;
    HKP_CHECK_ARG(dy_split && phase_split && phase_inv_scale && dx, "hkp_conv2d_bwd_data_x3_strided: null tensor");
    HKP_CHECK_ARG(d->in_layout == HKP_LAYOUT_NHWC && d->stride == 2 && d->dilation == 1,
                  "hkp_conv2d_bwd_data_x3_strided: stride-2, dilation-1 NHWC convs only");
    HKP_CHECK_ARG(d->c % 64 == 0 && d->k % 32 == 0, "hkp_conv2d_bwd_data_x3_strided: need Cin%%64==0, Cout%%32==0");
    HKP_CHECK_ARG((long)d->n * d->h * d->w < (1L << 31) && x3_offsets_fit(d->n, ho, wo, d->k / 32 * 64, d->c,
                                                                         d->r * d->s),
                  "hkp_conv2d_bwd_data_x3_strided: too large");
    hipStream_t st = as_stream(stream);
    for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px) {
            const int ph = py * 2 + px;
            const int Ha = (d->h - py + 1) / 2, Wa = (d->w - px + 1) / 2;
            if (Ha <= 0 || Wa <= 0) continue;
            X3Problem p;
            int col_pad = 0;
            if (!x3_problem_dgrad_phase(d, ho, wo, py, px, &p, &col_pad)) {
                HKP_CHECK_ARG(phase_split[ph] == nullptr, "hkp_conv2d_bwd_data_x3_strided: phase %d has no taps", ph);
                const long total = (long)d->n * Ha * Wa * (d->c / 4);
                long g = (total + 255) / 256;
                if (g > 8192) g = 8192;
                hipLaunchKernelGGL(phase_fill_kernel, dim3((unsigned)g), dim3(256), 0, st, total, d->c / 4, Ha, Wa,
                                   d->h, d->w, 2, py, px, (const f32x4*)add, (f32x4*)dx);
                HKP_LAUNCH_CHECK("hkp_conv2d_bwd_data_x3_strided(fill)");
                continue;
            }
            HKP_CHECK_ARG(phase_split[ph] && phase_inv_scale[ph], "hkp_conv2d_bwd_data_x3_strided: phase %d weights",
                          ph);
            X3Args a;
            a.xs = (const _Float16*)dy_split; a.ws = (const _Float16*)phase_split[ph]; a.wscale = phase_inv_scale[ph];
            a.y = dx; a.part = nullptr; a.amax = (const unsigned*)dy_amax_bits; a.add = add; a.plane = 0;
            // the column offset: the kernel applies one pad to both axes
            HKP_CHECK_ARG(col_pad == p.pad, "hkp_conv2d_bwd_data_x3_strided: row/column phase offsets differ (%d, %d)",
                          -p.pad, -col_pad);
            launch_x3(p, x3_plan_of(p, d->tile, sk_workspace, sk_ws_bytes), st, a, sk_workspace);
            HKP_LAUNCH_CHECK("hkp_conv2d_bwd_data_x3_strided");
        }
    return HKP_OK;
}

extern "C" int hkp_conv2d_fwd_stem_x3(const hkp_conv_desc* d, const uint16_t* x_split, const uint16_t* w_split,
                                      const float* w_inv_scale, float* y, float* stat_partials, hkp_stream_t stream) {
    int ho, wo;
    int rc = hkp_conv_out_hw(d, &ho, &wo);
    if (rc) return rc;
    HKP_CHECK_ARG(stem_x3_shape(d), "hkp_conv2d_fwd_stem_x3: needs the 7x7/s2/p3 NCHW stem with C<=4, Cout%%64==0");
    HKP_CHECK_ARG(x_split && w_split && y, "hkp_conv2d_fwd_stem_x3: null tensor");
    const long M = (long)d->n * ho * wo;
    HKP_CHECK_ARG(M < (1L << 31) && x3_offsets_fit(d->n, 2L * ho + 6, 2L * wo + 6, 8, d->k, 7),
                  "hkp_conv2d_fwd_stem_x3: too large");
    X3Args a;
    a.xs = (const _Float16*)x_split; a.ws = (const _Float16*)w_split; a.wscale = w_inv_scale;
    a.y = y; a.part = stat_partials; a.amax = nullptr; a.add = nullptr;
    a.N = d->n; a.H = 2 * ho + 6; a.W = 2 * wo + 6; a.C = 4; a.K = d->k; a.R = 7; a.S = 1;
    a.stride = 2; a.pad = 0; a.dil = 1; a.Ho = ho; a.Wo = wo;
    a.M = (int)M; a.cch = 1; a.RS = 7; a.nks = 7;
    a.plane = (long)d->n * a.H * a.W * 4;
    a.n_tiles = d->k / 64;
    a.stamps = g_x3_stamps;
    a.st_kind = g_x3_store;
    const long m_tiles = (M + 255) / 256;
    if (stem_patch_ok(d, ho, wo, x3_knobs())) {
        hipLaunchKernelGGL(conv_x3_stem_patch_kernel<0>, dim3(m_tiles * a.n_tiles), dim3(512), 0, as_stream(stream), a);
        HKP_LAUNCH_CHECK("hkp_conv2d_fwd_stem_x3");
        return HKP_OK;
    }
    // two blocks per CU (7 K-steps per tile: prologue / epilogue dominate one
    // block), 16x16x32 body on a 2-stage ring (the layer1 256x64 pair's body)
    hipLaunchKernelGGL((conv_x3_kernel<64, true, true, 16, false, 3>), dim3(m_tiles * a.n_tiles), dim3(512), 0,
                       as_stream(stream), a);
    HKP_LAUNCH_CHECK("hkp_conv2d_fwd_stem_x3");
    return HKP_OK;
}

// the stem straight from the image (conv_x3_stem_patch_kernel<1 | 2>): no packed
// planes, where the patch body takes the shape (hkp_stem_x3_image_ok)
extern "C" int32_t hkp_stem_x3_image_ok(const hkp_conv_desc* d) {
    int ho, wo;
    if (!stem_x3_shape(d) || hkp_conv_out_hw(d, &ho, &wo) != HKP_OK) return 0;
    return stem_patch_ok(d, ho, wo, x3_knobs()) && (long)d->n * ho * wo < (1L << 31) ? 1 : 0;
}

extern "C" int hkp_conv2d_fwd_stem_x3_image(const hkp_conv_desc* d, const void* image, int32_t image_u8,
                                            const uint16_t* w_split, const float* w_inv_scale, float* y,
                                            float* stat_partials, hkp_stream_t stream) {
    HKP_CHECK_ARG(hkp_stem_x3_image_ok(d), "hkp_conv2d_fwd_stem_x3_image: shape not on the patch body "
                                           "(hkp_stem_x3_image_ok; use hkp_stem_pack_x3 + hkp_conv2d_fwd_stem_x3)");
    HKP_CHECK_ARG(image && w_split && y, "hkp_conv2d_fwd_stem_x3_image: null tensor");
    int ho, wo;
    hkp_conv_out_hw(d, &ho, &wo);
    X3Args a;
    a.xs = (const _Float16*)image; a.ws = (const _Float16*)w_split; a.wscale = w_inv_scale;
    a.y = y; a.part = stat_partials; a.amax = nullptr; a.add = nullptr;
    a.N = d->n; a.H = d->h; a.W = d->w; a.C = d->c; a.K = d->k; a.R = 7; a.S = 1;
    a.stride = 2; a.pad = 0; a.dil = 1; a.Ho = ho; a.Wo = wo;
    a.M = d->n * ho * wo; a.cch = 1; a.RS = 7; a.nks = 7; a.plane = 0;
    a.n_tiles = d->k / 64;
    a.stamps = g_x3_stamps;
    a.st_kind = g_x3_store;
    const dim3 grid((unsigned)(((long)a.M + 255) / 256 * a.n_tiles));
    if (image_u8) hipLaunchKernelGGL(conv_x3_stem_patch_kernel<2>, grid, dim3(512), 0, as_stream(stream), a);
    else hipLaunchKernelGGL(conv_x3_stem_patch_kernel<1>, grid, dim3(512), 0, as_stream(stream), a);
    HKP_LAUNCH_CHECK("hkp_conv2d_fwd_stem_x3_image");
    return HKP_OK;
}

// The plan of the launch that entry point `op` (HKP_KOP_*: the f16x3 / fp16 forwards, the
// stride-1 dgrad, the stem) runs for d on cus CUs, with or without a stream-K workspace;
// *P its operand layout.  The one reading of a descriptor that the name, the BN-partial
// layout and the plan queries share with the launcher (x3_problem_* and x3_launch_plan).
static int x3_op_plan(const hkp_conv_desc* d, int32_t op, bool sk, int cus, X3LaunchPlan* pl, X3Problem* p,
                      const char* who) {
    int ho, wo;
    int rc = hkp_conv_out_hw(d, &ho, &wo);
    if (rc) return rc;
    rc = check_tile(d, who);
    if (rc) return rc;
    switch (op) {
        case HKP_KOP_FWD_X3: *p = x3_problem_fwd(d, ho, wo, 3); break;
        case HKP_KOP_FWD_X3_W16: *p = x3_problem_fwd(d, ho, wo, 2); break;
        case HKP_KOP_FWD_X3_X16: *p = x3_problem_fwd(d, ho, wo, 4); break;
        case HKP_KOP_FWD_F16: *p = x3_problem_fwd(d, ho, wo, 1); break;
        case HKP_KOP_FWD_F16_BN:
            *p = x3_problem_fwd(d, ho, wo, 1);
            p->out_bn = true;
            break;
        case HKP_KOP_DGRAD_X3: *p = x3_problem_dgrad(d, ho, wo); break;
        case HKP_KOP_STEM_X3:
        case HKP_KOP_STEM_X3_IMAGE:
        case HKP_KOP_STEM_X3_IMAGE_U8: {   // one launch of 256x64 tiles over the 7 filter rows, 128-row partials
            HKP_CHECK_ARG(op == HKP_KOP_STEM_X3 || hkp_stem_x3_image_ok(d),
                          "%s: the image stem needs the patch body's shape", who);
            *p = x3_problem_fwd(d, ho, wo, 3);
            X3Launch& l = pl->launch[0];
            l.kernel = op == HKP_KOP_STEM_X3_IMAGE      ? HKP_X3K_STEM_PATCH_IMAGE
                       : op == HKP_KOP_STEM_X3_IMAGE_U8 ? HKP_X3K_STEM_PATCH_U8
                       : stem_patch_ok(d, ho, wo, x3_knobs()) ? HKP_X3K_STEM_PATCH
                                                        : HKP_X3K_STEM_PAIR;
            l.n_tiles = d->k / 64;
            l.nks = 7;
            l.blocks = p->m_tiles() * l.n_tiles;
            pl->n_launches = 1;
            pl->n_seg = 1;
            pl->seg[0] = 128;
            pl->seg[1] = (int)((p->M + 127) / 128);
            return HKP_OK;
        }
        default:
            HKP_CHECK_ARG(false, "%s: not an f16x3 / fp16 conv op %d", who, op);
    }
    *pl = x3_launch_plan(*p, d->tile, sk ? x3_sk_ws_bytes(256, cus) : 0, cus, x3_knobs());
    return HKP_OK;
}

static bool x3_stat_op(int32_t op) {
    return op == HKP_KOP_FWD_X3 || op == HKP_KOP_FWD_X3_W16 || op == HKP_KOP_FWD_X3_X16 || op == HKP_KOP_FWD_F16;
}

// rows per BN statistic tile of a packed forward conv (see hulkkp.h)
extern "C" int32_t hkp_conv_x3_stat_tile_rows(const hkp_conv_desc* d, int32_t op) {
    HKP_CHECK_ARG(d, "hkp_conv_x3_stat_tile_rows: null descriptor");
    if (!x3_stat_op(op)) return 128;
    int32_t seg[6];
    const int n = hkp_conv_x3_stat_layout(d, op, seg);
    return n < 0 ? n : seg[0];         // a mix launch's list has several (hkp_conv_x3_stat_layout)
}

// the segments of a forward conv's BN partial list (see hulkkp.h): the plan's, for a call
// that passes the stream-K workspace
extern "C" int32_t hkp_conv_x3_stat_layout(const hkp_conv_desc* d, int32_t op, int32_t* segments) {
    HKP_CHECK_ARG(d && segments, "hkp_conv_x3_stat_layout: null argument");
    HKP_CHECK_ARG(x3_stat_op(op), "hkp_conv_x3_stat_layout: not a forward conv op %d", op);
    X3LaunchPlan pl;
    X3Problem p;
    const int rc = x3_op_plan(d, op, true, x3_cus(), &pl, &p, "hkp_conv_x3_stat_layout");
    if (rc) return rc < 0 ? rc : -rc;
    for (int i = 0; i < 6; ++i) segments[i] = pl.seg[i];
    return pl.n_seg;
}

// the regions of a mixed-height launch (see hulkkp.h): pure host arithmetic
extern "C" int32_t hkp_conv_x3_mix_plan(int64_t m, int32_t n_tiles, int32_t cus, int32_t* out) {
    HKP_CHECK_ARG(out && m > 0 && m < (1L << 31) && n_tiles > 0 && cus > 0, "hkp_conv_x3_mix_plan: bad args");
    const X3Mix mp = x3_mix_plan(m, n_tiles, cus);
    out[0] = mp.cost;
    int n = 0;
    for (int r = 0; r < 3; ++r) {
        out[1 + r] = mp.rounds[r];
        out[4 + r] = (int32_t)mp.mt[r];
        out[7 + r] = (int32_t)mp.m_base[r];
        out[10 + r] = (int32_t)mp.part_base[r];
        n += mp.mt[r] > 0;
    }
    out[13] = (int32_t)mp.part_tiles;
    return n;
}

// the wgrad kernel of d and its grid
static int wg_kernel_name(const hkp_conv_desc* d, int ho, int wo, char* buf, int len, long* blocks) {
    int sp, mps, ka, rt;
    wg_x3_plan(d, (long)d->n * ho * wo, wo, &sp, &mps, &ka, &rt);
    *blocks = (long)(d->k / (ka ? ka : 64)) * rt * sp;
    if (ka == 0) return snprintf(buf, len, "wgrad_x3_halo_kernel");
    return snprintf(buf, len, "wgrad_x3_kernel<%d>", ka);
}

// the launches of a conv entry point (see hulkkp.h): pure host arithmetic
extern "C" int32_t hkp_conv_x3_launch_plan(const hkp_conv_desc* d, int32_t op, int32_t stream_k_ok, int32_t cus,
                                           int32_t launch_index, char* name_buf, int32_t len, int64_t* out) {
    HKP_CHECK_ARG(d && name_buf && len > 0 && out && cus >= 0, "hkp_conv_x3_launch_plan: bad args");
    if (cus == 0) cus = x3_cus();
    for (int i = 0; i < HKP_X3_LAUNCH_PLAN_LEN; ++i) out[i] = 0;
    out[29] = cus;
    if (op == HKP_KOP_WGRAD_X3) {          // a wgrad's d->tile is its CU budget: its own planner (wg_x3_plan)
        int ho, wo;
        const int rc = hkp_conv_out_hw(d, &ho, &wo);
        if (rc) return rc;
        HKP_CHECK_ARG(d->k % 64 == 0, "hkp_conv_x3_launch_plan: wgrad needs Cout%%64==0");
        HKP_CHECK_ARG(launch_index == 0, "hkp_conv_x3_launch_plan: launch %d of 1", launch_index);
        long blocks = 0;
        wg_kernel_name(d, ho, wo, name_buf, len, &blocks);
        out[0] = -1;
        out[1] = blocks;
        out[2] = 512;
        out[30] = (long)d->n * ho * wo;
        return 1;
    }
    X3LaunchPlan pl;
    X3Problem p;
    const int rc = x3_op_plan(d, op, stream_k_ok != 0, cus, &pl, &p, "hkp_conv_x3_launch_plan");
    if (rc) return rc;
    HKP_CHECK_ARG(launch_index >= 0 && launch_index < std::max(1, pl.n_launches),
                  "hkp_conv_x3_launch_plan: launch %d of %d", launch_index, pl.n_launches);
    const X3Launch& l = pl.launch[launch_index];
    x3_kernel_name(l.kernel, p.P, name_buf, len);
    const int64_t v[22] = {l.kernel, l.blocks, l.threads, l.n_tiles, l.nks, l.sk_units, l.sk_one, l.mt0,
                           l.main_blocks, l.tail_groups, l.tail_mt0, l.tail_units, l.mix_b1, l.mix_b2, l.mix_m1,
                           l.mix_m2, l.mix_p1, l.mix_p2, l.stagger_blocks, l.stagger_ns, l.uses_ws, l.ws_bytes};
    for (int i = 0; i < 22; ++i) out[i] = v[i];
    for (int i = 0; i < 6; ++i) out[22 + i] = pl.seg[i];
    out[28] = pl.n_seg;
    out[30] = p.M;
    out[31] = p.m_tiles();
    out[32] = pl.c.bn;
    out[33] = pl.c.bm;
    return pl.n_launches;
}

// the kernel symbol a launch with this descriptor runs (see hulkkp.h): the plan's first launch
extern "C" int32_t hkp_conv_kernel_name(const hkp_conv_desc* d, int32_t op, int32_t stream_k_ok, char* buf,
                                        int32_t len) {
    HKP_CHECK_ARG(d && buf && len > 0, "hkp_conv_kernel_name: bad args");
    if (op == HKP_KOP_WGRAD_X3) {
        int ho, wo;
        const int rc = hkp_conv_out_hw(d, &ho, &wo);
        if (rc) return rc;
        HKP_CHECK_ARG(d->k % 64 == 0, "hkp_conv_kernel_name: wgrad needs Cout%%64==0");
        long blocks = 0;
        return wg_kernel_name(d, ho, wo, buf, len, &blocks);
    }
    X3LaunchPlan pl;
    X3Problem p;
    const int rc = x3_op_plan(d, op, stream_k_ok != 0, x3_cus(), &pl, &p, "hkp_conv_kernel_name");
    if (rc) return rc;
    return x3_kernel_name(pl.launch[0].kernel, p.P, buf, len);
}

#ifdef HKP_AB_KNOBS   // the A/B instruments (tools/ab_lib build only; include/hulkkp_ab.h)
// Debug: forward conv launches record per-block phase clocks into buf (8 slots of
// s_memrealtime per block: start, pipeline filled, K loop done, BN partials
// done, fp16 tile staged, stores issued; 0 where a body records none); NULL
// turns it off.  Not thread-safe; for tools/ only.
extern "C" void hkp_debug_x3_stamps(uint64_t* buf) { g_x3_stamps = (unsigned long long*)buf; }

// Debug / tuning (tools/ only, not thread-safe): the first-round stagger of the
// one-tile forward conv launches, in ns (0 = off; X3Args::stagger_ticks).
extern "C" void hkp_debug_x3_stagger(int32_t ns) { g_x3_stagger_ns = ns > 0 ? ns : 0; }

// Debug / A/B (tools/ only, not thread-safe): nonzero runs an A3 grid's split-K
// tail as its own conv_x3_tail_kernel launch instead of inside the A3 launch.
extern "C" void hkp_debug_x3_split_tail(int32_t on) { g_x3_split_tail = on != 0; }
extern "C" void hkp_debug_stem_pair(int32_t on) { g_stem_pair = on != 0; }
extern "C" void hkp_debug_x3_pair128(int32_t on) { g_x3_pair128 = on != 0; }

// Debug / A/B (tools/ only, not thread-safe): the flavour of the forward convs'
// epilogue output stores (X3Args::st_kind: 0 each site's own, 1 plain, 2
// nontemporal, 3 sc1, 4 sc0 sc1).
extern "C" void hkp_debug_x3_store(int32_t kind) { g_x3_store = kind >= 0 && kind <= 4 ? kind : 0; }

// Debug / A/B (tools/ only, not thread-safe): the DUO body's first-round stagger of
// the second block on each CU, in ns (0 = off; < 0 = the planner's estimate).
extern "C" void hkp_debug_duo_stagger(int32_t ns) { g_duo_stagger_ns = ns; }

// Debug / A/B (tools/ only, not thread-safe): static wave priority in the A3 body's
// K loop (X3Args::prio: 0 none, 1 waves 4-7, 2 waves 0-3 at s_setprio 1).
extern "C" void hkp_debug_x3_prio(int32_t mode) { g_x3_prio = mode >= 0 && mode <= 2 ? mode : 0; }

// A/B probe (tools/ only, not thread-safe): the one-tile and DUO conv bodies read A row m
// from row m % rows (0 = off) — an L2-resident activation stream, wrong outputs
extern "C" void hkp_debug_x3_a_wrap(int32_t rows) { g_x3_a_wrap = rows > 0 ? rows : 0; }
#endif

