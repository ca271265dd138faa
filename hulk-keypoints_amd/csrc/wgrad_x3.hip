// f16x3 backward-filter (weight gradient) on packed split operands: the tiled
// bodies, the halo body for 3x3 convs, and the fixed-order reduction of their
// split-K slabs.  Arithmetic and operand layouts: conv_x3.hip.
#include "common.h"
#include "x3_plan.h"
#include "x3_dev.h"

namespace hkp {

// ---------------------------------------------------------------------------
// Weight gradient on packed split operands:
//     dW[k][tap][c] = sum_p dy[p][k] * x[pixel(p, tap)][c]        (p: output pixels)
// GEMM rows = Cout (dy side, KA per tile), columns = (tap, c) flattened (x side,
// 256 per tile = 8 channel groups, one per wave for staging), reduction over
// output pixels, split-K over pixel ranges into fixed-order fp32 slabs
// [split][K][R*S*C] (summed by wg_x3_reduce_kernel — deterministic).
// Both LDS images are pixel-major per channel group: line (group, pixel) =
// 128 B [hi32|lo32], 32 pixels per K-step, written by LDS-DMA; the MFMA
// fragments (8 consecutive pixels of one channel per lane) come from
// ds_read_b64_tr_b16 transposed reads.  Swizzle: 16-B chunk ^= ((pixel>>1)&1)<<2
// makes every 32-lane half of a transposed read cover all 64 banks once.
typedef short s16x4 __attribute__((ext_vector_type(4)));

struct WgX3Args {
    const _Float16* xs;     // packed x  [N*H*W][C/32][64]
    const _Float16* dys;    // packed, scaled dy [M][K/32][64]
    const unsigned* amax;   // the scale dy was split with (pow2_scale_for), nullable
    float* ws;              // slabs [splits][K][RSC]
    int N, H, W, C, K, R, S, stride, pad, dil, Ho, Wo;
    int M, RSC, r_tiles, mps, tiles;
};

// ds_read_b64_tr_b16 as inline asm: the builtin makes hipcc drain the whole
// LDS-DMA queue (vmcnt(0)) before every transposed read, since it cannot tell
// the read from the in-flight DMA's destination.  The caller waits lgkmcnt
// itself before the MFMAs that consume the result (explicit waits below, each
// followed by sched_barrier(0) so no MFMA is scheduled ahead of it).
template <int OFF>
__device__ __forceinline__ s16x4 ds_tr16(unsigned lds_addr) {
    s16x4 r;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(lds_addr), "i"(OFF));
    return r;
}

__device__ __forceinline__ unsigned lds_addr_of(const char* p) {
    return (unsigned)(size_t)(const __attribute__((address_space(3))) char*)p;
}

__device__ __forceinline__ f16x8 cat_tr(s16x4 lo, s16x4 hi) {
    const auto v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(f16x8, v);
}

// KA = 256 (Cout % 256 == 0): a 256x256 tile, 96 MAC per staged byte instead of
// 64 (KA 128) — the 256x128 body is bound by operand delivery, not the MFMAs
// (MFMA-busy scales with the intensity: 0.25 at KA 64, 0.42 at KA 128).  Its
// stage holds PX = 16 pixels (one MFMA k-slice) so three stages fit in 96 KB.
// The PX = 16 body runs a 4-stage ring (128 KB, inside the epilogue's 132 KB) and
// issues each stage's DMA as GL = TM pieces placed after the MFMAs of one row
// (address math branch-free: one wrap per stage, Wo >= PX, see wg_x3_plan), so
// the per-lane address VALU runs in the MFMA shadow instead of between the
// barrier and the first MFMA of every stage.
template <int KA>
__global__ __launch_bounds__(512, 1) void wgrad_x3_kernel(WgX3Args a) {
    constexpr int BR = 256, GX = BR / 32, GD = KA / 32;
    constexpr int PX = KA == 256 ? 16 : 32;                  // pixels per stage
    constexpr int NS = PX == 16 ? 4 : 3;                     // LDS ring depth
    constexpr int ROW = 128, STAGE = (GX + GD) * PX * ROW;
    constexpr int NX = PX / 8, ND = GD * PX / 64, GL = NX + ND;
    constexpr int TM = KA / 64, TN = 2;
    static_assert(ND >= 1 && (KA == 64 || KA == 128 || KA == 256), "KA must be 64, 128 or 256");
    // the epilogue stages the slab tile (KA x 256 fp32, pitch 264) in passes of
    // 128 rows through the drained ring: at least 132 KiB
    constexpr int EPI_ROWS = KA < 128 ? KA : 128, EPI_PITCH = BR + 8;
    constexpr int LDS = NS * STAGE > EPI_ROWS * EPI_PITCH * 4 ? NS * STAGE : EPI_ROWS * EPI_PITCH * 4;
    __shared__ __attribute__((aligned(1024))) char smem[LDS];

    const int bid = xcd_remap(blockIdx.x, gridDim.x);       // same pixel range → same XCD
    const int split = bid / a.tiles, tile = bid - split * a.tiles;
    const int kt = tile / a.r_tiles, rt = tile - kt * a.r_tiles;
    const int k0 = kt * KA, r0 = rt * BR;
    const int p_begin = split * a.mps;
    const int p_end = min(a.M, p_begin + a.mps);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);

    // ---- staging bookkeeping ----
    const int Lx = ((lane & 7) ^ (((lane >> 4) & 1) << 2)) * 8;   // logical chunk (halves) this lane fetches
    const int mg = r0 + 32 * w;                                   // first column of this wave's x group
    const bool gvalid = mg < a.RSC;
    const int tap = gvalid ? mg / a.C : 0;
    const int cg = gvalid ? (mg - tap * a.C) >> 5 : 0;
    const int rr = tap / a.S, ss = tap - rr * a.S;
    const int dh = rr * a.dil - a.pad, dw = ss * a.dil - a.pad;
    const int xstride = a.C * 2, dstride = a.K * 2;
    const _Float16* xg = a.xs + cg * 64 + Lx;
    const _Float16* zero = (const _Float16*)g_x3_zero_line;
    int xn[NX], xho[NX], xwo[NX];
    const int hw = a.Ho * a.Wo;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        const int p = p_begin + 8 * i + (lane >> 3);
        xn[i] = p / hw;
        const int rem = p - xn[i] * hw;
        xho[i] = rem / a.Wo;
        xwo[i] = rem - xho[i] * a.Wo;
    }
    const _Float16* dg[ND];
    int dpp[ND];
#pragma unroll
    for (int j = 0; j < ND; ++j) {
        const int line = 8 * (w * ND + j) + (lane >> 3);
        dpp[j] = line % PX;
        dg[j] = a.dys + (k0 >> 5) * 64 + (line / PX) * 64 + Lx;
    }

    auto issue = [&](int t) {
        char* st = smem + (t % NS) * STAGE;
        const int pb = p_begin + PX * t;
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int p = pb + 8 * i + (lane >> 3);
            const int hi = xho[i] * a.stride + dh, wi = xwo[i] * a.stride + dw;
            const bool in = gvalid && p < p_end && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
            const long pix = ((long)xn[i] * a.H + hi) * a.W + wi;
            glds16(in ? xg + pix * xstride : zero, st + (w * PX + 8 * i) * ROW);
            xwo[i] += PX;                                    // this slot's pixel for the next K-step
            while (xwo[i] >= a.Wo) {
                xwo[i] -= a.Wo;
                if (++xho[i] == a.Ho) {
                    xho[i] = 0;
                    ++xn[i];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < ND; ++j) {
            const int p = pb + dpp[j];
            glds16(p < p_end ? dg[j] + (long)p * dstride : zero, st + (GX * PX + 8 * (w * ND + j)) * ROW);
        }
    };

    // one DMA piece of stage t (PX == 16 body): k < NX an x slot, else a dy slot.
    // The x slot's pixel advances by PX per stage with at most one row wrap
    // (Wo >= PX): selects, no branches, so the piece can sit between MFMAs.
    auto piece = [&](int t, const int k) {
        char* st = smem + (t & (NS - 1)) * STAGE;
        const int pb = p_begin + PX * t;
        // 32-bit byte offsets (wg_x3_plan: both operands < 4 GiB for KA 256), the
        // validity as a mask and the zero line as a select: no branch
        if (k < NX) {
            const int i = k;
            const int p = pb + 8 * i + (lane >> 3);
            const int hi = xho[i] * a.stride + dh, wi = xwo[i] * a.stride + dw;
            const bool in = gvalid & (p < p_end) & ((unsigned)hi < (unsigned)a.H) & ((unsigned)wi < (unsigned)a.W);
            const unsigned off = (((unsigned)xn[i] * a.H + hi) * a.W + wi) * (unsigned)(xstride * 2);
            const char* src = in ? (const char*)xg : (const char*)zero;
            glds16(src + (in ? off : 0u), st + (w * PX + 8 * i) * ROW);
            const int w2 = xwo[i] + PX;
            const bool wrap = w2 >= a.Wo;
            xwo[i] = wrap ? w2 - a.Wo : w2;
            const int h2 = xho[i] + (wrap ? 1 : 0);
            const bool wrap2 = h2 == a.Ho;
            xho[i] = wrap2 ? 0 : h2;
            xn[i] += wrap2 ? 1 : 0;
        } else {
            const int j = k - NX;
            const int p = pb + dpp[j];
            const bool in = p < p_end;
            const char* src = in ? (const char*)dg[j] : (const char*)zero;
            glds16(src + (in ? (unsigned)p * (unsigned)(dstride * 2) : 0u), st + (GX * PX + 8 * (w * ND + j)) * ROW);
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // transposed-read addressing: 16-lane group G reads 4 pixel rows (q) x 16
    // channels (column block cb = G&1); lane 4q+p supplies row q, channels 4p..4p+3
    const int wk = w & 1, wr = w >> 1;
    const int h = lane >> 5, cb = (lane >> 4) & 1, q = (lane >> 2) & 3, pq = lane & 3;
    int toff[2];
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
        toff[pl] = (8 * h + q) * ROW + (((4 * pl + 2 * cb + (pq >> 1)) ^ (((q >> 1) & 1) << 2)) << 4) + 8 * (pq & 1);
    const int a_line = (GX + wk * TM) * PX * ROW;     // dy groups of this wave
    const int b_line = (wr * TN) * PX * ROW;          // x groups of this wave

    struct Frag {
        f16x8 dh[TM], dl[TM], xh[TN], xl[TN];
    };
    // per-lane LDS byte addresses of the two planes' transposed-read blocks
    const unsigned lds0 = lds_addr_of(smem);
    const unsigned ta0 = lds0 + a_line + toff[0], ta1 = lds0 + a_line + toff[1];
    const unsigned tb0 = lds0 + b_line + toff[0], tb1 = lds0 + b_line + toff[1];
    auto read_frag = [&](Frag& f, int buf, const int s) {
        const unsigned so = buf * STAGE;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            // immediate offsets: tile i (32 rows), half s (16 rows), second read +4 rows
            if (s == 0) {
                f.dh[i] = cat_tr(ds_tr16<0>(ta0 + so + i * PX * ROW), ds_tr16<4 * ROW>(ta0 + so + i * PX * ROW));
                f.dl[i] = cat_tr(ds_tr16<0>(ta1 + so + i * PX * ROW), ds_tr16<4 * ROW>(ta1 + so + i * PX * ROW));
            } else {
                f.dh[i] = cat_tr(ds_tr16<16 * ROW>(ta0 + so + i * PX * ROW),
                                 ds_tr16<20 * ROW>(ta0 + so + i * PX * ROW));
                f.dl[i] = cat_tr(ds_tr16<16 * ROW>(ta1 + so + i * PX * ROW),
                                 ds_tr16<20 * ROW>(ta1 + so + i * PX * ROW));
            }
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            if (s == 0) {
                f.xh[j] = cat_tr(ds_tr16<0>(tb0 + so + j * PX * ROW), ds_tr16<4 * ROW>(tb0 + so + j * PX * ROW));
                f.xl[j] = cat_tr(ds_tr16<0>(tb1 + so + j * PX * ROW), ds_tr16<4 * ROW>(tb1 + so + j * PX * ROW));
            } else {
                f.xh[j] = cat_tr(ds_tr16<16 * ROW>(tb0 + so + j * PX * ROW),
                                 ds_tr16<20 * ROW>(tb0 + so + j * PX * ROW));
                f.xl[j] = cat_tr(ds_tr16<16 * ROW>(tb1 + so + j * PX * ROW),
                                 ds_tr16<20 * ROW>(tb1 + so + j * PX * ROW));
            }
        }
    };
    auto mma = [&](const Frag& f) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.dh[i], f.xh[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.dh[i], f.xl[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.dl[i], f.xh[j], acc[i][j], 0, 0, 0);
            }
    };
    // same software pipeline as conv_x3_kernel<*, 2> (see there); 4*(TM+TN)
    // transposed b64 reads per half, two per MFMA gap.  The reads are inline
    // asm: every consumer MFMA sits behind an explicit lgkmcnt wait + sched_barrier.
    constexpr int NR = 4 * (TM + TN), NM = 3 * TM * TN;
    const int nsteps = p_end > p_begin ? (p_end - p_begin + PX - 1) / PX : 0;
    if constexpr (PX == 16) {
        // one dy fragment set, refilled row by row right after its MFMAs issue
        // (128 accumulators + 32 dy + 2x16 x registers): per stage t
        // [wait own DMA t+1 and this wave's reads, barrier | t+1's x fragments |
        //  rows i = 0..TM-1: t's MFMAs, one DMA piece of stage t+3, t+1's row i]
        struct XF {
            f16x8 xh[TN], xl[TN];
        };
        f16x8 dh[TM], dl[TM];
        XF x0, x1;
        auto read_d = [&](const int i, const unsigned so) {
            dh[i] = cat_tr(ds_tr16<0>(ta0 + so + i * PX * ROW), ds_tr16<4 * ROW>(ta0 + so + i * PX * ROW));
            dl[i] = cat_tr(ds_tr16<0>(ta1 + so + i * PX * ROW), ds_tr16<4 * ROW>(ta1 + so + i * PX * ROW));
        };
        auto read_x = [&](XF& x, const unsigned so) {
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                x.xh[j] = cat_tr(ds_tr16<0>(tb0 + so + j * PX * ROW), ds_tr16<4 * ROW>(tb0 + so + j * PX * ROW));
                x.xl[j] = cat_tr(ds_tr16<0>(tb1 + so + j * PX * ROW), ds_tr16<4 * ROW>(tb1 + so + j * PX * ROW));
            }
        };
        auto mma_row = [&](const int i, const XF& x) {
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(dh[i], x.xh[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(dh[i], x.xl[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(dl[i], x.xh[j], acc[i][j], 0, 0, 0);
            }
        };
        static_assert(PX != 16 || GL == TM, "one DMA piece per MFMA row");
        if (nsteps > 0) {
            // prologue: stages 0..NS-2 (past the end: zero lines, never read)
#pragma unroll
            for (int u = 0; u < NS - 1; ++u)
#pragma unroll
                for (int k = 0; k < GL; ++k) piece(u, k);
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * GL) : "memory");
            lds_barrier();
            read_x(x0, 0);
#pragma unroll
            for (int i = 0; i < TM; ++i) read_d(i, 0);
            // step t: wait for stage t+1 (stage t+2's pieces stay in flight), barrier,
            // read t+1's fragments row by row beside t's MFMAs, and issue stage
            // t+3's pieces (into the buffer stage t-1 used: every wave finished
            // reading it before this step's barrier) one per MFMA row.  Stages past
            // the end load zero lines into buffers no later stage reads, so every
            // non-final step is the same branch-free code.
            auto step = [&](const int t, const XF& xa, XF& xb) {
                asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((NS - 3) * GL) : "memory");
                lds_barrier();
                __builtin_amdgcn_sched_barrier(0);
                const unsigned so = ((t + 1) & (NS - 1)) * STAGE;
                read_x(xb, so);
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    mma_row(i, xa);
                    piece(t + NS - 1, i);
                    read_d(i, so);
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            auto last = [&](const XF& xa) {
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // + the dummy DMAs
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < TM; ++i) mma_row(i, xa);
            };
            int t = 0;
            for (; t + 2 < nsteps; t += 2) {
                step(t, x0, x1);
                step(t + 1, x1, x0);
            }
            // the x fragments' reads retire before the join's register copies read
            // them (asm reads are untracked; tools/trcheck.py)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            if (t + 1 < nsteps) {
                step(t, x0, x1);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                x0 = x1;                                     // one last() call site
            }
            last(x0);
        }
    } else if (nsteps > 0) {
        int q_t = 0;
        auto issue_next = [&]() { issue(q_t++); };
        issue_next();
        if (nsteps > 1) issue_next();
        if (nsteps > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GL) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        lds_barrier();
        Frag f0, f1;
        int cur = 0;
        read_frag(f0, 0, 0);
        auto step = [&](const bool ISSUE, const bool NEXT) {
            const int bcur = cur;
            if (ISSUE) issue_next();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // f0 (read last half) landed
            __builtin_amdgcn_sched_barrier(0);
            read_frag(f1, bcur, 1);
            mma(f0);
#pragma unroll
            for (int k = 0; k < NR / 2; ++k) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x001, 2, 0);   // the asm reads count as ALU
            }
            __builtin_amdgcn_sched_group_barrier(0x008, NM - NR / 2, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (NEXT) {
                if (ISSUE) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(GL) : "memory");
                else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                lds_barrier();
                __builtin_amdgcn_sched_barrier(0);
                cur = cur == 2 ? 0 : cur + 1;
                mma(f1);
                read_frag(f0, cur, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
#pragma unroll
                for (int k = 0; k < NR / 2; ++k) {
                    __builtin_amdgcn_sched_group_barrier(0x001, 2, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, NM - 1 - NR / 2, 0);
                __builtin_amdgcn_sched_barrier(0);
            } else {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                mma(f1);
            }
        };
        int t = 0;
        for (; t + 2 < nsteps; ++t) step(true, true);
        if (t + 1 < nsteps) {
            step(false, true);
            ++t;
        }
        step(false, false);
    }

    // ---- epilogue: the slab tile staged through the drained ring in passes of
    // EPI_ROWS output-channel rows and written as 16-B row chunks (whole 128-B
    // lines, 32-64 stores per thread).  Per-element stores from the fragments
    // (128 per thread, past a wave's 63 outstanding memory ops) stalled every
    // wave on their completion while all CUs wrote their slabs at once.
    const float inv = 1.f / pow2_scale_for(a.amax);
    float* out = a.ws + (long)split * a.K * a.RSC;
    float* t = (float*)smem;
    constexpr int PASSES = KA / EPI_ROWS, C4 = BR / 4;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    lds_barrier();                                             // every wave done with the ring
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        // wave rows: k_local = wk*TM*32 + i*32 + 8*(r>>2) + 4*h + (r&3) in [ps*EPI_ROWS, +EPI_ROWS)
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int kb = wk * TM * 32 + i * 32;
            if (kb / EPI_ROWS != ps) continue;                 // wave-uniform
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    t[(kb - ps * EPI_ROWS + 8 * (r >> 2) + 4 * h + (r & 3)) * EPI_PITCH + wr * 64 + j * 32 + (lane & 31)] =
                        acc[i][j][r] * inv;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        lds_barrier();
        const int mcols = min(BR, a.RSC - r0);                 // multiple of 4 (RSC = R*S*C, C % 32 == 0)
#pragma unroll 4
        for (int e = tid; e < EPI_ROWS * C4; e += 512) {
            const int row = e / C4, c4 = e - row * C4;
            if (c4 * 4 < mcols)
                *(f32x4*)(out + (long)(k0 + ps * EPI_ROWS + row) * a.RSC + r0 + c4 * 4) =
                    *(const f32x4*)(t + row * EPI_PITCH + c4 * 4);
        }
        if (ps + 1 < PASSES) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            lds_barrier();
        }
    }
}

// Weight gradient of a 3x3, stride-1, pad-1, dilation-1 conv from one staged halo
// (round 6; the small-channel layers).  The tiled body above stages a pixel's x
// line once per 256-column group — for C = 64 three groups, the third 1/4 used —
// so its K-step moves 40 KiB per 64x256 tile and runs at MFMA busy 0.25.  Here a
// block owns 64 output channels x all 9 taps x 64 input channels (576 slab
// columns); a K-step is one patch of 4 output rows x 16 columns (Ho % 4 == 0,
// Wo % 16 == 0), staged as its 6 x 18 input halo x 2 channel groups (every tap
// of every row of the patch reads from it) beside the patch's dy lines: 43 KiB
// for 64 pixels.  16x16x32 MFMAs over two 32-pixel k-slices (patch rows 0-1,
// 2-3): wave w owns K rows 32*(w&1).. (2 m-tiles) x input channels 16*(w>>1)..
// of every tap (9 n-tiles, 72 accumulators); the x fragment of tap (r, s) for
// patch row i is staged row i + r read s lines further.  Both operands come from
// ds_read_b64_tr_b16 (8 consecutive pixels of one channel per lane).  Swizzle:
// 16-B chunk ^= 2*(((j>>1)&1) | ((j>>3)&1)<<1) for line j of a run, so the 8
// lines a 32-lane half of a transposed read touches ({a..a+3} u {a+8..a+11}, any
// shift a) fall on 8 distinct 32-B bank slots.  3-stage ring, one barrier per
// K-step; slabs [split][K][R*S*C] as wgrad_x3_kernel's (same reduce), the pixel
// ranges whole patches.
constexpr int WGH_LX = 18, WGH_XL = 12 * WGH_LX, WGH_SL = WGH_XL + 128, WGH_STAGE = WGH_SL * 128, WGH_NS = 3;
constexpr int WGH_PITCH = 580;                       // epilogue rows: 576 slab columns + 4 (conflict-free stores)
// s_waitcnt lgkmcnt(N) for a compile-time N (after unrolling)
__device__ __forceinline__ void wait_lgkm(const int n) {
    switch (n) {
        case 0: asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory"); break;
        case 8: asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory"); break;
        default: asm volatile("s_waitcnt lgkmcnt(12)" ::: "memory"); break;
    }
}
__global__ __launch_bounds__(512, 1) void wgrad_x3_halo_kernel(WgX3Args a) {
    constexpr int ROW = 128, LX = WGH_LX, XL = WGH_XL, STAGE = WGH_STAGE, NS = WGH_NS;
    // DMA pieces per stage: XP x pieces as slots 0-3 of the 8 waves (piece w + 8 i;
    // past XP the sink), the 16 dy pieces as slots 4-5 (piece w + 8 (i - 4))
    constexpr int XP = XL / 8, XS = 4, SLOTS = XS + 2;
    static_assert(XP <= 8 * XS, "x pieces");
    constexpr int SINK = NS * STAGE;
    static_assert(XL % 8 == 0 && 32 * WGH_PITCH * 4 <= SINK, "wgrad halo LDS");
    __shared__ __attribute__((aligned(1024))) char smem[SINK + 1024];

    const int bid = xcd_remap(blockIdx.x, gridDim.x);       // same pixel range → same XCD
    const int split = bid / a.tiles, tile = bid - split * a.tiles;
    const int kt = tile / a.r_tiles, ct = tile - kt * a.r_tiles;
    const int k0 = kt * 64, c0 = ct * 64;
    const int HP = a.Ho / 4, WP = a.Wo / 16, npatch = a.N * HP * WP;
    const int P0 = split * a.mps;                            // this split's patches [P0, P1)
    const int P1 = min(npatch, P0 + a.mps);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    auto xsw = [](int j) { return (((j >> 1) & 1) | (((j >> 3) & 1) << 1)) << 1; };

    // ---- DMA sources: raw-buffer loads (an offset past num_records loads zeros:
    // halo lines outside the image, patches past the range, the sink pieces; the
    // operands are under 2 GiB, wg_halo_shape, so bit 31 marks them).  Stride 1,
    // pad 1: input pixel of halo line (staged row R, column j) of the patch at
    // output pixel p (its top-left) is p + (R - 1) W + j - 1, so a lane's byte
    // offset is the stage's p * 4C plus a constant ----
    const i32x4 xr = buffer_rsrc(a.xs, (unsigned)((long)a.N * a.H * a.W * a.C * 4));
    const i32x4 dr = buffer_rsrc(a.dys, (unsigned)((long)a.M * a.K * 4));
    int xk[XS];                 // byte offset from the stage's p * 4C (signed)
    int xg[XS];                 // halo edge of the line: top row | bottom row << 1 | left column << 2 | right << 3
#pragma unroll
    for (int i = 0; i < XS; ++i) {
        const int pc = min(w + 8 * i, XP - 1);               // past XP: a valid line, loaded into the sink
        const int L = 8 * pc + (lane >> 3), run = L / LX, j = L - run * LX;
        const int R = run >> 1, cg = run & 1;
        xk[i] = ((R - 1) * a.W + j - 1) * (a.C * 4) + ((c0 / 32 + cg) * 64 + ((lane & 7) ^ xsw(j)) * 8) * 2;
        xg[i] = (R == 0 ? 1 : 0) | (R == 5 ? 2 : 0) | (j == 0 ? 4 : 0) | (j == LX - 1 ? 8 : 0);
    }
    int dk[2];                  // dy: byte offset from the stage's p * 4K (line: K group | patch row | column)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int L = 8 * (w + 8 * i) + (lane >> 3), pr = (L >> 4) & 3, cc = L & 15;
        dk[i] = (pr * a.W + cc) * (a.K * 4) + ((k0 / 32 + (L >> 6)) * 64 + ((lane & 7) ^ xsw(L & 31)) * 8) * 2;
    }
    // the patch being issued: index, top-left output pixel, patch row / column (wave-uniform)
    int q_P = P0, q_hp, q_wp, q_p;
    {
        const int n = P0 / (HP * WP), rem = P0 - n * (HP * WP);
        q_hp = rem / WP;
        q_wp = rem - q_hp * WP;
        q_p = (n * a.Ho + 4 * q_hp) * a.Wo + 16 * q_wp;
    }
    int q_t = 0, q_em = 0, q_bad = 0;
    auto begin_issue = [&]() {
        q_em = (q_hp == 0 ? 1 : 0) | (q_hp == HP - 1 ? 2 : 0) | (q_wp == 0 ? 4 : 0) | (q_wp == WP - 1 ? 8 : 0);
        q_bad = q_P >= P1 ? 1 : 0;
    };
    auto piece = [&](const int i) {
        char* st = smem + (q_t % NS) * STAGE;
        if (i < XS) {
            // branch-free: an invalid line gets bit 31 (past num_records) or'd in
            const int pc = w + 8 * i;                        // wave-uniform
            const unsigned bad = (unsigned)q_bad | (unsigned)((xg[i] & q_em) != 0) | (unsigned)(pc >= XP);
            blds16(xr, (unsigned)(q_p * (a.C * 4) + xk[i]) | (bad << 31), 0, pc < XP ? st + pc * 1024 : smem + SINK);
        } else {
            blds16(dr, (unsigned)(q_p * (a.K * 4) + dk[i - XS]) | ((unsigned)q_bad << 31), 0,
                   st + XL * ROW + (w + 8 * (i - XS)) * 1024);
        }
    };
    auto end_issue = [&]() {                                 // the next patch
        ++q_t;
        ++q_P;
        q_p += 16;
        if (++q_wp == WP) {
            q_wp = 0;
            q_p += 3 * a.Wo;
            q_hp = q_hp + 1 == HP ? 0 : q_hp + 1;
        }
    };
    auto issue = [&]() {
        begin_issue();
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) piece(i);
        end_issue();
    };

    f32x4 acc[2][9];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- transposed-read addresses (stage-relative bytes, k-slice 0): 16-lane
    // group G reads patch row G >> 1 (+2 in k-slice 1), pixels 8 (G & 1) + q (+4 the
    // second read) of 16 channels; lane 4q + pp supplies row q, channels 4pp..4pp+3 ----
    const int G = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
    const int kh = w & 1, cb4 = w >> 1, cg = cb4 >> 1, cbl = cb4 & 1;
    unsigned a_ad[2][2];        // dy: [m-tile][plane]; line 8G + q of the wave's K group (+4: same swizzle)
    {
        const int j = 8 * G + q;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl)
                a_ad[mi][pl] = (unsigned)((XL + 64 * kh + j) * ROW + ((((pl * 4 + mi * 2 + (pp >> 1)) ^ xsw(j))) << 4) +
                                          8 * (pp & 1));
    }
    unsigned b_ad[3][2][2];     // x: [tap column s][read half][plane], staged row G >> 1 (+ k-slice * 2 + r)
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
            const int j = 8 * (G & 1) + q + s + 4 * h2;
            const int run = (G >> 1) * 2 + cg;
#pragma unroll
            for (int pl = 0; pl < 2; ++pl)
                b_ad[s][h2][pl] = (unsigned)((run * LX + j) * ROW + ((((pl * 4 + cbl * 2 + (pp >> 1)) ^ xsw(j))) << 4) +
                                             8 * (pp & 1));
        }
    const unsigned lds0 = lds_addr_of(smem);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) a_ad[mi][pl] += lds0;
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) b_ad[s][h2][pl] += lds0;

    // Per K-step t (stage t in LDS): 18 tap-slices v = 9 * k-slice + tap, each's x
    // fragments read two ahead, k-slice 1's dy fragments in two halves at v = 3 and
    // 6; after v = 15 the step's one barrier (stage t+1 landed everywhere, stage
    // t-1 read by everyone), then stage t+1's k-slice-0 dy and first x fragments
    // read beside v = 16-17, and stage t+NS-1's DMA pieces (into stage t-1's
    // buffer) issued between them — the barrier and the next stage's first LDS
    // latency sit behind this wave's own MFMAs.  lgkmcnt counts this wave's
    // transposed reads in issue order (at most 15 outstanding: waits of 8 and 12).
    // A step with no stage after it reads none (an asm read whose result is never
    // used leaves its registers free to the compiler while it is in flight).
    const int nsteps = P1 - P0;
    f16x8 dfa[2][2], dfb[2][2], xfr[3][2];
    auto read_d = [&](f16x8 (&d)[2][2], const int mi, const unsigned so) {
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
            d[mi][pl] = cat_tr(ds_tr16<0>(a_ad[mi][pl] + so), ds_tr16<4 * ROW>(a_ad[mi][pl] + so));
    };
    auto read_x = [&](const int v, const unsigned so) {
        const int kk = v / 9, tap = v - 9 * (v / 9), r = tap / 3, s = tap - 3 * (tap / 3);
        const unsigned ro = so + (unsigned)((2 * kk + r) * 2 * LX * ROW);
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
            xfr[v % 3][pl] = cat_tr(ds_tr16<0>(b_ad[s][0][pl] + ro), ds_tr16<0>(b_ad[s][1][pl] + ro));
    };
    auto mfma_v = [&](const f16x8 (&d)[2][2], const int v) {
        const int tap = v % 9;
        const f16x8* xf = xfr[v % 3];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
            acc[mi][tap] = __builtin_amdgcn_mfma_f32_16x16x32_f16(d[mi][0], xf[0], acc[mi][tap], 0, 0, 0);
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
            acc[mi][tap] = __builtin_amdgcn_mfma_f32_16x16x32_f16(d[mi][0], xf[1], acc[mi][tap], 0, 0, 0);
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
            acc[mi][tap] = __builtin_amdgcn_mfma_f32_16x16x32_f16(d[mi][1], xf[0], acc[mi][tap], 0, 0, 0);
    };
    if (nsteps > 0) {
#pragma unroll
        for (int u = 0; u < NS - 1; ++u) issue();           // stages past the end: zero lines, never read
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * SLOTS) : "memory");
        lds_barrier();
        __builtin_amdgcn_sched_barrier(0);
        read_d(dfa, 0, 0u);
        read_d(dfa, 1, 0u);
        read_x(0, 0u);
        read_x(1, 0u);
        unsigned so = 0;
        auto step = [&](const bool next) {
            const unsigned sn = so == (unsigned)((NS - 1) * STAGE) ? 0u : so + STAGE;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                read_x(v + 2, so);
                if (v == 3) read_d(dfb, 0, so + 32 * ROW);
                if (v == 6) read_d(dfb, 1, so + 32 * ROW);
                wait_lgkm(v >= 3 && v <= 8 ? 12 : 8);
                __builtin_amdgcn_sched_barrier(0);
                mfma_v(v < 9 ? dfa : dfb, v);
                __builtin_amdgcn_sched_barrier(0);
            }
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 3) * SLOTS) : "memory");   // stage t+1
            lds_barrier();
            __builtin_amdgcn_sched_barrier(0);
            if (next) {
                read_d(dfa, 0, sn);
                read_d(dfa, 1, sn);
                wait_lgkm(12);                                          // x of v = 16
            } else {
                wait_lgkm(4);
            }
            __builtin_amdgcn_sched_barrier(0);
            mfma_v(dfb, 16);
            __builtin_amdgcn_sched_barrier(0);
            if (next) read_x(0, sn);
            begin_issue();
            piece(0);
            piece(1);
            piece(2);
            wait_lgkm(next ? 12 : 0);                                   // x of v = 17
            __builtin_amdgcn_sched_barrier(0);
            mfma_v(dfb, 17);
            __builtin_amdgcn_sched_barrier(0);
            if (next) read_x(1, sn);
#pragma unroll
            for (int i = 3; i < SLOTS; ++i) piece(i);
            end_issue();
            __builtin_amdgcn_sched_barrier(0);
            so = sn;
        };
        for (int t = 0; t + 1 < nsteps; ++t) step(true);
        step(false);
    }

    // ---- epilogue: the 64 x 576 slab tile through the drained ring in two passes
    // of 32 K rows (one per wave row), stored as 16-B row chunks ----
    const float inv = 1.f / pow2_scale_for(a.amax);
    float* out = a.ws + (long)split * a.K * a.RSC;
    float* T = (float*)smem;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // + the DMAs past the end
    lds_barrier();
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
        if (kh == ps) {
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        T[(16 * mi + 4 * G + e) * WGH_PITCH + tap * 64 + 16 * cb4 + (lane & 15)] = acc[mi][tap][e] * inv;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        lds_barrier();
        for (int e = tid; e < 32 * 144; e += 512) {
            const int row = e / 144, c4 = e - row * 144, tap = c4 >> 4, cc = (c4 & 15) * 4;
            *(f32x4*)(out + (long)(k0 + 32 * ps + row) * a.RSC + tap * a.C + c0 + cc) =
                *(const f32x4*)(T + row * WGH_PITCH + tap * 64 + cc);
        }
        if (ps == 0) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            lds_barrier();
        }
    }
}

// dw[i] = sum_split ws[split][i], fixed order
// Sum of the split-K slabs [splits][n4] (fixed order, deterministic).  G = 1: a
// thread per float4 element, its slabs summed left to right with 16 loads in
// flight; G = 4 (8 loads in flight per thread) (many splits: the small layers' wgrads split over up to ~75
// pixel ranges): the four waves of a block take the same 64 elements, wave g
// summing slabs g, g+4, g+8, ... left to right, and the four partial sums are
// added in wave order through LDS — 4x fewer dependent load round trips per
// element.
template <int G>
__global__ __launch_bounds__(256) void wg_x3_reduce_kernel(long n4, int splits, const f32x4* __restrict__ ws,
                                                          f32x4* __restrict__ dw) {
    constexpr int B = G == 1 ? 16 : 8;      // slab loads in flight per thread
    auto sum_from = [&](long i, int k0, int step) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        bool first = true;
        for (int k = k0; k < splits; k += B * step) {
            f32x4 v[B];
#pragma unroll
            for (int u = 0; u < B; ++u)
                if (k + u * step < splits) v[u] = __builtin_nontemporal_load(&ws[(long)(k + u * step) * n4 + i]);
#pragma unroll
            for (int u = 0; u < B; ++u)
                if (k + u * step < splits) {
                    if (first) s = v[u];
                    else
#pragma unroll
                        for (int e = 0; e < 4; ++e) s[e] += v[u][e];
                    first = false;
                }
        }
        return s;
    };
    if constexpr (G == 1) {
        const long stride = (long)gridDim.x * blockDim.x;
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) dw[i] = sum_from(i, 0, 1);
    } else {
        static_assert(G == 4, "wg_x3_reduce_kernel: G is 1 or 4");
        __shared__ f32x4 part[G][64];
        const int g = threadIdx.x >> 6, l = threadIdx.x & 63;
        for (long b0 = (long)blockIdx.x * 64; b0 < n4; b0 += (long)gridDim.x * 64) {
            const long i = b0 + l;
            if (i < n4 && g < splits) part[g][l] = sum_from(i, g, G);
            __syncthreads();
            if (g == 0 && i < n4) {
                f32x4 s = part[0][l];
                for (int q = 1; q < G && q < splits; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[e] += part[q][l][e];
                dw[i] = s;
            }
            __syncthreads();
        }
    }
}

}  // namespace hkp

using namespace hkp;

extern "C" int64_t hkp_conv_bwd_filter_x3_workspace(const hkp_conv_desc* d) {
    int ho, wo;
    if (hkp_conv_out_hw(d, &ho, &wo) != HKP_OK) return -1;
    int sp, mps, ka, rt;
    wg_x3_plan(d, (long)d->n * ho * wo, wo, &sp, &mps, &ka, &rt);
    return (int64_t)sp * d->k * d->r * d->s * d->c * (int64_t)sizeof(float);
}

extern "C" int hkp_conv2d_bwd_filter_x3(const hkp_conv_desc* d, const uint16_t* x_split, const uint16_t* dy_split,
                                        const uint32_t* dy_amax_bits, float* dw, void* workspace, int64_t ws_bytes,
                                        hkp_stream_t stream) {
    int ho, wo;
    int rc = hkp_conv_out_hw(d, &ho, &wo);
    if (rc) return rc;
    HKP_CHECK_ARG(x_split && dy_split && dw && workspace, "hkp_conv2d_bwd_filter_x3: null tensor");
    HKP_CHECK_ARG(d->in_layout == HKP_LAYOUT_NHWC, "hkp_conv2d_bwd_filter_x3: NHWC convs only");
    HKP_CHECK_ARG(d->k % 64 == 0 && d->c % 32 == 0, "hkp_conv2d_bwd_filter_x3: need Cout%%64==0, Cin%%32==0");
    const long M = (long)d->n * ho * wo;
    HKP_CHECK_ARG(M < (1L << 31), "hkp_conv2d_bwd_filter_x3: too large");
    int sp, mps, ka, rt;
    wg_x3_plan(d, M, wo, &sp, &mps, &ka, &rt);
    const long n = (long)d->k * d->r * d->s * d->c;
    HKP_CHECK_ARG(ws_bytes >= sp * n * (long)sizeof(float), "hkp_conv2d_bwd_filter_x3: workspace %ld < %ld",
                  (long)ws_bytes, sp * n * (long)sizeof(float));
    WgX3Args a;
    a.xs = (const _Float16*)x_split; a.dys = (const _Float16*)dy_split; a.amax = (const unsigned*)dy_amax_bits;
    a.ws = (float*)workspace;
    a.N = d->n; a.H = d->h; a.W = d->w; a.C = d->c; a.K = d->k; a.R = d->r; a.S = d->s;
    a.stride = d->stride; a.pad = d->pad; a.dil = d->dilation; a.Ho = ho; a.Wo = wo;
    a.M = (int)M; a.RSC = d->r * d->s * d->c; a.r_tiles = rt; a.mps = mps;
    a.tiles = (d->k / (ka ? ka : 64)) * rt;
    hipStream_t st = as_stream(stream);
    const unsigned grid = (unsigned)(a.tiles * sp);
    if (ka == 0) hipLaunchKernelGGL(wgrad_x3_halo_kernel, dim3(grid), dim3(512), 0, st, a);
    else if (ka == 256) hipLaunchKernelGGL(wgrad_x3_kernel<256>, dim3(grid), dim3(512), 0, st, a);
    else if (ka == 128) hipLaunchKernelGGL(wgrad_x3_kernel<128>, dim3(grid), dim3(512), 0, st, a);
    else hipLaunchKernelGGL(wgrad_x3_kernel<64>, dim3(grid), dim3(512), 0, st, a);
    HKP_LAUNCH_CHECK("hkp_conv2d_bwd_filter_x3");
    if (sp > 16) {
        long g = (n / 4 + 63) / 64;
        if (g > 4096) g = 4096;
        hipLaunchKernelGGL(wg_x3_reduce_kernel<4>, dim3((unsigned)g), dim3(256), 0, st, n / 4, sp,
                           (const f32x4*)workspace, (f32x4*)dw);
    } else {
        long g = (n / 4 + 255) / 256;
        if (g > 4096) g = 4096;
        hipLaunchKernelGGL(wg_x3_reduce_kernel<1>, dim3((unsigned)g), dim3(256), 0, st, n / 4, sp,
                           (const f32x4*)workspace, (f32x4*)dw);
    }
    HKP_LAUNCH_CHECK("hkp_conv2d_bwd_filter_x3 (reduce)");
    return HKP_OK;
}
