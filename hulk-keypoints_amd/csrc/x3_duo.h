// Part of conv_x3.hip's translation unit: included there after x3_stem.h (it uses
// conv_x3.hip's epilogue helpers; x3_start launches it).
#pragma once

namespace hkp {

// ---------------------------------------------------------------------------
// DUO body (conv_x3_duo_kernel<1>): plain-fp16 (P 1, config C4) convs on 256 x 128
// tiles run by TWO 4-wave blocks per CU.  The one-tile 256x256 bodies hold a
// whole CU, so each tile's pipeline fill, BN partials, fp16 staging and stores
// run with the CU's matrix pipes idle — on C4's short-K 1x1 GEMMs (8-16 K-steps
// per tile) about half of a tile's time (DESIGN "C4's 1x1 GEMMs").  Here two
// independent blocks share the CU: one block's fill and epilogue run beside the
// other's K loop, and their vmcnt / barriers are separate (a persistent body's
// epilogue stores, by contrast, shared vmcnt with its next tile's DMA).
// Per block: 4 waves as 2 x 2, wave tile 128 x 64 (8 x 4 16x16x32 MFMA tiles,
// 128 accumulator registers); a 3-stage LDS ring of HALF lines — a stage holds
// 32 channels (64 B) of every A row (256) and B row (128): 24 KiB — so three
// stages (72 KiB, which also holds the fp16 epilogue tile) fit twice per CU.
// K order: channel group (64 channels), tap, half; a half-line is one k32 step,
// one MFMA per (16-row, 16-column) pair.  64-B rows: lane l of a DMA piece writes
// row l/4, 16-B chunk l%4; the chunk swizzle (4 - (row >> 2)) & 3 makes every
// ds_read_b128 lane group of the fragment reads (rows r16 = lane & 15, chunk
// lane >> 4) hit 16 distinct 16-B bank groups.  Epilogue: BN partials per
// 128-row half straight from one wave's accumulators (a wave holds a whole
// half: no LDS merge), then the fp16 tile staged in the drained ring and written
// as 16-B row chunks, optionally through the fused BN + residual + ReLU
// (hkp_conv2d_fwd_f16_bn) — the 256x256 body's arithmetic, element for element.
constexpr int DUO_BM = 256, DUO_ROW = 64, DUO_NST = 3;              // (DUO_BN = 128: x3_plan.h)
// first-round arrivals per CU (key: XCC id x the HW_ID's SE / SH / CU bits): the
// second block to arrive on a CU starts late, so the two blocks sharing it run
// half a block apart (see conv_x3_duo_kernel); parity of a running count, never reset
__device__ unsigned g_duo_cu_cnt[8 * 128];
constexpr int DUO_STAGE = (DUO_BM + DUO_BN) * DUO_ROW;                 // 24 KiB
constexpr int DUO_LDS = DUO_NST * DUO_STAGE;                           // 72 KiB: two blocks per CU
static_assert(DUO_BM * (DUO_BN + 8) * 2 + 4 * DUO_BN * 4 <= DUO_LDS, "DUO epilogue staging");

__device__ __forceinline__ int duo_swz(int row) { return (4 - ((row >> 2) & 3)) & 3; }

// BN partials (sum, M2 about the half's mean) of one wave's 128-row half of the
// tile: each lane reduces its 32 rows of a column, then lanes l, l^16, l^32, l^48
// (the column's four row groups) merge by Chan's formula — equal counts, so the
// factors are constants and the result is symmetric in each pair (all four lanes
// hold the same bits).  Rows past M (the last tile) take the counted form.
template <int UM, int UN>
__device__ __forceinline__ void duo_bn_partials(const X3Args& a, const f32x4 (&acc)[UM][UN], const float (&sc)[UN],
                                                int m0h, int ncol0, int lane) {
    const int q = lane >> 4, r16 = lane & 15;
    const long tile128 = (long)(m0h >> 7);
    if (m0h + 128 <= a.M) {                                  // block-uniform
#pragma unroll
        for (int j = 0; j < UN; ++j) {
            f32x4 s4 = acc[0][j];
#pragma unroll
            for (int i = 1; i < UM; ++i) s4 += acc[i][j];
            float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
            constexpr float inv = 1.f / (UM * 4);
            const f32x4 mu = {s * inv, s * inv, s * inv, s * inv};
            f32x4 q4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < UM; ++i) {
                const f32x4 d = acc[i][j] - mu;
                q4 += d * d;
            }
            float m2 = (q4[0] + q4[1]) + (q4[2] + q4[3]);
            x3_chan_merge(s, m2, __shfl_xor(s, 16), __shfl_xor(m2, 16), 1.f / (UM * 4), UM * 2.f);
            x3_chan_merge(s, m2, __shfl_xor(s, 32), __shfl_xor(m2, 32), 1.f / (UM * 8), UM * 4.f);
            if (q == 0) {
                const int c = ncol0 + 16 * j + r16;
                a.part[(tile128 * a.K + c) * 2 + 0] = s * sc[j];
                a.part[(tile128 * a.K + c) * 2 + 1] = m2 * (sc[j] * sc[j]);
            }
        }
        return;
    }
    if (m0h >= a.M) return;
    float ln = 0.f;
#pragma unroll
    for (int i = 0; i < UM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) ln += (m0h + 16 * i + 4 * q + r < a.M) ? 1.f : 0.f;
    const float linv = ln > 0.f ? 1.f / ln : 0.f;
#pragma unroll
    for (int j = 0; j < UN; ++j) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < UM; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) s += (m0h + 16 * i + 4 * q + r < a.M) ? acc[i][j][r] : 0.f;
        const float mu = s * linv;
        float m2 = 0.f;
#pragma unroll
        for (int i = 0; i < UM; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float d = acc[i][j][r] - mu;
                m2 += (m0h + 16 * i + 4 * q + r < a.M) ? d * d : 0.f;
            }
        float n = ln;
        for (int o = 16; o < 64; o <<= 1) {
            const float nb = __shfl_xor(n, o), sb = __shfl_xor(s, o), qb = __shfl_xor(m2, o);
            const float nt = n + nb;
            const float f = nt > 0.f ? n * nb / nt : 0.f;
            const float ia = n > 0.f ? 1.f / n : 0.f, ib = nb > 0.f ? 1.f / nb : 0.f;
            const float d = sb * ib - s * ia;
            s = s + sb;
            m2 = (m2 + qb) + d * d * f;
            n = nt;
        }
        if (q == 0) {
            const int c = ncol0 + 16 * j + r16;
            a.part[(tile128 * a.K + c) * 2 + 0] = s * sc[j];
            a.part[(tile128 * a.K + c) * 2 + 1] = m2 * (sc[j] * sc[j]);
        }
    }
}

template <int P>
__global__ __launch_bounds__(256, 2) void conv_x3_duo_kernel(X3Args a) {
    static_assert(P == 1, "DUO: the plain-fp16 operand layout");
    __shared__ __attribute__((aligned(1024))) char smem[DUO_LDS];
    constexpr int BM = DUO_BM, BN = DUO_BN, ROW = DUO_ROW, NST = DUO_NST, STAGE = DUO_STAGE;
    constexpr int UM = 8, UN = 4;                    // 16x16 tiles per wave (wave tile 128 x 64)
    constexpr int GA = 4, GB = 2, GL = GA + GB;      // DMA pieces (16 rows each) per wave per stage

    x3_stamp(a, 0);
    x3_stamp_where(a);
    // Co-resident blocks of a one-round-per-tile grid start together and, doing the
    // same work, stay in phase: both fill, both run the K loop, both run the
    // epilogue — nothing overlaps.  In the first round the second block to arrive
    // on each CU waits about half a block's lifetime (X3Args::stagger_ticks), so
    // from then on one block's fill and epilogue run beside the other's K loop.
    if (a.stagger_ticks > 0 && blockIdx.x < (unsigned)a.stagger_blocks) {
        __shared__ int late;
        if (threadIdx.x == 0) {
            const unsigned hw = (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);     // HW_REG_HW_ID
            const unsigned xcc = (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 20);   // HW_REG_XCC_ID
            const unsigned key = (xcc & 7) * 128 + ((hw >> 8) & 127);
            late = (int)(atomicAdd(&g_duo_cu_cnt[key], 1u) & 1u);
        }
        __syncthreads();
        if (late) {
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
            while (__builtin_amdgcn_s_memrealtime() - t0 < (unsigned long long)a.stagger_ticks) __builtin_amdgcn_s_sleep(8);
        }
    }
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int mt = tile / a.n_tiles, nt = tile - mt * a.n_tiles;
    const int m0 = mt * BM, n0 = nt * BN;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = w >> 1, wn = w & 1;
    const int nst = 2 * a.nks;                       // half-line stages

    // ---- DMA sources (the one-tile bodies' bookkeeping, 64-B rows) ----
    const int cstride = a.cch * 64;                  // halves per pixel
    const long xbias = (long)a.pad * (a.W + 1) * cstride;
    const _Float16* xbase = a.xs - xbias;
    const _Float16* zero = (const _Float16*)g_x3_zero_line;
    int a_org[GA];
    unsigned a_off[GA];
#pragma unroll
    for (int i = 0; i < GA; ++i) {
        const int row = 64 * w + 16 * i + (lane >> 2);
        const int Lc = (lane & 3) ^ duo_swz(row);
#ifdef HKP_AB_KNOBS
        const int m = a.a_wrap ? (m0 + row) % a.a_wrap : m0 + row;
#else
        const int m = m0 + row;
#endif
        int hb = -16384, wb = -16384;
        long off = 0;
        if (m < a.M) {
            const int hw = a.Ho * a.Wo;
            const int n = m / hw, rem = m - n * hw;
            const int ho = rem / a.Wo, wo = rem - ho * a.Wo;
            hb = ho * a.stride - a.pad;
            wb = wo * a.stride - a.pad;
            off = (((long)n * a.H + hb) * a.W + wb) * cstride + Lc * 8;
        }
        a_org[i] = (int)(((unsigned)hb << 16) | ((unsigned)wb & 0xFFFFu));
        a_off[i] = (unsigned)(off + xbias);
    }
    const int bline = a.RS * a.cch * 64;             // halves per weight row
    int b_off[GB];
#pragma unroll
    for (int j = 0; j < GB; ++j) {
        const int row = 32 * w + 16 * j + (lane >> 2);
        b_off[j] = (n0 + row) * bline + ((lane & 3) ^ duo_swz(row)) * 8;
    }
    // staging position of the next stage to issue: (channel group, tap, half)
    int q_buf = 0, q_cc = 0, q_tap = 0, q_rr = 0, q_ss = 0, q_half = 0;
    auto issue = [&]() {
        char* st = smem + q_buf * STAGE;
        const int dh = q_rr * a.dil, dw = q_ss * a.dil;
        const long toff = ((long)dh * a.W + dw) * cstride + q_cc * 64 + q_half * 32;
#pragma unroll
        for (int i = 0; i < GA; ++i) {
            const int hb = a_org[i] >> 16, wb = (int)(short)(a_org[i] & 0xFFFF);
            const bool in = (unsigned)(hb + dh) < (unsigned)a.H && (unsigned)(wb + dw) < (unsigned)a.W;
            glds16(in ? xbase + ((unsigned long)a_off[i] + toff) : zero, st + (64 * w + 16 * i) * ROW);
        }
        const int boff = (q_tap * a.cch + q_cc) * 64 + q_half * 32;
#pragma unroll
        for (int j = 0; j < GB; ++j) glds16(a.ws + (unsigned)(b_off[j] + boff), st + (BM + 32 * w + 16 * j) * ROW);
        q_buf = q_buf == NST - 1 ? 0 : q_buf + 1;
        if (++q_half == 2) {
            q_half = 0;
            if (++q_ss == a.S) {
                q_ss = 0;
                ++q_rr;
            }
            if (++q_tap == a.RS) {
                q_tap = 0;
                q_rr = 0;
                ++q_cc;
            }
        }
    };

    // ---- fragments: lane reads row r16 of a 16-row tile, logical chunk q ----
    const int r16 = lane & 15, q = lane >> 4;
    const int fo = r16 * ROW + ((q ^ duo_swz(r16)) << 4);
    const int a_base = (wm * 128) * ROW + fo, b_base = (BM + wn * 64) * ROW + fo;
    f32x4 acc[UM][UN];
#pragma unroll
    for (int i = 0; i < UM; ++i)
#pragma unroll
        for (int j = 0; j < UN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    f16x8 fa[UM], fb[UN];
    auto read_a = [&](const char* st) {
#pragma unroll
        for (int i = 0; i < UM; ++i) fa[i] = *(const f16x8*)(st + a_base + i * 16 * ROW);
    };
    auto read_b = [&](int j, const char* st) { fb[j] = *(const f16x8*)(st + b_base + j * 16 * ROW); };
    auto mma_col = [&](int j) {
#pragma unroll
        for (int i = 0; i < UM; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    };

    // column scales (weight scale), issued before the fill
    float sc[UN];
#pragma unroll
    for (int j = 0; j < UN; ++j) sc[j] = a.wscale ? a.wscale[n0 + wn * 64 + 16 * j + r16] : 1.f;

    // ---- pipeline (the 3-stage ring schedule of conv_x3_mf16_body): per stage t —
    // wait own DMA of t+1 (t+2 stays in flight), barrier, DMA of t+3 into t's
    // buffer (its fragments were read during step t-1) spread over the columns,
    // per column j [MFMAs of t with B_j] [read B_j of t+1], then A of t+1 ----
    for (int s = 0; s < NST; ++s)
        if (s < nst) issue();
    {
        const int after = min(nst, NST) - 1;
        if (after >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * GL) : "memory");
        else if (after == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GL) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    lds_barrier();
    x3_stamp(a, 1);
    read_a(smem);
#pragma unroll
    for (int j = 0; j < UN; ++j) read_b(j, smem);
    int cur = 0;
    auto kstep = [&](const int t, const bool dma) {
        if (t + 2 < nst) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(GL) : "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        lds_barrier();
        cur = cur == NST - 1 ? 0 : cur + 1;
        const char* st = smem + cur * STAGE;
        if (dma) issue();
#pragma unroll
        for (int j = 0; j < UN; ++j) {
            mma_col(j);
            read_b(j, st);
        }
        read_a(st);
#pragma unroll
        for (int j = 0; j < UN; ++j) {
            __builtin_amdgcn_sched_group_barrier(0x008, UM, 0);     // column j's MFMAs
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      // refill B_j
            if (dma && j * ((GL + UN - 1) / UN) < GL)
                __builtin_amdgcn_sched_group_barrier(0x020, (GL + UN - 1) / UN, 0);   // DMA pieces
        }
        __builtin_amdgcn_sched_group_barrier(0x100, UM, 0);         // next A frags
        __builtin_amdgcn_sched_barrier(0);
    };
    int t = 0;
    for (; t + 3 < nst; ++t) kstep(t, true);
    for (; t + 1 < nst; ++t) kstep(t, false);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int j = 0; j < UN; ++j) mma_col(j);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // no DMA in flight into the ring past here
    x3_stamp(a, 2);

    // ---- epilogue: BN partials of this wave's 128-row half, then the fp16 tile ----
    if (a.part) duo_bn_partials<UM, UN>(a, acc, sc, m0 + 128 * wm, n0 + wn * 64, lane);
    x3_stamp(a, 3);
    constexpr int PITCH = BN + 8, CH = BN / 8, SS_OFF = BM * PITCH * 2;
    constexpr int NT = 256, NPT = BM * CH / NT;              // 16-B chunks per thread
    static_assert(NT % CH == 0, "a thread keeps its 8 channels");
    const int cc = tid % CH;
    // fused BN epilogue: per-column parameters and the residual chunks in flight
    // before the tile is staged (their latency hides behind it)
    float ep0 = 0.f, ep1 = 0.f;
    f16x8 res[NPT];
    if (a.ep_ss) {
        const int h = tid / BN, c = tid - h * BN;                // tid < 2 * BN: all 256 threads
        ep0 = a.ep_ss[h * a.K + n0 + c];
        ep1 = a.ep_rss ? a.ep_rss[h * a.K + n0 + c] : 0.f;
#pragma unroll
        for (int u = 0; u < NPT; ++u) {
            const int row = (tid + NT * u) / CH, m = m0 + row;
            res[u] = f16x8{};
            if (a.ep_res && m < a.M)
                res[u] = __builtin_nontemporal_load((const f16x8*)(a.ep_res + (long)m * a.K + n0 + cc * 8));
        }
    }
    lds_sync();                                              // every wave done reading the ring
    _Float16* tl = (_Float16*)smem;
#pragma unroll
    for (int i = 0; i < UM; ++i)
#pragma unroll
        for (int j = 0; j < UN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                tl[(wm * 128 + i * 16 + 4 * q + r) * PITCH + wn * 64 + j * 16 + r16] = (_Float16)(acc[i][j][r] * sc[j]);
    float* ssl = (float*)(smem + SS_OFF);                    // [4][BN]: scale, shift, residual scale, shift
    if (a.ep_ss) {
        ssl[tid] = ep0;
        ssl[2 * BN + tid] = ep1;
    }
    lds_sync();
    x3_stamp(a, 4);
    if (!a.ep_ss) {
#pragma unroll 4
        for (int u = 0; u < NPT; ++u) {
            const int row = (tid + NT * u) / CH, m = m0 + row;
            if (m < a.M)
                x3_st16((uint4*)(a.y16 + (long)m * a.K + n0 + cc * 8), *(const uint4*)(smem + (row * PITCH + cc * 8) * 2), a.st_kind, 1);
        }
        x3_stamp(a, 5);
        return;
    }
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
    for (int u = 0; u < NPT; ++u) {
        const int row = (tid + NT * u) / CH, m = m0 + row;
        if (m >= a.M) continue;
        const f16x8 v = *(const f16x8*)(smem + (row * PITCH + cc * 8) * 2);
        const f16x8 rv = res[u];
        f16x8 h;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float o = __fadd_rn(__fmul_rn((float)v[k], sa[k]), sb[k]);
            if (hres) o = rsc ? __fadd_rn(o, __fadd_rn(__fmul_rn((float)rv[k], ra[k]), rb[k])) : __fadd_rn(o, (float)rv[k]);
            if (relu) o = o > 0.f ? o : 0.f;
            h[k] = (_Float16)o;
        }
        x3_st16((f16x8*)(a.y16 + (long)m * a.K + n0 + cc * 8), h, a.st_kind, 2);
    }
    x3_stamp(a, 5);
}

}  // namespace hkp
