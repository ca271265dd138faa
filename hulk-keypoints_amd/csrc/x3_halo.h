// Part of conv_x3.hip's translation unit: included there after the ring / A3 / tail
// kernels (it uses their epilogue helpers; x3_start launches it).
#pragma once

namespace hkp {

// ---------------------------------------------------------------------------
// Halo-tile body (conv_x3_halo_kernel<P>) for stride-1 3x3 convs with pad =
// dilation = 1 whose output tiles exactly into 8 x 32 pixel patches (Ho % 8 ==
// 0, Wo % 32 == 0): layer1 of every R-net here (64 channels at 120x160 in
// C2-C4, 240x320 in C5), forward and stride-1 dgrad.  The one-tile kernels
// stage, per K-step, a tap-shifted 256-row A window — every input line is
// fetched from L2 nine times, and at Cin = 64 (2 channel groups x 9 taps) the
// 256x64 tile is bound by that operand stream, not by its MFMAs.  Here a tile is
// an 8 x 32 patch of one image: per channel group its (8+2) x (32+2) = 340
// input lines are staged ONCE by LDS-DMA into a halo image and the nine taps
// read their fragments from it (tile row m = pixel (m/32, m%32) reads halo line
// (m/32 + r) * 34 + m%32 + s for tap (r, s)); only the 64-row weight stage
// streams per K-step (a 3-slot ring).  A tile moves 2 x 42.5 + 18 x 8 = 229 KB
// from L2 instead of 18 x 40 = 720 KB.  Lines past the image are zero lines.
// The 16-B chunk swizzle (halo_swz: line & 6) is keyed on the halo line, so any
// 16 consecutive lines a fragment read touches are conflict-free, as in the ring.
// Two blocks per CU (72 KB each): one block's halo reload / epilogue overlaps the
// other's MFMAs.  256 x 64 tile, 8 waves 4 x 2 (wave tile 64 x 32), 16x16x32
// MFMAs; epilogue = the one-tile kernels' (BN tile partials from the
// accumulators, LDS-staged 16-B row chunks), rows remapped to the patch pixels.
constexpr int HALO_LW = HALO_PW + 2, HALO_NL = (HALO_PH + 2) * HALO_LW;   // 340 lines (HALO_PH x HALO_PW patches: x3_plan.h)
constexpr int HALO_GA = 6;                                   // halo DMA instructions per wave (48 x 8 lines >= 340)
constexpr int HALO_ABYTES = 8 * HALO_GA * 8 * 128;           // 48 KiB: halo image (+ 44 dummy lines)
constexpr int HALO_NSTB = 3, HALO_BSTAGE = 64 * 128;         // weight ring: 3 x 8 KiB
constexpr int HALO_LDS = HALO_ABYTES + HALO_NSTB * HALO_BSTAGE;

// 16-B chunk swizzle of halo line L: physical chunk = logical ^ (L & 6).  A
// fragment read covers 16 consecutive lines from ANY start (the tap offsets and
// the 34-line patch rows put it anywhere), so the ring bodies' (row >> 1) & 7 —
// conflict-free only from a 4-aligned start — cost ~3 extra LDS cycles per
// ds_read_b128 here (0.30 of the halo kernels' LDS cycles, PMC r04); keyed on
// bits 1-2 of L alone, every ds_read_b128 lane group of a read from any start
// line hits 16 distinct 16-B bank slots (bit 0 of L picks the 128-B half, and the
// group's two q values differ in bit 0 of the chunk).
__device__ __forceinline__ int halo_swz(int L) { return L & 6; }

// BNIN: the input is the producer's raw output and its BN + ReLU (+ the f16x3
// split, P 3) is applied to each channel group's halo image in LDS after it
// lands (X3Args::in_ss) — the bn_apply pass between the two convs disappears.
// Each lane transforms whole 8-channel pieces: P 3 reads the piece's two fp32
// chunks and writes its hi and lo chunks in place (the four pieces of a line are
// four adjacent lanes of one wave instruction, so every read of the line precedes
// its writes); P 1 rewrites one fp16 chunk.  Out-of-image lines are NaN lines
// (relu(NaN*s + t) = 0).
template <int P, bool BNIN>
__device__ __forceinline__ void x3_halo_bnin(const X3Args& a, char* smem, int g, int tid) {
    constexpr int ROW = 128;
    constexpr int PIECES = P == 1 ? 8 : 4;                       // 8-channel pieces per line
    constexpr int LPI = 512 / PIECES;                            // lines per block-wide pass
    constexpr int NL = 8 * HALO_GA * 8;                          // halo lines incl. the dummies (384)
    const int j = tid % PIECES;
    const int c0 = g * (P == 1 ? 64 : 32) + 8 * j;
    float sa[8], sb[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        sa[e] = a.in_ss[c0 + e];
        sb[e] = a.in_ss[a.C + c0 + e];
    }
#pragma unroll
    for (int L0 = 0; L0 < NL; L0 += LPI) {
        const int L = L0 + tid / PIECES;
        const int sw = halo_swz(L);
        char* line = smem + L * ROW;
        if constexpr (P == 1) {
            f16x8* ch = (f16x8*)(line + ((j ^ sw) << 4));
            const f16x8 v = *ch;
            f16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float x = __fadd_rn(__fmul_rn((float)v[e], sa[e]), sb[e]);
                o[e] = (_Float16)(x > 0.f ? x : 0.f);
            }
            *ch = o;
        } else {
            const f32x4 v0 = *(const f32x4*)(line + (((2 * j) ^ sw) << 4));
            const f32x4 v1 = *(const f32x4*)(line + (((2 * j + 1) ^ sw) << 4));
            f16x8 h, l;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float y = e < 4 ? v0[e] : v1[e - 4];
                float x = __fadd_rn(__fmul_rn(y, sa[e]), sb[e]);
                x = x > 0.f ? x : 0.f;
                const _Float16 hv = (_Float16)x;
                h[e] = hv;
                l[e] = (_Float16)(x - (float)hv);
            }
            *(f16x8*)(line + ((j ^ sw) << 4)) = h;
            *(f16x8*)(line + (((4 + j) ^ sw) << 4)) = l;
        }
    }
}

template <int P, bool BNIN>
__device__ __forceinline__ void conv_x3_halo_body(const X3Args& a, char* smem) {
    constexpr int BM = 256, BN = 64, WM = 4, WN = 2, ROW = 128;
    constexpr int UM = BM / (WM * 16), UN = BN / (WN * 16);     // 4 x 2 16x16 sub-tiles per wave
    static_assert(256 * (BN + 4) * 4 <= HALO_LDS && 8 * BN * 4 <= HALO_LDS, "epilogue staging");
    static_assert(!BNIN || P == 3 || P == 1, "fused input BN: f16x3 or plain fp16");

    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int mt = tile / a.n_tiles, nt = tile - mt * a.n_tiles;
    const int pwn = a.Wo / HALO_PW, tpi = (a.Ho / HALO_PH) * pwn;
    const int img = mt / tpi, rem = mt - img * tpi;
    const int h0 = (rem / pwn) * HALO_PH, w0 = (rem - (rem / pwn) * pwn) * HALO_PW;
    const int m0 = mt * BM, n0 = nt * BN;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = w / WN, wn = w % WN;
    const int cstride = a.cch * 64;                             // halves per pixel
    const int nks = a.nks;                                      // 9 taps x channel groups
    const _Float16* zero = (const _Float16*)(BNIN ? g_x3_nan_line : g_x3_zero_line);

    // ---- halo DMA: instruction i of wave w fills lines 8 (w*GA + i) .. +7 ----
    unsigned h_off[HALO_GA];                                    // element offsets from a.xs (or ~0u: zero line)
#pragma unroll
    for (int i = 0; i < HALO_GA; ++i) {
        const int L = 8 * (w * HALO_GA + i) + lane / 8;
        const int Lc = (lane % 8) ^ halo_swz(L);
        const int hl = L / HALO_LW, wl = L - hl * HALO_LW;
        const int hi = h0 - 1 + hl, wi = w0 - 1 + wl;
        const bool in = L < HALO_NL && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
        h_off[i] = in ? (unsigned)((((long)img * a.H + hi) * a.W + wi) * cstride + Lc * 8) : ~0u;
    }
    auto issue_halo = [&](int g) {
#pragma unroll
        for (int i = 0; i < HALO_GA; ++i)
            glds16(h_off[i] != ~0u ? a.xs + ((unsigned long)h_off[i] + g * 64) : zero,
                   smem + 8 * (w * HALO_GA + i) * ROW);
    };
    // ---- weight stage DMA: one instruction per wave, rows 8w .. 8w+7 ----
    const int brow = 8 * w + lane / 8;
    const int bline = a.RS * a.cch * 64;
    const unsigned b_off = (unsigned)((n0 + brow) * bline + (((lane % 8) ^ ((brow >> 1) & 7)) * 8));
    auto issue_b = [&](int t) {
        const int g = t / 9, u = t - g * 9;
        glds16(a.ws + (b_off + (unsigned)((u * a.cch + g) * 64)),
               smem + HALO_ABYTES + (t % HALO_NSTB) * HALO_BSTAGE + 8 * w * ROW);
    };

    // ---- fragment addressing ----
    const int r16 = lane & 15, q = lane >> 4;
    int lb[UM];                                                 // halo line of tap (0, 0) for sub-tile i
#pragma unroll
    for (int i = 0; i < UM; ++i) {
        const int m = wm * 64 + 16 * i + r16;
        lb[i] = (m >> 5) * HALO_LW + (m & 31);
    }
    const int sw = (r16 >> 1) & 7;                              // B rows: 16-row tiles, as the ring's
    const int fb_h = (wn * 32 + r16) * ROW + ((q ^ sw) << 4), fb_l = (wn * 32 + r16) * ROW + (((4 + q) ^ sw) << 4);

    f32x4 acc[UM][UN];
#pragma unroll
    for (int i = 0; i < UM; ++i)
#pragma unroll
        for (int j = 0; j < UN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto mfma = [](const f16x8& x, const f16x8& y, const f32x4& c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(x, y, c, 0, 0, 0);
    };

    // column scale (weight scale x gradient scale), issued before the pipeline
    const float ginv = a.amax ? 1.f / pow2_scale_for(a.amax) : 1.f;
    float scv[UN];
#pragma unroll
    for (int j = 0; j < UN; ++j) scv[j] = (a.wscale ? a.wscale[n0 + wn * 32 + 16 * j + r16] : 1.f) * ginv;

    // prologue: halo of group 0, weight stages 0 and 1
    issue_halo(0);
    issue_b(0);
    if (nks > 1) issue_b(1);
    if (nks > 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();
    if constexpr (BNIN) {
        x3_halo_bnin<P, BNIN>(a, smem, 0, tid);
        lds_sync();
    }
    for (int t = 0; t < nks; ++t) {
        const int g = t / 9, u = t - g * 9;
        const int toff = (u / 3) * HALO_LW + (u - (u / 3) * 3);
        // fragments of step t
        f16x8 ah[UM], al[UM], bh[UN], bl[UN];
#pragma unroll
        for (int i = 0; i < UM; ++i) {
            const int L = lb[i] + toff;
            const int ls = halo_swz(L);
            ah[i] = *(const f16x8*)(smem + L * ROW + ((q ^ ls) << 4));
            al[i] = *(const f16x8*)(smem + L * ROW + (((4 + q) ^ ls) << 4));
        }
        const char* bst = smem + HALO_ABYTES + (t % HALO_NSTB) * HALO_BSTAGE;
#pragma unroll
        for (int j = 0; j < UN; ++j) {
            bh[j] = *(const f16x8*)(bst + j * 16 * ROW + fb_h);
            bl[j] = *(const f16x8*)(bst + j * 16 * ROW + fb_l);
        }
        // weight stage t+2 goes into the slot step t-1 read (every wave is past
        // this step's barrier, so done reading it)
        if (t + 2 < nks) issue_b(t + 2);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < UM; ++i)
#pragma unroll
            for (int j = 0; j < UN; ++j) x3_products<P>(acc[i][j], ah[i], al[i], bh[j], bl[j], mfma);
        if (t + 1 >= nks) break;
        if (u == 8) {
            // the group's last tap: every wave done with the halo, then the next
            // group's halo (the youngest DMA: wait for everything)
            lds_barrier();
            issue_halo(g + 1);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if constexpr (BNIN) {
                lds_barrier();                                   // the whole halo landed
                x3_halo_bnin<P, BNIN>(a, smem, g + 1, tid);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
        } else if (t + 2 < nks) {
            asm volatile("s_waitcnt vmcnt(1)" ::: "memory");     // stage t+1 landed, t+2 in flight
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        lds_barrier();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---- epilogue: BN tile partials (rows all valid: exact patch tiling), then
    // the scaled tile staged through the drained LDS and written as 16-B row
    // chunks; tile row m -> pixel (img, h0 + m/32, w0 + m%32) ----
    const int rbase = m0 + wm * UM * 16 + 4 * q;
    lds_sync();                                                  // every wave done with the halo / ring
    if (a.part) {
        x3_bn_partials_w<BN, UM, UN, 16, 16>(
            a, (float*)smem, m0, n0, wm, wn, lane, [&](int i, int j) { return acc[i][j]; },
            [&](int i, int r) { return rbase + i * 16 + r; }, [&](int j) { return scv[j]; }, (float*)smem);
        lds_sync();
    }
    auto out_pix = [&](int row) { return ((long)img * a.Ho + h0 + (row >> 5)) * a.Wo + w0 + (row & 31); };
    if constexpr (P == 1) {
        constexpr int PITCH = BN + 8, CH = BN / 8;
        _Float16* st = (_Float16*)smem;
#pragma unroll
        for (int i = 0; i < UM; ++i)
#pragma unroll
            for (int j = 0; j < UN; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    st[(wm * UM * 16 + i * 16 + 4 * q + r) * PITCH + wn * 32 + j * 16 + r16] =
                        (_Float16)(acc[i][j][r] * scv[j]);
        lds_sync();
#pragma unroll 4
        for (int e = tid; e < BM * CH; e += 512) {
            const int row = e / CH, cc = e - row * CH;
            x3_st16((uint4*)(a.y16 + out_pix(row) * a.K + n0 + cc * 8), *(const uint4*)(smem + (row * PITCH + cc * 8) * 2), a.st_kind, 1);
        }
    } else {
        constexpr int PITCH = BN + 4, C4 = BN / 4;
        float* st = (float*)smem;
#pragma unroll
        for (int i = 0; i < UM; ++i)
#pragma unroll
            for (int j = 0; j < UN; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    st[(wm * UM * 16 + i * 16 + 4 * q + r) * PITCH + wn * 32 + j * 16 + r16] = acc[i][j][r] * scv[j];
        lds_sync();
#pragma unroll 4
        for (int e = tid; e < BM * C4; e += 512) {
            const int row = e / C4, c4 = e - row * C4;
            const long off = out_pix(row) * a.K + n0 + c4 * 4;
            f32x4 v = *(const f32x4*)(st + row * PITCH + c4 * 4);
            if (a.add) {
                const f32x4 ad = *(const f32x4*)(a.add + off);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = v[k] + ad[k];
            }
            *(f32x4*)(a.y + off) = v;
        }
    }
}

template <int P>
__global__ __launch_bounds__(512, 2) void conv_x3_halo_kernel(X3Args a) {
    __shared__ __attribute__((aligned(1024))) char smem[HALO_LDS];
    conv_x3_halo_body<P, false>(a, smem);
}

// the same with the input's BN + ReLU applied to each halo image (X3Args::in_ss)
template <int P>
__global__ __launch_bounds__(512, 2) void conv_x3_halo_bnin_kernel(X3Args a) {
    __shared__ __attribute__((aligned(1024))) char smem[HALO_LDS];
    conv_x3_halo_body<P, true>(a, smem);
}

}  // namespace hkp
