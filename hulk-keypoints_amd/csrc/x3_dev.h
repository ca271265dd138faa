// Device-side pieces shared by the f16x3 conv families: the forward / dgrad / stem
// kernels of conv_x3.hip (with x3_halo.h, x3_stem.h, x3_duo.h) and the weight
// gradient of wgrad_x3.hip.  The argument block of the forward kernels, the
// epilogue store, the debug stamps, the LDS barriers and the LDS-DMA helpers.
#pragma once

#include "common.h"

namespace hkp {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// The zero line and the NaN line have internal linkage: every translation unit
// that includes this header holds its own copy (one device symbol and one host
// shadow per unit; nothing reads them from the host).
static __device__ __attribute__((aligned(256))) uint4 g_x3_zero_line[8];   // 128 B of zeros (static, zero-initialised)
// 128 B of all-ones bytes: a NaN in fp32 and in fp16.  The halo body's
// out-of-image lines when it applies the input's BN itself (X3Args::in_ss):
// relu(NaN * s + t) = 0 for any s, t, as a zero-padded post-ReLU input.
static __device__ __attribute__((aligned(256))) uint4 g_x3_nan_line[8] = {
    {~0u, ~0u, ~0u, ~0u}, {~0u, ~0u, ~0u, ~0u}, {~0u, ~0u, ~0u, ~0u}, {~0u, ~0u, ~0u, ~0u},
    {~0u, ~0u, ~0u, ~0u}, {~0u, ~0u, ~0u, ~0u}, {~0u, ~0u, ~0u, ~0u}, {~0u, ~0u, ~0u, ~0u}};

struct X3Args {
    const _Float16* xs;
    const _Float16* ws;
    const float* wscale;   // per output channel inverse weight scale [K] (nullable: 1)
    float* y;              // fp32 output, or
    _Float16* y16 = nullptr;   // fp16 output (plain-fp16 path, autocast semantics)
    float* part;
    const unsigned* amax;  // max|input| bits: the input was scaled by pow2_scale_for(amax) (dgrad)
    const float* add;      // addend of the output (dgrad: the residual-branch gradient), nullable
    int N, H, W, C, K, R, S, stride, pad, dil, Ho, Wo;
    int M, nks, cch, n_tiles, RS;
    long plane;            // STEM: halves between the hi and lo image planes
    // phase output (strided dgrad): output pixel (n, ho, wo) of this launch is
    // written at (n, ho*ost + oy, wo*ost + ox) of an [N][OH][OW][K] tensor; ost = 0: dense
    int ost = 0, OH = 0, OW = 0, oy = 0, ox = 0;
    // stream-K (sk_units > 0): the grid's blocks split tiles x K-steps into equal
    // unit ranges; a tile split between blocks is summed by its last-arriving
    // block from per-segment fp32 slabs (sk_ws) — sk_cnt[tile] arrival counters,
    // zero on entry and left zero
    int mt0 = 0;           // m-tile offset of this launch (the split-K tail launch of conv_x3_tail_kernel)
    // region base (a region of conv_x3_a3_mix_kernel; 0 everywhere else): the tiles'
    // rows start at m_base — tile mt is rows m_base + (mt + mt0) * BM — and their BN
    // partial tiles at part_base
    int m_base = 0, part_base = 0;
    // mixed-height launch (conv_x3_a3_mix_kernel): blocks [0, mix_b1) are the 256-row
    // region's tiles, [mix_b1, mix_b2) the 192-row region's (from row mix_m1, partial
    // tile mix_p1), the rest the 160-row region's (mix_m2, mix_p2); a region may be empty
    int mix_b1 = 0, mix_b2 = 0, mix_m1 = 0, mix_m2 = 0, mix_p1 = 0, mix_p2 = 0;
    long sk_units = 0;
    float* sk_ws = nullptr;
    unsigned* sk_cnt = nullptr;
    // the stream-K grid sk_combine works in when it is not the launch's grid: its
    // block count (0: gridDim.x) and this block's index in it (after the XCD remap)
    int sk_grid = 0, sk_b = 0;
    // split-K tail (every group's range inside one m-tile): one slab per group
    // (slot gg * n_tiles + nt) instead of the stream-K grid's two
    int sk_one = 0;
    // A3 launches with the split-K tail appended (conv_x3_a3_kernel): blocks
    // [0, main_blocks) run the full rounds' tiles, the rest the tail's segments —
    // tail_groups groups of n_tiles blocks over tail_units (m-tile, K-step) units
    // from m-tile tail_mt0 (the one-launch form of conv_x3_tail_kernel)
    int main_blocks = 0, tail_groups = 0, tail_mt0 = 0;
    long tail_units = 0;
    unsigned long long* stamps = nullptr;   // debug: per-block phase clocks (hkp_debug_x3_stamps)
    // first-round stagger: blocks b < stagger_blocks with (b >> 3) & 1 (half the CUs
    // of every XCD) wait stagger_ticks (s_memrealtime, 100 MHz) before starting, so
    // the CUs' epilogues (HBM-bound stores) do not all coincide with each other
    int stagger_blocks = 0, stagger_ticks = 0;
    // fused BN apply of the output (P 1, hkp_conv2d_fwd_f16_bn): out = [relu](y*s + t
    // [+ res | + res*rs + rt]) on the fp16-rounded y, bn_apply_f16's arithmetic
    const float* ep_ss = nullptr;          // [2K] scale | shift
    const _Float16* ep_res = nullptr;      // residual [M][K] fp16, nullable
    const float* ep_rss = nullptr;         // residual scale | shift [2K], nullable (raw residual)
    int ep_relu = 0;
    // fused input BN (the halo body, inference): xs is the producer conv's raw
    // NHWC output (fp32 for P 3, fp16 for P 1) and the A operand is
    // relu(x * s + t) — bn_apply's arithmetic — split into hi | lo (P 3) in LDS
    const float* in_ss = nullptr;          // [2C] scale | shift
    // epilogue output stores (A/B: hkp_debug_x3_store): 0 each site's own flavour,
    // 1 plain, 2 nontemporal, 3 sc1 (written through, not kept in the XCD's L2), 4 sc0 sc1
    int st_kind = 0;
    // A/B (hkp_debug_x3_prio): static wave priority in the A3 K loop — 0 none, 1
    // s_setprio 1 on waves 4-7 (the second wave on each SIMD), 2 on waves 0-3
    int prio = 0;
#ifdef HKP_AB_KNOBS
    // A/B probe (hkp_debug_x3_a_wrap): the one-tile and DUO bodies read the A operand of row
    // m from row m % a_wrap (0: off) — wrong outputs, but an L2-resident A stream —
    // to time a conv's K loop without the activation lines' HBM / MALL latency
    int a_wrap = 0;
#endif
};

// One 16-B epilogue output store of flavour `kind` (X3Args::st_kind); dflt: the
// site's own flavour for kind 0 (1 plain, 2 nontemporal).  Measured per site
// (tools/conv_ab.py / infer_ab.py --stores, profiles/r05_store_ab.log): the fp32
// ring-body tile nontemporal (C2 +0.8 %); the plain-fp16 tile plain (C4: nt -0.4 %,
// sc1 -1.6 % end to end, although nt wins 4-7 % per conv in isolation), the fused
// BN epilogue nontemporal
typedef unsigned x3u32x4 __attribute__((ext_vector_type(4)));
template <typename V>
__device__ __forceinline__ void x3_st16(V* p, const V& val, int kind, int dflt) {
    static_assert(sizeof(V) == 16, "16-B store");
    x3u32x4 v;
    __builtin_memcpy(&v, &val, 16);
    x3u32x4* q = (x3u32x4*)p;
    const int k = kind ? kind : dflt;
    if (k == 2) {
        __builtin_nontemporal_store(v, q);
    } else if (k == 3) {
        asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(q), "v"(v) : "memory");
    } else if (k == 4) {
        asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" ::"v"(q), "v"(v) : "memory");
    } else {
        *q = v;
    }
}

// debug phase stamps (s_memrealtime, 100 MHz) of one-tile conv blocks: slot k of
// block b at stamps[b * 8 + k]; written by lane 0 of wave 0
__device__ __forceinline__ void x3_stamp(const X3Args& a, int k) {
    if (a.stamps && threadIdx.x == 0) a.stamps[blockIdx.x * 8 + k] = __builtin_amdgcn_s_memrealtime();
}
// debug: where the block runs — slot 6: HW_REG_HW_ID (CU / SH / SE ids), slot 7: HW_REG_XCC_ID
__device__ __forceinline__ void x3_stamp_where(const X3Args& a) {
    if (a.stamps && threadIdx.x == 0) {
        a.stamps[blockIdx.x * 8 + 6] = (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);
        a.stamps[blockIdx.x * 8 + 7] = (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 20);
    }
}

// raw workgroup barrier (no vmcnt(0) drain: LDS-DMA stays in flight across it) +
// compiler fence so no LDS access is moved across it
__device__ __forceinline__ void lds_barrier() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// workgroup barrier for LDS traffic only: this wave's LDS ops retired, no
// vmcnt(0) — __syncthreads() would also wait for every global store of the
// epilogue to complete (~2-5 us under the other CUs' output writes)
__device__ __forceinline__ void lds_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    lds_barrier();
}

__device__ __forceinline__ void glds16(const void* src, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// LDS-DMA through a raw buffer resource: address = base + soffset + voffset; a
// voffset >= num_records (soffset is not range-checked) loads zeros — the
// out-of-image taps and the rows past M cost one v_cndmask instead of a 64-bit
// address select, and the per-K-step tap offset rides in the scalar soffset.
typedef int i32x4 __attribute__((ext_vector_type(4)));
extern "C" __device__ void hkp_raw_buffer_load_lds(i32x4 rsrc, __attribute__((address_space(3))) void* lds, int size,
                                                   int voffset, int soffset, int offset,
                                                   int aux) __asm("llvm.amdgcn.raw.buffer.load.lds");
__device__ __forceinline__ i32x4 buffer_rsrc(const void* base, unsigned bytes) {
    const unsigned long long p = (unsigned long long)base;
    i32x4 r;
    r[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)p);
    r[1] = __builtin_amdgcn_readfirstlane((int)(unsigned)(p >> 32) & 0xFFFF);   // stride 0
    r[2] = __builtin_amdgcn_readfirstlane((int)bytes);                          // num_records
    r[3] = 0x00020000;                                                            // gfx9 raw-buffer config
    return r;
}
__device__ __forceinline__ void blds16(i32x4 rsrc, unsigned voff, unsigned soff, char* lds_wave_base) {
    hkp_raw_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)lds_wave_base, 16, (int)voff, (int)soff, 0, 0);
}

// schedule NM MFMAs and NR ds_reads of one basic block as evenly spread
// groups: MFMA first, then one read after every NM/NR MFMAs
template <int NM, int NR>
__device__ __forceinline__ void interleave() {
    constexpr int per = NM >= NR ? NM / NR : 1;
    constexpr int nr = NM >= NR ? NR : NM;          // reads paired with MFMA groups
#pragma unroll
    for (int k = 0; k < nr; ++k) {
        __builtin_amdgcn_sched_group_barrier(0x008, per, 0);   // MFMA
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);     // ds_read
    }
    if constexpr (NR > nr) __builtin_amdgcn_sched_group_barrier(0x100, NR - nr, 0);
    if constexpr (NM > per * nr) __builtin_amdgcn_sched_group_barrier(0x008, NM - per * nr, 0);
}

}  // namespace hkp
