// How an f16x3 / plain-fp16 conv is launched (conv_x3.hip; wg_x3_plan: wgrad_x3.hip),
// decided on the host: the body, the tile height and width, stream-K or not, the split-K tail, the mixed-height
// regions, the grids and the BN-partial tile sizes, as one plan (x3_launch_plan) that
// the launcher, the kernel-name query and the BN-partial layout queries all read.
// Plain C++17: nothing here asks a GPU runtime for anything — the CU count and the A/B
// knobs are arguments — so the whole decision can be tested and sanitized on a CPU.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "../../include/hulkkp.h"

namespace hkp {

// constants of the kernels that the planner needs too
constexpr int DUO_BN = 128;                    // conv_x3_duo_kernel's tile width
constexpr int HALO_PH = 8, HALO_PW = 32;       // conv_x3_halo_kernel's output patch
constexpr int STEM_PH = 8, STEM_PW = 32;       // conv_x3_stem_patch_kernel's output patch

// operand layout of P: the packed hi|lo split (P 2, 3, 4) or plain fp16 (P 1)
constexpr bool x3_packed(int P) { return P != 1; }

// The A/B knobs the planner reads (tools/ only: the HKP_AB_KNOBS build passes its
// hkp_debug_* values in); the defaults are the product's
struct X3Knobs {
    bool pair128 = true;           // hkp_debug_x3_pair128
    bool split_tail = false;       // hkp_debug_x3_split_tail
    bool stem_pair = false;        // hkp_debug_stem_pair
    int duo_stagger_ns = -1;       // hkp_debug_duo_stagger
};

// the name of kernel id `kernel` (HKP_X3K_*, hulkkp.h) on operand layout P, as rocprofv3 reports it
static int x3_kernel_name(int kernel, int P, char* buf, int len) {
    switch (kernel) {
        case HKP_X3K_TILE_256: return snprintf(buf, len, "conv_x3_kernel<256, false, false, 16, false, %d>", P);
        case HKP_X3K_TILE_128_MF16: return snprintf(buf, len, "conv_x3_kernel<128, false, false, 16, false, %d>", P);
        case HKP_X3K_TILE_128_MF32: return snprintf(buf, len, "conv_x3_kernel<128, false, false, 32, false, %d>", P);
        case HKP_X3K_PAIR_64: return snprintf(buf, len, "conv_x3_kernel<64, false, true, 16, false, %d>", P);
        case HKP_X3K_SK_128: return snprintf(buf, len, "conv_x3_kernel<128, false, false, 16, true, %d>", P);
        case HKP_X3K_SK_64: return snprintf(buf, len, "conv_x3_kernel<64, false, false, 32, true, %d>", P);
        case HKP_X3K_A3: return snprintf(buf, len, "conv_x3_a3_kernel<%d>", P);
        case HKP_X3K_A3_192: return snprintf(buf, len, "conv_x3_a3_192_kernel<%d>", P);
        case HKP_X3K_A3_160: return snprintf(buf, len, "conv_x3_a3_160_kernel<%d>", P);
        case HKP_X3K_A3_160X128: return snprintf(buf, len, "conv_x3_a3_160x128_kernel<%d>", P);
        case HKP_X3K_A3_MIX: return snprintf(buf, len, "conv_x3_a3_mix_kernel<%d>", P);
        case HKP_X3K_TAIL: return snprintf(buf, len, "conv_x3_tail_kernel<256, %d>", P);
        case HKP_X3K_HALO: return snprintf(buf, len, "conv_x3_halo_kernel<%d>", P);
        case HKP_X3K_HALO_BNIN: return snprintf(buf, len, "conv_x3_halo_bnin_kernel<%d>", P);
        case HKP_X3K_DUO: return snprintf(buf, len, "conv_x3_duo_kernel<%d>", P);
        case HKP_X3K_STEM_PAIR: return snprintf(buf, len, "conv_x3_kernel<64, true, true, 16, false, %d>", P);
        case HKP_X3K_STEM_PATCH: return snprintf(buf, len, "conv_x3_stem_patch_kernel<0>");
        case HKP_X3K_STEM_PATCH_IMAGE: return snprintf(buf, len, "conv_x3_stem_patch_kernel<1>");
        case HKP_X3K_STEM_PATCH_U8: return snprintf(buf, len, "conv_x3_stem_patch_kernel<2>");
        default: return snprintf(buf, len, "?");
    }
}

// ---------------------------------------------------------------- shape rules ----

// conv_x3_halo_kernel's shapes
static bool halo_shape(int stride, int r, int s, int pad, int dil, int ho, int wo, int k) {
    return stride == 1 && r == 3 && s == 3 && pad == 1 && dil == 1 && ho % HALO_PH == 0 && wo % HALO_PW == 0 &&
           k % 64 == 0;
}

static bool stem_x3_shape(const hkp_conv_desc* d) {
    return d && d->in_layout == HKP_LAYOUT_NCHW && d->c >= 1 && d->c <= 4 && d->r == 7 && d->s == 7 &&
           d->stride == 2 && d->pad == 3 && d->dilation == 1 && d->k % 64 == 0;
}

static bool stem_patch_shape(int ho, int wo, int k, const X3Knobs& kn) {
    return !kn.stem_pair && ho % STEM_PH == 0 && wo % STEM_PW == 0 && k % 64 == 0;
}

// the stem runs the patch body (patch-divisible outputs: 480x640 and 960x1280 images);
// HKP_TILE_64_PAIR keeps the one-tile stem (A/B, parity tests)
static bool stem_patch_ok(const hkp_conv_desc* d, int ho, int wo, const X3Knobs& kn) {
    return stem_patch_shape(ho, wo, d->k, kn) && d->tile != HKP_TILE_64_PAIR;
}

// the kernels address operands with 32-bit element offsets (see conv_x3_tile):
// the input ([n][h][w][cstride] halves, plus a padded-out margin of up to 64
// rows) and the weights ([k][rs][cstride]) must fit
static bool x3_offsets_fit(long n, long h, long w, long cstride, long k, long rs) {
    return (n * h * w + 64 * (w + 65)) * cstride < (1L << 32) && k * rs * cstride < (1L << 31);
}

// wgrad_x3_halo_kernel's shapes: 3x3, stride 1, pad = dilation = 1, C and K
// multiples of 64 up to 128 (the layers it was measured on), whole 4x16-pixel
// patches, operands under 2 GiB (32-bit byte offsets); d->tile == -1 keeps the
// tiled body (A/B, tests)
static bool wg_halo_shape(const hkp_conv_desc* d, int ho, int wo) {
    return d->tile != -1 && d->r == 3 && d->s == 3 && d->stride == 1 && d->pad == 1 && d->dilation == 1 &&
           d->k % 64 == 0 && d->c % 64 == 0 && d->k <= 128 && d->c <= 128 && wo % 16 == 0 && ho % 4 == 0 &&
           ho == d->h &&
           wo == d->w && (long)d->n * d->h * d->w * d->c * 4 < (1L << 31) && (long)d->n * ho * wo * d->k * 4 < (1L << 31);
}

// ka = 0: the halo body (r_tiles = its 64-channel column tiles, mps = patches per split)
static void wg_x3_plan(const hkp_conv_desc* d, long M, int wo, int* splits, int* mps, int* ka, int* r_tiles) {
    if (wg_halo_shape(d, (int)(M / ((long)d->n * wo)), wo)) {
        const long tiles = (long)(d->k / 64) * (d->c / 64), np = M / 64;   // 4x16-pixel patches
        // one 130 KiB block per CU: one round of 256, or the caller's CU budget
        long sp = std::max(1L, (d->tile > 0 ? d->tile : 256) / tiles);
        sp = std::min(sp, np);
        const long per = (np + sp - 1) / sp;
        *ka = 0;
        *r_tiles = d->c / 64;
        *mps = (int)per;                                   // patches per split
        *splits = (int)((np + per - 1) / per);
        return;
    }
    // KA 256's 16-pixel stages advance each x slot with at most one row wrap
    // (and 32-bit byte offsets into both operands)
    const bool ka256 = d->k % 256 == 0 && wo >= 16 && (long)d->n * d->h * d->w * d->c * 4 < (1L << 32) &&
                       M * d->k * 4 < (1L << 32);
    *ka = ka256 ? 256 : d->k % 128 == 0 ? 128 : 64;
    const long rsc = (long)d->r * d->s * d->c;
    *r_tiles = (int)((rsc + 255) / 256);
    const long tiles = (long)(d->k / *ka) * *r_tiles;
    // One 512-thread block per CU at a time: pick the split count whose block
    // count best fills whole rounds of 256 CUs (few rounds, few slabs to reduce),
    // with at least 16 K-steps (512 pixels) per block.
    const long max_sp = std::max(1L, (M + 511) / 512);
    long sp = 1;
    double best = -1.0;
    for (long c = 1; c <= max_sp && d->tile <= 0; ++c) {
        const long blocks = tiles * c;
        const long rounds = (blocks + 255) / 256;
        if (rounds > 4) break;
        const double fill = (double)blocks / (256.0 * rounds);
        const double score = fill - 0.03 * rounds;            // prefer fewer rounds / slabs at equal fill
        if (score > best + 1e-9) {
            best = score;
            sp = c;
        }
    }
    if (d->tile > 0) sp = std::max(1L, std::min<long>(max_sp, d->tile / tiles));   // the caller's CU budget
    long m = (M + sp - 1) / sp;
    m = (m + 31) / 32 * 32;
    *splits = (int)((M + m - 1) / m);
    *mps = (int)m;
}

// Strided dgrad as stride-1 convs, one per output phase (py, px) of dx: dx pixel
// (2a+py, 2b+px) receives the taps r = r_max - 2r' (r ≡ py + pad mod 2) at dy row
// a + o_min + r', o_min = (py + pad - r_max) / 2 (likewise for columns); a phase
// no tap reaches (e.g. odd pixels of a 1x1 stride-2 conv) is dx = add (or 0).
static int phase_taps(int R, int pad, int stride, int ph, int* r_max, int* o_min) {
    int rm = -1;
    for (int r = R - 1; r >= 0; --r)
        if ((((ph + pad - r) % stride) + stride) % stride == 0) {
            rm = r;
            break;
        }
    if (rm < 0) return 0;
    *r_max = rm;
    *o_min = (ph + pad - rm) / stride;
    return rm / stride + 1;
}

// ---------------------------------------------------------------- the problem ----

// The implicit GEMM one launch runs: M = N Ho Wo output rows by K output channels
// over RS taps of cch 128-B input lines per pixel (32 channels each for P 3, 64 for
// P 1), in the launch's own terms (a dgrad's input is dy, its K the conv's Cin)
struct X3Problem {
    int N = 0, H = 0, W = 0, C = 0, K = 0, R = 0, S = 0, stride = 1, pad = 0, dil = 1, Ho = 0, Wo = 0;
    long M = 0;
    int cch = 0, RS = 0;
    int P = 3;                     // operand layout: 3 packed f16x3 split (2, 4: two products), 1 plain fp16
    bool dense = true;             // every output pixel written in place (false: one phase of a strided dgrad)
    bool out_bn = false;           // the output's BN apply fused into the epilogue (hkp_conv2d_fwd_f16_bn)
    bool in_bn = false;            // the input's BN + ReLU applied in the kernel (hkp_conv2d_fwd_x3_bnin / _f16_bnin)
    // strided dgrad phase: the output pixel stride and offsets (X3Args::ost, oy, ox)
    int ost = 0, OH = 0, OW = 0, oy = 0, ox = 0;

    long m_tiles() const { return (M + 255) / 256; }
    int nks() const { return RS * cch; }
};

// forward conv of d (output ho x wo: hkp_conv_out_hw) on operand layout P
static X3Problem x3_problem_fwd(const hkp_conv_desc* d, int ho, int wo, int P) {
    X3Problem p;
    p.N = d->n; p.H = d->h; p.W = d->w; p.C = d->c; p.K = d->k; p.R = d->r; p.S = d->s;
    p.stride = d->stride; p.pad = d->pad; p.dil = d->dilation; p.Ho = ho; p.Wo = wo;
    p.M = (long)d->n * ho * wo; p.cch = d->c / (x3_packed(P) ? 32 : 64); p.RS = d->r * d->s; p.P = P;
    return p;
}

// stride-1 dgrad of d: a conv of dy (ho x wo, d->k channels) with the flipped filter (the
// entry point takes stride 1 only; a strided descriptor keeps its stride here, so that no
// stride-1 body rule applies to it)
static X3Problem x3_problem_dgrad(const hkp_conv_desc* d, int ho, int wo) {
    X3Problem p;
    p.N = d->n; p.H = ho; p.W = wo; p.C = d->k; p.K = d->c; p.R = d->r; p.S = d->s;
    p.stride = d->stride; p.pad = d->dilation * (d->r - 1) - d->pad; p.dil = d->dilation; p.Ho = d->h; p.Wo = d->w;
    p.M = (long)d->n * d->h * d->w; p.cch = d->k / 32; p.RS = d->r * d->s; p.P = 3;
    return p;
}

// phase (py, px) of the stride-2 dgrad of d; false: no tap reaches the phase (or it has
// no pixels).  *col_pad: the column offset, which the kernels need equal to p.pad
static bool x3_problem_dgrad_phase(const hkp_conv_desc* d, int ho, int wo, int py, int px, X3Problem* out,
                                   int* col_pad) {
    X3Problem p;
    const int Ha = (d->h - py + 1) / 2, Wa = (d->w - px + 1) / 2;
    int rmx = 0, omy = 0, smx = 0, omx = 0;
    const int R2 = phase_taps(d->r, d->pad, 2, py, &rmx, &omy);
    const int S2 = phase_taps(d->s, d->pad, 2, px, &smx, &omx);
    p.N = d->n; p.H = ho; p.W = wo; p.C = d->k; p.K = d->c; p.R = R2; p.S = S2;
    p.stride = 1; p.pad = -omy; p.dil = 1; p.Ho = Ha; p.Wo = Wa;
    p.M = (long)d->n * Ha * Wa; p.cch = d->k / 32; p.RS = R2 * S2; p.P = 3;
    p.dense = false; p.ost = 2; p.OH = d->h; p.OW = d->w; p.oy = py; p.ox = px;
    *out = p;
    *col_pad = -omx;
    return Ha > 0 && Wa > 0 && R2 > 0 && S2 > 0;
}

// halo: 0 the halo-tile body cannot take the shape, 1 it can (HKP_TILE_HALO
// forces it), 2 it is also the default (64 input channels: measured faster;
// at 128 channels it ties the ring bodies, which then stay)
// lines: 128-B input lines per pixel (32 channels each for P 3, 64 for P 1)
static int x3_halo_level(bool ok, int lines, int P) {
    return !ok ? 0 : lines * (x3_packed(P) ? 32 : 64) <= 64 ? 2 : 1;
}

// the halo-tile body takes this launch (shape, plain dense output, no fused
// epilogue, 32-bit halo offsets): the one place that says so
static int x3_halo(const X3Problem& p) {
    const bool ok = halo_shape(p.stride, p.R, p.S, p.pad, p.dil, p.Ho, p.Wo, p.K) && p.dense && !p.out_bn &&
                    (long)p.N * p.H * p.W * p.cch * 64L + 64 < (1L << 32);
    return x3_halo_level(ok, p.cch, p.P);
}

// ---------------------------------------------------------------- the planner ----

// stream-K: per-tile arrival counters in the first X3_SK_CNT_BYTES of the
// workspace, then two fp32 slabs per block (a block splits at most its first
// and its last tile): 2 * CUs * BN * 1 KiB (256 x BN floats per slab)
constexpr long X3_SK_CNT_BYTES = 64 << 10;
static long x3_sk_ws_bytes(int bn, int cus) { return X3_SK_CNT_BYTES + 2L * cus * bn * 1024; }

// stream-K overhead per block in tile times: every block writes up to two
// fp32 slabs and most reduce a tile from two (~0.4 MB per CU, all CUs at once),
// plus a second pipeline fill — so it shrinks with the K depth nks of a tile.
// Fitted to in-process A/Bs on the box (column-grouped stream-K vs one tile per
// block): t4 nks 144 0.34, t3 / layer3 nks 72 0.46 / 0.48, t2 nks 36 0.63,
// t1 / layer1 nks 18 1.18 / 1.46 tile-times: 0.2 + 19 / nks.
static double sk_over(int nks) { return 0.2 + 19.0 / nks; }

// Tile width (and data-parallel vs stream-K) for Cout = k over m_tiles 256-row
// tiles: data-parallel costs ceil(blocks / CUs) rounds of one tile each,
// stream-K blocks / CUs + the overhead above; minimise rounds x the measured
// per-column tile cost (256x256: 0.9, 256x128: 1.0, 256x64: 1.25 — wider tiles
// reuse each A line more).  E.g. C2 layer4 (600 m-tiles, Cout 512): 1200
// 256x256 tiles = 4.69 rounds, data-parallel (5 rounds); training layer4 (150
// m-tiles): 600 256x128 tiles stream-K (2.34 + 0.25 rounds) beats 3 rounds of
// 256x128 (data-parallel's best).  Measured on C2 layer4: 256x256 1.70 ms vs
// 256x128 1.82 ms; on C2 layer3 (Cout 256, 600 m-tiles) 256x256 loses to round
// quantisation (0.53 vs 0.47 ms).  No stream-K with 256x256 tiles (the one-tile
// 256x256 kernel sits at 255 VGPRs; the stream-K loop would spill).
// Split-K tail (conv_x3_tail_kernel) for a one-tile grid of m_tiles x nt tiles:
// the group count NG = tm*S of the tail grid (0: no tail) — each of the tm
// m-tiles past the last full round in S equal K segments, one per group — and its
// cost in tile times, 1/S + 0.08 (a segment's fill, slab hand-off and combine)
// per round of segments.  C2 layer3 on 256x256 tiles (88 tail tiles): S = 2,
// ~0.58 instead of 1; training t4: S = 5.  C2 layer4 (88 tail m-tiles x 2
// columns) has no S >= 2 that beats one plain round.  (A fractional tail — every
// CU's group a fraction of a tile, two segments per block — was built in round 5
// and measured slower end to end: DESIGN "Fractional split-K tail".)
// (Multi-round tails — S segments per tail m-tile past one round, one slab per
// segment — measured slower in round 5: the B=8 shard's layer3 0.138 -> 0.164 ms
// at S = 3, C2 layer3 0.384 -> 0.418 ms at S = 5; profiles/r05_multi_*.  The tail
// on 256x128 grids of >= 2 rounds (C2 layer2) measured neutral: C2 1753.0 vs 1755.5
// img/s, C4 / C3 unchanged; profiles/r05_tail128_*_v2.)
static long x3_tail_groups(long m_tiles, int nt, int nks, int cus, double* cost = nullptr) {
    const long G = cus, tiles = m_tiles * nt, tr = tiles % G;
    const long tm = m_tiles - tiles / G * G / nt;
    double best = 1.0;
    long ng = 0;
    if (tr > 0) {
        for (int S = 2; S <= 8 && nks / S >= 4 && tm * S * nt <= G; ++S)
            if (1.0 / S + 0.08 < best - 1e-9) {
                best = 1.0 / S + 0.08;
                ng = tm * S;
            }
    }
    if (cost) *cost = tr > 0 ? best : 0.0;
    return ng;
}

struct X3Plan {
    int bn;
    bool sk;
};
static X3Plan x3_plan(int k, long m_tiles, int nks, bool sk_ok, double over, int cus) {
    const int G = cus;
    X3Plan best{64, false};
    double best_cost = 1e300;
    for (int bn : {256, 128, 64}) {
        if (k % bn) continue;
        const long tiles = m_tiles * (k / bn);
        const double col = bn * (bn == 256 ? 0.9 : bn == 128 ? 1.0 : 1.25);
        double tail = (tiles % G) ? 1.0 : 0.0;             // the last, partly filled round
        if (bn == 256 && sk_ok) x3_tail_groups(m_tiles, k / bn, nks, cus, &tail);
        const double dp = ((double)(tiles / G) + tail) * col;
        if (dp < best_cost - 1e-9) {
            best_cost = dp;
            best = {bn, false};
        }
        const int ng = G / (k / bn);       // column-grouped stream-K: groups of k/bn blocks
        if (sk_ok && bn != 256 && ng > 0 && m_tiles % ng && tiles * 4 <= X3_SK_CNT_BYTES) {
            const double skc = ((double)m_tiles / ng + over) * col;
            if (skc < best_cost - 1e-9) {
                best_cost = skc;
                best = {bn, true};
            }
        }
    }
    return best;
}

// The kernel a launch runs (conv_x3_kernel<bn, STEM, pair, mfd, sk, P>):
//   256x256                 16x16x32 body, 2-stage ring (C2 layer4 1.79 -> 1.62 ms
//                           vs the 32x32x16 body: same cycles per FLOP at lower
//                           power, so the chip holds a higher clock —
//                           MI355X_MICROARCH.md DVFS item 7)
//   256x128, >= 2 rounds    16x16x32 body, 3-stage ring (C2 layer3 +6 %, layer2 +5 %)
//   256x128, one round      32x32x16 body (the 16x16 body's longer fill lost 8-11 %;
//                           round 5: AUTO on packed f16x3 runs the 16x16 body here
//                           and 256x64 pairs for >= 1 round — x3_choose)
//   256x64                  16x16x32 body, two blocks per CU (layer1 0.223 -> 0.166 ms)
//   stream-K 256x128 / 64   16x16x32 / 32x32x16 bodies (training t4 fwd +3-6 %, t3 +6 %)
// hkp_conv_desc.tile (HKP_TILE_*) forces one of them — every body is reachable
// for the parity tests; results agree to fp32 summation order.
struct X3Choice {
    int bn, mfd;
    bool pair, sk;
    bool halo = false;                 // conv_x3_halo_kernel<P>
    bool a3 = false;                   // conv_x3_a3_kernel<P> (256x256, 3-stage A ring)
    bool duo = false;                  // conv_x3_duo_kernel<1> (256x128, two 4-wave blocks per CU)
    int bm = 256;                      // rows per tile (192 / 160: conv_x3_a3_192 / _160_kernel<P>)
    bool mix = false;                  // conv_x3_a3_mix_kernel<P>: the regions of x3_mix_plan
};

// The regions of a mixed-height launch (conv_x3_a3_mix_kernel) over M rows and
// n_tiles column tiles on G CUs: a, b, c rounds of 256-, 192- and 160-row tiles,
// G / n_tiles m-tiles to a round, minimising the 16-row blocks a CU runs, 16 a +
// 12 b + 10 c, subject to (G / n_tiles) (256 a + 192 b + 160 c) >= M.  The three
// heights cost the same per row, so plans of equal cost tie: the one with the most
// 256-row rounds, then the most 192-row rounds (the fewest blocks), is taken; four
// 192-row or eight 160-row rounds are three / five 256-row ones, so b <= 3, c <= 7.
// Regions in that order; every region but the last non-empty one holds its whole
// rounds, the last only the tiles that the rows left need.
struct X3Mix {
    int cost = 0;                      // 16-row blocks per CU; 0: no plan
    int rounds[3] = {0, 0, 0};
    long mt[3] = {0, 0, 0};            // m-tiles per region
    long m_base[3] = {0, 0, 0};        // first output row
    long part_base[3] = {0, 0, 0};     // first BN partial tile (128- / 96- / 80-row tiles)
    long part_tiles = 0;               // BN partial tiles in all
};
static constexpr int X3_MIX_BM[3] = {256, 192, 160};
static X3Mix x3_mix_plan(long M, int n_tiles, int G) {
    X3Mix p;
    if (M <= 0 || n_tiles <= 0 || G / n_tiles <= 0) return p;
    const long R = G / n_tiles, need = (M + R - 1) / R;        // m-tiles per round, rows a CU column must cover
    const long a_hi = (need + 255) / 256, a_lo = std::max<long>(0, (need - 3 * 192 - 7 * 160) / 256);
    long best = -1, ba = 0, bb = 0, bc = 0;
    for (long a = a_hi; a >= a_lo; --a)
        for (long b = 3; b >= 0; --b)
            for (long c = 0; c <= 7; ++c) {
                if (256 * a + 192 * b + 160 * c < need) continue;
                const long cost = 16 * a + 12 * b + 10 * c;
                if (best < 0 || cost < best) { best = cost; ba = a; bb = b; bc = c; }
                break;                                         // more 160-row rounds only cost more
            }
    if (best < 0 || best > (1L << 30)) return p;
    p.cost = (int)best;
    p.rounds[0] = (int)ba; p.rounds[1] = (int)bb; p.rounds[2] = (int)bc;
    const int last = bc ? 2 : bb ? 1 : 0;
    long row = 0, pt = 0;
    for (int r = 0; r < 3; ++r) {
        const long bm = X3_MIX_BM[r], left = M - row;
        p.m_base[r] = row;
        p.part_base[r] = pt;
        p.mt[r] = r == last ? (left + bm - 1) / bm : p.rounds[r] * R;
        const long rows = r == last ? left : p.mt[r] * bm;
        row += rows;
        pt += (rows + bm / 2 - 1) / (bm / 2);
    }
    p.part_tiles = pt;
    return p;
}
// a mix launch's shape rule: packed operands, 256-wide output tiles, more than one
// round of 256-row tiles, at least one m-tile to a round (x3_choose; the A3 operand-size
// limits are the entry points')
static bool x3_mix_ok(int k, long m_tiles, int P, int cus) {
    return x3_packed(P) && k % 256 == 0 && m_tiles * (k / 256) > cus && cus >= k / 256;
}
static X3Choice x3_choose_base(int k, long m_tiles, int nks, bool sk_ok, int policy, int halo, int cus);
// AUTO (= AUTO_A3): the planner's choice, its 256x256 one-tile grids on the A3
// body (measured in-process on one box: C2 1721 -> 1741 img/s, C4 2616 -> 2657;
// per conv -1...-4 % on the 1x1 and 3x3 shapes of C4, -1 % on C2's layer3/4;
// HKP_TILE_256 / 256_TAIL keep the 2-stage body)
// DUO (the plain-fp16 256x128 two-blocks-per-CU body) where forced and legal;
// other operand layouts plan as AUTO
static X3Choice x3_choose(int k, long m_tiles, int nks, bool sk_ok, int policy, int halo, int P, int cus,
                          const X3Knobs& kn) {
    if (policy == HKP_TILE_DUO) {
        if (P == 1 && k % DUO_BN == 0) {
            X3Choice c{DUO_BN, 16, false, false};
            c.duo = true;
            return c;
        }
        policy = HKP_TILE_AUTO;
    }
    // the overlapped dgrad's A3 request (Policy.dgrad_overlap_tile) on a 64- or
    // 128-channel output, which A3 cannot take: plan it as AUTO (the rules below)
    if (policy == HKP_TILE_256_A3 && P == 3 && k % 256 != 0 && kn.pair128) policy = HKP_TILE_AUTO;
    // 192-row A3 tiles: packed operands with 256-divisible outputs; AUTO otherwise
    if (policy == HKP_TILE_192_A3 && (!x3_packed(P) || k % 256 != 0)) policy = HKP_TILE_AUTO;
    if (policy == HKP_TILE_160_A3 && (!x3_packed(P) || k % 128 != 0)) policy = HKP_TILE_AUTO;
    // mixed tile heights: the same operands over more than one round of tiles; AUTO otherwise
    if (policy == HKP_TILE_MIX_A3 && !x3_mix_ok(k, m_tiles, P, cus)) policy = HKP_TILE_AUTO;
    if (policy != HKP_TILE_AUTO_A3 && policy != HKP_TILE_AUTO)
        return x3_choose_base(k, m_tiles, nks, sk_ok, policy, halo, cus);
    X3Choice c = x3_choose_base(k, m_tiles, nks, sk_ok, HKP_TILE_AUTO, halo, cus);
    if (c.bn == 256 && !c.sk && !c.halo && !c.pair) c.a3 = true;
    // AUTO, plain fp16: the DUO body where it measured faster than the one-tile
    // bodies (tools/conv_ab.py, in-process, profiles/r05_duo_*): K-depth 64 (one
    // K-step: C4's layer1 1x1 expansions, 64 -> 256: -12 %, all fill and epilogue)
    // and 128-wide outputs (layer2: -4...-10 % against the one-block 256x128 body);
    // the long-K 256-wide shapes stay on A3 (DUO +10...+33 %: its half-line stream
    // moves 1.5x the operand bytes per MAC).  AUTO_A3 keeps the round-4 planner.
    if (policy == HKP_TILE_AUTO && P == 1 && !c.halo && k % DUO_BN == 0 && (nks == 1 || k == DUO_BN)) {
        X3Choice d{DUO_BN, 16, false, false};
        d.duo = true;
        return d;
    }
    // AUTO, packed f16x3, one-tile grids: the 256x64 two-blocks-per-CU tiles (one
    // block's fill and epilogue overlap the other's K loop) for short-K convs (the
    // 1x1 downsamples, K-depth <= 256 channels: C2 128 -> 256 0.061 -> 0.052 ms;
    // B=8 256 -> 512 0.061 -> 0.040 and 128 -> 256 0.021 -> 0.019) and where the
    // cost table picks 256x128 tiles over at least a round of them (C2 layer2 3x3
    // 0.140 -> 0.125 ms, its stride-2 conv1 0.086 -> 0.073, the 64 -> 128 downsample
    // 0.033 -> 0.025); a one-round 256x128 grid on the 16x16x32 body (the B=8 shard's
    // layer2 0.053 -> 0.040 ms: the 32x32x16 body's shorter fill no longer wins).
    // Stream-K plans stay (B=8 layer3: 0.128 ms vs 0.138 on pairs), and so do grids
    // of more than 3 rounds of 256x256 tiles, where the longer grid's steady state
    // favours the larger tiles (C2 256 -> 512 downsample at 4.7 rounds: even; config
    // C5 at 1280x960, 4.7-37 rounds: its 128-wide 3x3 1.05x, its 1x1s 1.04-1.27x
    // slower on pairs).  tools/conv_ab.py, profiles/r05_l2_conv_ab*.log
    if (policy == HKP_TILE_AUTO && P == 3 && !c.halo && !c.sk && kn.pair128) {
        const bool small = (double)m_tiles * k <= 3.0 * 256 * cus;
        if (small && (nks <= 8 || (c.bn == 128 && m_tiles * (k / 128) >= cus))) return {64, 16, true, false};
        if (c.bn == 128 && m_tiles * (k / 128) < cus) c.mfd = 16;
    }
    return c;
}
static X3Choice x3_choose_base(int k, long m_tiles, int nks, bool sk_ok, int policy, int halo, int cus) {
    // the halo-tile body wherever the shape allows it, unless a tile body is forced
    if ((halo >= 1 && policy == HKP_TILE_HALO) ||
        (halo == 2 && (policy == HKP_TILE_AUTO || policy == HKP_TILE_256_TAIL || policy == HKP_TILE_256_A3 ||
                       policy == HKP_TILE_192_A3 || policy == HKP_TILE_160_A3 || policy == HKP_TILE_MIX_A3))) {
        X3Choice c{64, 16, true, false};
        c.halo = true;
        return c;
    }
    switch (policy) {
        case HKP_TILE_256:
            if (k % 256 == 0) return {256, 16, false, false};
            break;
        case HKP_TILE_128_MF16:
            if (k % 128 == 0) return {128, 16, false, false};
            break;
        case HKP_TILE_128_MF32:
            if (k % 128 == 0) return {128, 32, false, false};
            break;
        case HKP_TILE_64_PAIR:
            return {64, 16, true, false};
        case HKP_TILE_256_TAIL:            // 256x256, the partial last round as split-K segments
            if (k % 256 == 0) return {256, 16, false, false};
            break;
        case HKP_TILE_256_A3:              // the same on the A3 body
            if (k % 256 == 0) return {256, 16, false, false, false, true};
            break;
        case HKP_TILE_192_A3:              // 192x256 / 160x256 (160x128) tiles on the A3 body
        case HKP_TILE_160_A3:              // (x3_choose checked the operands)
            if (k % 256 == 0 || (policy == HKP_TILE_160_A3 && k % 128 == 0)) {
                X3Choice c{k % 256 == 0 ? 256 : 128, 16, false, false, false, true};
                c.bm = policy == HKP_TILE_192_A3 ? 192 : 160;
                return c;
            }
            break;
        case HKP_TILE_MIX_A3: {           // 256 / 192 / 160 x 256 regions in one launch (x3_choose checked)
            X3Choice c{256, 16, false, false, false, true};
            c.mix = true;
            return c;
        }
        default:
            break;
    }
    const bool sk = sk_ok && policy != HKP_TILE_NO_SK && policy != HKP_TILE_256_TAIL && policy != HKP_TILE_256_A3;
    const X3Plan pl = x3_plan(k, m_tiles, nks, sk, policy == HKP_TILE_SK ? 0.0 : sk_over(nks), cus);
    if (pl.sk) return {pl.bn, pl.bn == 128 ? 16 : 32, false, true};
    if (pl.bn == 256) return {256, 16, false, false};
    if (pl.bn == 128) return {128, (double)m_tiles * (k / 128) >= 2.0 * cus ? 16 : 32, false, false};
    return {64, 16, true, false};
}

// ---------------------------------------------------------------- the launch plan ----

// One kernel launch: the kernel, its grid, and the X3Args values the plan owns
// (everything else in X3Args is the problem's geometry and the caller's pointers)
struct X3Launch {
    int kernel = HKP_X3K_PAIR_64;
    long blocks = 0;
    int threads = 512;
    int n_tiles = 0, nks = 0;
    long sk_units = 0;
    int sk_one = 0, mt0 = 0;
    int main_blocks = 0, tail_groups = 0, tail_mt0 = 0;
    long tail_units = 0;
    int mix_b1 = 0, mix_b2 = 0, mix_m1 = 0, mix_m2 = 0, mix_p1 = 0, mix_p2 = 0;
    int stagger_blocks = 0;
    int stagger_ns = -1;           // DUO: the second block's first-round stagger in ns; -1: the caller's own
    bool uses_ws = false;          // reads sk_cnt / sk_ws: the counters, then ws_bytes - X3_SK_CNT_BYTES of slabs
    long ws_bytes = 0;
};

struct X3LaunchPlan {
    X3Choice c{64, 16, true, false};
    int n_launches = 0;            // 0: the entry points reject the shape (K % 64, no whole input line)
    X3Launch launch[2];            // launch[0].kernel is the choice's kernel even then
    int n_seg = 0;
    int seg[6] = {0, 0, 0, 0, 0, 0};   // BN partial segments: (rows per tile, tiles) pairs
};

// the kernel of a one-tile grid (conv_x3_kernel's forms, or A3)
static int x3_tile_kernel(const X3Choice& c) {
    return c.a3                       ? HKP_X3K_A3
           : c.sk && c.bn == 128      ? HKP_X3K_SK_128
           : c.sk                     ? HKP_X3K_SK_64
           : c.bn == 256              ? HKP_X3K_TILE_256
           : c.bn == 128 && c.mfd == 16 ? HKP_X3K_TILE_128_MF16
           : c.bn == 128              ? HKP_X3K_TILE_128_MF32
                                      : HKP_X3K_PAIR_64;
}

// policy: hkp_conv_desc.tile; ws_bytes: the stream-K workspace the call passes (0: none)
static X3LaunchPlan x3_launch_plan(const X3Problem& p, int policy, long ws_bytes, int cus, const X3Knobs& kn = X3Knobs()) {
    X3LaunchPlan pl;
    const int k = p.K, nks = p.nks(), P = p.P;
    const long m_tiles = p.m_tiles(), G = cus;
    const bool sk_ok = ws_bytes >= x3_sk_ws_bytes(256, cus);
    const X3Choice c = pl.c = x3_choose(k, m_tiles, nks, sk_ok, policy, x3_halo(p), P, cus, kn);
    X3Launch& l = pl.launch[0];
    l.kernel = c.halo    ? (p.in_bn ? HKP_X3K_HALO_BNIN : HKP_X3K_HALO)
               : c.duo   ? HKP_X3K_DUO
               : c.mix   ? HKP_X3K_A3_MIX
               : c.bm == 192 ? HKP_X3K_A3_192
               : c.bm == 160 ? (c.bn == 128 ? HKP_X3K_A3_160X128 : HKP_X3K_A3_160)
                         : x3_tile_kernel(c);
    // the BN partial list: a mix launch's regions, else one tile height (the halo-tile and
    // DUO bodies write 128-row partials whatever the policy asked for)
    const X3Mix mp = c.mix ? x3_mix_plan(p.M, k / 256, cus) : X3Mix();
    if (c.mix) {
        for (int r = 0; r < 3; ++r) {
            if (mp.mt[r] == 0) continue;
            const long end = r == 2 ? mp.part_tiles : mp.part_base[r + 1];
            pl.seg[2 * pl.n_seg] = X3_MIX_BM[r] / 2;
            pl.seg[2 * pl.n_seg + 1] = (int)(end - mp.part_base[r]);
            ++pl.n_seg;
        }
    } else {
        const int rows = c.halo || c.duo || c.bm == 256 ? 128 : c.bm / 2;
        pl.n_seg = 1;
        pl.seg[0] = rows;
        pl.seg[1] = (int)((p.M + rows - 1) / rows);
    }
    if (k % 64 != 0 || nks <= 0) return pl;
    const int nt = k / c.bn;
    l.n_tiles = nt;
    l.nks = nks;
    l.stagger_blocks = cus;
    l.blocks = m_tiles * nt;
    pl.n_launches = 1;
    if (c.duo) {
        // first-round stagger of the second block on each CU: half a block's
        // lifetime, ~(fill + epilogue + K loop) / 2 — hkp_debug_duo_stagger overrides
        // (ns; 0 = off, < 0 = this estimate)
        const int ns = kn.duo_stagger_ns < 0 ? 5500 + 450 * 2 * nks : kn.duo_stagger_ns;
        l.threads = 256;
        l.stagger_ns = l.blocks > 2L * cus ? ns : 0;
        l.stagger_blocks = 2 * cus;
        return pl;
    }
    if (c.halo) return pl;
    if (c.mix) {                           // one tile per block in up to three regions; no tail, no workspace
        l.mix_b1 = (int)(mp.mt[0] * nt);
        l.mix_b2 = (int)((mp.mt[0] + mp.mt[1]) * nt);
        l.mix_m1 = (int)mp.m_base[1]; l.mix_m2 = (int)mp.m_base[2];
        l.mix_p1 = (int)mp.part_base[1]; l.mix_p2 = (int)mp.part_base[2];
        l.blocks = (mp.mt[0] + mp.mt[1] + mp.mt[2]) * nt;
        return pl;
    }
    if (c.bm != 256) {                     // one tile per block, no split-K tail
        l.blocks = (p.M + c.bm - 1) / c.bm * nt;
        return pl;
    }
    if (c.sk) {
        l.sk_units = m_tiles * nks;
        // at least one unit per group: an empty group range inside a tile's group
        // span would be counted as a segment that never arrives
        const long ng = std::min<long>(G / nt, l.sk_units);
        l.blocks = ng * nt;
        l.uses_ws = true;
        l.ws_bytes = X3_SK_CNT_BYTES + 2 * l.blocks * c.bn * 1024;
        return pl;
    }
    // split-K tail for the 256x256 one-tile grid (auto, or forced by HKP_TILE_256_TAIL)
    const long tiles = m_tiles * nt;
    const long rm = tiles / G * G / nt;                     // m-tiles of the full rounds
    const long tm = m_tiles - rm;
    long NG = (c.bn == 256 && sk_ok &&
               (policy == HKP_TILE_AUTO || policy == HKP_TILE_256_TAIL || policy == HKP_TILE_256_A3 ||
                policy == HKP_TILE_AUTO_A3))
                  ? x3_tail_groups(m_tiles, nt, nks, cus)
                  : 0;
    // one round, every group non-empty and inside one tile (NG = tm * S), one slab
    // per block and the counters in the workspace
    if (NG > 0 && !(tm > 0 && NG % tm == 0 && NG * nt <= G && tm * nks >= NG &&
                    NG * nt * 256L * 1024 + X3_SK_CNT_BYTES <= ws_bytes && tm * nt * 4 <= X3_SK_CNT_BYTES))
        NG = 0;
    if (NG == 0) return pl;
    l.sk_one = 1;
    const long tail_ws = X3_SK_CNT_BYTES + NG * nt * 256L * 1024;
    // one launch: the full rounds, then the tail's segments
    if (c.a3 && !kn.split_tail) {
        l.main_blocks = (int)(rm * nt);
        l.tail_groups = (int)NG;
        l.tail_mt0 = (int)rm;
        l.tail_units = tm * nks;
        l.blocks = (rm + NG) * nt;
        l.uses_ws = true;
        l.ws_bytes = tail_ws;
        return pl;
    }
    // two: the full rounds on the one-tile kernel (the A3 body: A/B only; no blocks and not
    // started where the grid is less than a round), then conv_x3_tail_kernel
    X3Launch& t = pl.launch[1] = l;
    t.kernel = HKP_X3K_TAIL;
    t.mt0 = (int)rm;
    t.sk_units = tm * nks;
    t.blocks = NG * nt;
    t.uses_ws = true;
    t.ws_bytes = tail_ws;
    l.blocks = rm * nt;
    pl.n_launches = 2;
    return pl;
}

}  // namespace hkp
