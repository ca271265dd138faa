// Procedural cable scenes: uint8 [n][h][w][3] BGR pictures rendered from a scene
// description (hkp/synth.py), one launch per batch, straight into the device data
// path.  A block owns one SYN_TH x SYN_TW tile of one image; a thread makes 4
// consecutive pixels of one row.
//
//   1. the block culls the image's pieces against the tile's box grown by each
//      piece's outer radius; the survivors are bits of a 512-bit mask in LDS (set
//      with LDS atomics: order-free).  The cull only drops pieces whose alpha is 0 on
//      every pixel of the tile (proof at synth_touches), so the picture does not
//      depend on the tiling;
//   2. the lattice values of the background noise the tile needs are hashed once per
//      tile into LDS;
//   3. every thread walks the set bits in ascending order for its pixels.  The walk
//      is block-uniform, so the piece records are uniform loads.
//
// Arithmetic: integers only (include/hulkkp.h spells it out and proves the word
// widths; tests/_synth_ref.py restates it in numpy int64).  No floating point, no
// scratch: the per-pixel state lives in fully unrolled arrays of SYN_PX.  Products of
// small factors (colours, alphas, Q8 fractions: all far below 2^23) are __mul24: the
// 24-bit multiply runs at the full vector rate, the 32-bit one at a quarter of it.
#include "common.h"

namespace hkp {

constexpr int SYN_TH = HKP_SYNTH_TILE_H, SYN_TW = HKP_SYNTH_TILE_W, SYN_PX = 4;
constexpr int SYN_WORDS = HKP_SYNTH_MAX_SEGS / 32;
constexpr int SYN_LAT = 32;          // lattice points per octave and tile: at most 9 x 3 (sh = 3)
static_assert(SYN_TH * SYN_TW == 256 * SYN_PX, "one tile per 256-thread block");
static_assert((SYN_TW / 8 + 1) * (SYN_TH / 8 + 1) <= SYN_LAT, "octave 1 at cell_log2 = 4");

// first output word of Philox4x32-10 at counter (c0, c1, c2, 0)
__device__ __forceinline__ uint32_t syn_philox_x0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t k0, uint32_t k1) {
    uint32_t c3 = 0;
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

// Can the piece have alpha > 0 on a pixel of the tile [tx0, tx1] x [ty0, ty1] (pixels,
// both ends included)?  The axis point the kernel measures from is q(s) = (x0, y0) +
// ((s*ux) >> 14, (s*uy) >> 14) with 0 <= s <= len; floor(s*u / 2^14) is monotone in s, so
// each coordinate of q(s) lies between that of q(0) and q(len).  alpha > 0 needs
// d2 < r_out2, hence |cx| < r + 8 and |cy| < r + 8: the pixel lies strictly inside the box
// of q(0), q(len) grown by r + 8.  Everything else is dropped.
__device__ __forceinline__ bool syn_touches(const hkp_synth_seg& sg, int tx0, int ty0, int tx1, int ty1) {
    const int ex = sg.x0 + (int)(((int64_t)sg.len * sg.ux) >> 14), ey = sg.y0 + (int)(((int64_t)sg.len * sg.uy) >> 14);
    const int ro = sg.r + 8;
    const int lox = (sg.x0 < ex ? sg.x0 : ex) - ro, hix = (sg.x0 < ex ? ex : sg.x0) + ro;
    const int loy = (sg.y0 < ey ? sg.y0 : ey) - ro, hiy = (sg.y0 < ey ? ey : sg.y0) + ro;
    return tx1 * 16 > lox && tx0 * 16 < hix && ty1 * 16 > loy && ty0 * 16 < hiy;
}

// one octave of the tile's lattice: point (i, j) of the tile's ncol x nrow window
__device__ __forceinline__ void syn_hash_lattice(uint8_t* lat, int tid, int tx0, int ty0, int sh, int octave,
                                                 uint32_t k0, uint32_t k1) {
    const int ix0 = tx0 >> sh, iy0 = ty0 >> sh;
    const int ncol = ((tx0 + SYN_TW - 1) >> sh) - ix0 + 2, nrow = ((ty0 + SYN_TH - 1) >> sh) - iy0 + 2;
    if (tid < ncol * nrow && tid < SYN_LAT)
        lat[tid] = (uint8_t)(syn_philox_x0((uint32_t)(ix0 + tid % ncol), (uint32_t)(iy0 + tid / ncol), (uint32_t)octave,
                                           k0, k1) & 255u);
}

// One octave's noise n_o of the SYN_PX pixels x .. x + SYN_PX - 1 of row y (x % SYN_PX == 0: a
// cell is at least 8 pixels wide, so they share their cell).  The definition interpolates along
// x first; nothing is rounded before the final shift, so the sum may be taken along y first
// (integer arithmetic distributes exactly) and the two column values serve all the pixels:
//   (v00*(256-fx) + v01*fx)*(256-fy) + (v10*(256-fx) + v11*fx)*fy
//     = (v00*(256-fy) + v10*fy)*(256-fx) + (v01*(256-fy) + v11*fy)*fx
__device__ __forceinline__ void syn_noise4(const uint8_t* lat, int x, int y, int tx0, int ty0, int sh, int* n) {
    static_assert(SYN_PX == 4, "the pixels of a thread share a lattice cell");
    const int ix0 = tx0 >> sh, iy0 = ty0 >> sh;
    const int ncol = ((tx0 + SYN_TW - 1) >> sh) - ix0 + 2;
    const int m = (1 << sh) - 1;
    const int fy = ((y & m) << 8) >> sh;
    const uint8_t* p = lat + __mul24((y >> sh) - iy0, ncol) + ((x >> sh) - ix0);
    const int left = __mul24(p[0], 256 - fy) + __mul24(p[ncol], fy);
    const int right = __mul24(p[1], 256 - fy) + __mul24(p[ncol + 1], fy);
#pragma unroll
    for (int j = 0; j < SYN_PX; ++j) {
        const int fx = (((x + j) & m) << 8) >> sh;
        n[j] = (__mul24(left, 256 - fx) + __mul24(right, fx) + 32768) >> 16;
    }
}

// top (0..255) at alpha (0..256) over below (0..255)
__device__ __forceinline__ int syn_over(int top, int alpha, int below) {
    return (__mul24(top, alpha) + __mul24(below, 256 - alpha) + 128) >> 8;
}

template <bool DWORD>
__global__ __launch_bounds__(256) void synth_cables_u8_kernel(int h, int w, uint8_t* __restrict__ out,
                                                             const hkp_synth_scene* __restrict__ scenes,
                                                             const hkp_synth_seg* __restrict__ segs) {
    __shared__ uint32_t mask[SYN_WORDS];
    __shared__ uint8_t lat[2][SYN_LAT];
    const int tid = threadIdx.x, n = blockIdx.z;
    const int tx0 = blockIdx.x * SYN_TW, ty0 = blockIdx.y * SYN_TH;
    const hkp_synth_scene& sc = scenes[n];                   // block-uniform
    const int cnt = sc.seg_cnt, sh0 = sc.cell_log2;
    const hkp_synth_seg* sg = segs + sc.seg_off;
    if (tid < SYN_WORDS) mask[tid] = 0;
    syn_hash_lattice(lat[0], tid, tx0, ty0, sh0, 0, sc.key[0], sc.key[1]);
    syn_hash_lattice(lat[1], tid, tx0, ty0, sh0 - 1, 1, sc.key[0], sc.key[1]);
    __syncthreads();
    {
        const int tx1 = (tx0 + SYN_TW - 1 < w - 1) ? tx0 + SYN_TW - 1 : w - 1;
        const int ty1 = (ty0 + SYN_TH - 1 < h - 1) ? ty0 + SYN_TH - 1 : h - 1;
        for (int i = tid; i < cnt; i += 256)
            if (syn_touches(sg[i], tx0, ty0, tx1, ty1)) atomicOr(&mask[i >> 5], 1u << (i & 31));
    }
    __syncthreads();
    // (no early return above: every thread of the block reaches both barriers)
    const int x = tx0 + (tid % (SYN_TW / SYN_PX)) * SYN_PX;
    const int y = ty0 + tid / (SYN_TW / SYN_PX);
    if (x >= w || y >= h) return;

    int o[SYN_PX][3];                                        // what lies below, per pixel
    int run_arc[SYN_PX], run_last[SYN_PX], run_a[SYN_PX], run_d2[SYN_PX], run_c[SYN_PX][3];
    // (past the row's end in the byte path: the lattice window covers the whole tile)
    int n0[SYN_PX], n1[SYN_PX];
    syn_noise4(lat[0], x, y, tx0, ty0, sh0, n0);
    syn_noise4(lat[1], x, y, tx0, ty0, sh0 - 1, n1);
#pragma unroll
    for (int j = 0; j < SYN_PX; ++j) {
        const int nz = (3 * n0[j] + n1[j] + 2) >> 2;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[j][c] = sc.bg0[c] + ((__mul24((int)sc.bg1[c] - (int)sc.bg0[c], nz) + 128) >> 8);
        run_a[j] = 0, run_arc[j] = -1, run_last[j] = -2, run_d2[j] = 0;
        run_c[j][0] = run_c[j][1] = run_c[j][2] = 0;
    }
    const int py = y * 16;
    for (int wd = 0; wd < SYN_WORDS; ++wd) {
        uint32_t bits = mask[wd];                            // block-uniform
        while (bits) {
            const int i = wd * 32 + __builtin_ctz(bits);
            bits &= bits - 1;
            const hkp_synth_seg& s = sg[i];
            const int64_t ux = s.ux, uy = s.uy;
            const int64_t ay = py - s.y0;
#pragma unroll
            for (int j = 0; j < SYN_PX; ++j) {
                const int64_t ax = (x + j) * 16 - s.x0;
                int64_t t = (ax * ux + ay * uy) >> 14;
                t = t < 0 ? 0 : (t > s.len ? (int64_t)s.len : t);
                const int64_t cx = ax - ((t * ux) >> 14), cy = ay - ((t * uy) >> 14);
                const int64_t d2l = cx * cx + cy * cy;
                if (d2l >= s.r_out2) continue;               // alpha 0: the piece does not cover the pixel
                const int d2 = (int)d2l;
                const int alpha = d2 <= s.r_in2 ? 256 : (int)(((uint32_t)(s.r_out2 - d2) * s.inv) >> 24);
                if (alpha <= 0) continue;
                const int dm = d2 < s.r2 ? d2 : s.r2;
                const int lum = 256 - (__mul24(s.shade, (int)(((uint64_t)dm * s.inv_r2) >> 24)) >> 8);
                if (!(s.arc == run_arc[j] && i == run_last[j] + 1)) {
                    // the run below ends: blend it (alpha 0 before the first run: a no-op)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        o[j][c] = syn_over(run_c[j][c], run_a[j], o[j][c]);
                    run_a[j] = 0;
                    run_arc[j] = s.arc;
                }
                run_last[j] = i;
                if (alpha > run_a[j] || (alpha == run_a[j] && d2 <= run_d2[j])) {
                    run_a[j] = alpha;
                    run_d2[j] = d2;
#pragma unroll
                    for (int c = 0; c < 3; ++c) run_c[j][c] = (__mul24(s.bgr[c], lum) + 128) >> 8;
                }
            }
        }
    }
    int px[SYN_PX * 3];
#pragma unroll
    for (int j = 0; j < SYN_PX; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            px[3 * j + c] = syn_over(run_c[j][c], run_a[j], o[j][c]);
    uint8_t* dst = out + (((size_t)n * h + y) * w + x) * 3;
    if (DWORD) {                                             // w % 4 == 0, out 4-byte aligned: x + 3 < w
        uint32_t d[3] = {0, 0, 0};
#pragma unroll
        for (int k = 0; k < SYN_PX * 3; ++k) d[k >> 2] |= (uint32_t)px[k] << (8 * (k & 3));
        uint32_t* q = (uint32_t*)dst;
        q[0] = d[0];
        q[1] = d[1];
        q[2] = d[2];
    } else {
#pragma unroll
        for (int j = 0; j < SYN_PX; ++j) {
            if (x + j < w) {
                dst[3 * j] = (uint8_t)px[3 * j];
                dst[3 * j + 1] = (uint8_t)px[3 * j + 1];
                dst[3 * j + 2] = (uint8_t)px[3 * j + 2];
            }
        }
    }
}

}  // namespace hkp

using namespace hkp;

extern "C" int hkp_synth_cables_u8(int32_t n, int32_t h, int32_t w, uint8_t* img_out, const hkp_synth_scene* scenes_host,
                                   const hkp_synth_scene* scenes, const hkp_synth_seg* segs_host,
                                   const hkp_synth_seg* segs, int32_t nsegs, hkp_stream_t stream) {
    static_assert(sizeof(hkp_synth_scene) == 64 && sizeof(hkp_synth_seg) == 64, "hkp_synth record layout");
    HKP_CHECK_ARG(n >= 1 && n <= 65535, "hkp_synth_cables_u8: bad batch size n=%d (1..65535)", n);
    HKP_CHECK_ARG(h >= 1 && h <= HKP_SYNTH_MAX_DIM && w >= 1 && w <= HKP_SYNTH_MAX_DIM,
                  "hkp_synth_cables_u8: output %dx%d outside 1..%d", h, w, HKP_SYNTH_MAX_DIM);
    HKP_CHECK_ARG(nsegs >= 0, "hkp_synth_cables_u8: bad table size nsegs=%d", nsegs);
    HKP_CHECK_ARG(img_out && scenes_host && scenes, "hkp_synth_cables_u8: null pointer");
    HKP_CHECK_ARG(nsegs == 0 || (segs_host && segs), "hkp_synth_cables_u8: null piece table with nsegs=%d", nsegs);
    HKP_CHECK_ARG(((uintptr_t)scenes & 3) == 0 && ((uintptr_t)segs & 3) == 0,
                  "hkp_synth_cables_u8: scenes and segs must be 4-byte aligned");
    for (int32_t b = 0; b < n; ++b) {
        const hkp_synth_scene& sc = scenes_host[b];
        HKP_CHECK_ARG(sc.seg_cnt >= 0 && sc.seg_cnt <= HKP_SYNTH_MAX_SEGS,
                      "hkp_synth_cables_u8: image %d has %d pieces (0..%d)", b, sc.seg_cnt, HKP_SYNTH_MAX_SEGS);
        HKP_CHECK_ARG(sc.seg_off >= 0 && (int64_t)sc.seg_off + sc.seg_cnt <= nsegs,
                      "hkp_synth_cables_u8: image %d's pieces [%d, %d + %d) run past the table of %d", b, sc.seg_off,
                      sc.seg_off, sc.seg_cnt, nsegs);
        HKP_CHECK_ARG(sc.cell_log2 >= 4 && sc.cell_log2 <= 12, "hkp_synth_cables_u8: image %d: cell_log2 %d outside 4..12",
                      b, sc.cell_log2);
        for (int i = 0; i < 9; ++i)
            HKP_CHECK_ARG(sc.reserved[i] == 0, "hkp_synth_cables_u8: image %d has a non-zero reserved field", b);
        for (int32_t i = 0; i < sc.seg_cnt; ++i) {
            const hkp_synth_seg& s = segs_host[sc.seg_off + i];
            HKP_CHECK_ARG(s.r >= 16 && s.r <= 512, "hkp_synth_cables_u8: image %d piece %d: radius %d/16 px outside 1..32 px",
                          b, i, s.r);
            HKP_CHECK_ARG(s.x0 >= -(1 << 17) && s.x0 <= (1 << 17) && s.y0 >= -(1 << 17) && s.y0 <= (1 << 17),
                          "hkp_synth_cables_u8: image %d piece %d: vertex (%d, %d)/16 px outside +-8192 px", b, i, s.x0, s.y0);
            HKP_CHECK_ARG(s.ux >= -16384 && s.ux <= 16384 && s.uy >= -16384 && s.uy <= 16384,
                          "hkp_synth_cables_u8: image %d piece %d: direction (%d, %d) outside Q14", b, i, s.ux, s.uy);
            HKP_CHECK_ARG(s.len >= 0 && s.len <= (1 << 18), "hkp_synth_cables_u8: image %d piece %d: length %d/16 px outside 0..16384 px",
                          b, i, s.len);
            const int32_t ri = (s.r - 8) * (s.r - 8), ro = (s.r + 8) * (s.r + 8), r2 = s.r * s.r;
            HKP_CHECK_ARG(s.r_in2 == ri && s.r_out2 == ro && s.r2 == r2 &&
                              s.inv == (uint32_t)((1ull << 32) / (uint64_t)(ro - ri)) &&
                              s.inv_r2 == (uint32_t)((1ull << 32) / (uint64_t)r2),
                          "hkp_synth_cables_u8: image %d piece %d: r_in2, r_out2, r2, inv or inv_r2 do not belong to r=%d",
                          b, i, s.r);
            HKP_CHECK_ARG(s.shade >= 0 && s.shade <= 256, "hkp_synth_cables_u8: image %d piece %d: shade %d outside 0..256",
                          b, i, s.shade);
            HKP_CHECK_ARG(s.reserved[0] == 0 && s.reserved[1] == 0,
                          "hkp_synth_cables_u8: image %d piece %d has a non-zero reserved field", b, i);
        }
    }
    const bool dword = w % 4 == 0 && ((uintptr_t)img_out & 3) == 0;
    const dim3 grid((unsigned)((w + SYN_TW - 1) / SYN_TW), (unsigned)((h + SYN_TH - 1) / SYN_TH), (unsigned)n);
    const hipStream_t s = as_stream(stream);
    if (dword)
        hipLaunchKernelGGL((synth_cables_u8_kernel<true>), grid, dim3(256), 0, s, h, w, img_out, scenes, segs);
    else
        hipLaunchKernelGGL((synth_cables_u8_kernel<false>), grid, dim3(256), 0, s, h, w, img_out, scenes, segs);
    HKP_LAUNCH_CHECK("hkp_synth_cables_u8");
    return HKP_OK;
}
