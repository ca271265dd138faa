// Batched antialiased resize of uint8 images of any size into [n][h][w][3]: Pillow's
// separable fixed-point resampler (Image.resize, RGB, reducing_gap=None), bit for
// bit, one launch per batch.  Image i has its own source size, destination
// rectangle and axis tables (hkp/resample.py builds them; include/hulkkp.h spells
// the arithmetic out; tests/_resample_ref.py restates it in numpy int64).
//
// A block owns one RS_TH x RS_TW tile of one output image.  A thread owns one output
// column and RS_R consecutive output rows (one wave = one row group, so everything
// about rows is wave-uniform) and keeps RS_R x 3 int32 accumulators in registers.
// It walks the source rows of its row group's vertical span; for each it forms the
// horizontal result of its column, rounded and clipped to 0..255 in a register --
// exactly Pillow's uint8 intermediate pixel, which therefore never exists in memory
// -- and adds it times ky into every accumulator whose window holds the row.
// Adjacent row groups recompute the rows their spans share.  Trip counts come from
// the tables at run time; nothing is sized by a tap count.  The tile's kx rows sit
// in LDS when they fit RS_LDS_BYTES (else they are read from global memory); source
// pixels are direct global byte loads (DESIGN "Antialiased resize").
//
// Addresses: the host validates records and tables before the launch; the kernel
// still clamps every (xmin, cnt) it reads against the source extent and ksize, so a
// source address is formed from in-range indices only.
#include "common.h"

namespace hkp {

constexpr int RS_TH = 32, RS_TW = 64, RS_R = 8;              // tile, output rows per thread
constexpr int RS_LDS_BYTES = 32768;                          // budget of the tile's kx rows
static_assert(RS_TW == 64 && RS_TH == 4 * RS_R, "one wave per row group, 256-thread blocks");
constexpr int RS_BITS = 22;

__device__ __forceinline__ int rs_clip8(int acc) {
    const int v = (acc + (1 << (RS_BITS - 1))) >> RS_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// (lo, cnt) of one table row, clamped into the source extent and to ksize
__device__ __forceinline__ void rs_bounds(const int32_t* __restrict__ tab, int i, int extent, int ksize, int& lo,
                                          int& cnt) {
    lo = tab[2 + 2 * i];
    cnt = tab[3 + 2 * i];
    lo = lo < 0 ? 0 : (lo > extent ? extent : lo);
    const int room = extent - lo < ksize ? extent - lo : ksize;
    cnt = cnt < 0 ? 0 : (cnt > room ? room : cnt);
}

template <bool DWORD, bool KX_LDS>
__global__ __launch_bounds__(256) void resample_u8_kernel(const uint8_t* __restrict__ in,
                                                         const hkp_resample_image* __restrict__ recs,
                                                         const int32_t* __restrict__ tables, int h, int w,
                                                         uint8_t* __restrict__ out, int lds_stride) {
    extern __shared__ int32_t kx_s[];                        // [RS_TW][kss]: kss is odd, so a wave's reads of
                                                             // one tap index fall into 64 different banks
    const hkp_resample_image& rc = recs[blockIdx.z];         // block-uniform
    const int tid = threadIdx.x, col = tid & (RS_TW - 1), grp = tid / RS_TW;
    const int hs = rc.hs, ws = rc.ws, x0 = rc.x0, y0 = rc.y0, wd = rc.wd, hd = rc.hd;
    const int32_t* __restrict__ xt = tables + rc.xtab;
    const int32_t* __restrict__ yt = tables + rc.ytab;
    const int ksx = xt[0], ksy = yt[0];
    const int kss = KX_LDS ? (ksx < lds_stride ? ksx : lds_stride) : ksx;
    const int32_t* __restrict__ kxg = xt + 2 + 2 * (int64_t)wd;
    const int32_t* __restrict__ kyg = yt + 2 + 2 * (int64_t)hd;
    const int tx0 = blockIdx.x * RS_TW - x0;                 // rectangle column of the tile's column 0
    if (KX_LDS) {
        for (int i = tid; i < RS_TW * kss; i += 256) {
            const int c = i / kss, t = i - c * kss, xc = tx0 + c;
            if (xc >= 0 && xc < wd) kx_s[i] = kxg[(int64_t)xc * ksx + t];
        }
        __syncthreads();
    }
    const int x = blockIdx.x * RS_TW + col, xi = tx0 + col;
    const int gy = blockIdx.y * RS_TH + grp * RS_R;          // first output row of the row group
    const bool in_x = x < w && xi >= 0 && xi < wd;
    int xmin = 0, xcnt = 0;
    if (in_x) rs_bounds(xt, xi, ws, kss, xmin, xcnt);

    int ymin[RS_R], ycnt[RS_R], lo = 0x7fffffff, hi = 0;
#pragma unroll
    for (int r = 0; r < RS_R; ++r) {
        const int y = gy + r, yi = y - y0;
        ymin[r] = 0, ycnt[r] = 0;
        if (y < h && yi >= 0 && yi < hd) rs_bounds(yt, yi, hs, ksy, ymin[r], ycnt[r]);
        if (ycnt[r] > 0) {
            lo = ymin[r] < lo ? ymin[r] : lo;
            hi = ymin[r] + ycnt[r] > hi ? ymin[r] + ycnt[r] : hi;
        }
    }
    if (!in_x) hi = 0;

    int acc[RS_R][3];
#pragma unroll
    for (int r = 0; r < RS_R; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 0;
    const uint8_t* __restrict__ src = in + rc.offset;
    const int32_t* __restrict__ kxc = kxg + (int64_t)(in_x ? xi : 0) * ksx;
    const int64_t ky0 = (int64_t)(gy - y0) * ksy;            // (rows before the rectangle have ycnt = 0: never read)
    for (int sy = lo; sy < hi; ++sy) {
        const uint8_t* __restrict__ p = src + ((size_t)sy * ws + xmin) * 3;
        int a0 = 0, a1 = 0, a2 = 0;
        for (int t = 0; t < xcnt; ++t) {
            const int k = KX_LDS ? kx_s[col * kss + t] : kxc[t];
            a0 += (int)p[3 * t] * k;
            a1 += (int)p[3 * t + 1] * k;
            a2 += (int)p[3 * t + 2] * k;
        }
        const int m0 = rs_clip8(a0), m1 = rs_clip8(a1), m2 = rs_clip8(a2);   // Pillow's intermediate pixel
#pragma unroll
        for (int r = 0; r < RS_R; ++r) {
            const int t = sy - ymin[r];
            if ((unsigned)t < (unsigned)ycnt[r]) {
                const int k = kyg[ky0 + (int64_t)r * ksy + t];
                acc[r][0] += m0 * k;
                acc[r][1] += m1 * k;
                acc[r][2] += m2 * k;
            }
        }
    }

    const uint32_t fill = (uint32_t)rc.fill[0] | (uint32_t)rc.fill[1] << 8 | (uint32_t)rc.fill[2] << 16;
#pragma unroll
    for (int r = 0; r < RS_R; ++r) {
        const int y = gy + r, yi = y - y0;
        if (y >= h) break;                                   // wave-uniform
        uint32_t px = fill;
        if (in_x && yi >= 0 && yi < hd)
            px = (uint32_t)rs_clip8(acc[r][0]) | (uint32_t)rs_clip8(acc[r][1]) << 8 | (uint32_t)rs_clip8(acc[r][2]) << 16;
        uint8_t* row = out + ((size_t)blockIdx.z * h + y) * (size_t)w * 3;
        if (DWORD) {                                         // w % 4 == 0, out 4-byte aligned: 4 lanes' 12 bytes
            const int q = col & ~3, j = col & 3;             // leave as 3 dwords (every lane takes part)
            const uint32_t p0 = __shfl(px, q), p1 = __shfl(px, q + 1), p2 = __shfl(px, q + 2), p3 = __shfl(px, q + 3);
            const uint32_t d = j == 0 ? (p0 | p1 << 24) : (j == 1 ? (p1 >> 8 | p2 << 16) : (p2 >> 16 | p3 << 8));
            if (x < w && j < 3) ((uint32_t*)(row + (size_t)(x - j) * 3))[j] = d;
        } else if (x < w) {
            uint8_t* o = row + (size_t)x * 3;
            o[0] = (uint8_t)px;
            o[1] = (uint8_t)(px >> 8);
            o[2] = (uint8_t)(px >> 16);
        }
    }
}

// one axis table of one image, host copy: 0 when it is sound, else a message in `why`
static bool rs_table_ok(const int32_t* tab, int64_t words, int64_t off, int32_t out, int32_t extent, int32_t* ksize,
                        char* why, size_t n) {
    if (off < 0 || off > words - 2) {
        snprintf(why, n, "table offset %lld outside table_words=%lld", (long long)off, (long long)words);
        return false;
    }
    const int32_t ks = tab[off], o = tab[off + 1];
    if (ks < 1 || o != out) {
        snprintf(why, n, "table at word %lld has ksize=%d, out=%d (the rectangle needs out=%d)", (long long)off, ks, o,
                 out);
        return false;
    }
    if (2 + 2 * (int64_t)o + (int64_t)o * ks > words - off) {
        snprintf(why, n, "table offset %lld plus its size passes table_words=%lld", (long long)off, (long long)words);
        return false;
    }
    for (int32_t i = 0; i < o; ++i) {
        const int64_t lo = tab[off + 2 + 2 * (int64_t)i], cnt = tab[off + 3 + 2 * (int64_t)i];
        if (lo < 0 || cnt < 0 || lo + cnt > extent || cnt > ks) {
            snprintf(why, n, "output index %d: xmin=%lld, cnt=%lld: need xmin >= 0, cnt >= 0, xmin + cnt <= %d (the "
                     "source extent) and cnt <= ksize=%d", i, (long long)lo, (long long)cnt, extent, ks);
            return false;
        }
    }
    *ksize = ks;
    return true;
}

}  // namespace hkp

using namespace hkp;

extern "C" int hkp_resample_u8(int32_t n, const uint8_t* img_in, int64_t in_bytes,
                               const hkp_resample_image* records_host, const hkp_resample_image* records,
                               const int32_t* tables_host, const int32_t* tables, int64_t table_words, int32_t h,
                               int32_t w, uint8_t* img_out, hkp_stream_t stream) {
    static_assert(sizeof(hkp_resample_image) == 64, "hkp_resample_image layout");
    HKP_CHECK_ARG(n >= 1 && n <= 65535, "hkp_resample_u8: bad batch size n=%d (1..65535)", n);
    HKP_CHECK_ARG(h >= 1 && h <= HKP_WARP_MAX_DIM && w >= 1 && w <= HKP_WARP_MAX_DIM,
                  "hkp_resample_u8: output %dx%d outside 1..%d", h, w, HKP_WARP_MAX_DIM);
    HKP_CHECK_ARG(img_in && img_out && records_host && records && tables_host && tables,
                  "hkp_resample_u8: null pointer");
    HKP_CHECK_ARG(in_bytes >= 1 && table_words >= 2, "hkp_resample_u8: in_bytes=%lld, table_words=%lld",
                  (long long)in_bytes, (long long)table_words);
    HKP_CHECK_ARG(((uintptr_t)records & 7) == 0 && ((uintptr_t)tables & 3) == 0,
                  "hkp_resample_u8: records must be 8-byte and tables 4-byte aligned");
    const int64_t out_bytes = (int64_t)n * h * w * 3;
    HKP_CHECK_ARG(img_out + out_bytes <= img_in || img_in + in_bytes <= img_out,
                  "hkp_resample_u8: img_out must not overlap img_in");
    int32_t ksx_max = 1;
    char why[256];
    for (int32_t i = 0; i < n; ++i) {
        const hkp_resample_image& r = records_host[i];
        HKP_CHECK_ARG(r.reserved[0] == 0 && r.reserved[1] == 0 && r.reserved[2] == 0,
                      "hkp_resample_u8: image %d has a non-zero reserved field", i);
        HKP_CHECK_ARG(r.hs >= 1 && r.hs <= HKP_WARP_MAX_DIM && r.ws >= 1 && r.ws <= HKP_WARP_MAX_DIM,
                      "hkp_resample_u8: image %d: source %dx%d outside 1..%d", i, r.hs, r.ws, HKP_WARP_MAX_DIM);
        HKP_CHECK_ARG(r.offset >= 0 && r.offset <= in_bytes - (int64_t)r.hs * r.ws * 3,
                      "hkp_resample_u8: image %d: offset %lld + %dx%dx3 bytes passes in_bytes=%lld", i,
                      (long long)r.offset, r.hs, r.ws, (long long)in_bytes);
        HKP_CHECK_ARG(r.wd >= 1 && r.hd >= 1 && r.x0 >= 0 && r.y0 >= 0 && r.x0 <= w - r.wd && r.y0 <= h - r.hd,
                      "hkp_resample_u8: image %d: rectangle x0=%d y0=%d wd=%d hd=%d outside the %dx%d output", i, r.x0,
                      r.y0, r.wd, r.hd, h, w);
        int32_t ksx = 0, ksy = 0;
        HKP_CHECK_ARG(rs_table_ok(tables_host, table_words, r.xtab, r.wd, r.ws, &ksx, why, sizeof(why)),
                      "hkp_resample_u8: image %d, x table: %s", i, why);
        HKP_CHECK_ARG(rs_table_ok(tables_host, table_words, r.ytab, r.hd, r.hs, &ksy, why, sizeof(why)),
                      "hkp_resample_u8: image %d, y table: %s", i, why);
        ksx_max = ksx > ksx_max ? ksx : ksx_max;
    }
    const bool dword = w % 4 == 0 && ((uintptr_t)img_out & 3) == 0;
    const bool lds = (int64_t)ksx_max * RS_TW * 4 <= RS_LDS_BYTES;
    const dim3 grid((unsigned)((w + RS_TW - 1) / RS_TW), (unsigned)((h + RS_TH - 1) / RS_TH), (unsigned)n);
    const hipStream_t s = as_stream(stream);
    const size_t shm = lds ? (size_t)ksx_max * RS_TW * 4 : 0;
#define HKP_RS_CASE(D, L)                                                                                          \
    if (dword == D && lds == L)                                                                                    \
    hipLaunchKernelGGL((resample_u8_kernel<D, L>), grid, dim3(256), shm, s, img_in, records, tables, h, w, img_out, \
                       ksx_max)
    HKP_RS_CASE(true, true);
    HKP_RS_CASE(true, false);
    HKP_RS_CASE(false, true);
    HKP_RS_CASE(false, false);
#undef HKP_RS_CASE
    HKP_LAUNCH_CHECK("hkp_resample_u8");
    return HKP_OK;
}
