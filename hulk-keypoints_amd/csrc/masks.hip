// Ignore masks from region records (include/hulkkp.h has the definition):
// hkp_mask_regions_u8 rasterises up to 64 boxes and discs per image into the class-bit
// bytes hkp_heat_loss_masked reads, uint8 [n][H][W], every byte written in one launch.
// A block owns one MASK_TH x MASK_TW tile of one image; wave 0 stages the image's records
// in LDS (an empty slot as kind 0: its other fields are never read into the result), and a
// thread makes 4 consecutive pixels of one row.  The inside tests are fp32 comparisons with
// every product and sum rounded on its own; tests/_masks_ref.py restates them in numpy.
#include "common.h"

#pragma clang fp contract(off)

namespace hkp {

constexpr int MASK_TH = 16, MASK_TW = 64, MASK_PX = 4;       // tile, pixels per thread
static_assert(MASK_TH * MASK_TW == 256 * MASK_PX, "one tile per 256-thread block");

template <bool DWORD>
__global__ __launch_bounds__(256) void mask_regions_u8_kernel(int r, int H, int W, const float* __restrict__ regions,
                                                             uint8_t* __restrict__ out) {
    __shared__ float sa[HKP_MASK_MAX_REGIONS], sb[HKP_MASK_MAX_REGIONS], sc[HKP_MASK_MAX_REGIONS],
        sd[HKP_MASK_MAX_REGIONS];
    __shared__ int skind[HKP_MASK_MAX_REGIONS], sbits[HKP_MASK_MAX_REGIONS];
    const int tid = threadIdx.x, n = blockIdx.z;
    if (tid < r) {
        const float* rec = regions + ((size_t)n * r + tid) * 6;
        const float kf = rec[0];
        const int kind = kf == 1.f ? HKP_MASK_BOX : (kf == 2.f ? HKP_MASK_DISC : 0);
        float a = 0.f, b = 0.f, c = 0.f, d = 0.f, bf = 0.f;
        if (kind != 0) a = rec[1], b = rec[2], c = rec[3], d = rec[4], bf = rec[5];
        sa[tid] = a, sb[tid] = b, sd[tid] = d;
        sc[tid] = kind == HKP_MASK_DISC ? c * c : c;         // the disc's r^2, once
        skind[tid] = kind;
        sbits[tid] = (bf >= 0.f && bf <= 255.f) ? (int)bf : 0;
    }
    __syncthreads();
    const int x = blockIdx.x * MASK_TW + (tid % (MASK_TW / MASK_PX)) * MASK_PX;
    const int y = blockIdx.y * MASK_TH + tid / (MASK_TW / MASK_PX);
    if (x >= W || y >= H) return;
    const float fy = (float)y;
    int px[MASK_PX] = {0, 0, 0, 0};
    for (int j = 0; j < r; ++j) {                            // block-uniform trip count
        const int kind = skind[j];
        if (kind == 0) continue;
        const float a = sa[j], b = sb[j], c = sc[j], d = sd[j];
        const int bits = sbits[j];
        if (kind == HKP_MASK_BOX) {
            const bool rowin = b <= fy && fy <= d;
#pragma unroll
            for (int e = 0; e < MASK_PX; ++e) {
                const float fx = (float)(x + e);
                if (rowin && a <= fx && fx <= c) px[e] |= bits;
            }
        } else {
            const float dy = fy - b;
            const float dy2 = dy * dy;
#pragma unroll
            for (int e = 0; e < MASK_PX; ++e) {
                const float dx = (float)(x + e) - a;
                if (dx * dx + dy2 <= c) px[e] |= bits;
            }
        }
    }
    uint8_t* dst = out + ((size_t)n * H + y) * W + x;
    if (DWORD) {                                             // W % 4 == 0, out 4-byte aligned: x + 3 < W
        *(uint32_t*)dst = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16) | ((uint32_t)px[3] << 24);
    } else {
#pragma unroll
        for (int e = 0; e < MASK_PX; ++e)
            if (x + e < W) dst[e] = (uint8_t)px[e];
    }
}

}  // namespace hkp

using namespace hkp;

extern "C" int hkp_mask_regions_u8(int32_t n, int32_t r, int32_t H, int32_t W, const float* regions, uint8_t* out,
                                   hkp_stream_t stream) {
    HKP_CHECK_ARG(n >= 1 && n <= 65535, "hkp_mask_regions_u8: bad batch size n=%d (1..65535)", n);
    HKP_CHECK_ARG(r >= 1 && r <= HKP_MASK_MAX_REGIONS, "hkp_mask_regions_u8: r = %d regions outside 1..%d", r,
                  HKP_MASK_MAX_REGIONS);
    HKP_CHECK_ARG(H >= 1 && H <= HKP_MASK_MAX_DIM && W >= 1 && W <= HKP_MASK_MAX_DIM,
                  "hkp_mask_regions_u8: mask %dx%d outside 1..%d", H, W, HKP_MASK_MAX_DIM);
    HKP_CHECK_ARG(regions && out, "hkp_mask_regions_u8: null pointer");
    HKP_CHECK_ARG(((uintptr_t)regions & 3) == 0, "hkp_mask_regions_u8: regions must be 4-byte aligned");
    const bool dword = W % 4 == 0 && ((uintptr_t)out & 3) == 0;
    const dim3 grid((unsigned)((W + MASK_TW - 1) / MASK_TW), (unsigned)((H + MASK_TH - 1) / MASK_TH), (unsigned)n);
    const hipStream_t s = as_stream(stream);
    if (dword)
        hipLaunchKernelGGL(mask_regions_u8_kernel<true>, grid, dim3(256), 0, s, r, H, W, regions, out);
    else
        hipLaunchKernelGGL(mask_regions_u8_kernel<false>, grid, dim3(256), 0, s, r, H, W, regions, out);
    HKP_LAUNCH_CHECK("hkp_mask_regions_u8");
    return HKP_OK;
}
