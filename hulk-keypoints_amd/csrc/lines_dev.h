// What the line kernels share (lines.hip, loss_multi.hip's line walk): the tile, the cull
// margin and the definition's squared distance to a segment.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace hkp {

constexpr int LINE_TW = 32, LINE_TH = 32;   // the tile: 8 threads x 4 pixels across, 32 rows
constexpr float CULL_MARGIN = 2.f;          // pixels

// the definition's squared distance from (fx, fy) to the segment (x0, y0) + t (dx, dy)
__device__ __forceinline__ float seg_d2(float fx, float fy, float x0, float y0, float dx, float dy, float inv) {
    const float px = fx - x0, py = fy - y0;
    const float t = fminf(fmaxf((px * dx + py * dy) * inv, 0.f), 1.f);
    const float cx = px - t * dx, cy = py - t * dy;
    return cx * cx + cy * cy;
}

}  // namespace hkp
