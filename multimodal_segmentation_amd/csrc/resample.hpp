// The bilinear resampling of a raw slice onto the loader's RH x RW frame, shared by the units that must meet the same values bit for
// bit (preprocess.hip: min / max, quantiles and the containers; align.hip: the quantised frames).  Nothing is contracted.
#pragma once
#include "common.hpp"

// source coordinate of resampled pixel d; `ratio` = in / out computed in fp64 by the launcher
__device__ __forceinline__ double pp_coord(int d, double ratio) {
#pragma clang fp contract(off)
    return ((double)d + 0.5) * ratio - 0.5;
}

// bilinear sample of one raw slice at resampled pixel (dr, dc); 0 outside (strict)
__device__ __forceinline__ float pp_bilinear(const float* __restrict__ s, int H, int W, int dr, int dc, double ry, double rx) {
#pragma clang fp contract(off)
    const double sy = pp_coord(dr, ry), sx = pp_coord(dc, rx);
    if (!(sy >= 0.0 && sy <= (double)(H - 1) && sx >= 0.0 && sx <= (double)(W - 1))) return 0.f;
    const double fyd = floor(sy), fxd = floor(sx);
    const float fy = (float)(sy - fyd), fx = (float)(sx - fxd);
    const int r0 = (int)fyd, c0 = (int)fxd;
    const int r1 = min(r0 + 1, H - 1), c1 = min(c0 + 1, W - 1);        // a tap beyond the edge carries weight 0
    const float a00 = s[(size_t)r0 * W + c0], a01 = s[(size_t)r0 * W + c1];
    const float a10 = s[(size_t)r1 * W + c0], a11 = s[(size_t)r1 * W + c1];
    const float top = (1.f - fx) * a00 + fx * a01;
    const float bot = (1.f - fx) * a10 + fx * a11;
    return (1.f - fy) * top + fy * bot;
}
