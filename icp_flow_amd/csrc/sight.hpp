// sight.hpp -- what the kernels of sight.hip share: the view of one destination sweep as the device sees it (every
// parameter narrowed to float once, on the host), the pixel map and the ray test.  The arithmetic is the one
// include/icpflow_hip.h states ("8(h) line of sight"): no transcendental function, every operation rounded by itself in fp32
// (-ffp-contract=off), IEEE division and sqrtf (-fhip-fp32-correctly-rounded-divide-sqrt), so that a NumPy float32
// restatement equals the kernels bit for bit (tests/sight_restatement.py).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nnresid.hpp"
#include "../../include/icpflow_hip.h"

namespace icpflow {
namespace sight {

constexpr int kMaxW = 8192, kMaxH = 2048, kMaxPixels = 1 << 22;
constexpr double kMaxRange = 1e6;
constexpr uint32_t kEmpty = 0x7f800000u;            // the bits of +inf: a pixel without a return
constexpr int kCodes = 5;                           // ICPFLOW_SIGHT_OUTSIDE .. ICPFLOW_SIGHT_BEHIND
constexpr int kBadRow = -2;

struct View {
    float ox, oy, oz;                               // the sensor origin
    float tan_lo, tan_hi, rs;                       // rs = (float)H / (tan_hi - tan_lo)
    float min_range, max_range, margin_abs, margin_rel;
    float quarter;                                  // (float)(W / 4)
    int W, H;
};

// (x, y, z) -> its pixel row * W + col and rho, or -1 (OUTSIDE: no pixel; rho is still the range)
__device__ __forceinline__ int pixel_of(const View &v, float x, float y, float z, float &rho)
{
    const float ux = x - v.ox, uy = y - v.oy, uz = z - v.oz;
    const float h2 = ux * ux + uy * uy;
    const float d2 = h2 + uz * uz;
    rho = sqrtf(d2);
    const float s = fabsf(ux) + fabsf(uy);
    if (s == 0.0f) return -1;                       // on the vertical axis
    const float g = uy / s;
    float p;                                        // the diamond angle in [0, 4]
    if (ux >= 0.0f) p = uy >= 0.0f ? g : 4.0f + g;  // (-0.0 >= 0)
    else p = 2.0f - g;
    int col = (int)floorf(p * v.quarter);
    if (col >= v.W) col = 0;                        // p rounded to 4
    const float t = uz / sqrtf(h2);
    if (!(t >= v.tan_lo && t < v.tan_hi)) return -1;   // (an infinite or NaN t too)
    if (rho < v.min_range || rho > v.max_range) return -1;
    int row = (int)floorf((t - v.tan_lo) * v.rs);
    if (row >= v.H) row = v.H - 1;                  // (t - tan_lo) * rs rounded up to H
    return row * v.W + col;
}

// the ray test of one query against plane 1 of the image: -> its code, near = n9 (+inf where the row has no pixel)
__device__ __forceinline__ int classify(const View &v, const uint32_t *__restrict__ plane1, float x, float y, float z, float &near)
{
    near = __uint_as_float(kEmpty);
    if (!nnr::good_coord(x, y, z)) return kBadRow;
    float rho;
    const int pix = pixel_of(v, x, y, z, rho);
    if (pix < 0) return ICPFLOW_SIGHT_OUTSIDE;
    const uint32_t bits = plane1[pix];
    near = __uint_as_float(bits);
    if (bits == kEmpty) return ICPFLOW_SIGHT_NO_RETURN;
    const float thr = v.margin_abs + v.margin_rel * rho;
    if (rho + thr < near) return ICPFLOW_SIGHT_SEEN_THROUGH;
    if (rho - thr <= near) return ICPFLOW_SIGHT_AT_FIRST_RETURN;
    return ICPFLOW_SIGHT_BEHIND;
}

}  // namespace sight
}  // namespace icpflow
