// boxes.hpp -- the oriented boxes of include/icpflow_hip.h, "8(j) object boxes", as the kernels of boxes.hip compute them: the
// columns of the two tables, the direction table that travels in the kernel arguments, which rows of a segment are used, and
// the two projections of a row -- each stated once, so that the extrema and the counts are taken from the same u and v.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "labelkey.hpp"
#include "../../include/icpflow_hip.h"

namespace icpflow {
namespace boxes {

constexpr int kLmax = 4096;
constexpr int kMaxRows = 1 << 29;
constexpr int kMaxDirs = ICPFLOW_BOX_MAX_DIRECTIONS;
constexpr int kBoxCols = ICPFLOW_BOX_COLS, kObjectCols = ICPFLOW_OBJECT_COLS, kCounts = ICPFLOW_OBJECT_COUNTS;
constexpr int kOrderCols = icpflow::kLabelOrderCols;   // label, count, start, centroid x y z, ...
constexpr int kChunk = icpflow::kSegmentChunk;

// the caller's unit vectors (c_k, s_k): 2880 bytes of kernel arguments, indexed wave-uniformly
struct Dirs {
    float cs[kMaxDirs][2];
};

// the rows of the stable order that segment `seg` may use: its start and count as the table has them, clipped to [0, n) -- a
// start outside [0, n] leaves nothing, a count is cut at n - start (a NaN fails every comparison and leaves nothing)
__device__ __forceinline__ void segment_rows(const double *__restrict__ seg, int n, int *start, int *count)
{
    const double c = seg[1], s = seg[2];
    int st = 0, cn = 0;
    if (s >= 0.0 && s <= (double)n && c > 0.0) {
        st = (int)s;
        cn = c < (double)(n - st) ? (int)c : n - st;
    }
    *start = st, *count = cn;
}

__device__ __forceinline__ bool finite3(float x, float y, float z)
{
    return fabsf(x) < __int_as_float(0x7f800000) && fabsf(y) < __int_as_float(0x7f800000) && fabsf(z) < __int_as_float(0x7f800000);
}

// the projections of a row already moved to the reference point (-ffp-contract=off: every fused operation is written out)
__device__ __forceinline__ float proj_u(float x, float y, float c, float s) { return fmaf(y, s, x * c); }
__device__ __forceinline__ float proj_v(float x, float y, float c, float s) { return fmaf(y, c, -(x * s)); }

// a NaN label as the tables' float64 column holds it: widening a float quiets a signalling NaN, its payload kept (trust.hpp)
__device__ __forceinline__ float quieted(float f)
{
    return f != f ? __uint_as_float(__float_as_uint(f) | 0x00400000u) : f;
}

}  // namespace boxes
}  // namespace icpflow
