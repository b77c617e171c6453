// gridhash.hpp -- cell and bucket of a point in the hashed uniform grid: the build (icp_prep.hip) and the search (icp.hip)
// must agree on both.
#pragma once
#include <hip/hip_runtime.h>

namespace icpflow {

// ---------------------------------------------------------------------------------
// Exact nearest neighbour within the gate radius through a hashed uniform grid.
//
// The ICP loop consumes the NN search only through the gate d^2 <= thres^2 and the neighbour of
// gated points (utils_icp_pytorch3d.py:160-164), and the fixed cloud never changes during a
// registration.  So the fixed cloud is binned ONCE into cells of edge h = 1.01 * thres (hashed
// into H = 2^k >= 2N buckets, counting sort); a query then evaluates only the points of the 27
// cells around it.  Every point within the gate radius of the query lies in those cells
// (|coordinate difference| <= thres < h  =>  cell index difference <= 1; the cell index is a
// monotone function of the coordinate), distances are evaluated with the SAME fp32 instruction
// sequence as the brute-force scan and ties go to the lowest original index, so gate decisions
// and neighbours -- hence every transform -- are bit-identical to the all-pairs search, at
// ~30 instead of n distance evaluations per query.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ int grid_cell(float v, float o, float invh)
{
    return (int)floorf((v - o) * invh);
}

__device__ __forceinline__ unsigned grid_hash(int cx, int cy, int cz, unsigned mask)
{
    return ((unsigned)cx * 73856093u ^ (unsigned)cy * 19349663u ^ (unsigned)cz * 83492791u) & mask;
}

}  // namespace icpflow
