// nnresid.hpp -- what nnresid.hip shares with segresid.hip: the hashed grid over one cloud, its carve, its build and the launch
// of the binned query.  Declarations only: the kernels and every definition stay in nnresid.hip, so both entry points run the
// same device code.  The inline functions are the bad-row rule, which sight.hip applies word for word, and the cell of a coordinate.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "carver.hpp"
#include "../../include/icpflow_hip.h"

namespace icpflow {
namespace nnr {

constexpr int kMaxEdges = ICPFLOW_NNR_MAX_EDGES;
constexpr int kMaxRows = 1 << 29;                   // of either cloud: 2^k >= 2 rows buckets stay an int
constexpr double kMinRadius = 1e-3, kMaxRadius = 1e3;

constexpr float kFar = 1e6f;                        // a coordinate beyond it is a bad row

// the bad-row rule of every entry point that judges rows of a cloud (sight.hip's too)
__device__ __forceinline__ bool good_coord(float x, float y, float z)   // (a NaN fails every comparison)
{
    return fabsf(x) <= kFar && fabsf(y) <= kFar && fabsf(z) <= kFar;
}

// the cell of a coordinate on a grid of edge h: one IEEE fp64 division (nnresid.hip states why the index fits an int)
__device__ __forceinline__ int cell_of(float v, double h) { return (int)floor((double)v / h); }

struct Edges {
    int E;
    double edge[kMaxEdges];
};

// a cloud as the binning kernels see it: the targets (no flow, no groups) or the queries (q = p + f, a group per row)
struct Cloud {
    const float *pts, *flow;
    const int32_t *group;
    int rows, G;
};

// a hashed grid over one cloud in the workspace: H buckets (cursor: counts, then running ends; start), the scan's words per
// tile of 1024 buckets, the number of rows in the table, the records
struct Grid {
    unsigned *cursor, *start, *tile_sum, *tile_occupied, *tile_longest, *tile_offset, *rows;
    float4 *records;
    int H, tiles;
};

Grid carve_grid(Carver &ws, int rows);

// count / scan / scatter of one cloud into its grid, enqueued on `st`; `bad_rows`: the word the bad rows are counted into (the
// caller has cleared it); d_info (the targets' grid only, or NULL): d_info[2] the occupied buckets, d_info[3] the longest one;
// d2 / idx (the queries only): the outputs of the bad rows
hipError_t bin_cloud(const Cloud &cloud, const Grid &g, double h, unsigned long long *bad_rows, unsigned long long *d_info, float r2,
                     float *d2, int32_t *idx, hipStream_t st);

// the middle of bin_cloud on its own, for a caller that counts and scatters with kernels of its own (carry.hip moves its rows
// first): g.cursor holds the count of every bucket (grid_hash of the rows' cells, mask H - 1); after it g.start has every
// bucket's first slot, g.cursor the same as a running cursor, *g.rows the total; d_info as bin_cloud's
void scan_grid(const Grid &g, unsigned long long *d_info, hipStream_t st);

// the binned query: the n rows that bin_cloud left in `queries` against the grid `targets`; writes d2 and idx of every good
// query row (the bad ones have theirs from bin_cloud).  n == 0: nothing is launched.
hipError_t launch_binned_query(const Grid &queries, const Grid &targets, int n, float r2, double h, float *d2, int32_t *idx,
                               hipStream_t st);

}  // namespace nnr
}  // namespace icpflow
