// overlap.hpp -- the overlap of two labellings of the same rows (include/icpflow_hip.h, "8(k) object tracks") as overlap.hip
// computes it and tracks.hip reuses it: the workspace's layout, the chain of launches, and what makes a label linkable -- each
// stated once, so that a track inherits by the same partner, mutual and IoU that icpflow_label_overlap reports.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "carver.hpp"
#include "kernels.hpp"
#include "labelkey.hpp"
#include "../../include/icpflow_hip.h"

namespace icpflow {
namespace overlap {

constexpr int kLmax = 4096;
constexpr int kMaxRows = 1 << 29;
constexpr int kCols = ICPFLOW_OVERLAP_COLS, kCounts = ICPFLOW_OVERLAP_COUNTS;
constexpr int kOrderCols = icpflow::kLabelOrderCols;   // label, count, start, ...
constexpr int kChunk = icpflow::kSegmentChunk;

// a label is a segment to link unless it is negative (ground -1e8, noise -1, -inf); a NaN is no negative number
__host__ __device__ __forceinline__ bool linkable(double label) { return !(label < 0.0); }

// one labelling's part of the workspace
struct Side {
    int64_t *order;        // [n] rows sorted by label, stable
    double *ctable;        // [Lmax][kOrderCols] label, count, start
    int *chunkStart;       // [Lmax + 1] first chunk of every segment, then the number of chunks
    int32_t *segOf;        // [n] the row's segment, -1 when its label is not linkable
    int *listCount;        // [max chunks] entries of the chunk's list
    uint32_t *list;        // [max chunks][kChunk] the chunk's non-zero counters, (other segment << 16) | rows, ascending
    int *link;             // [Lmax][4] partner, inter, second, rows whose other label is linkable
};

struct Carve {
    Side side[2];
    void *sort;            // table.hip's own workspace, one side after the other
    size_t sortBytes;
};

// the regions of one overlap, taken from `ws` in this order -> false when table.hip has no layout for these sizes
bool carve(Carver &ws, int n, int Lmax, Carve *c);

// The chain up to the folds: both label orders (the numbers of segments land in numA and numB, negative on overflow), the
// plans, the rows' segments, the chunk histograms and the fold per segment -> side[].link.  n > 0.
hipError_t launch_links(const float *labelsA, const float *labelsB, int n, int Lmax, int32_t *numA, int32_t *numB, const Carve &c,
                        hipStream_t s);
// ... and the closing kernel: both tables and the counts (nothing of the tables when either number is not positive)
hipError_t launch_tables(const Carve &c, const int32_t *numA, const int32_t *numB, int Lmax, double *tableA, double *tableB,
                         int64_t *counts, hipStream_t s);

}  // namespace overlap
}  // namespace icpflow
