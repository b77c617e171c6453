// segresid.hip -- the nearest-neighbour residual PER SEGMENT of a labelled cloud, before and after the flow, on the GPU
// (include/icpflow_hip.h, "8(g) nearest-neighbour residual", icpflow_nn_residual_segments): which cluster was registered
// wrongly, without ground truth.
//
// The search is icpflow_nn_residual's (nnresid.hip through nnresid.hpp: the same kernels, no copy): the grid over the target is
// built ONCE; each side's queries -- BEFORE: d_before; AFTER: d_after + d_flow -- are binned into the one query grid of the
// workspace and run through the binned query kernel, one side after the other on the stream, so the second side's binning
// overwrites the first's only after its query kernel is through.
//
// Segments are the distinct labels in ascending order, as icpflow_cluster_table defines them (table.hip's launch_label_order),
// cut into chunks of 1024 rows of the stable order by segeval.hip's plan (launch_segment_plan).  Per side one launch of
// segr_chunk_kernel, a workgroup of 256 threads per chunk, behind that side's query: the one idx array of the workspace holds
// the side that ran last.
//
// Determinism: every number is a function of the arguments alone.
//   1. thread t of a chunk's workgroup takes the chunk's rows t, t + 256, t + 512, t + 768 (positions in the stable order), in
//      that order; its two sums grow in that order;
//   2. counts by ballot and popcount; the 64 partial sums of a wave through one fixed butterfly (wave_sum), the four waves added
//      in wave order;
//   3. segr_final_kernel adds the chunks of a segment in ascending chunk order.
// No floating-point atomic anywhere; every workgroup of either side stores its whole partial and the final kernel reads only
// the chunks the plan counts, so nothing in the workspace is read before it is written.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"
#include "host.hpp"
#include "kernels.hpp"
#include "nnresid.hpp"

using icpflow::kWave;
using icpflow::pointer_error;
using icpflow::report_error;
using icpflow::report_errorf;
using icpflow::workspace_error;
using icpflow::nnr::Cloud;
using icpflow::nnr::Edges;
using icpflow::nnr::Grid;
using icpflow::nnr::kMaxEdges;
using icpflow::nnr::kMaxRadius;
using icpflow::nnr::kMaxRows;
using icpflow::nnr::kMinRadius;

namespace {

constexpr int kChunk = icpflow::kSegmentChunk;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kPerThread = kChunk / kThreads;
constexpr int kCols = ICPFLOW_NNRS_COLS;
constexpr int kSide = 4 + kMaxEdges;                  // good rows, hits, kMaxEdges counts, sum d, sum d * d: a side's eight columns
constexpr int kLmax = 4096;
constexpr int kOrderCols = icpflow::kLabelOrderCols;  // label, count, start, ...
static_assert(kCols == 2 + 2 * kSide, "label, rows, and a side's columns twice");

// what the call carves out of its workspace, in this order (the size query runs it on a null base)
struct Carve {
    Grid targets, queries;   // one grid over the target; ONE query grid, reused by the second side
    float *d2[2];            // [n] each: before, after (the caller's arrays are used where given)
    int32_t *idx;            // [n] the side that ran last
    int64_t *order;          // [n] rows sorted by label, stable
    double *ctable;          // [Lmax][kOrderCols] label, count, start
    int *chunkStart;         // [Lmax + 1] first chunk of every segment, then the number of chunks
    double *partial;         // [max chunks][2][kSide]
    void *sort;              // table.hip's own workspace
    size_t sortBytes, total;
};

bool carve(void *base, int n, int m, int Lmax, Carve *c)
{
    size_t sortBytes = 0;
    if (icpflow::cluster_table_workspace_bytes(n > 1 ? n : 1, Lmax, &sortBytes) != hipSuccess) return false;
    icpflow::Carver ws(base);
    c->targets = icpflow::nnr::carve_grid(ws, m);
    c->queries = icpflow::nnr::carve_grid(ws, n);
    c->d2[0] = ws.take<float>((size_t)n * sizeof(float));
    c->d2[1] = ws.take<float>((size_t)n * sizeof(float));
    c->idx = ws.take<int32_t>((size_t)n * sizeof(int32_t));
    c->order = ws.take<int64_t>((size_t)n * sizeof(int64_t));
    c->ctable = ws.take<double>((size_t)Lmax * kOrderCols * sizeof(double));
    c->chunkStart = ws.take<int>(((size_t)Lmax + 1) * sizeof(int));
    c->partial = ws.take<double>((size_t)icpflow::segment_max_chunks(n, Lmax) * 2 * kSide * sizeof(double));
    c->sort = ws.take<void>(sortBytes);
    c->sortBytes = sortBytes;
    c->total = ws.total();
    return true;
}

// One workgroup per chunk, one side: partial[chunk][side][kSide].
__global__ __launch_bounds__(kThreads) void segr_chunk_kernel(const float *__restrict__ d2_in, const int32_t *__restrict__ idx_in, Edges ed,
                                                              const int64_t *__restrict__ order, const double *__restrict__ ctable,
                                                              const int32_t *__restrict__ num, const int *__restrict__ chunkStart, int side,
                                                              double *__restrict__ partial)
{
    __shared__ double sh[kWaves][kSide];
    const int L = *num, b = blockIdx.x;
    if (L <= 0 || b >= chunkStart[L]) return;          // (workgroup-uniform)
    int lo = 0, hi = L - 1;                            // the segment of chunk b: the last one that starts at or before it
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (chunkStart[mid] <= b) lo = mid; else hi = mid - 1;
    }
    const double *seg = ctable + (size_t)lo * kOrderCols;
    const int count = (int)seg[1], start = (int)seg[2];
    const int first = (b - chunkStart[lo]) * kChunk;
    const int rows = min(kChunk, count - first);
    double sum_d = 0.0, sum_dd = 0.0;                  // this thread's rows, in their order
    int good = 0, hits = 0, under[kMaxEdges] = {0, 0, 0, 0};   // the wave's counts (wave-uniform)
#pragma unroll
    for (int u = 0; u < kPerThread; ++u) {             // (every lane takes every round: the ballots see whole waves)
        const int j = u * kThreads + (int)threadIdx.x;
        bool counted = false, hit = false;
        double d = 0.0;
        if (j < rows) {
            const size_t i = (size_t)order[(size_t)start + first + j];
            const int at = idx_in[i];
            counted = at != -2;                        // a bad query enters nothing
            hit = at >= 0;
            if (counted) d = (double)sqrtf(d2_in[i]);  // (a miss holds r2: the distance truncated at the radius)
        }
        good += __popcll(__ballot(counted));
        hits += __popcll(__ballot(counted && hit));
#pragma unroll
        for (int e = 0; e < kMaxEdges; ++e) under[e] += __popcll(__ballot(counted && e < ed.E && d <= ed.edge[e]));
        if (counted) sum_d += d, sum_dd += d * d;
    }
    sum_d = icpflow::wave_sum(sum_d), sum_dd = icpflow::wave_sum(sum_dd);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & (kWave - 1)) == 0) {
        double *w = sh[wave];
        w[0] = (double)good, w[1] = (double)hits;
#pragma unroll
        for (int e = 0; e < kMaxEdges; ++e) w[2 + e] = (double)under[e];
        w[2 + kMaxEdges] = sum_d, w[3 + kMaxEdges] = sum_dd;
    }
    __syncthreads();
    if (threadIdx.x < kSide) {                         // the waves in wave order
        double t = sh[0][threadIdx.x];
        for (int w = 1; w < kWaves; ++w) t += sh[w][threadIdx.x];
        partial[((size_t)b * 2 + side) * kSide + threadIdx.x] = t;
    }
}

// One thread per (segment, column): the chunks of the segment in ascending order.
__global__ __launch_bounds__(kThreads) void segr_final_kernel(const double *__restrict__ ctable, const int32_t *__restrict__ num,
                                                              const int *__restrict__ chunkStart, const double *__restrict__ partial,
                                                              double *__restrict__ table)
{
    const int L = *num;
    const int at = blockIdx.x * kThreads + threadIdx.x, c = at / kCols, col = at % kCols;
    if (c >= L) return;                                // (also when L < 0: nothing of the table is written)
    double out;
    if (col < 2) {
        out = ctable[(size_t)c * kOrderCols + col];
    } else {
        const int k = col - 2;                         // (side, column of the side): the partial's own layout
        const int c0 = chunkStart[c], c1 = chunkStart[c + 1];
        out = partial[(size_t)c0 * 2 * kSide + k];
        for (int q = c0 + 1; q < c1; ++q) out += partial[(size_t)q * 2 * kSide + k];
    }
    table[(size_t)c * kCols + col] = out;
}

bool sizes_ok(int n, int m, int Lmax, int E) { return n >= 0 && m >= 0 && n <= kMaxRows && m <= kMaxRows && Lmax >= 1 && Lmax <= kLmax && E >= 0 && E <= kMaxEdges; }

}  // namespace

extern "C" {

size_t icpflow_nn_residual_segments_workspace_bytes(int n, int m, int Lmax, int E)
{
    if (!sizes_ok(n, m, Lmax, E)) return 0;
    Carve c{};
    return carve(nullptr, n, m, Lmax, &c) ? c.total : 0;
}

int icpflow_nn_residual_segments(const float *d_before, const float *d_after, const float *d_flow, const float *d_labels, int n,
                                 const float *d_target, int m, double radius, const double *h_edges, int E, double *d_table, int Lmax,
                                 int32_t *d_num, float *d_d2_before, float *d_d2_after, int64_t *d_info, void *d_ws, size_t ws_bytes,
                                 icpflow_stream_t stream)
{
    const char *fn = "icpflow_nn_residual_segments";
    if (n < 0 || m < 0) return report_error(ICPFLOW_E_ARG, "icpflow_nn_residual_segments: n < 0 or m < 0");
    if (n > kMaxRows || m > kMaxRows)
        return report_errorf(ICPFLOW_E_LIMIT, "icpflow_nn_residual_segments: n = %d, m = %d: at most %d rows a cloud (twice as many buckets are indexed by an int)", n, m, kMaxRows);
    if (Lmax < 1) return report_errorf(ICPFLOW_E_ARG, "icpflow_nn_residual_segments: Lmax = %d: Lmax must be at least 1", Lmax);
    if (Lmax > kLmax) return report_errorf(ICPFLOW_E_LIMIT, "icpflow_nn_residual_segments: Lmax = %d: at most %d segments", Lmax, kLmax);
    if (!(radius >= kMinRadius && radius <= kMaxRadius))
        return report_errorf(ICPFLOW_E_ARG, "icpflow_nn_residual_segments: radius = %g: the radius must lie in [1e-3, 1e3] metres", radius);
    if (E < 0 || E > kMaxEdges) return report_errorf(ICPFLOW_E_ARG, "icpflow_nn_residual_segments: E = %d: E must lie in [0, %d]", E, kMaxEdges);
    if (!d_info || !d_table || !d_num || (E > 0 && !h_edges) || (n > 0 && (!d_before || !d_after || !d_labels)) || (m > 0 && !d_target))
        return pointer_error(fn);
    if (!icpflow::edges_ok(h_edges, E) || (E > 0 && (!(h_edges[0] > 0.0) || !(h_edges[E - 1] <= radius))))
        return report_error(ICPFLOW_E_ARG, "icpflow_nn_residual_segments: the edges must be finite, positive, strictly ascending and at most the radius");
    Carve c{};
    if (!carve(d_ws, n, m, Lmax, &c)) return report_error(ICPFLOW_E_ARG, "icpflow_nn_residual_segments: no workspace layout for these sizes");
    if (!d_ws || ws_bytes < c.total) return workspace_error(fn, "icpflow_nn_residual_segments_workspace_bytes", d_ws, ws_bytes, c.total);
    if (((uintptr_t)d_ws & 15) != 0) return report_error(ICPFLOW_E_ARG, "icpflow_nn_residual_segments: d_ws must be 16-byte aligned");

    hipStream_t st = (hipStream_t)stream;
    const float rf = (float)radius, r2 = rf * rf;
    const double h = 1.01 * radius;
    unsigned long long *info = (unsigned long long *)d_info;   // bad queries before, after, bad targets, occupied, longest, 0
    const Cloud targets = {d_target, nullptr, nullptr, m, 1};
    const Cloud sides[2] = {{d_before, nullptr, nullptr, n, 1}, {d_after, d_flow, nullptr, n, 1}};
    float *d2[2] = {d_d2_before ? d_d2_before : c.d2[0], d_d2_after ? d_d2_after : c.d2[1]};

    ICPFLOW_TRY(hipMemsetAsync(info, 0, 6 * sizeof(unsigned long long), st));
    // (the scan writes the occupied buckets and the longest one to words 2 and 3 of what it is given: words 3 and 4 of d_info)
    ICPFLOW_TRY(icpflow::nnr::bin_cloud(targets, c.targets, h, info + 2, info + 1, r2, nullptr, nullptr, st));
    if (n == 0) {
        ICPFLOW_TRY(hipMemsetAsync(d_num, 0, sizeof(int32_t), st));
        return ICPFLOW_OK;
    }
    bool tooSmall = false;
    ICPFLOW_TRY(icpflow::launch_label_order(d_labels, n, c.order, c.ctable, Lmax, d_num, c.sort, c.sortBytes, &tooSmall, st));
    if (tooSmall) return workspace_error(fn, "icpflow_nn_residual_segments_workspace_bytes", d_ws, ws_bytes, c.total);   // (cannot happen: same carve)
    ICPFLOW_TRY(icpflow::launch_segment_plan(c.ctable, d_num, c.chunkStart, st));
    Edges ed;
    ed.E = E;
    for (int k = 0; k < kMaxEdges; ++k) ed.edge[k] = k < E ? h_edges[k] : 0.0;
    const int chunks = icpflow::segment_max_chunks(n, Lmax);
    for (int side = 0; side < 2; ++side) {
        ICPFLOW_TRY(icpflow::nnr::bin_cloud(sides[side], c.queries, h, info + side, nullptr, r2, d2[side], c.idx, st));
        ICPFLOW_TRY(icpflow::nnr::launch_binned_query(c.queries, c.targets, n, r2, h, d2[side], c.idx, st));
        segr_chunk_kernel<<<chunks, kThreads, 0, st>>>(d2[side], c.idx, ed, c.order, c.ctable, d_num, c.chunkStart, side, c.partial);
        ICPFLOW_TRY(hipGetLastError());
    }
    segr_final_kernel<<<(Lmax * kCols + kThreads - 1) / kThreads, kThreads, 0, st>>>(c.ctable, d_num, c.chunkStart, c.partial, d_table);
    ICPFLOW_TRY(hipGetLastError());
    return ICPFLOW_OK;
}

}  // extern "C"
