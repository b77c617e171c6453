// segeval.hip -- the per-segment evaluation of one labelled cloud on the GPU (include/icpflow_hip.h, "8(f) per-segment
// evaluation"): what the reference's flow_evaluation computes per np.unique(labels) with boolean masks over all points
// (utils_flow.py:86-95, 110, 123) and debug_frame's z crop before it (utils_debug.py:37-46) -- per segment the rows, the kept
// rows, the sum of the end point error, the four predicate counts of compute_epe_test (utils_eval.py:162-180) and the
// coordinate sums behind mean_i, mean_j and mean(x + flow).
//
// Segments are the distinct labels in ascending order, as icpflow_cluster_table defines them: table.hip's dictionary and
// stable counting sort (launch_label_order) give the order of the rows and each segment's (label, count, start).
//
// Load balance: a segment is cut into CHUNKS OF C = 1024 ROWS (kChunk) taken through the order; one workgroup of 256 threads
// per chunk, whichever segment it belongs to -- the ground or a 60 000-point wall is 59 workgroups, not one wave.
//
// Determinism: every sum is a function of the arguments alone.
//   1. thread t of a chunk's workgroup adds the chunk's rows t, t + 256, t + 512, t + 768 (positions in the stable order,
//      which is the row order inside a segment), in that order;
//   2. the 64 partials of a wave go through one fixed butterfly (wave_sum), the four waves are added in wave order;
//   3. a final kernel adds the chunks of a segment in ascending chunk order.
// Counts are integers.  No floating-point atomic anywhere; every workgroup stores its whole partial, so nothing in the
// workspace is read before it is written.  Compiled with -ffp-contract=off (build.py: CFLAGS): x + (double)f is one rounding.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"
#include "kernels.hpp"
#include "host.hpp"
#include "rowerr.hpp"

using icpflow::kWave;
using icpflow::pointer_error;
using icpflow::report_error;
using icpflow::report_errorf;
using icpflow::workspace_error;

namespace {

constexpr int kChunk = 1024;                          // C: rows of a chunk
static_assert(kChunk == icpflow::kSegmentChunk, "the chunk the plan below is shared for (kernels.hpp)");
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kPerThread = kChunk / kThreads;
constexpr int kCols = ICPFLOW_SEG_COLS;
constexpr int kValues = 12;                           // kept, sum e, 4 predicates, sum xyz, sum (xyz + flow): columns 2 .. 13
constexpr int kLmax = 4096;
constexpr int kOrderCols = icpflow::kLabelOrderCols;  // label, count, start, ...

// chunks at most: sum over the segments of ceil(count / C) <= n / C + (number of segments)
int max_chunks(int n, int Lmax) { return n / kChunk + (n < Lmax ? n : Lmax) + 1; }

struct SegCarve {
    int64_t *order;        // [n] rows sorted by label, stable
    double *ctable;        // [Lmax][kOrderCols] label, count, start
    int *chunkStart;       // [Lmax + 1] first chunk of every segment, then the number of chunks
    double *partial;       // [max_chunks][kValues]
    void *sort;            // table.hip's own workspace
    size_t sortBytes, total;
};

bool seg_carve(int n, int Lmax, void *ws, SegCarve *c)
{
    size_t sortBytes = 0;
    if (icpflow::cluster_table_workspace_bytes(n, Lmax, &sortBytes) != hipSuccess) return false;
    icpflow::Carver mem(ws);
    c->order = mem.take<int64_t>((size_t)n * sizeof(int64_t));
    c->ctable = mem.take<double>((size_t)Lmax * kOrderCols * sizeof(double));
    c->chunkStart = mem.take<int>(((size_t)Lmax + 1) * sizeof(int));
    c->partial = mem.take<double>((size_t)max_chunks(n, Lmax) * kValues * sizeof(double));
    c->sort = mem.take<void>(sortBytes);
    c->sortBytes = sortBytes;
    c->total = mem.total();
    return true;
}

// One workgroup: the exclusive scan of the segments' chunk counts, in rounds of 1024 segments.
__global__ __launch_bounds__(1024) void seg_plan_kernel(const double *__restrict__ ctable, const int32_t *__restrict__ num,
                                                        int *__restrict__ chunkStart)
{
    __shared__ int part[1024 / kWave];
    __shared__ int carrySh;
    const int L = *num, tid = threadIdx.x;
    if (L <= 0) return;                                // (nothing, or more labels than the table holds)
    if (tid == 0) carrySh = 0;
    __syncthreads();
    for (int r0 = 0; r0 < L; r0 += 1024) {
        const int r = r0 + tid;
        const int v = r < L ? ((int)ctable[(size_t)r * kOrderCols + 1] + kChunk - 1) / kChunk : 0;
        int incl = v;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const int up = __shfl_up(incl, o, kWave);
            if ((tid & (kWave - 1)) >= o) incl += up;
        }
        if ((tid & (kWave - 1)) == kWave - 1) part[tid >> 6] = incl;
        __syncthreads();
        int before = carrySh;
        for (int w = 0; w < (tid >> 6); ++w) before += part[w];
        if (r < L) chunkStart[r] = before + incl - v;
        __syncthreads();
        if (tid == 1023) carrySh = before + incl;
        __syncthreads();
    }
    if (tid == 0) chunkStart[L] = carrySh;
}

// One workgroup per chunk.
__global__ __launch_bounds__(kThreads) void seg_chunk_kernel(const double *__restrict__ pts, const double *__restrict__ gt,
                                                             const float *__restrict__ pred, double zmin,
                                                             const int64_t *__restrict__ order, const double *__restrict__ ctable,
                                                             const int32_t *__restrict__ num, const int *__restrict__ chunkStart,
                                                             double *__restrict__ partial)
{
    __shared__ double sh[kWaves][kValues];
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
    const bool flows = gt != nullptr;
    double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // sum e, sum xyz, sum (xyz + flow)
    int c[5] = {0, 0, 0, 0, 0};                             // kept, the four predicates
#pragma unroll
    for (int u = 0; u < kPerThread; ++u) {
        const int j = u * kThreads + (int)threadIdx.x;
        if (j >= rows) break;
        const size_t i = (size_t)order[(size_t)start + first + j];
        const double x = pts[3 * i + 0], y = pts[3 * i + 1], z = pts[3 * i + 2];
        if (!(z > zmin)) continue;                          // utils_debug.py:38 (a NaN fails the comparison there and here)
        c[0] += 1;
        v[1] += x, v[2] += y, v[3] += z;
        if (flows) {
            const float fx = pred[3 * i + 0], fy = pred[3 * i + 1], fz = pred[3 * i + 2];
            const icpflow::RowError q = icpflow::row_error(gt[3 * i + 0], gt[3 * i + 1], gt[3 * i + 2], fx, fy, fz);
            v[0] += q.e;
            c[1] += q.p0, c[2] += q.p1, c[3] += q.p2, c[4] += q.p3;
            v[4] += x + (double)fx, v[5] += y + (double)fy, v[6] += z + (double)fz;     // utils_flow.py:123
        }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) v[k] = icpflow::wave_sum(v[k]);
#pragma unroll
    for (int k = 0; k < 5; ++k) c[k] = icpflow::wave_sum(c[k]);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & (kWave - 1)) == 0) {
        double *w = sh[wave];
        w[0] = (double)c[0], w[1] = v[0];
        w[2] = (double)c[1], w[3] = (double)c[2], w[4] = (double)c[3], w[5] = (double)c[4];
        for (int k = 0; k < 6; ++k) w[6 + k] = v[1 + k];
    }
    __syncthreads();
    if (threadIdx.x < kValues) {                            // the waves in wave order
        double t = sh[0][threadIdx.x];
        for (int w = 1; w < kWaves; ++w) t += sh[w][threadIdx.x];
        partial[(size_t)b * kValues + threadIdx.x] = t;
    }
}

// One thread per (segment, column): the chunks of the segment in ascending order.
__global__ __launch_bounds__(kThreads) void seg_final_kernel(const double *__restrict__ ctable, const int32_t *__restrict__ num,
                                                             const int *__restrict__ chunkStart, const double *__restrict__ partial,
                                                             int flows, double *__restrict__ table)
{
    const int L = *num;
    const int idx = blockIdx.x * kThreads + threadIdx.x, c = idx / kCols, col = idx % kCols;
    if (c >= L) return;                                     // (also when L < 0: nothing of the table is written)
    double out = 0.0;
    if (col < 2) {
        out = ctable[(size_t)c * kOrderCols + col];
    } else if (col < 2 + kValues) {
        const int k = col - 2;
        const bool flow_col = (k >= 1 && k <= 5) || k >= 9;
        if (flows || !flow_col) {
            const int c0 = chunkStart[c], c1 = chunkStart[c + 1];
            out = partial[(size_t)c0 * kValues + k];
            for (int q = c0 + 1; q < c1; ++q) out += partial[(size_t)q * kValues + k];
        }
    }
    table[(size_t)c * kCols + col] = out;
}

}  // namespace

// the chunk plan, for segresid.hip as well (kernels.hpp)
namespace icpflow {

int segment_max_chunks(int n, int Lmax) { return max_chunks(n, Lmax); }

hipError_t launch_segment_plan(const double *ctable, const int32_t *num, int *chunkStart, hipStream_t s)
{
    seg_plan_kernel<<<1, 1024, 0, s>>>(ctable, num, chunkStart);
    return hipGetLastError();
}

}  // namespace icpflow

extern "C" {

size_t icpflow_seq_segment_table_workspace_bytes(int n, int Lmax)
{
    if (n < 0 || Lmax < 1 || Lmax > kLmax) return 0;
    SegCarve c{};
    return seg_carve(n, Lmax, nullptr, &c) ? c.total : 0;
}

int icpflow_seq_segment_table(const double *d_points, const float *d_labels, int n, const double *d_gt_flow, const float *d_pred_flow,
                              double z_min, double *d_table, int Lmax, int32_t *d_num, void *d_ws, size_t ws_bytes,
                              icpflow_stream_t stream)
{
    const char *fn = "icpflow_seq_segment_table";
    if (n < 0) return report_error(ICPFLOW_E_ARG, "icpflow_seq_segment_table: n < 0");
    if (Lmax < 1 || Lmax > kLmax) return report_errorf(ICPFLOW_E_LIMIT, "icpflow_seq_segment_table: 1 <= Lmax <= %d (got %d)", kLmax, Lmax);
    if ((d_gt_flow == nullptr) != (d_pred_flow == nullptr))
        return report_error(ICPFLOW_E_ARG, "icpflow_seq_segment_table: d_gt_flow and d_pred_flow are given together or both NULL");
    if (z_min != z_min) return report_error(ICPFLOW_E_ARG, "icpflow_seq_segment_table: z_min is NaN (-inf for no crop)");
    if (!d_table || !d_num || (n > 0 && (!d_points || !d_labels))) return pointer_error(fn);
    SegCarve c{};
    if (!seg_carve(n, Lmax, d_ws, &c)) return report_error(ICPFLOW_E_ARG, "icpflow_seq_segment_table: no workspace layout for these sizes");
    if (!d_ws || ws_bytes < c.total) return workspace_error(fn, "icpflow_seq_segment_table_workspace_bytes", d_ws, ws_bytes, c.total);
    if (((uintptr_t)d_ws & 7) != 0) return report_error(ICPFLOW_E_ARG, "icpflow_seq_segment_table: d_ws must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        ICPFLOW_TRY(hipMemsetAsync(d_num, 0, sizeof(int32_t), st));
        return ICPFLOW_OK;
    }
    bool tooSmall = false;
    ICPFLOW_TRY(icpflow::launch_label_order(d_labels, n, c.order, c.ctable, Lmax, d_num, c.sort, c.sortBytes, &tooSmall, st));
    if (tooSmall) return workspace_error(fn, "icpflow_seq_segment_table_workspace_bytes", d_ws, ws_bytes, c.total);   // (cannot happen: same carve)
    seg_plan_kernel<<<1, 1024, 0, st>>>(c.ctable, d_num, c.chunkStart);
    ICPFLOW_TRY(hipGetLastError());
    seg_chunk_kernel<<<max_chunks(n, Lmax), kThreads, 0, st>>>(d_points, d_gt_flow, d_pred_flow, z_min, c.order, c.ctable, d_num,
                                                              c.chunkStart, c.partial);
    ICPFLOW_TRY(hipGetLastError());
    seg_final_kernel<<<(Lmax * kCols + kThreads - 1) / kThreads, kThreads, 0, st>>>(c.ctable, d_num, c.chunkStart, c.partial,
                                                                                   d_gt_flow ? 1 : 0, d_table);
    ICPFLOW_TRY(hipGetLastError());
    return ICPFLOW_OK;
}

}  // extern "C"
