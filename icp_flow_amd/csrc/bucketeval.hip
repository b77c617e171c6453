// bucketeval.hip -- the cells behind Argoverse 2's bucket-normalised EPE on the GPU (include/icpflow_hip.h, "8(f) sequence
// evaluation", icpflow_seq_bucket_table): one pass over the rows, one table of G classes x S speed buckets x (rows, sum of e,
// sum of |gt|).  classeval.hip keeps a table per WAVE in LDS, which caps it at 1024 words; the protocol's 33 x 51 x 3 = 5049
// words need a table per WORKGROUP, in dynamic LDS (96 KB at the limits of 64 x 64).  The row test, a row's e and |gt|, its
// class row, its bucket and the grid are rowerr.hpp's, shared with classeval.hip; the edges and the grouping into the
// challenge's classes are Python data (icp_flow_amd/utils_eval.py).
//
// Determinism, item by item the contract of seqeval.hip's and classeval.hip's header comments.  Counts are integers: exact
// whatever the order.  The two floating-point sums of a cell are added in an order that is a function of the arguments alone:
//   1. the grid's waves walk the 64-row tiles in rounds: in round r, wave w (its number in the grid, W = waves in the grid;
//      the grid follows from m, never from the device) takes tile r W + w.  The number of rounds is the same for every wave
//      of the grid: a wave without a tile has no records and still reaches every barrier;
//   2. inside a tile the cells are taken in the order of their first row; the 64 values of a cell go through one fixed
//      butterfly (wave_sum), and record k of the tile -- (cell, rows, sum of e, sum of |gt|), at most 64 of them -- is kept by
//      lane k.  The wave does not touch the shared table while it does this;
//   3. the records of a round are applied to the workgroup's table in (wave, record) order: the waves take turns, a
//      workgroup barrier between two turns, and inside a turn the records of one wave name distinct cells, so lane k adds
//      record k.  A cell therefore sees its additions in the order (round, wave);
//   4. the workgroup's table and its two info words go to the workspace (every workgroup stores all of its words: nothing
//      there needs to be zero beforehand);
//   5. a second kernel, a thread per word, adds the partials of its word in workgroup order.  (A word's sum does not depend
//      on how the words are spread over workgroups, so this kernel runs as many of them as the table needs instead of one.)
// No floating-point atomic anywhere, and no integer one either.  A tile whose 64 rows fall into 64 cells runs 64 butterflies:
// slow, rare, and right.  The file is compiled with -ffp-contract=off (build.py: CFLAGS).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdint>

#include "common.hpp"
#include "host.hpp"
#include "kernels.hpp"
#include "rowerr.hpp"

using icpflow::align256;
using icpflow::Crop;
using icpflow::kWave;
using icpflow::pointer_error;
using icpflow::report_error;
using icpflow::workspace_error;

static_assert(ICPFLOW_SEQ_CROP_NONE == 0 && ICPFLOW_SEQ_CROP_XY == 1 && ICPFLOW_SEQ_CROP_XYZ == 2, "rowerr.hpp: crop_keep's modes");

namespace {

constexpr int kThreads = icpflow::kTableThreads;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxClasses = ICPFLOW_BUCKET_MAX_ROWS, kMaxBuckets = ICPFLOW_BUCKET_MAX_BUCKETS;
constexpr int kPitch = 3;                               // words of a cell: rows, bits of the sum of e, bits of the sum of |gt|
constexpr int kInfo = 2;                                // kept rows of frame 0, rows whose time index is outside [0, F)

// what travels with the launch: the rows' classes and the interior edges
struct Buckets {
    int G, S;
    double class_lo;
    double edge[kMaxBuckets - 1];
};

__device__ __forceinline__ unsigned long long add_bits(unsigned long long bits, double v)
{
    return (unsigned long long)__double_as_longlong(__longlong_as_double((long long)bits) + v);
}

__global__ __launch_bounds__(kThreads) void bucket_table_kernel(const double *__restrict__ pts, const int32_t *__restrict__ tim,
                                                                const double *__restrict__ cls, const double *__restrict__ gt,
                                                                const float *__restrict__ pred, int m, int F, Crop crop, Buckets bk,
                                                                unsigned long long *__restrict__ partial)
{
    extern __shared__ unsigned long long table[];                 // the workgroup's cells: [class][speed bucket][kPitch]
    __shared__ unsigned long long info[kWaves][kInfo];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int words = bk.G * bk.S * kPitch;
    for (int k = threadIdx.x; k < words; k += kThreads) table[k] = 0;   // (the bits of +0.0 are zero too)
    __syncthreads();

    const size_t tiles = ((size_t)m + kWave - 1) / kWave;
    const size_t W = (size_t)gridDim.x * kWaves;
    const size_t rounds = (tiles + W - 1) / W;                    // uniform over the grid
    unsigned long long kept0 = 0, outside = 0;                    // wave-uniform, kept by every lane
    for (size_t round = 0; round < rounds; ++round) {
        const size_t tile = round * W + (size_t)blockIdx.x * kWaves + wave;
        int records = 0;                                          // wave-uniform
        int my_cell = 0;                                          // lane k: record k of the tile
        unsigned long long my_n = 0;
        double my_e = 0.0, my_s = 0.0;
        if (tile < tiles) {                                       // (wave-uniform)
            const size_t i = tile * kWave + lane;
            const bool row = i < (size_t)m;
            int t = -1, c = 0;
            bool keep = false;
            double e = 0.0, speed = 0.0;
            if (row) {
                t = tim[i];
                keep = icpflow::crop_keep(crop, pts[3 * i + 0], pts[3 * i + 1], pts[3 * i + 2]);
                const double gx = gt[3 * i + 0], gy = gt[3 * i + 1], gz = gt[3 * i + 2];
                e = icpflow::row_error(gx, gy, gz, pred[3 * i + 0], pred[3 * i + 1], pred[3 * i + 2]).e;
                speed = icpflow::row_speed(gx, gy, gz);
                c = icpflow::class_row(cls[i], bk.class_lo, bk.G) * bk.S + icpflow::edge_bucket(speed, bk.edge, bk.S - 1);
            }
            outside += __popcll(__ballot(row && (t < 0 || t >= F)));
            kept0 += __popcll(__ballot(row && keep && t == 0));
            const bool counted = row && keep && t >= 1 && t < F;
            unsigned long long todo = __ballot(counted);
            while (todo) {                                         // the cells of the tile, in the order of their first row
                const int leader = __ffsll((long long)todo) - 1;
                const int j = __shfl(c, leader, kWave);
                const bool mine = counted && c == j;
                const unsigned long long rows = __ballot(mine);
                todo &= ~rows;
                const double sum_e = icpflow::wave_sum(mine ? e : 0.0), sum_s = icpflow::wave_sum(mine ? speed : 0.0);
                if (lane == records) my_cell = j, my_n = __popcll(rows), my_e = sum_e, my_s = sum_s;
                ++records;
            }
        }
        for (int w = 0; w < kWaves; ++w) {                        // the round's records in (wave, record) order
            if (wave == w && lane < records) {
                unsigned long long *v = table + (size_t)my_cell * kPitch;
                v[0] += my_n;
                v[1] = add_bits(v[1], my_e);
                v[2] = add_bits(v[2], my_s);
            }
            __syncthreads();
        }
    }
    if (lane == 0) info[wave][0] = kept0, info[wave][1] = outside;
    __syncthreads();
    unsigned long long *mine = partial + (size_t)blockIdx.x * ((size_t)words + kInfo);
    for (int k = threadIdx.x; k < words + kInfo; k += kThreads) {
        unsigned long long v;
        if (k < words) {
            v = table[k];
        } else {
            v = 0;
            for (int w = 0; w < kWaves; ++w) v += info[w][k - words];
        }
        mine[k] = v;
    }
}

// A thread per word: the partials of the word in workgroup order.
__global__ __launch_bounds__(kThreads) void bucket_table_final_kernel(const unsigned long long *__restrict__ partial, int grid, int words,
                                                                      unsigned long long *__restrict__ table,
                                                                      unsigned long long *__restrict__ d_info)
{
    const size_t pitch = (size_t)words + kInfo;
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= words + kInfo) return;
    const bool is_sum = k < words && (k % kPitch) != 0;
    unsigned long long acc = 0;
    double accd = 0.0;
    for (int g = 0; g < grid; ++g) {
        const unsigned long long v = partial[(size_t)g * pitch + k];
        if (is_sum) accd += __longlong_as_double((long long)v);
        else acc += v;
    }
    const unsigned long long out = is_sum ? (unsigned long long)__double_as_longlong(accd) : acc;
    if (k < words) table[k] = out;
    else d_info[k - words] = out;
}

bool within_limits(int G, int S) { return G <= kMaxClasses && S <= kMaxBuckets; }

}  // namespace

extern "C" {

size_t icpflow_seq_bucket_table_workspace_bytes(int m, int G, int S)
{
    if (m < 0 || G < 2 || S < 1 || !within_limits(G, S)) return 0;
    return align256((size_t)icpflow::table_grid(m) * ((size_t)G * S * kPitch + kInfo) * sizeof(unsigned long long));
}

int icpflow_seq_bucket_table(const double *d_points, const int32_t *d_time_indice, const double *d_classes, const double *d_gt_flow,
                             const float *d_pred_flow, int m, int F, int crop, double range_x, double range_y, double z_min,
                             double class_lo, int G, const double *h_speed_edges, int S, int64_t *d_table, int64_t *d_info, void *d_ws,
                             size_t ws_bytes, icpflow_stream_t stream)
{
    const char *fn = "icpflow_seq_bucket_table";
    if (m < 0) return report_error(ICPFLOW_E_ARG, "icpflow_seq_bucket_table: m < 0");
    if (F < 1) return report_error(ICPFLOW_E_ARG, "icpflow_seq_bucket_table: F must be >= 1");
    if (crop != ICPFLOW_SEQ_CROP_NONE && crop != ICPFLOW_SEQ_CROP_XY && crop != ICPFLOW_SEQ_CROP_XYZ)
        return report_error(ICPFLOW_E_ARG, "icpflow_seq_bucket_table: crop must be ICPFLOW_SEQ_CROP_NONE, _XY or _XYZ");
    if (G < 2) return report_error(ICPFLOW_E_ARG, "icpflow_seq_bucket_table: G must be >= 2 (one class row and the row of everything else)");
    if (S < 1) return report_error(ICPFLOW_E_ARG, "icpflow_seq_bucket_table: S must be >= 1");
    if (!within_limits(G, S))
        return icpflow::report_errorf(ICPFLOW_E_LIMIT,
                                      "icpflow_seq_bucket_table: G = %d, S = %d: at most %d rows and %d buckets (a workgroup's table is "
                                      "kept in LDS)",
                                      G, S, kMaxClasses, kMaxBuckets);
    if (!std::isfinite(class_lo) || class_lo != std::floor(class_lo))
        return report_error(ICPFLOW_E_ARG, "icpflow_seq_bucket_table: class_lo must be a finite integer value");
    if (!d_table || !d_info || (S > 1 && !h_speed_edges) ||
        (m > 0 && (!d_points || !d_time_indice || !d_classes || !d_gt_flow || !d_pred_flow)))
        return pointer_error(fn);
    if (!icpflow::edges_ok(h_speed_edges, S - 1))
        return report_error(ICPFLOW_E_ARG, "icpflow_seq_bucket_table: the edges must be finite and strictly ascending");
    const size_t need = icpflow_seq_bucket_table_workspace_bytes(m, G, S);
    if (!d_ws || ws_bytes < need) return workspace_error(fn, "icpflow_seq_bucket_table_workspace_bytes", d_ws, ws_bytes, need);
    if (((uintptr_t)d_ws & 7) != 0) return report_error(ICPFLOW_E_ARG, "icpflow_seq_bucket_table: d_ws must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    Buckets bk;
    bk.G = G, bk.S = S, bk.class_lo = class_lo;
    for (int k = 0; k < kMaxBuckets - 1; ++k) bk.edge[k] = k < S - 1 ? h_speed_edges[k] : 0.0;
    const int grid = icpflow::table_grid(m);
    const int words = G * S * kPitch;
    const size_t lds = (size_t)words * sizeof(unsigned long long);
    if (lds > 48 * 1024) {   // dynamic LDS above the default needs the attribute once per kernel and device
        static std::atomic<unsigned long long> attr{0ull};
        icpflow::ensure_dynamic_lds(reinterpret_cast<const void *>(&bucket_table_kernel),
                                    kMaxClasses * kMaxBuckets * kPitch * (int)sizeof(unsigned long long), &attr);
    }
    unsigned long long *partial = (unsigned long long *)d_ws;
    const Crop c = {crop, range_x, range_y, z_min};
    bucket_table_kernel<<<grid, kThreads, lds, st>>>(d_points, d_time_indice, d_classes, d_gt_flow, d_pred_flow, m, F, c, bk, partial);
    ICPFLOW_TRY(hipGetLastError());
    bucket_table_final_kernel<<<(words + kInfo + kThreads - 1) / kThreads, kThreads, 0, st>>>(partial, grid, words, (unsigned long long *)d_table,
                                                                                               (unsigned long long *)d_info);
    ICPFLOW_TRY(hipGetLastError());
    return ICPFLOW_OK;
}

}  // extern "C"
