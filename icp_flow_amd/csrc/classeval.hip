// classeval.hip -- the per-class numbers of a sample on the GPU (include/icpflow_hip.h, "8(f) sequence evaluation",
// icpflow_seq_class_table): one pass over the rows, one table of G classes x S speed buckets x (E error splits, sum of e, sum
// of |gt|).  The tables that name the rows for Argoverse 2 (dataset_argo.py:145-217) are Python data (icp_flow_amd/utils_eval.py).
//
// Determinism, item by item the contract of seqeval.hip's header comment.  Counts are integers (ballots and popcounts): exact
// whatever the order.  The two floating-point sums of a cell (class, speed bucket) are added in an order that is a function
// of the arguments alone:
//   1. a wave takes the 64-row tiles  w, w + W, w + 2 W, ...  (w = its number in the grid, W = waves in the grid; the grid
//      follows from m, never from the device), and inside a tile the cells in the order of their first row;
//   2. the 64 values of a tile go through one fixed butterfly (wave_sum), and lane 0 adds the total to the wave's own cell in
//      LDS -- tile after tile, in the order of 1.;
//   3. a workgroup's partial is its waves' cells added in wave order, stored to the workspace (every workgroup stores all of
//      its words: nothing there needs to be zero beforehand);
//   4. a second, single-workgroup kernel adds the partials of a word in workgroup order.
// No floating-point atomic anywhere.  A tile whose 64 rows fall into 64 cells runs 64 butterflies: slow, rare, and right.
// The file is compiled with -ffp-contract=off (build.py: CFLAGS): a row's e and |gt| are the separately rounded operations of
// rowerr.hpp and of seqeval.hip's row_norm.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.hpp"
#include "host.hpp"
#include "rowerr.hpp"

using icpflow::align256;
using icpflow::Crop;
using icpflow::kWave;
using icpflow::pointer_error;
using icpflow::report_error;
using icpflow::workspace_error;

static_assert(ICPFLOW_SEQ_CROP_NONE == 0 && ICPFLOW_SEQ_CROP_XY == 1 && ICPFLOW_SEQ_CROP_XYZ == 2, "rowerr.hpp: crop_keep's modes");

namespace {

constexpr int kThreads = icpflow::kTableThreads;        // the grid: rowerr.hpp's table_grid (icpflow_seq_metrics' rule)
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxWords = ICPFLOW_CLASS_MAX_WORDS;      // 64-bit words of a wave's table in LDS: 4 waves x 1024 x 8 B = 32 KB
constexpr int kMaxClasses = ICPFLOW_CLASS_MAX_ROWS, kMaxBuckets = ICPFLOW_CLASS_MAX_BUCKETS;
constexpr int kInfo = 2;                                // kept rows of frame 0, rows whose time index is outside [0, F)

// what travels with the launch: the rows' classes and the two lists of interior edges
struct Split {
    int G, S, E;
    double class_lo;
    double speed[kMaxBuckets - 1], error[kMaxBuckets - 1];
};

__global__ __launch_bounds__(kThreads) void class_table_kernel(const double *__restrict__ pts, const int32_t *__restrict__ tim,
                                                               const double *__restrict__ cls, const double *__restrict__ gt,
                                                               const float *__restrict__ pred, int m, int F, Crop crop, Split sp,
                                                               unsigned long long *__restrict__ partial)
{
    // a wave's own cells: [wave][class][speed bucket][E counts, sum of e, sum of |gt|]; the last two hold doubles
    __shared__ unsigned long long cell[kWaves][kMaxWords];
    __shared__ unsigned long long info[kWaves][kInfo];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int pitch = sp.E + 2;
    const int words = sp.G * sp.S * pitch;
    for (int k = lane; k < words; k += kWave) cell[wave][k] = 0;   // (the bits of +0.0 are zero too)
    if (lane < kInfo) info[wave][lane] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    const size_t tiles = ((size_t)m + kWave - 1) / kWave;
    const size_t W = (size_t)gridDim.x * kWaves;
    unsigned long long kept0 = 0, outside = 0;                    // wave-uniform, kept by every lane
    for (size_t tile = (size_t)blockIdx.x * kWaves + wave; tile < tiles; tile += W) {
        const size_t i = tile * kWave + lane;
        const bool row = i < (size_t)m;
        int t = -1, c = 0, split = 0;
        bool keep = false;
        double e = 0.0, speed = 0.0;
        if (row) {
            t = tim[i];
            keep = icpflow::crop_keep(crop, pts[3 * i + 0], pts[3 * i + 1], pts[3 * i + 2]);
            const double gx = gt[3 * i + 0], gy = gt[3 * i + 1], gz = gt[3 * i + 2];
            e = icpflow::row_error(gx, gy, gz, pred[3 * i + 0], pred[3 * i + 1], pred[3 * i + 2]).e;
            speed = icpflow::row_speed(gx, gy, gz);
            const int g = icpflow::class_row(cls[i], sp.class_lo, sp.G);
            const int s = icpflow::edge_bucket(speed, sp.speed, sp.S - 1);
            split = icpflow::edge_bucket(e, sp.error, sp.E - 1);
            c = g * sp.S + s;
        }
        outside += __popcll(__ballot(row && (t < 0 || t >= F)));
        kept0 += __popcll(__ballot(row && keep && t == 0));
        const bool counted = row && keep && t >= 1 && t < F;
        unsigned long long todo = __ballot(counted);
        while (todo) {                                             // the cells of the tile, in the order of their first row
            const int leader = __ffsll((long long)todo) - 1;
            const int j = __shfl(c, leader, kWave);
            const bool mine = counted && c == j;
            todo &= ~__ballot(mine);
            const double sum_e = icpflow::wave_sum(mine ? e : 0.0), sum_s = icpflow::wave_sum(mine ? speed : 0.0);
            unsigned long long *v = cell[wave] + (size_t)j * pitch;
            for (int k = 0; k < sp.E; ++k) {                       // (wave-uniform)
                const unsigned long long n = __popcll(__ballot(mine && split == k));
                if (lane == 0) v[k] += n;
            }
            if (lane == 0) {
                v[sp.E] = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)v[sp.E]) + sum_e);
                v[sp.E + 1] = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)v[sp.E + 1]) + sum_s);
            }
        }
    }
    if (lane == 0) info[wave][0] = kept0, info[wave][1] = outside;
    __syncthreads();
    // the workgroup's partial: its waves in wave order
    unsigned long long *mine = partial + (size_t)blockIdx.x * ((size_t)words + kInfo);
    for (int k = threadIdx.x; k < words + kInfo; k += kThreads) {
        const bool is_info = k >= words;
        const bool is_sum = !is_info && (k % pitch) >= sp.E;
        unsigned long long acc = 0;
        double accd = 0.0;
        for (int w = 0; w < kWaves; ++w) {
            const unsigned long long v = is_info ? info[w][k - words] : cell[w][k];
            if (is_sum) accd += __longlong_as_double((long long)v);
            else acc += v;
        }
        mine[k] = is_sum ? (unsigned long long)__double_as_longlong(accd) : acc;
    }
}

// One workgroup: the partials of a word in workgroup order.
__global__ __launch_bounds__(kThreads) void class_table_final_kernel(const unsigned long long *__restrict__ partial, int grid, int words,
                                                                     int E, unsigned long long *__restrict__ table,
                                                                     unsigned long long *__restrict__ d_info)
{
    const size_t pitch = (size_t)words + kInfo;
    for (int k = threadIdx.x; k < words + kInfo; k += kThreads) {
        const bool is_sum = k < words && (k % (E + 2)) >= E;
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
}

bool within_limits(int G, int S, int E)
{
    return G <= kMaxClasses && S <= kMaxBuckets && E <= kMaxBuckets && (long long)G * S * (E + 2) <= kMaxWords;
}

}  // namespace

extern "C" {

size_t icpflow_seq_class_table_workspace_bytes(int m, int G, int S, int E)
{
    if (m < 0 || G < 2 || S < 1 || E < 1 || !within_limits(G, S, E)) return 0;
    return align256((size_t)icpflow::table_grid(m) * ((size_t)G * S * (E + 2) + kInfo) * sizeof(unsigned long long));
}

int icpflow_seq_class_table(const double *d_points, const int32_t *d_time_indice, const double *d_classes, const double *d_gt_flow,
                            const float *d_pred_flow, int m, int F, int crop, double range_x, double range_y, double z_min,
                            double class_lo, int G, const double *h_speed_edges, int S, const double *h_error_edges, int E,
                            int64_t *d_table, int64_t *d_info, void *d_ws, size_t ws_bytes, icpflow_stream_t stream)
{
    const char *fn = "icpflow_seq_class_table";
    if (m < 0) return report_error(ICPFLOW_E_ARG, "icpflow_seq_class_table: m < 0");
    if (F < 1) return report_error(ICPFLOW_E_ARG, "icpflow_seq_class_table: F must be >= 1");
    if (crop != ICPFLOW_SEQ_CROP_NONE && crop != ICPFLOW_SEQ_CROP_XY && crop != ICPFLOW_SEQ_CROP_XYZ)
        return report_error(ICPFLOW_E_ARG, "icpflow_seq_class_table: crop must be ICPFLOW_SEQ_CROP_NONE, _XY or _XYZ");
    if (G < 2) return report_error(ICPFLOW_E_ARG, "icpflow_seq_class_table: G must be >= 2 (one class row and the row of everything else)");
    if (S < 1 || E < 1) return report_error(ICPFLOW_E_ARG, "icpflow_seq_class_table: S and E must be >= 1");
    if (!within_limits(G, S, E))
        return icpflow::report_errorf(ICPFLOW_E_LIMIT,
                                      "icpflow_seq_class_table: G = %d, S = %d, E = %d: at most %d rows, %d buckets, %d splits and "
                                      "G * S * (E + 2) <= %d words (a wave's table is kept in LDS)",
                                      G, S, E, kMaxClasses, kMaxBuckets, kMaxBuckets, kMaxWords);
    if (!std::isfinite(class_lo) || class_lo != std::floor(class_lo))
        return report_error(ICPFLOW_E_ARG, "icpflow_seq_class_table: class_lo must be a finite integer value");
    if (!d_table || !d_info || (S > 1 && !h_speed_edges) || (E > 1 && !h_error_edges) ||
        (m > 0 && (!d_points || !d_time_indice || !d_classes || !d_gt_flow || !d_pred_flow)))
        return pointer_error(fn);
    if (!icpflow::edges_ok(h_speed_edges, S - 1) || !icpflow::edges_ok(h_error_edges, E - 1))
        return report_error(ICPFLOW_E_ARG, "icpflow_seq_class_table: the edges must be finite and strictly ascending");
    const size_t need = icpflow_seq_class_table_workspace_bytes(m, G, S, E);
    if (!d_ws || ws_bytes < need) return workspace_error(fn, "icpflow_seq_class_table_workspace_bytes", d_ws, ws_bytes, need);
    if (((uintptr_t)d_ws & 7) != 0) return report_error(ICPFLOW_E_ARG, "icpflow_seq_class_table: d_ws must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    Split sp;
    sp.G = G, sp.S = S, sp.E = E, sp.class_lo = class_lo;
    for (int k = 0; k < kMaxBuckets - 1; ++k) {
        sp.speed[k] = k < S - 1 ? h_speed_edges[k] : 0.0;
        sp.error[k] = k < E - 1 ? h_error_edges[k] : 0.0;
    }
    const int grid = icpflow::table_grid(m);
    unsigned long long *partial = (unsigned long long *)d_ws;
    const Crop c = {crop, range_x, range_y, z_min};
    class_table_kernel<<<grid, kThreads, 0, st>>>(d_points, d_time_indice, d_classes, d_gt_flow, d_pred_flow, m, F, c, sp, partial);
    ICPFLOW_TRY(hipGetLastError());
    class_table_final_kernel<<<1, kThreads, 0, st>>>(partial, grid, G * S * (E + 2), E, (unsigned long long *)d_table,
                                                     (unsigned long long *)d_info);
    ICPFLOW_TRY(hipGetLastError());
    return ICPFLOW_OK;
}

}  // extern "C"
