// seqeval.hip -- the evaluation of a whole sequence on the GPU (include/icpflow_hip.h, "8(f) sequence evaluation"):
// the ground-truth scene flow the reference builds from its poses (utils_loading.py:21-48, dataset_pca.py:66-69), the
// two-frame sample it builds from an Argoverse 2 file (dataset_argo.py:47-50, 66-71, 83-89) and the sums behind the table its
// calculate_metrics fills (utils_eval.py:24-63, 162-180, 185-368).
//
// Determinism of icpflow_seq_metrics.  Counts are integers (ballots and popcounts): exact whatever the order.  The one
// floating-point sum, the end point error of a (gap, class) cell, is added in an order that is a function of the arguments
// alone:
//   1. a wave takes the 64-row tiles  w, w + W, w + 2 W, ...  (w = its number in the grid, W = waves in the grid; the grid
//      follows from m, never from the device), and inside a tile the gaps in the order of their first row;
//   2. the 64 values of a tile go through one fixed butterfly (wave_sum), and lane 0 adds the total to the wave's own cell in
//      LDS -- tile after tile, in the order of 1.;
//   3. a workgroup's partial is its waves' cells added in wave order, stored to the workspace (every workgroup stores all of
//      its cells: nothing there needs to be zero beforehand);
//   4. a second, single-workgroup kernel adds the partials of a cell in workgroup order, then row 0 as the gap rows in gap order.
// No floating-point atomic anywhere.  The file is compiled with -ffp-contract=off (build.py: CFLAGS): the squares, the two
// additions, the square root and the division of a row's error are the separately rounded operations numpy performs.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"
#include "host.hpp"
#include "rowerr.hpp"

using icpflow::align256;
using icpflow::kWave;
using icpflow::pointer_error;
using icpflow::report_error;
using icpflow::workspace_error;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kRowsPerThread = 8;                       // rows a workgroup is sized for: kThreads * kRowsPerThread
constexpr int kMaxGrid = 256;                           // workgroups at most (a CU each)
constexpr int kClasses = 6, kValues = 6;                // overall static static_bg static_fg dynamic dynamic_fg; count, sum e, 4 predicates
constexpr int kCell = kClasses * kValues;               // 64-bit words of one gap row
constexpr int kMaxFrames = ICPFLOW_SEQ_MAX_FRAMES;
constexpr int kInfo = 2;                                // kept rows of frame 0, rows whose time index is outside [0, F)

int grid_for(int m)
{
    const long long per = (long long)kThreads * kRowsPerThread;
    const long long g = ((long long)m + per - 1) / per;
    return (int)(g < 1 ? 1 : g > kMaxGrid ? kMaxGrid : g);
}

// words a workgroup of icpflow_seq_metrics leaves in the workspace
size_t partial_words(int F) { return (size_t)(F - 1) * kCell + kInfo; }

// ---- ground-truth flow -------------------------------------------------------------------------------------------
// x' = R x + t with the rows of a row-major 4x4, every operation rounded by itself: ((R0 x + R1 y) + R2 z) + t
__device__ __forceinline__ void rigid_apply(const double *__restrict__ T, double &x, double &y, double &z)
{
    const double ox = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    const double oy = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    const double oz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
    x = ox, y = oy, z = oz;
}

__global__ __launch_bounds__(kThreads) void seq_gt_flow_kernel(const double *__restrict__ pts, const int32_t *__restrict__ tim,
                                                               const int32_t *__restrict__ inst, int m, const double *__restrict__ ego,
                                                               int F, const double *__restrict__ tsfm, int K, int output,
                                                               double *__restrict__ out, unsigned long long *__restrict__ partial)
{
    __shared__ unsigned long long bad_s[kWaves];
    unsigned long long bad = 0;
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < (size_t)m; i += stride) {
        const int t = tim[i];
        const int k = tsfm ? inst[i] : 0;
        if (t < 0 || t >= F || k < 0 || (tsfm && k >= K)) {   // not computed, counted; nothing is written for the row
            ++bad;
            continue;
        }
        const double px = pts[3 * i + 0], py = pts[3 * i + 1], pz = pts[3 * i + 2];
        double x = px, y = py, z = pz;
        if (ego) rigid_apply(ego + (size_t)t * 16, x, y, z);
        if (tsfm) rigid_apply(tsfm + ((size_t)k * F + t) * 16, x, y, z);
        if (output == ICPFLOW_SEQ_OUT_FLOW) x -= px, y -= py, z -= pz;
        out[3 * i + 0] = x, out[3 * i + 1] = y, out[3 * i + 2] = z;
    }
    bad = icpflow::wave_sum(bad);
    if ((threadIdx.x & (kWave - 1)) == 0) bad_s[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < kWaves; ++w) s += bad_s[w];
        partial[blockIdx.x] = s;
    }
}

__global__ void seq_count_final_kernel(const unsigned long long *__restrict__ partial, int G, long long *__restrict__ d_bad)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    unsigned long long s = 0;
    for (int g = 0; g < G; ++g) s += partial[g];
    *d_bad = (long long)s;
}

// ---- an Argoverse 2 sample -----------------------------------------------------------------------------------------
// dataset_argo.py:47-50, 66-71, 83-89: output row i < m2 is pc2[valid2[i]] (frame 0: no labels, no flow), row m2 + k is
// pc1[valid1[k]] (frame 1) with its flow row and the two labels.  P, Q: the types the file stores points and flow in.
struct Background {
    int n;
    int32_t id[ICPFLOW_ARGO_MAX_BACKGROUND];
};

// np.linalg.norm(flow, axis=-1) in the flow's own type: (x x + y y) + z z, every operation rounded by itself, and a
// correctly rounded square root (-fhip-fp32-correctly-rounded-divide-sqrt for float)
__device__ __forceinline__ float row_norm(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }
__device__ __forceinline__ double row_norm(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

template <typename P, typename Q>
__global__ __launch_bounds__(kThreads) void seq_argo_sample_kernel(const P *__restrict__ pc1, int n1, const P *__restrict__ pc2, int n2,
                                                                   const Q *__restrict__ flow, const double *__restrict__ cls,
                                                                   const long long *__restrict__ valid1, int m1,
                                                                   const long long *__restrict__ valid2, int m2, Background bg,
                                                                   double threshold, double *__restrict__ pts, int32_t *__restrict__ tim,
                                                                   int32_t *__restrict__ sd, int32_t *__restrict__ fb,
                                                                   double *__restrict__ out_flow, unsigned long long *__restrict__ d_bad)
{
    const size_t m = (size_t)m1 + (size_t)m2;
    const size_t stride = (size_t)gridDim.x * kThreads;
    unsigned long long bad = 0;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < m; i += stride) {
        const bool first = i < (size_t)m2;                         // frame 0
        const long long idx = first ? valid2[i] : valid1[i - (size_t)m2];
        if (idx < 0 || idx >= (long long)(first ? n2 : n1)) {      // not gathered, counted; nothing is written for the row
            ++bad;
            continue;
        }
        const P *p = (first ? pc2 : pc1) + 3 * (size_t)idx;
        pts[3 * i + 0] = (double)p[0], pts[3 * i + 1] = (double)p[1], pts[3 * i + 2] = (double)p[2];
        if (first) {
            tim[i] = 0, sd[i] = 0, fb[i] = 0;
            out_flow[3 * i + 0] = 0.0, out_flow[3 * i + 1] = 0.0, out_flow[3 * i + 2] = 0.0;
            continue;
        }
        const Q fx = flow[3 * (size_t)idx + 0], fy = flow[3 * (size_t)idx + 1], fz = flow[3 * (size_t)idx + 2];
        out_flow[3 * i + 0] = (double)fx, out_flow[3 * i + 1] = (double)fy, out_flow[3 * i + 2] = (double)fz;
        // dataset_argo.py:67: a float norm is compared with the threshold rounded to float; widening both is the same test
        const bool moving = (double)row_norm(fx, fy, fz) > threshold;
        const double c = cls[idx];
        bool object = !(c == -1.0);                                // dataset_argo.py:68-71 (a NaN class equals nothing)
        for (int k = 0; k < bg.n; ++k) object = object && !(c == (double)bg.id[k]);
        tim[i] = 1, sd[i] = moving ? 1 : 0, fb[i] = object ? 1 : 0;
    }
    // integers: the total is the same whatever order the waves arrive in
    bad = icpflow::wave_sum(bad);
    if ((threadIdx.x & (kWave - 1)) == 0 && bad) atomicAdd(d_bad, bad);
}

// ---- the table ---------------------------------------------------------------------------------------------------
using icpflow::Crop;

__global__ __launch_bounds__(kThreads) void seq_metrics_kernel(const double *__restrict__ pts, const int32_t *__restrict__ tim,
                                                               const int32_t *__restrict__ sd, const int32_t *__restrict__ fb,
                                                               const double *__restrict__ gt, const float *__restrict__ pred, int m, int F,
                                                               Crop crop, unsigned long long *__restrict__ partial)
{
    // a wave's own cells: [wave][gap - 1][class][value]; value 1 holds a double
    __shared__ unsigned long long cell[kWaves][(kMaxFrames - 1) * kCell];
    __shared__ unsigned long long info[kWaves][kInfo];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int words = (F - 1) * kCell;
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
        int t = -1;
        bool keep = false;
        icpflow::RowError q = icpflow::row_predicates(0.0, 0.0);   // (of no row: read by none of the sums below)
        int s = 2, f = 2;
        if (row) {
            t = tim[i];
            const double x = pts[3 * i + 0], y = pts[3 * i + 1], z = pts[3 * i + 2];
            // crop_data, utils_eval.py:33-38 (rowerr.hpp)
            keep = icpflow::crop_keep(crop, x, y, z);
            // compute_epe_test, utils_eval.py:163-168 (rowerr.hpp)
            q = icpflow::row_error(gt[3 * i + 0], gt[3 * i + 1], gt[3 * i + 2], pred[3 * i + 0], pred[3 * i + 1], pred[3 * i + 2]);
            s = sd[i], f = fb[i];
        }
        outside += __popcll(__ballot(row && (t < 0 || t >= F)));
        kept0 += __popcll(__ballot(row && keep && t == 0));
        const double e = q.e;
        const bool p0 = q.p0, p1 = q.p1, p2 = q.p2, p3 = q.p3;     // utils_eval.py:170-180
        const bool counted = row && keep && t >= 1 && t < F;
        unsigned long long todo = __ballot(counted);
        while (todo) {                                             // the gaps of the tile, in the order of their first row
            const int leader = __ffsll((long long)todo) - 1;
            const int j = __shfl(t, leader, kWave);
            const bool mine = counted && t == j;
            todo &= ~__ballot(mine);
            unsigned long long *c = cell[wave] + (size_t)(j - 1) * kCell;
#pragma unroll
            for (int k = 0; k < kClasses; ++k) {
                // utils_eval.py:217, 225, 233, 241, 253: a label that is neither 0 nor 1 counts in `overall` only
                const bool in = mine && (k == 0 || (k == 1 && s == 0) || (k == 2 && s == 0 && f == 0) || (k == 3 && s == 0 && f == 1) ||
                                         (k == 4 && s == 1) || (k == 5 && s == 1 && f == 1));
                const unsigned long long members = __ballot(in);
                if (members == 0) continue;                        // (wave-uniform)
                const double sum = icpflow::wave_sum(in ? e : 0.0);
                const unsigned long long n0 = __popcll(__ballot(in && p0)), n1 = __popcll(__ballot(in && p1));
                const unsigned long long n2 = __popcll(__ballot(in && p2)), n3 = __popcll(__ballot(in && p3));
                if (lane == 0) {
                    unsigned long long *v = c + k * kValues;
                    v[0] += __popcll(members);
                    v[1] = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)v[1]) + sum);
                    v[2] += n0, v[3] += n1, v[4] += n2, v[5] += n3;
                }
            }
        }
    }
    if (lane == 0) info[wave][0] = kept0, info[wave][1] = outside;
    __syncthreads();
    // the workgroup's partial: its waves in wave order
    unsigned long long *mine = partial + (size_t)blockIdx.x * ((size_t)words + kInfo);
    for (int k = threadIdx.x; k < words + kInfo; k += kThreads) {
        const bool is_info = k >= words;
        const bool is_sum = !is_info && (k % kValues) == 1;
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

// One workgroup: the partials of a cell in workgroup order, then row 0 as the gap rows in gap order.
__global__ __launch_bounds__(kThreads) void seq_metrics_final_kernel(const unsigned long long *__restrict__ partial, int G, int F,
                                                                     unsigned long long *__restrict__ table,
                                                                     unsigned long long *__restrict__ d_info)
{
    __shared__ unsigned long long total[(kMaxFrames - 1) * kCell + kInfo];
    const int words = (F - 1) * kCell;
    const size_t pitch = (size_t)words + kInfo;
    for (int k = threadIdx.x; k < words + kInfo; k += kThreads) {
        const bool is_sum = k < words && (k % kValues) == 1;
        unsigned long long acc = 0;
        double accd = 0.0;
        for (int g = 0; g < G; ++g) {
            const unsigned long long v = partial[(size_t)g * pitch + k];
            if (is_sum) accd += __longlong_as_double((long long)v);
            else acc += v;
        }
        total[k] = is_sum ? (unsigned long long)__double_as_longlong(accd) : acc;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < words; k += kThreads) table[kCell + k] = total[k];
    if (threadIdx.x < kInfo) d_info[threadIdx.x] = total[words + threadIdx.x];
    if (threadIdx.x < kCell) {
        const bool is_sum = (threadIdx.x % kValues) == 1;
        unsigned long long acc = 0;
        double accd = 0.0;
        for (int j = 1; j < F; ++j) {
            const unsigned long long v = total[(j - 1) * kCell + threadIdx.x];
            if (is_sum) accd += __longlong_as_double((long long)v);
            else acc += v;
        }
        table[threadIdx.x] = is_sum ? (unsigned long long)__double_as_longlong(accd) : acc;
    }
}

}  // namespace

extern "C" {

size_t icpflow_seq_gt_flow_workspace_bytes(int m)
{
    if (m < 0) return 0;
    return align256((size_t)grid_for(m) * sizeof(unsigned long long));
}

int icpflow_seq_gt_flow(const double *d_points, const int32_t *d_time_indice, const int32_t *d_inst_labels, int m, const double *d_ego,
                        int F, const double *d_inst_tsfm, int K, int output, double *d_out, int64_t *d_bad_rows, void *d_ws,
                        size_t ws_bytes, icpflow_stream_t stream)
{
    const char *fn = "icpflow_seq_gt_flow";
    if (m < 0) return report_error(ICPFLOW_E_ARG, "icpflow_seq_gt_flow: m < 0");
    if (F < 1 || K < 0) return report_error(ICPFLOW_E_ARG, "icpflow_seq_gt_flow: F must be >= 1 and K >= 0");
    if (output != ICPFLOW_SEQ_OUT_FLOW && output != ICPFLOW_SEQ_OUT_POINTS)
        return report_error(ICPFLOW_E_ARG, "icpflow_seq_gt_flow: output must be ICPFLOW_SEQ_OUT_FLOW or ICPFLOW_SEQ_OUT_POINTS");
    if (!d_bad_rows || (!d_ego && !d_inst_tsfm) || (m > 0 && (!d_points || !d_time_indice || !d_out || (d_inst_tsfm && !d_inst_labels))))
        return pointer_error(fn);
    const size_t need = icpflow_seq_gt_flow_workspace_bytes(m);
    if (!d_ws || ws_bytes < need) return workspace_error(fn, "icpflow_seq_gt_flow_workspace_bytes", d_ws, ws_bytes, need);
    if (((uintptr_t)d_ws & 7) != 0) return report_error(ICPFLOW_E_ARG, "icpflow_seq_gt_flow: d_ws must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int G = grid_for(m);
    unsigned long long *partial = (unsigned long long *)d_ws;
    seq_gt_flow_kernel<<<G, kThreads, 0, st>>>(d_points, d_time_indice, d_inst_labels, m, d_ego, F, d_inst_tsfm, K, output, d_out, partial);
    ICPFLOW_TRY(hipGetLastError());
    seq_count_final_kernel<<<1, kWave, 0, st>>>(partial, G, (long long *)d_bad_rows);
    ICPFLOW_TRY(hipGetLastError());
    return ICPFLOW_OK;
}

int icpflow_seq_argo_sample(const void *d_pc1, int n1, const void *d_pc2, int n2, int points_dtype, const void *d_flow_0_1, int flow_dtype,
                            const double *d_classes1, const int64_t *d_valid1, int m1, const int64_t *d_valid2, int m2,
                            const int32_t *h_background, int n_background, double sd_threshold, double *d_points, int32_t *d_time_indice,
                            int32_t *d_sd_labels, int32_t *d_fb_labels, double *d_scene_flow, int64_t *d_bad_rows, icpflow_stream_t stream)
{
    const char *fn = "icpflow_seq_argo_sample";
    if (n1 < 0 || n2 < 0 || m1 < 0 || m2 < 0) return report_error(ICPFLOW_E_ARG, "icpflow_seq_argo_sample: n1, n2, m1 and m2 must be >= 0");
    if (n_background < 0) return report_error(ICPFLOW_E_ARG, "icpflow_seq_argo_sample: n_background < 0");
    const bool p32 = points_dtype == ICPFLOW_DTYPE_FLOAT32, f32 = flow_dtype == ICPFLOW_DTYPE_FLOAT32;
    if ((!p32 && points_dtype != ICPFLOW_DTYPE_FLOAT64) || (!f32 && flow_dtype != ICPFLOW_DTYPE_FLOAT64))
        return report_error(ICPFLOW_E_ARG, "icpflow_seq_argo_sample: points_dtype and flow_dtype must be ICPFLOW_DTYPE_FLOAT32 or _FLOAT64");
    if (n_background > ICPFLOW_ARGO_MAX_BACKGROUND)
        return icpflow::report_errorf(ICPFLOW_E_LIMIT, "icpflow_seq_argo_sample: %d background classes, at most %d go with the launch",
                                      n_background, ICPFLOW_ARGO_MAX_BACKGROUND);
    if ((long long)m1 + m2 > 0x7fffffffLL) return report_error(ICPFLOW_E_LIMIT, "icpflow_seq_argo_sample: m1 + m2 beyond 2^31 - 1 rows");
    const int m = m1 + m2;
    if (!d_bad_rows || (n_background > 0 && !h_background) || (m1 > 0 && (!d_pc1 || !d_flow_0_1 || !d_classes1 || !d_valid1)) ||
        (m2 > 0 && (!d_pc2 || !d_valid2)) || (m > 0 && (!d_points || !d_time_indice || !d_sd_labels || !d_fb_labels || !d_scene_flow)))
        return pointer_error(fn);
    hipStream_t st = (hipStream_t)stream;
    ICPFLOW_TRY(hipMemsetAsync(d_bad_rows, 0, sizeof(int64_t), st));
    if (m == 0) return ICPFLOW_OK;
    Background bg;
    bg.n = n_background;
    for (int k = 0; k < ICPFLOW_ARGO_MAX_BACKGROUND; ++k) bg.id[k] = k < n_background ? h_background[k] : 0;
    const int G = grid_for(m);
    const long long *v1 = (const long long *)d_valid1, *v2 = (const long long *)d_valid2;
    unsigned long long *bad = (unsigned long long *)d_bad_rows;
#define ICPFLOW_ARGO_LAUNCH(P, Q)                                                                                                  \
    seq_argo_sample_kernel<P, Q><<<G, kThreads, 0, st>>>((const P *)d_pc1, n1, (const P *)d_pc2, n2, (const Q *)d_flow_0_1, d_classes1, \
                                                         v1, m1, v2, m2, bg, sd_threshold, d_points, d_time_indice, d_sd_labels,       \
                                                         d_fb_labels, d_scene_flow, bad)
    if (p32 && f32) ICPFLOW_ARGO_LAUNCH(float, float);
    else if (p32) ICPFLOW_ARGO_LAUNCH(float, double);
    else if (f32) ICPFLOW_ARGO_LAUNCH(double, float);
    else ICPFLOW_ARGO_LAUNCH(double, double);
#undef ICPFLOW_ARGO_LAUNCH
    ICPFLOW_TRY(hipGetLastError());
    return ICPFLOW_OK;
}

size_t icpflow_seq_metrics_workspace_bytes(int m, int F)
{
    if (m < 0 || F < 1 || F > kMaxFrames) return 0;
    return align256((size_t)grid_for(m) * partial_words(F) * sizeof(unsigned long long));
}

int icpflow_seq_metrics(const double *d_points, const int32_t *d_time_indice, const int32_t *d_sd_labels, const int32_t *d_fb_labels,
                        const double *d_gt_flow, const float *d_pred_flow, int m, int F, int crop, double range_x, double range_y,
                        double z_min, int64_t *d_table, int64_t *d_info, void *d_ws, size_t ws_bytes, icpflow_stream_t stream)
{
    const char *fn = "icpflow_seq_metrics";
    if (m < 0) return report_error(ICPFLOW_E_ARG, "icpflow_seq_metrics: m < 0");
    if (F < 1) return report_error(ICPFLOW_E_ARG, "icpflow_seq_metrics: F must be >= 1");
    if (F > kMaxFrames)
        return icpflow::report_errorf(ICPFLOW_E_LIMIT, "icpflow_seq_metrics: F = %d frames, the table of at most %d is kept in LDS", F, kMaxFrames);
    if (crop != ICPFLOW_SEQ_CROP_NONE && crop != ICPFLOW_SEQ_CROP_XY && crop != ICPFLOW_SEQ_CROP_XYZ)
        return report_error(ICPFLOW_E_ARG, "icpflow_seq_metrics: crop must be ICPFLOW_SEQ_CROP_NONE, _XY or _XYZ");
    if (!d_table || !d_info || (m > 0 && (!d_points || !d_time_indice || !d_sd_labels || !d_fb_labels || !d_gt_flow || !d_pred_flow)))
        return pointer_error(fn);
    const size_t need = icpflow_seq_metrics_workspace_bytes(m, F);
    if (!d_ws || ws_bytes < need) return workspace_error(fn, "icpflow_seq_metrics_workspace_bytes", d_ws, ws_bytes, need);
    if (((uintptr_t)d_ws & 7) != 0) return report_error(ICPFLOW_E_ARG, "icpflow_seq_metrics: d_ws must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int G = grid_for(m);
    unsigned long long *partial = (unsigned long long *)d_ws;
    const Crop c = {crop, range_x, range_y, z_min};
    seq_metrics_kernel<<<G, kThreads, 0, st>>>(d_points, d_time_indice, d_sd_labels, d_fb_labels, d_gt_flow, d_pred_flow, m, F, c, partial);
    ICPFLOW_TRY(hipGetLastError());
    seq_metrics_final_kernel<<<1, kThreads, 0, st>>>(partial, G, F, (unsigned long long *)d_table, (unsigned long long *)d_info);
    ICPFLOW_TRY(hipGetLastError());
    return ICPFLOW_OK;
}

}  // extern "C"
