// repair.hip -- the gaps that break a track's constant velocity registered again from the motion the other gaps predict
// (include/icpflow_hip.h, "8(m) track repair": icpflow_pairs_repair_select, icpflow_pairs_reregister; the plan that names the
// gaps is tracks.hip's icpflow_object_tracks_suspects).  No counterpart in the reference.
//
// icpflow_pairs_reregister enqueues, on the caller's stream and nothing else:
//   1. icpflow_gather_segments   both clouds of the K retried pairs, padded to N
//   2. icpflow_apply_icp         source onto destination from d_init (no swap by length), the reference's roll-back included
//   3. icpflow_match_eval        of the new poses
//   4. icpflow_match_eval        of the old poses, on the same clouds
//   5. repair_select_kernel      a thread per pair: the first test that fails is the reason; T_new or, bit for bit, T_old
// 1 to 4 are the existing cores, called through their entry points; the reject test of 5 is the association's
// (rejecttest.hpp).  The select is a few dozen operations per pair: one launch, one thread per pair, no workspace.
//
// icpflow_pairs_fill_candidates ("8(n) track fill"; the plan that names the gaps is tracks.hip's icpflow_object_tracks_missing):
// the source cluster of a gap in which a track found no pair -- the nearest unmatched box within a radius of the predicted
// centre.  fill_choose_kernel, a workgroup per missing row; fill_settle_kernel, a thread per row, settles rows that chose one
// segment.  The pair is then registered by icpflow_pairs_reregister from [I | p] with T_old the identity.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.hpp"
#include "host.hpp"
#include "rejecttest.hpp"

using icpflow::kWave;
using icpflow::pointer_error;
using icpflow::report_errorf;
using icpflow::workspace_error;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kCols = ICPFLOW_REPAIR_COLS, kCounts = ICPFLOW_REPAIR_COUNTS, kReasons = 6;
constexpr int kMaxIterations = 1024;                   // icpflow_apply_icp's bound on max_iterations
static_assert(ICPFLOW_REPAIR_COUNTS == 8, "one count per reason 0 to 5, the host's reason 6, one word kept");

struct SelectArgs {
    const float *Tnew, *Told;
    const int32_t *iters;
    const float *errors, *ious, *translations, *rotations, *errorsOld;
    const double *centre, *pred;
    float tf, iouMin, rotMax, errMax;
    double maxResidual;
    float *Tout;
    double *report;
    unsigned long long *counts;
    int K;
};

__global__ __launch_bounds__(kThreads) void repair_select_kernel(SelectArgs a)
{
    __shared__ int sh[kWaves][kReasons];
    const int k = blockIdx.x * kThreads + (int)threadIdx.x;
    const bool live = k < a.K;
    int reason = -1;
    if (live) {
        const int iters = *a.iters;
        const icpflow::RejectTest t = icpflow::reject_test(a.errors, a.ious, a.translations, a.rotations, k, a.tf, a.iouMin, a.rotMax);
        const float eNew = t.err;
        const float o0 = a.errorsOld[2 * k], o1 = a.errorsOld[2 * k + 1];
        const float eOld = (o0 != o0 || o1 != o1) ? __int_as_float(0x7fc00000) : fminf(o0, o1);
        // d = T_new c - c in the order of icpflow_pair_objects' columns 7-9
        const float *m = a.Tnew + (size_t)k * 16;
        const double cx = a.centre[3 * k], cy = a.centre[3 * k + 1], cz = a.centre[3 * k + 2];
        const double d[3] = {((((double)m[0] * cx + (double)m[1] * cy) + (double)m[2] * cz) + (double)m[3]) - cx,
                             ((((double)m[4] * cx + (double)m[5] * cy) + (double)m[6] * cz) + (double)m[7]) - cy,
                             ((((double)m[8] * cx + (double)m[9] * cy) + (double)m[10] * cz) + (double)m[11]) - cz};
        const double qx = d[0] - a.pred[3 * k], qy = d[1] - a.pred[3 * k + 1];
        const double q2 = qx * qx + qy * qy, m2 = a.maxResidual * a.maxResidual;
        const bool oldIsNan = eOld != eOld;
        if (iters < 0) reason = 5;                                    // the batch was abandoned: every pose of it is NaN
        else if (!t.keep) reason = 1;
        else if (eNew != eNew || !(eNew < a.errMax)) reason = 2;      // (float32, as the association compares: utils_match.py:112)
        else if (q2 > m2) reason = 3;
        else if (!oldIsNan && eNew > eOld) reason = 4;                // (a NaN e_old is +inf: nothing is larger)
        else reason = 0;
        const float *take = reason == 0 ? m : a.Told + (size_t)k * 16;
        float *out = a.Tout + (size_t)k * 16;
#pragma unroll
        for (int c = 0; c < 16; ++c) out[c] = take[c];
        double *row = a.report + (size_t)k * kCols;
        row[0] = (double)reason, row[1] = (double)eNew, row[2] = (double)eOld;
        row[3] = d[0], row[4] = d[1], row[5] = d[2], row[6] = sqrt(q2), row[7] = (double)iters;
        row[8] = (double)t.iou, row[9] = (double)t.nrm, row[10] = (double)t.angle, row[11] = reason == 0 ? 1.0 : 0.0;
    }
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < kReasons; ++r) {               // (every lane takes every round: the ballots see whole waves)
        const int c = __popcll(__ballot(reason == r));
        if ((threadIdx.x & (kWave - 1)) == 0) sh[wave][r] = c;
    }
    __syncthreads();
    if (threadIdx.x < kReasons) {
        int c = 0;
        for (int w = 0; w < kWaves; ++w) c += sh[w][threadIdx.x];
        if (c != 0) atomicAdd(&a.counts[threadIdx.x], (unsigned long long)c);
    }
}

// -> 0, or the status of a refused parameter block
int check_params(const char *fn, const icpflow_repair_params_t *p)
{
    if (p->struct_size != sizeof(icpflow_repair_params_t))
        return report_errorf(ICPFLOW_E_ARG, "%s: params->struct_size = %zu, this library's icpflow_repair_params_t has %zu bytes", fn, p->struct_size,
                             sizeof(icpflow_repair_params_t));
    const struct { const char *name; double v; } all[] = {{"translation_frame", p->translation_frame}, {"thres_iou", p->thres_iou},
                                                          {"rot_limit_deg", p->rot_limit_deg}, {"thres_error", p->thres_error},
                                                          {"max_residual", p->max_residual}};
    for (const auto &e : all)
        if (!(e.v >= 0.0) || !std::isfinite(e.v)) return report_errorf(ICPFLOW_E_ARG, "%s: %s = %g: %s must be finite and not negative", fn, e.name, e.v, e.name);
    return ICPFLOW_OK;
}

// the select behind its argument checks
int enqueue_select(const float *Tnew, const float *Told, const int32_t *iters, const float *errors, const float *ious, const float *translations,
                   const float *rotations, const float *errorsOld, const double *centre, const double *pred, int K,
                   const icpflow_repair_params_t *p, float *Tout, double *report, int64_t *counts, hipStream_t st)
{
    ICPFLOW_TRY(hipMemsetAsync(counts, 0, kCounts * sizeof(int64_t), st));
    if (K == 0) return ICPFLOW_OK;
    const SelectArgs a{Tnew, Told, iters, errors, ious, translations, rotations, errorsOld, centre, pred, (float)p->translation_frame, (float)p->thres_iou,
                       (float)p->rot_limit_deg, (float)p->thres_error, p->max_residual, Tout, report, (unsigned long long *)counts, K};
    repair_select_kernel<<<(K + kThreads - 1) / kThreads, kThreads, 0, st>>>(a);
    ICPFLOW_TRY(hipGetLastError());
    return ICPFLOW_OK;
}

// what a re-registration carves out of its workspace, in this order (the size query runs it on a null base)
struct Carve {
    float *result;           // [44 K + 1]: T_new 16K | the new metrics 14K (errors, inliers, ratios, ious 2K each, translations, rotations
                             // 3K each) | the old metrics 14K | the iteration count (int32)
    void *cores;             // icpflow_workspace_bytes(K, N, 0, 0, 0): the cores', one after the other
    size_t coreBytes, total;
};

bool sizes_ok(int K, int N) { return K >= 1 && N >= 1 && (long long)K * N <= (1ll << 30); }

void carve(void *base, int K, int N, Carve *c)
{
    icpflow::Carver ws(base);
    c->result = ws.take<float>(((size_t)44 * K + 1) * sizeof(float));
    c->coreBytes = icpflow_workspace_bytes(K, N, 0, 0, 0);
    c->cores = ws.take<char>(c->coreBytes);
    c->total = ws.total();
}

// ---- 8(n): the source cluster of a gap in which a track found no pair ----------------------------------------------------------
constexpr int kChoiceCols = ICPFLOW_FILL_CHOICE_COLS, kFillCounts = ICPFLOW_FILL_COUNTS, kBoxCols = ICPFLOW_BOX_COLS;
constexpr int kFillLmax = 4096, kFillEach = kFillLmax / kThreads, kPairTile = 1024, kMaxFillRows = 1 << 16;
static_assert(ICPFLOW_FILL_CHOICE_COLS == 8 && ICPFLOW_FILL_COUNTS == 4, "reason, segment, label, rows, distance, centre; chosen, none, lost, candidates");

// d2 of box centre (X, Y) from q in xy: fp64, every operation written out -- both launches compute it, bit for bit the same
__device__ __forceinline__ double fill_d2(const double *__restrict__ box, const double *__restrict__ q)
{
    const double dx = box[6] - q[0], dy = box[7] - q[1];
    return dx * dx + dy * dy;
}

// Launch 1: workgroup k strides over the segments -- thread t holds segments t, t + 256, ... -- marks the ones a pair row already
// names (the rows' column 0 through LDS in tiles of 1024), and reduces the minimum of (d2, c) among the reachable candidates
// through the wave and then LDS.  Row k of `choice` is written whole, reason 0 or 1; workgroup 0 counts the candidates.
__global__ __launch_bounds__(kThreads) void fill_choose_kernel(const double *__restrict__ q, const double *__restrict__ boxes,
                                                               const int32_t *__restrict__ numSrc, int Lmax, const float *__restrict__ pairRows, int P,
                                                               int stride, double radius, double maxRows, double *__restrict__ choice,
                                                               unsigned long long *__restrict__ counts)
{
    __shared__ float tile[kPairTile];
    __shared__ double shD[kWaves];
    __shared__ int shC[kWaves], shN[kWaves];
    const int k = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & (kWave - 1);
    const int L = max(0, min(*numSrc, Lmax));
    float label[kFillEach];
    unsigned open = 0u;                                 // bit e: segment tid + 256 e has a box, is short enough and (so far) unmatched
#pragma unroll
    for (int e = 0; e < kFillEach; ++e) {
        const int c = tid + e * kThreads;
        label[e] = 0.0f;
        if (c < L) {
            const double *box = boxes + (size_t)c * kBoxCols;
            label[e] = (float)box[0];
            if (box[3] >= 0.0 && box[1] <= maxRows) open |= 1u << e;
        }
    }
    for (int base = 0; base < P; base += kPairTile) {
        const int rows = min(kPairTile, P - base);
        __syncthreads();                                // (the tile before is read out)
        for (int r = tid; r < rows; r += kThreads) tile[r] = pairRows[(size_t)(base + r) * stride];
        __syncthreads();
#pragma unroll
        for (int e = 0; e < kFillEach; ++e) {
            if (!(open >> e & 1u)) continue;
            bool hit = false;
            for (int r = 0; r < rows; ++r) hit |= tile[r] == label[e];     // IEEE ==: +0 and -0 are one label, a NaN equals none
            if (hit) open &= ~(1u << e);
        }
    }
    const double r2 = radius * radius;
    double best = 0.0;
    int bestC = -1;
#pragma unroll
    for (int e = 0; e < kFillEach; ++e) {               // ascending c: a tie keeps the lower one
        if (!(open >> e & 1u)) continue;
        const int c = tid + e * kThreads;
        const double d2 = fill_d2(boxes + (size_t)c * kBoxCols, q + (size_t)k * 3);
        if (d2 <= r2 && (bestC < 0 || d2 < best)) best = d2, bestC = c;      // (a NaN is not within reach)
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const double od = __shfl_xor(best, o, kWave);
        const int oc = __shfl_xor(bestC, o, kWave);
        if (oc >= 0 && (bestC < 0 || od < best || (od == best && oc < bestC))) best = od, bestC = oc;
    }
    const int mine = icpflow::wave_sum((int)__popc(open));
    if (lane == 0) shD[wave] = best, shC[wave] = bestC, shN[wave] = mine;
    __syncthreads();
    if (tid != 0) return;
    int candidates = 0;
    best = 0.0, bestC = -1;
    for (int w = 0; w < kWaves; ++w) {
        candidates += shN[w];
        if (shC[w] >= 0 && (bestC < 0 || shD[w] < best || (shD[w] == best && shC[w] < bestC))) best = shD[w], bestC = shC[w];
    }
    double *row = choice + (size_t)k * kChoiceCols;
    if (bestC < 0) {
        row[0] = 1.0, row[1] = -1.0;
#pragma unroll
        for (int c = 2; c < kChoiceCols; ++c) row[c] = 0.0;
    } else {
        const double *box = boxes + (size_t)bestC * kBoxCols;
        row[0] = 0.0, row[1] = (double)bestC, row[2] = box[0], row[3] = box[1], row[4] = sqrt(best), row[5] = box[6], row[6] = box[7], row[7] = box[8];
    }
    if (k == 0 && candidates != 0) atomicAdd(&counts[3], (unsigned long long)candidates);
}

// Launch 2: a thread per row settles the shared choices.  It reads column 1 of the other rows (launch 1's, never written here)
// and computes their d2 again from the same box; it writes its own column 0 only.
__global__ __launch_bounds__(kThreads) void fill_settle_kernel(const double *__restrict__ q, const double *__restrict__ boxes, int K,
                                                               double *__restrict__ choice, unsigned long long *__restrict__ counts)
{
    __shared__ int sh[kWaves][3];
    const int k = blockIdx.x * kThreads + (int)threadIdx.x;
    int reason = -1;
    if (k < K) {
        const double seg = choice[(size_t)k * kChoiceCols + 1];
        reason = seg < 0.0 ? 1 : 0;
        if (reason == 0) {
            const double *box = boxes + (size_t)(int)seg * kBoxCols;
            const double mine = fill_d2(box, q + (size_t)k * 3);
            for (int j = 0; j < K; ++j) {
                if (j == k || choice[(size_t)j * kChoiceCols + 1] != seg) continue;
                const double d2 = fill_d2(box, q + (size_t)j * 3);
                if (d2 < mine || (d2 == mine && j < k)) reason = 2;
            }
            if (reason == 2) choice[(size_t)k * kChoiceCols] = 2.0;
        }
    }
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < 3; ++r) {                      // (every lane takes every round: the ballots see whole waves)
        const int c = __popcll(__ballot(reason == r));
        if ((threadIdx.x & (kWave - 1)) == 0) sh[wave][r] = c;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        int c = 0;
        for (int w = 0; w < kWaves; ++w) c += sh[w][threadIdx.x];
        if (c != 0) atomicAdd(&counts[threadIdx.x], (unsigned long long)c);
    }
}

}  // namespace

extern "C" {

int icpflow_pairs_fill_candidates(const double *d_q, int K, const double *d_boxes_src, const int32_t *d_num_src, int Lmax,
                                  const float *d_pair_rows, int P, int pair_stride, double radius, int max_rows, double *d_choice,
                                  int64_t *d_counts, icpflow_stream_t stream)
{
    const char *fn = "icpflow_pairs_fill_candidates";
    if (K < 0 || P < 0) return report_errorf(ICPFLOW_E_ARG, "icpflow_pairs_fill_candidates: K = %d, P = %d: a negative size", K, P);
    if (K > kMaxFillRows) return report_errorf(ICPFLOW_E_LIMIT, "icpflow_pairs_fill_candidates: K = %d: at most %d rows", K, kMaxFillRows);
    if (Lmax < 1) return report_errorf(ICPFLOW_E_ARG, "icpflow_pairs_fill_candidates: Lmax = %d: Lmax must be at least 1", Lmax);
    if (Lmax > kFillLmax) return report_errorf(ICPFLOW_E_LIMIT, "icpflow_pairs_fill_candidates: Lmax = %d: at most %d segments", Lmax, kFillLmax);
    if (pair_stride < 1) return report_errorf(ICPFLOW_E_ARG, "icpflow_pairs_fill_candidates: pair_stride = %d: pair_stride must be at least 1", pair_stride);
    if (!(radius > 0.0 && radius <= 1e3)) return report_errorf(ICPFLOW_E_ARG, "icpflow_pairs_fill_candidates: radius = %g: radius must lie in (0, 1e3]", radius);
    if (max_rows < 1) return report_errorf(ICPFLOW_E_ARG, "icpflow_pairs_fill_candidates: max_rows = %d: max_rows must be at least 1", max_rows);
    if (!d_boxes_src || !d_num_src || !d_counts || (K > 0 && (!d_q || !d_choice))) return pointer_error(fn);
    if (P > 0 && !d_pair_rows) return report_errorf(ICPFLOW_E_ARG, "icpflow_pairs_fill_candidates: P = %d and no pair rows", P);

    hipStream_t st = (hipStream_t)stream;
    ICPFLOW_TRY(hipMemsetAsync(d_counts, 0, kFillCounts * sizeof(int64_t), st));
    if (K == 0) return ICPFLOW_OK;
    fill_choose_kernel<<<K, kThreads, 0, st>>>(d_q, d_boxes_src, d_num_src, Lmax, d_pair_rows, P, pair_stride, radius, (double)max_rows, d_choice,
                                              (unsigned long long *)d_counts);
    ICPFLOW_TRY(hipGetLastError());
    fill_settle_kernel<<<(K + kThreads - 1) / kThreads, kThreads, 0, st>>>(d_q, d_boxes_src, K, d_choice, (unsigned long long *)d_counts);
    ICPFLOW_TRY(hipGetLastError());
    return ICPFLOW_OK;
}

int icpflow_pairs_repair_default_params(icpflow_repair_params_t *params)
{
    if (!params) return pointer_error("icpflow_pairs_repair_default_params");
    params->struct_size = sizeof(icpflow_repair_params_t);
    params->translation_frame = 2.0, params->thres_iou = 0.2, params->rot_limit_deg = 9.0, params->thres_error = 0.2, params->max_residual = 0.2;
    return ICPFLOW_OK;
}

int icpflow_pairs_repair_select(const float *d_T_new, const float *d_T_old, const int32_t *d_iters, const float *d_errors, const float *d_ious,
                                const float *d_translations, const float *d_rotations, const float *d_errors_old, const double *d_centre,
                                const double *d_pred, int K, const icpflow_repair_params_t *params, float *d_T_out, double *d_report,
                                int64_t *d_counts, icpflow_stream_t stream)
{
    const char *fn = "icpflow_pairs_repair_select";
    if (K < 0) return report_errorf(ICPFLOW_E_ARG, "icpflow_pairs_repair_select: K = %d: a negative size", K);
    if (K > (1 << 24)) return report_errorf(ICPFLOW_E_LIMIT, "icpflow_pairs_repair_select: K = %d: at most %d pairs", K, 1 << 24);
    if (!params || !d_counts ||
        (K > 0 && (!d_T_new || !d_T_old || !d_iters || !d_errors || !d_ious || !d_translations || !d_rotations || !d_errors_old || !d_centre ||
                   !d_pred || !d_T_out || !d_report)))
        return pointer_error(fn);
    if (const int rc = check_params(fn, params)) return rc;
    return enqueue_select(d_T_new, d_T_old, d_iters, d_errors, d_ious, d_translations, d_rotations, d_errors_old, d_centre, d_pred, K, params,
                          d_T_out, d_report, d_counts, (hipStream_t)stream);
}

size_t icpflow_pairs_reregister_workspace_bytes(int K, int N)
{
    if (!sizes_ok(K, N)) return 0;
    Carve c{};
    carve(nullptr, K, N, &c);
    return c.coreBytes ? c.total : 0;
}

int icpflow_pairs_reregister(const icpflow_tables_t *tables, int K, int N, const int64_t *d_seg, float *d_clouds, const float *d_init,
                             const float *d_T_old, const double *d_centre, const double *d_pred, const icpflow_registration_t *reg,
                             const icpflow_repair_params_t *params, float *d_T_out, double *d_report, int64_t *d_counts, void *d_ws,
                             size_t ws_bytes, icpflow_stream_t stream, const icpflow_options_t *opt)
{
    const char *fn = "icpflow_pairs_reregister";
    if (K < 0) return report_errorf(ICPFLOW_E_ARG, "icpflow_pairs_reregister: K = %d: a negative size", K);
    if (!params || !d_counts) return pointer_error(fn);
    if (const int rc = check_params(fn, params)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (K == 0) return enqueue_select(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, params, nullptr, nullptr,
                                      d_counts, st);
    if (N < 1) return report_errorf(ICPFLOW_E_ARG, "icpflow_pairs_reregister: N = %d: N must be at least 1", N);
    if ((long long)K * N > (1ll << 30)) return report_errorf(ICPFLOW_E_LIMIT, "icpflow_pairs_reregister: K = %d, N = %d: at most 2^30 rows in a batch", K, N);
    if (!tables || !reg || !d_seg || !d_clouds || !d_init || !d_T_old || !d_centre || !d_pred || !d_T_out || !d_report) return pointer_error(fn);
    if (!tables->d_points_src || !tables->d_order_src || !tables->d_points_dst || !tables->d_order_dst) return pointer_error(fn);
    if (reg->max_iterations < 1 || reg->max_iterations > kMaxIterations)
        return report_errorf(ICPFLOW_E_ARG, "icpflow_pairs_reregister: max_iterations = %d: max_iterations must lie in [1, %d]", reg->max_iterations,
                             kMaxIterations);
    if (reg->stop_mode != ICPFLOW_STOP_REFERENCE && reg->stop_mode != ICPFLOW_STOP_PER_PAIR)
        return report_errorf(ICPFLOW_E_ARG, "icpflow_pairs_reregister: stop_mode = %d: unknown", reg->stop_mode);
    if (!(reg->thres_dist >= 0.0) || !std::isfinite(reg->thres_dist))
        return report_errorf(ICPFLOW_E_ARG, "icpflow_pairs_reregister: thres_dist = %g: thres_dist must be finite and not negative", reg->thres_dist);
    Carve c{};
    carve(d_ws, K, N, &c);
    if (!d_ws || ws_bytes < c.total) return workspace_error(fn, "icpflow_pairs_reregister_workspace_bytes", d_ws, ws_bytes, c.total);
    if (((uintptr_t)d_ws & 15) != 0) return report_errorf(ICPFLOW_E_ARG, "%s: d_ws must be 16-byte aligned", fn);

    const size_t k = (size_t)K, cloud = k * N * 4;
    float *R = c.result, *src = d_clouds, *dst = d_clouds + cloud;
    float *O = R + 30 * k;                             // the old pose's metrics, the new ones' order
    int32_t *iters = reinterpret_cast<int32_t *>(R + 44 * k);
    if (const int rc = icpflow_gather_segments(tables->d_points_src, tables->d_order_src, d_seg, nullptr, K, N, src, stream)) return rc;
    if (const int rc = icpflow_gather_segments(tables->d_points_dst, tables->d_order_dst, d_seg + 3 * k, nullptr, K, N, dst, stream)) return rc;
    if (const int rc = icpflow_apply_icp(src, dst, d_init, K, N, reg->thres_dist, reg->max_iterations, reg->relative_rmse_thr, reg->stop_mode, R, iters,
                                         c.cores, c.coreBytes, stream, opt))
        return rc;
    if (const int rc = icpflow_match_eval(src, dst, R, K, N, reg->thres_dist, R + 16 * k, R + 18 * k, R + 20 * k, R + 22 * k, R + 24 * k, R + 27 * k,
                                          c.cores, c.coreBytes, stream, opt))
        return rc;
    if (const int rc = icpflow_match_eval(src, dst, d_T_old, K, N, reg->thres_dist, O, O + 2 * k, O + 4 * k, O + 6 * k, O + 8 * k, O + 11 * k, c.cores,
                                          c.coreBytes, stream, opt))
        return rc;
    return enqueue_select(R, d_T_old, iters, R + 16 * k, R + 22 * k, R + 24 * k, R + 27 * k, O, d_centre, d_pred, K, params, d_T_out, d_report,
                          d_counts, st);
}

}  // extern "C"
