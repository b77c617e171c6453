// trust.hip -- one trust byte per source point of a registered frame pair (include/icpflow_hip.h, "8(i) trust byte",
// icpflow_flow_trust): the verdicts that SegmentResidual.worst and SegmentSight.annotate reach on the host, taken on the device
// from the same two tables and spread over the rows, so that a saved flow can say which of its rows to train on.
//
// Two launches on the caller's stream, no workspace:
//   1. trust_segment_kernel  one thread per segment: its bits 3 - 6 (FIT, MATCHED, SKIPPED) -> d_segment; the pair labels pass
//                            through LDS in tiles of 1024, every thread of a workgroup comparing its label with the whole tile;
//                            workgroup 0 zeroes d_counts.
//   2. trust_row_kernel      a workgroup of 256 threads per 1024 rows, thread t rows t, t + 256, t + 512, t + 768 of them (as
//                            segresid.hip's chunks); the segments' keys and bytes staged in LDS (20 KB at Lmax = 4096), a row's
//                            segment by binary search on label_key -- table.hip's own order of the labels (labelkey.hpp).
// Counts by ballot and popcount, one integer atomic per count, wave and workgroup; nothing else is shared between workgroups,
// so every byte and every count is a function of the arguments alone.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"
#include "host.hpp"
#include "trust.hpp"

using icpflow::kWave;
using icpflow::pointer_error;
using icpflow::report_error;
using icpflow::report_errorf;
using icpflow::trust::kCounts;
using icpflow::trust::kLmax;
using icpflow::trust::kResidCols;
using icpflow::trust::kSightCols;
using icpflow::trust::Params;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kRowsBlock = 1024;
constexpr int kPerThread = kRowsBlock / kThreads;
constexpr int kPairTile = 1024;
constexpr int kMaxRows = icpflow::nnr::kMaxRows;

// the number of segments both kernels work with: *d_num, nothing when it reports overflow, never beyond the tables' rows
__device__ __forceinline__ int segments_of(const int32_t *__restrict__ num, int Lmax)
{
    const int L = *num;
    return L <= 0 ? 0 : min(L, Lmax);
}

__global__ __launch_bounds__(kThreads) void trust_segment_kernel(const double *__restrict__ resid, const double *__restrict__ sight,
                                                                 const int32_t *__restrict__ num, int Lmax, const float *__restrict__ pairs,
                                                                 int P, int stride, Params p, uint8_t *__restrict__ segment,
                                                                 unsigned long long *__restrict__ counts)
{
    __shared__ float tile[kPairTile];
    const int L = segments_of(num, Lmax);
    const int c = blockIdx.x * kThreads + (int)threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < kCounts) counts[threadIdx.x] = 0ull;
    if (blockIdx.x * kThreads >= L) return;            // (workgroup-uniform: no segment of this workgroup exists)
    const bool mine = c < L;
    const double label = mine ? resid[(size_t)c * kResidCols] : 0.0;
    bool matched = false;
    for (int p0 = 0; p0 < P; p0 += kPairTile) {        // (every thread takes every tile: the barriers see whole workgroups)
        const int rows = min(kPairTile, P - p0);
        for (int j = threadIdx.x; j < rows; j += kThreads) tile[j] = pairs[(size_t)(p0 + j) * stride];
        __syncthreads();
        if (mine)
            for (int j = 0; j < rows; ++j) matched |= label == (double)tile[j];   // (IEEE ==: -0.0 matches +0.0, a NaN nothing)
        __syncthreads();
    }
    if (mine)
        segment[c] = (uint8_t)icpflow::trust::segment_bits(p, resid + (size_t)c * kResidCols,
                                                           sight != nullptr ? sight + (size_t)c * kSightCols : nullptr, matched);
}

__global__ __launch_bounds__(kThreads) void trust_row_kernel(const float *__restrict__ after, const float *__restrict__ flow,
                                                             const float *__restrict__ labels, int n, const double *__restrict__ resid,
                                                             const int32_t *__restrict__ num, int Lmax, const uint8_t *__restrict__ segment,
                                                             const float *__restrict__ d2_after, const int32_t *__restrict__ code_after,
                                                             float far2, uint8_t *__restrict__ trust, unsigned long long *__restrict__ counts)
{
    __shared__ uint32_t key[kLmax];
    __shared__ uint8_t bits[kLmax];
    __shared__ int sh[kWaves][kCounts];
    const int L = segments_of(num, Lmax);
    for (int c = threadIdx.x; c < L; c += kThreads) {
        key[c] = icpflow::label_key(icpflow::trust::quieted((float)resid[(size_t)c * kResidCols]));
        bits[c] = segment[c];
    }
    __syncthreads();
    int count[kCounts];                                 // the wave's counts (wave-uniform)
#pragma unroll
    for (int k = 0; k < kCounts; ++k) count[k] = 0;
    const size_t base = (size_t)blockIdx.x * kRowsBlock;
#pragma unroll
    for (int u = 0; u < kPerThread; ++u) {              // (every lane takes every round: the ballots see whole waves)
        const size_t i = base + (size_t)(u * kThreads) + threadIdx.x;
        const bool live = i < (size_t)n;
        bool found = false;
        unsigned byte = 0;
        if (live) {
            const uint32_t want = icpflow::label_key(icpflow::trust::quieted(labels[i]));
            int lo = 0, hi = L;                         // the first segment whose key is not below `want`
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (key[mid] < want) lo = mid + 1; else hi = mid;
            }
            found = lo < L && key[lo] == want;
            if (found) {
                float x = after[3 * i], y = after[3 * i + 1], z = after[3 * i + 2];
                if (flow != nullptr) x += flow[3 * i], y += flow[3 * i + 1], z += flow[3 * i + 2];
                const int row = icpflow::trust::row_class(icpflow::nnr::good_coord(x, y, z), d2_after[i], far2, code_after != nullptr,
                                                          code_after != nullptr ? code_after[i] : 0);
                byte = icpflow::trust::trust_byte(bits[lo], row);
            }
            trust[i] = (uint8_t)byte;
        }
        const int row = (int)(byte & icpflow::trust::kRowMask), fit = (int)(byte >> icpflow::trust::kFitShift) & icpflow::trust::kFitMask;
        const bool skipped = (byte & icpflow::trust::kSkipped) != 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) count[k] += __popcll(__ballot(found && row == k));
#pragma unroll
        for (int k = 0; k < 4; ++k) count[8 + k] += __popcll(__ballot(found && row != 0 && !skipped && fit == k));
        count[12] += __popcll(__ballot((byte & icpflow::trust::kMatched) != 0));
        count[13] += __popcll(__ballot(skipped));
        count[14] += __popcll(__ballot((byte & icpflow::trust::kKeep) != 0));
        count[15] += __popcll(__ballot(live && !found));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & (kWave - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < kCounts; ++k) sh[wave][k] = count[k];
    }
    __syncthreads();
    if (threadIdx.x < kCounts) {
        int t = 0;
        for (int w = 0; w < kWaves; ++w) t += sh[w][threadIdx.x];
        if (t != 0) atomicAdd(&counts[threadIdx.x], (unsigned long long)t);
    }
}

bool in_range(double v, double lo, double hi) { return v >= lo && v <= hi; }   // (a NaN fails)

}  // namespace

extern "C" {

int icpflow_flow_trust_default_params(icpflow_trust_params_t *params)
{
    if (!params) return pointer_error("icpflow_flow_trust_default_params");
    params->struct_size = sizeof(icpflow_trust_params_t);
    params->above = 0.1, params->far = 0.1, params->share = 0.5;
    params->skip[0] = -1e8f, params->skip[1] = -1.0f;
    return ICPFLOW_OK;
}

int icpflow_flow_trust(const float *d_after, const float *d_flow, const float *d_labels, int n, const double *d_resid_table,
                       const double *d_sight_table, const int32_t *d_num, int Lmax, const float *d_d2_after, const int32_t *d_code_after,
                       const float *d_pair_rows, int P, int pair_stride, const icpflow_trust_params_t *params, uint8_t *d_trust,
                       uint8_t *d_segment, int64_t *d_counts, icpflow_stream_t stream)
{
    const char *fn = "icpflow_flow_trust";
    if (n < 0 || P < 0) return report_errorf(ICPFLOW_E_ARG, "icpflow_flow_trust: n = %d, P = %d: a negative size", n, P);
    if (n > kMaxRows) return report_errorf(ICPFLOW_E_LIMIT, "icpflow_flow_trust: n = %d: at most %d rows a cloud", n, kMaxRows);
    if (Lmax < 1) return report_errorf(ICPFLOW_E_ARG, "icpflow_flow_trust: Lmax = %d: Lmax must be at least 1", Lmax);
    if (Lmax > kLmax) return report_errorf(ICPFLOW_E_LIMIT, "icpflow_flow_trust: Lmax = %d: at most %d segments", Lmax, kLmax);
    if (pair_stride < 1) return report_errorf(ICPFLOW_E_ARG, "icpflow_flow_trust: pair_stride = %d: pair_stride must be at least 1", pair_stride);
    if (!d_resid_table || !d_num || !params || !d_segment || !d_counts || (n > 0 && (!d_after || !d_labels || !d_d2_after || !d_trust)))
        return pointer_error(fn);
    if (P > 0 && !d_pair_rows) return report_errorf(ICPFLOW_E_ARG, "icpflow_flow_trust: P = %d and no pair rows", P);
    if (d_code_after != nullptr && d_sight_table == nullptr)
        return report_error(ICPFLOW_E_ARG, "icpflow_flow_trust: line-of-sight codes without a sight table");
    if (n > 0 && d_sight_table != nullptr && d_code_after == nullptr)
        return report_error(ICPFLOW_E_ARG, "icpflow_flow_trust: a sight table without line-of-sight codes");
    if (params->struct_size != sizeof(icpflow_trust_params_t))
        return report_errorf(ICPFLOW_E_ARG, "icpflow_flow_trust: params->struct_size = %zu, this library's icpflow_trust_params_t has %zu bytes",
                             params->struct_size, sizeof(icpflow_trust_params_t));
    if (!in_range(params->above, 0.0, 1e3)) return report_errorf(ICPFLOW_E_ARG, "icpflow_flow_trust: above = %g: above must lie in [0, 1e3] metres", params->above);
    if (!in_range(params->far, 0.0, 1e3)) return report_errorf(ICPFLOW_E_ARG, "icpflow_flow_trust: far = %g: far must lie in [0, 1e3] metres", params->far);
    if (!(params->share >= 0.0 && params->share < 1.0))
        return report_errorf(ICPFLOW_E_ARG, "icpflow_flow_trust: share = %g: share must lie in [0, 1)", params->share);

    hipStream_t st = (hipStream_t)stream;
    const float farf = (float)params->far;
    const Params p = {params->above, params->share, farf * farf, {params->skip[0], params->skip[1]}};
    unsigned long long *counts = (unsigned long long *)d_counts;
    trust_segment_kernel<<<(Lmax + kThreads - 1) / kThreads, kThreads, 0, st>>>(d_resid_table, d_sight_table, d_num, Lmax, d_pair_rows, P, pair_stride,
                                                                                p, d_segment, counts);
    ICPFLOW_TRY(hipGetLastError());
    if (n == 0) return ICPFLOW_OK;
    trust_row_kernel<<<(n + kRowsBlock - 1) / kRowsBlock, kThreads, 0, st>>>(d_after, d_flow, d_labels, n, d_resid_table, d_num, Lmax, d_segment,
                                                                             d_d2_after, d_code_after, p.far2, d_trust, counts);
    ICPFLOW_TRY(hipGetLastError());
    return ICPFLOW_OK;
}

}  // extern "C"
