// sight.hip -- the line-of-sight check of a warped source cloud against the destination sweep it was registered to
// (include/icpflow_hip.h, "8(h) line of sight"): a LiDAR return certifies the ray in front of it as empty, so a warped point in
// front of the nearest return of its ray contradicts the flow, and one behind it, on a ray without a return or outside the
// field of view is merely unobserved.  No counterpart in the reference (COVERAGE.md, named deviations).
//
// icpflow_sight_build: the depth image of one sweep, uint32 [2][H][W].
//   1. sight_fill_kernel     plane 0 := the bits of +inf;
//   2. sight_scatter_kernel  a thread per target: its pixel (sight.hpp pixel_of) and atomicMin of the bits of its range -- non-negative
//                            floats order like their bits, an integer minimum does not depend on the order of arrival, and there is
//                            no floating-point atomic;
//   3. sight_spread_kernel   plane 1 := the minimum of plane 0 over the 3 x 3 pixels around each pixel, columns modulo W, rows
//                            clipped to [0, H): a point on an object's silhouette falls into a pixel that may hold background only.
// icpflow_sight_query: a thread per query row, sight.hpp's classify against plane 1; the six counts by ballot and popcount, the
//   waves of a workgroup added in LDS, one integer atomic per count and workgroup.
// icpflow_sight_segments: the same classify per row of either side, counted per segment by segresid.hip's scheme with integer
//   columns -- table.hip's label order, segeval.hip's plan of chunks of 1024 rows, a workgroup of 256 threads per chunk, counts
//   by ballot and popcount, sight_final_kernel adds a segment's chunks in ascending order.  Every workgroup the plan counts
//   stores its whole partial and the final kernel reads only those, so nothing in the workspace is read before it is written.
// Every number of every output is a function of the arguments alone.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.hpp"
#include "host.hpp"
#include "kernels.hpp"
#include "sight.hpp"

using icpflow::kWave;
using icpflow::pointer_error;
using icpflow::report_error;
using icpflow::report_errorf;
using icpflow::workspace_error;
using icpflow::nnr::kMaxRows;
using icpflow::sight::classify;
using icpflow::sight::kBadRow;
using icpflow::sight::kCodes;
using icpflow::sight::kEmpty;
using icpflow::sight::pixel_of;
using icpflow::sight::View;

namespace {

constexpr int kChunk = icpflow::kSegmentChunk;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kPerThread = kChunk / kThreads;
constexpr int kCols = ICPFLOW_SIGHT_COLS;
constexpr int kSide = 1 + 2 * kCodes;                 // good rows, then per code its rows and the FAR rows among them
constexpr int kCounts = 1 + kCodes;                   // bad rows, then the rows of every code
constexpr int kLmax = 4096;
constexpr int kOrderCols = icpflow::kLabelOrderCols;  // label, count, start, ...
constexpr int kAbsent = -3;                           // a lane without a row
static_assert(kCols == 2 + 2 * kSide, "label, rows, and a side's columns twice");
static_assert(2 * kSide <= kThreads, "a thread per column of a partial");

__global__ __launch_bounds__(kThreads) void sight_fill_kernel(uint32_t *__restrict__ plane0, int pixels)
{
    const int at = blockIdx.x * kThreads + threadIdx.x;
    if (at < pixels) plane0[at] = kEmpty;
}

// info: bad targets, targets outside (word 2, the occupied pixels, is the spread's)
__global__ __launch_bounds__(kThreads) void sight_scatter_kernel(const float *__restrict__ target, int m, View v, uint32_t *__restrict__ plane0,
                                                                 unsigned long long *__restrict__ info)
{
    const size_t j = (size_t)blockIdx.x * kThreads + threadIdx.x;
    bool bad = false, outside = false;
    if (j < (size_t)m) {
        const float x = target[3 * j + 0], y = target[3 * j + 1], z = target[3 * j + 2];
        if (!icpflow::nnr::good_coord(x, y, z)) {
            bad = true;
        } else {
            float rho;
            const int pix = pixel_of(v, x, y, z, rho);
            if (pix < 0) outside = true;
            else atomicMin(plane0 + pix, __float_as_uint(rho));
        }
    }
    const unsigned long long n_bad = __popcll(__ballot(bad)), n_out = __popcll(__ballot(outside));
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (n_bad) atomicAdd(info + 0, n_bad);
        if (n_out) atomicAdd(info + 1, n_out);
    }
}

__global__ __launch_bounds__(kThreads) void sight_spread_kernel(int W, int H, const uint32_t *__restrict__ plane0, uint32_t *__restrict__ plane1,
                                                                unsigned long long *__restrict__ info)
{
    const int at = blockIdx.x * kThreads + threadIdx.x;
    bool occupied = false;
    if (at < W * H) {
        const int row = at / W, col = at % W;
        const int left = col == 0 ? W - 1 : col - 1, right = col == W - 1 ? 0 : col + 1;
        uint32_t best = kEmpty;
        for (int r = max(row - 1, 0); r <= min(row + 1, H - 1); ++r) {
            const uint32_t *line = plane0 + (size_t)r * W;
            best = min(best, min(line[left], min(line[col], line[right])));
        }
        plane1[at] = best;
        occupied = plane0[at] != kEmpty;
    }
    const unsigned long long n_occ = __popcll(__ballot(occupied));
    if ((threadIdx.x & (kWave - 1)) == 0 && n_occ) atomicAdd(info + 2, n_occ);
}

// row i of a side: q = p + f
__device__ __forceinline__ void load_query(const float *__restrict__ pts, const float *__restrict__ flow, size_t i, float &x, float &y, float &z)
{
    x = pts[3 * i + 0], y = pts[3 * i + 1], z = pts[3 * i + 2];
    if (flow) x = x + flow[3 * i + 0], y = y + flow[3 * i + 1], z = z + flow[3 * i + 2];
}

__global__ __launch_bounds__(kThreads) void sight_query_kernel(View v, const uint32_t *__restrict__ plane1, const float *__restrict__ query,
                                                               const float *__restrict__ flow, int n, int32_t *__restrict__ code_out,
                                                               float *__restrict__ near_out, unsigned long long *__restrict__ counts)
{
    __shared__ int sh[kWaves][kCounts];
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    int code = kAbsent;
    if (i < (size_t)n) {
        float x, y, z, near;
        load_query(query, flow, i, x, y, z);
        code = classify(v, plane1, x, y, z, near);
        code_out[i] = code;
        if (near_out) near_out[i] = near;
    }
    const int wave = threadIdx.x >> 6;
    int mine = 0;                                      // lane c of a wave keeps count c (every lane takes every ballot)
#pragma unroll
    for (int c = 0; c < kCounts; ++c) {
        const int k = __popcll(__ballot(code == (c == 0 ? kBadRow : c - 1)));
        if ((int)(threadIdx.x & (kWave - 1)) == c) mine = k;
    }
    if ((threadIdx.x & (kWave - 1)) < kCounts) sh[wave][threadIdx.x & (kWave - 1)] = mine;
    __syncthreads();
    if (threadIdx.x < kCounts) {
        int t = sh[0][threadIdx.x];
        for (int w = 1; w < kWaves; ++w) t += sh[w][threadIdx.x];
        if (t) atomicAdd(counts + threadIdx.x, (unsigned long long)t);
    }
}

struct Side {
    const float *pts, *flow, *d2;
    int32_t *code;
};
struct Sides {
    Side s[2];
};

// One workgroup per chunk, both sides: partial[chunk][2][kSide]; info[side][kCounts] by integer atomics.
__global__ __launch_bounds__(kThreads) void sight_chunk_kernel(View v, const uint32_t *__restrict__ plane1, Sides sides, float far2,
                                                               const int64_t *__restrict__ order, const double *__restrict__ ctable,
                                                               const int32_t *__restrict__ num, const int *__restrict__ chunkStart,
                                                               int *__restrict__ partial, unsigned long long *__restrict__ info)
{
    __shared__ int sh[kWaves][2 * kSide];
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
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const Side s = sides.s[side];
        int cnt[kSide];                                // the wave's counts (wave-uniform)
#pragma unroll
        for (int c = 0; c < kSide; ++c) cnt[c] = 0;
#pragma unroll
        for (int u = 0; u < kPerThread; ++u) {         // (every lane takes every round: the ballots see whole waves)
            const int j = u * kThreads + (int)threadIdx.x;
            int code = kAbsent;
            bool far = false;
            if (j < rows) {
                const size_t i = (size_t)order[(size_t)start + first + j];
                float x, y, z, near;
                load_query(s.pts, s.flow, i, x, y, z);
                code = classify(v, plane1, x, y, z, near);
                if (s.code) s.code[i] = code;
                if (s.d2) far = s.d2[i] > far2;
            }
            cnt[0] += __popcll(__ballot(code >= 0));
#pragma unroll
            for (int k = 0; k < kCodes; ++k) {
                cnt[1 + 2 * k] += __popcll(__ballot(code == k));
                cnt[2 + 2 * k] += __popcll(__ballot(code == k && far));
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < kSide; ++c) sh[wave][side * kSide + c] = cnt[c];
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * kSide) {                     // the waves in wave order
        int t = sh[0][threadIdx.x];
        for (int w = 1; w < kWaves; ++w) t += sh[w][threadIdx.x];
        partial[(size_t)b * 2 * kSide + threadIdx.x] = t;
        const int side = threadIdx.x / kSide, c = threadIdx.x % kSide;
        if (c == 0 && rows - t) atomicAdd(info + side * kCounts, (unsigned long long)(rows - t));             // the bad rows
        if ((c & 1) && t) atomicAdd(info + side * kCounts + 1 + (c >> 1), (unsigned long long)t);            // the rows of code c / 2
    }
}

// One thread per (segment, column): the chunks of the segment in ascending order.
__global__ __launch_bounds__(kThreads) void sight_final_kernel(const double *__restrict__ ctable, const int32_t *__restrict__ num,
                                                               const int *__restrict__ chunkStart, const int *__restrict__ partial,
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
        long long sum = 0;
        for (int q = chunkStart[c]; q < chunkStart[c + 1]; ++q) sum += partial[(size_t)q * 2 * kSide + k];
        out = (double)sum;
    }
    table[(size_t)c * kCols + col] = out;
}

// ---- the host side ----------------------------------------------------------------------------------------------------------
// the parameters and the origin checked and narrowed: -> ICPFLOW_OK, or the refusal (reported)
int view_of(const char *fn, const icpflow_sight_params_t *p, const double *o, View *v)
{
    if (p->struct_size != sizeof(icpflow_sight_params_t))
        return report_errorf(ICPFLOW_E_ARG, "%s: params->struct_size = %zu, this library's icpflow_sight_params_t has %zu bytes", fn, p->struct_size,
                             sizeof(icpflow_sight_params_t));
    if (p->W < 4 || p->W > icpflow::sight::kMaxW || p->W % 4 != 0 || p->H < 1 || p->H > icpflow::sight::kMaxH ||
        (long long)p->W * p->H > icpflow::sight::kMaxPixels)
        return report_errorf(ICPFLOW_E_ARG, "%s: W = %d, H = %d: W must be a multiple of 4 in [4, 8192], H in [1, 2048], W * H at most 2^22", fn, p->W, p->H);
    const float lo = (float)p->tan_lo, hi = (float)p->tan_hi;
    if (!std::isfinite(p->tan_lo) || !std::isfinite(p->tan_hi) || !std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi))
        return report_errorf(ICPFLOW_E_ARG, "%s: tan_lo = %g, tan_hi = %g: both finite and tan_lo < tan_hi as floats", fn, p->tan_lo, p->tan_hi);
    const float rmin = (float)p->min_range, rmax = (float)p->max_range;
    if (!(p->min_range >= 0.0) || !(p->max_range <= icpflow::sight::kMaxRange) || !(rmin < rmax))
        return report_errorf(ICPFLOW_E_ARG, "%s: min_range = %g, max_range = %g: 0 <= min_range < max_range <= 1e6 metres", fn, p->min_range, p->max_range);
    if (!(p->margin_abs >= 0.0) || !std::isfinite(p->margin_abs) || !(p->margin_rel >= 0.0) || !(p->margin_rel < 1.0))
        return report_errorf(ICPFLOW_E_ARG, "%s: margin_abs = %g, margin_rel = %g: margin_abs >= 0 and finite, 0 <= margin_rel < 1", fn, p->margin_abs, p->margin_rel);
    for (int k = 0; k < 3; ++k)
        if (!(std::fabs(o[k]) <= 1e6))
            return report_errorf(ICPFLOW_E_ARG, "%s: h_origin[%d] = %g: the origin must be finite and within 1e6 metres", fn, k, o[k]);
    v->ox = (float)o[0], v->oy = (float)o[1], v->oz = (float)o[2];
    v->tan_lo = lo, v->tan_hi = hi, v->rs = (float)p->H / (hi - lo);
    v->min_range = rmin, v->max_range = rmax;
    v->margin_abs = (float)p->margin_abs, v->margin_rel = (float)p->margin_rel;
    v->quarter = (float)(p->W / 4);
    v->W = p->W, v->H = p->H;
    return ICPFLOW_OK;
}

inline int blocks_for(size_t items) { return (int)((items + kThreads - 1) / kThreads); }

// what icpflow_sight_segments carves out of its workspace, in this order (the size query runs it on a null base)
struct Carve {
    int64_t *order;          // [n] rows sorted by label, stable
    double *ctable;          // [Lmax][kOrderCols] label, count, start
    int *chunkStart;         // [Lmax + 1] first chunk of every segment, then the number of chunks
    int *partial;            // [max chunks][2][kSide]
    void *sort;              // table.hip's own workspace
    size_t sortBytes, total;
};

bool carve(void *base, int n, int Lmax, Carve *c)
{
    size_t sortBytes = 0;
    if (icpflow::cluster_table_workspace_bytes(n > 1 ? n : 1, Lmax, &sortBytes) != hipSuccess) return false;
    icpflow::Carver ws(base);
    c->order = ws.take<int64_t>((size_t)n * sizeof(int64_t));
    c->ctable = ws.take<double>((size_t)Lmax * kOrderCols * sizeof(double));
    c->chunkStart = ws.take<int>(((size_t)Lmax + 1) * sizeof(int));
    c->partial = ws.take<int>((size_t)icpflow::segment_max_chunks(n, Lmax) * 2 * kSide * sizeof(int));
    c->sort = ws.take<void>(sortBytes);
    c->sortBytes = sortBytes;
    c->total = ws.total();
    return true;
}

bool sizes_ok(int n, int Lmax) { return n >= 0 && n <= kMaxRows && Lmax >= 1 && Lmax <= kLmax; }

}  // namespace

extern "C" {

int icpflow_sight_default_params(icpflow_sight_params_t *params)
{
    if (!params) return pointer_error("icpflow_sight_default_params");
    params->struct_size = sizeof(icpflow_sight_params_t);
    params->W = 1024, params->H = 64;
    params->tan_lo = -0.6, params->tan_hi = 0.4;
    params->min_range = 1.0, params->max_range = 200.0;
    params->margin_abs = 0.2, params->margin_rel = 0.01;
    return ICPFLOW_OK;
}

int icpflow_sight_build(const float *d_target, int m, const double *h_origin, const icpflow_sight_params_t *params, uint32_t *d_image,
                        int64_t *d_info, icpflow_stream_t stream)
{
    const char *fn = "icpflow_sight_build";
    if (m < 0) return report_error(ICPFLOW_E_ARG, "icpflow_sight_build: m < 0");
    if (m > kMaxRows) return report_errorf(ICPFLOW_E_LIMIT, "icpflow_sight_build: m = %d: at most %d rows a cloud", m, kMaxRows);
    if (!h_origin || !params || !d_image || !d_info || (m > 0 && !d_target)) return pointer_error(fn);
    View v;
    if (const int rc = view_of(fn, params, h_origin, &v)) return rc;

    hipStream_t st = (hipStream_t)stream;
    const int pixels = v.W * v.H;
    unsigned long long *info = (unsigned long long *)d_info;   // bad targets, targets outside, occupied pixels
    ICPFLOW_TRY(hipMemsetAsync(info, 0, 3 * sizeof(unsigned long long), st));
    sight_fill_kernel<<<blocks_for(pixels), kThreads, 0, st>>>(d_image, pixels);
    ICPFLOW_TRY(hipGetLastError());
    if (m > 0) {
        sight_scatter_kernel<<<blocks_for(m), kThreads, 0, st>>>(d_target, m, v, d_image, info);
        ICPFLOW_TRY(hipGetLastError());
    }
    sight_spread_kernel<<<blocks_for(pixels), kThreads, 0, st>>>(v.W, v.H, d_image, d_image + pixels, info);
    ICPFLOW_TRY(hipGetLastError());
    return ICPFLOW_OK;
}

int icpflow_sight_query(const uint32_t *d_image, const icpflow_sight_params_t *params, const double *h_origin, const float *d_query,
                        const float *d_flow, int n, int32_t *d_code_out, float *d_near_out, int64_t *d_counts, icpflow_stream_t stream)
{
    const char *fn = "icpflow_sight_query";
    if (n < 0) return report_error(ICPFLOW_E_ARG, "icpflow_sight_query: n < 0");
    if (n > kMaxRows) return report_errorf(ICPFLOW_E_LIMIT, "icpflow_sight_query: n = %d: at most %d rows a cloud", n, kMaxRows);
    if (!d_image || !params || !h_origin || !d_counts || (n > 0 && (!d_query || !d_code_out))) return pointer_error(fn);
    View v;
    if (const int rc = view_of(fn, params, h_origin, &v)) return rc;

    hipStream_t st = (hipStream_t)stream;
    unsigned long long *counts = (unsigned long long *)d_counts;   // bad rows, then the rows of codes 0 .. 4
    ICPFLOW_TRY(hipMemsetAsync(counts, 0, kCounts * sizeof(unsigned long long), st));
    if (n == 0) return ICPFLOW_OK;
    sight_query_kernel<<<blocks_for(n), kThreads, 0, st>>>(v, d_image + (size_t)v.W * v.H, d_query, d_flow, n, d_code_out, d_near_out, counts);
    ICPFLOW_TRY(hipGetLastError());
    return ICPFLOW_OK;
}

size_t icpflow_sight_segments_workspace_bytes(int n, int Lmax)
{
    if (!sizes_ok(n, Lmax)) return 0;
    Carve c{};
    return carve(nullptr, n, Lmax, &c) ? c.total : 0;
}

int icpflow_sight_segments(const uint32_t *d_image, const icpflow_sight_params_t *params, const double *h_origin, const float *d_before,
                           const float *d_after, const float *d_flow, const float *d_labels, int n, const float *d_d2_before,
                           const float *d_d2_after, double far, double *d_table, int Lmax, int32_t *d_num, int32_t *d_code_before,
                           int32_t *d_code_after, int64_t *d_info, void *d_ws, size_t ws_bytes, icpflow_stream_t stream)
{
    const char *fn = "icpflow_sight_segments";
    if (n < 0) return report_error(ICPFLOW_E_ARG, "icpflow_sight_segments: n < 0");
    if (n > kMaxRows) return report_errorf(ICPFLOW_E_LIMIT, "icpflow_sight_segments: n = %d: at most %d rows a cloud", n, kMaxRows);
    if (Lmax < 1) return report_errorf(ICPFLOW_E_ARG, "icpflow_sight_segments: Lmax = %d: Lmax must be at least 1", Lmax);
    if (Lmax > kLmax) return report_errorf(ICPFLOW_E_LIMIT, "icpflow_sight_segments: Lmax = %d: at most %d segments", Lmax, kLmax);
    if (!(far >= 0.0 && far <= icpflow::nnr::kMaxRadius))
        return report_errorf(ICPFLOW_E_ARG, "icpflow_sight_segments: far = %g: far must lie in [0, 1e3] metres", far);
    if (!d_image || !params || !h_origin || !d_table || !d_num || !d_info || (n > 0 && (!d_before || !d_after || !d_labels))) return pointer_error(fn);
    View v;
    if (const int rc = view_of(fn, params, h_origin, &v)) return rc;
    Carve c{};
    if (!carve(d_ws, n, Lmax, &c)) return report_error(ICPFLOW_E_ARG, "icpflow_sight_segments: no workspace layout for these sizes");
    if (!d_ws || ws_bytes < c.total) return workspace_error(fn, "icpflow_sight_segments_workspace_bytes", d_ws, ws_bytes, c.total);
    if (((uintptr_t)d_ws & 15) != 0) return report_error(ICPFLOW_E_ARG, "icpflow_sight_segments: d_ws must be 16-byte aligned");

    hipStream_t st = (hipStream_t)stream;
    const float farf = (float)far, far2 = farf * farf;
    unsigned long long *info = (unsigned long long *)d_info;   // before: bad rows, the rows of codes 0 .. 4; after: the same six
    ICPFLOW_TRY(hipMemsetAsync(info, 0, 2 * kCounts * sizeof(unsigned long long), st));
    if (n == 0) {
        ICPFLOW_TRY(hipMemsetAsync(d_num, 0, sizeof(int32_t), st));
        return ICPFLOW_OK;
    }
    bool tooSmall = false;
    ICPFLOW_TRY(icpflow::launch_label_order(d_labels, n, c.order, c.ctable, Lmax, d_num, c.sort, c.sortBytes, &tooSmall, st));
    if (tooSmall) return workspace_error(fn, "icpflow_sight_segments_workspace_bytes", d_ws, ws_bytes, c.total);   // (cannot happen: same carve)
    ICPFLOW_TRY(icpflow::launch_segment_plan(c.ctable, d_num, c.chunkStart, st));
    const Sides sides = {{{d_before, nullptr, d_d2_before, d_code_before}, {d_after, d_flow, d_d2_after, d_code_after}}};
    sight_chunk_kernel<<<icpflow::segment_max_chunks(n, Lmax), kThreads, 0, st>>>(v, d_image + (size_t)v.W * v.H, sides, far2, c.order, c.ctable,
                                                                                   d_num, c.chunkStart, c.partial, info);
    ICPFLOW_TRY(hipGetLastError());
    sight_final_kernel<<<(Lmax * kCols + kThreads - 1) / kThreads, kThreads, 0, st>>>(c.ctable, d_num, c.chunkStart, c.partial, d_table);
    ICPFLOW_TRY(hipGetLastError());
    return ICPFLOW_OK;
}

}  // extern "C"
