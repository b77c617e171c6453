// overlap.hip -- which segments of two labellings of the same rows are the same set of rows (include/icpflow_hip.h, "8(k) object
// tracks": icpflow_label_overlap; tracks.hip runs the same chain on "this gap's labels" against "track id per row").
//
// Segments are the distinct labels in ascending order (table.hip's launch_label_order), cut into chunks of 1024 rows of the
// stable order by segeval.hip's plan (launch_segment_plan).  Both sides travel through every kernel (blockIdx.y = the side):
//   1. launch_label_order, launch_segment_plan     per side
//   2. ov_rows_kernel    a workgroup of 256 per chunk: segOf[row] = the chunk's segment, -1 where its label is negative
//   3. ov_chunk_kernel   a workgroup of 256 per chunk of a linkable segment: the OTHER side's segOf of the chunk's rows counted
//                        in an LDS histogram of at most 4096 integers (16 KiB, integer LDS atomics: a sum of ones has no order),
//                        then the non-zero counters compacted in ascending order, by ballots and a scan, into the chunk's list
//   4. ov_fold_kernel    a workgroup of 256 per segment: the lists of its chunks added into an LDS histogram again (integers),
//                        then the largest counter (ties to the lower index), the largest of the others and the sum, through a
//                        merge that is commutative and associative on (counter, index) -- its tree does not matter
//   5. ov_close_kernel   one workgroup: partner's label and rows, mutual, IoU (one fp64 division of integers), the counts
// A long segment is never walked by one workgroup: its rows are read by its chunks' workgroups, the fold reads what they found,
// at most min(1024, segments of the other side) words a chunk.  Every number is an integer count or one division of such: the
// output is a function of the arguments alone.  Every word a kernel reads was written by an earlier kernel of the same call.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"
#include "host.hpp"
#include "overlap.hpp"

using icpflow::kWave;
using icpflow::pointer_error;
using icpflow::report_error;
using icpflow::report_errorf;
using icpflow::workspace_error;
using icpflow::overlap::Carve;
using icpflow::overlap::kChunk;
using icpflow::overlap::kCols;
using icpflow::overlap::kCounts;
using icpflow::overlap::kLmax;
using icpflow::overlap::kMaxRows;
using icpflow::overlap::kOrderCols;
using icpflow::overlap::linkable;
using icpflow::overlap::Side;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kPerThread = kChunk / kThreads;
constexpr int kRounds = kLmax / kThreads;              // rounds of 256 counters a histogram is compacted in
constexpr int kCloseThreads = 1024;
static_assert(kChunk < (1 << 16) && kLmax <= (1 << 16), "a list entry is (segment << 16) | rows");

struct Sides {
    Side side[2];
    const int32_t *num[2];
};

// the two numbers of segments: both positive, or nothing is computed (workgroup-uniform)
__device__ __forceinline__ bool both(const Sides &s, int *La, int *Lb)
{
    *La = *s.num[0], *Lb = *s.num[1];
    return *La > 0 && *Lb > 0;
}

// the segment of chunk b: the last one that starts at or before it
__device__ __forceinline__ int segment_of_chunk(const int *__restrict__ chunkStart, int L, int b)
{
    int lo = 0, hi = L - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (chunkStart[mid] <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kThreads) void ov_rows_kernel(Sides s)
{
    int Ls[2];
    if (!both(s, &Ls[0], &Ls[1])) return;
    const int k = blockIdx.y, L = Ls[k], b = blockIdx.x;
    const Side &me = s.side[k];
    if (b >= me.chunkStart[L]) return;
    const int c = segment_of_chunk(me.chunkStart, L, b);
    const double *seg = me.ctable + (size_t)c * kOrderCols;
    const int count = (int)seg[1], start = (int)seg[2];
    const int first = (b - me.chunkStart[c]) * kChunk, rows = min(kChunk, count - first);
    const int32_t v = linkable(seg[0]) ? c : -1;
#pragma unroll
    for (int u = 0; u < kPerThread; ++u) {
        const int j = u * kThreads + (int)threadIdx.x;
        if (j < rows) me.segOf[me.order[(size_t)start + first + j]] = v;
    }
}

__global__ __launch_bounds__(kThreads) void ov_chunk_kernel(Sides s)
{
    __shared__ int hist[kLmax];
    __shared__ int cnt[kRounds][kWaves];
    int Ls[2];
    if (!both(s, &Ls[0], &Ls[1])) return;
    const int k = blockIdx.y, L = Ls[k], Lo = Ls[1 - k], b = blockIdx.x, tid = threadIdx.x;
    const Side &me = s.side[k];
    if (b >= me.chunkStart[L]) return;
    const int c = segment_of_chunk(me.chunkStart, L, b);
    const double *seg = me.ctable + (size_t)c * kOrderCols;
    if (!linkable(seg[0])) {                           // (workgroup-uniform) its rows enter no intersection
        if (tid == 0) me.listCount[b] = 0;
        return;
    }
    const int count = (int)seg[1], start = (int)seg[2];
    const int first = (b - me.chunkStart[c]) * kChunk, rows = min(kChunk, count - first);
    const int32_t *__restrict__ other = s.side[1 - k].segOf;
    for (int e = tid; e < Lo; e += kThreads) hist[e] = 0;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kPerThread; ++u) {
        const int j = u * kThreads + tid;
        if (j < rows) {
            const int o = other[me.order[(size_t)start + first + j]];
            if (o >= 0 && o < Lo) atomicAdd(&hist[o], 1);   // (o < Lo holds: ov_rows_kernel wrote segments of that side)
        }
    }
    __syncthreads();
    // the non-zero counters in ascending order: counter e = 256 r + tid belongs to round r, wave tid / 64
    const int rounds = (Lo + kThreads - 1) / kThreads, wave = tid >> 6, lane = tid & (kWave - 1);
    for (int r = 0; r < rounds; ++r) {                 // (every lane takes every round: the ballots see whole waves)
        const int e = r * kThreads + tid;
        const unsigned long long m = __ballot(e < Lo && hist[e] != 0);
        if (lane == 0) cnt[r][wave] = __popcll(m);
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int r = 0; r < rounds; ++r)
            for (int w = 0; w < kWaves; ++w) {
                const int t = cnt[r][w];
                cnt[r][w] = run;
                run += t;
            }
        me.listCount[b] = run;                         // (<= min(rows, Lo) <= kChunk)
    }
    __syncthreads();
    uint32_t *list = me.list + (size_t)b * kChunk;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int r = 0; r < rounds; ++r) {
        const int e = r * kThreads + tid;
        const int v = e < Lo ? hist[e] : 0;
        const unsigned long long m = __ballot(v != 0);
        if (v != 0) list[cnt[r][wave] + __popcll(m & below)] = ((uint32_t)e << 16) | (uint32_t)v;
    }
}

// the largest counter with its index, the largest of the others, the sum
struct Top {
    int best, idx, second, total;
};

__device__ __forceinline__ Top merge(const Top &a, const Top &b)
{
    const bool first = a.best > b.best || (a.best == b.best && a.idx < b.idx);
    const Top &w = first ? a : b, &l = first ? b : a;
    return Top{w.best, w.idx, max(w.second, l.best), a.total + b.total};
}

__global__ __launch_bounds__(kThreads) void ov_fold_kernel(Sides s)
{
    __shared__ int hist[kLmax];
    __shared__ Top tops[kWaves];
    int Ls[2];
    if (!both(s, &Ls[0], &Ls[1])) return;
    const int k = blockIdx.y, L = Ls[k], Lo = Ls[1 - k], c = blockIdx.x, tid = threadIdx.x;
    if (c >= L) return;
    const Side &me = s.side[k];
    int *out = me.link + (size_t)c * 4;
    if (!linkable(me.ctable[(size_t)c * kOrderCols])) {
        if (tid == 0) out[0] = -1, out[1] = 0, out[2] = 0, out[3] = 0;
        return;
    }
    for (int e = tid; e < Lo; e += kThreads) hist[e] = 0;
    __syncthreads();
    const int c0 = me.chunkStart[c], c1 = me.chunkStart[c + 1];
    for (int q = c0; q < c1; ++q) {
        const int m = min(me.listCount[q], kChunk);
        const uint32_t *list = me.list + (size_t)q * kChunk;
        for (int e = tid; e < m; e += kThreads) {
            const uint32_t v = list[e];
            if ((int)(v >> 16) < Lo) atomicAdd(&hist[v >> 16], (int)(v & 0xffffu));
        }
    }
    __syncthreads();
    Top t{0, kLmax, 0, 0};
    for (int e = tid; e < Lo; e += kThreads) {
        const int v = hist[e];
        if (v > 0) t = merge(t, Top{v, e, 0, v});
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const Top u{__shfl_xor(t.best, o, kWave), __shfl_xor(t.idx, o, kWave), __shfl_xor(t.second, o, kWave), __shfl_xor(t.total, o, kWave)};
        t = merge(t, u);
    }
    if ((tid & (kWave - 1)) == 0) tops[tid >> 6] = t;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kWaves; ++w) t = merge(t, tops[w]);
        out[0] = t.best > 0 ? t.idx : -1, out[1] = t.best, out[2] = t.second, out[3] = t.total;
    }
}

__global__ __launch_bounds__(kCloseThreads) void ov_close_kernel(Sides s, int Lmax, double *__restrict__ tableA, double *__restrict__ tableB,
                                                                 unsigned long long *__restrict__ counts)
{
    __shared__ unsigned long long tot[kCounts];
    int Ls[2];
    const int tid = threadIdx.x;
    if (!both(s, &Ls[0], &Ls[1])) {
        if (tid < kCounts) counts[tid] = 0ull;
        return;
    }
    if (tid < kCounts) tot[tid] = 0ull;
    __syncthreads();
    for (int k = 0; k < 2; ++k) {
        const Side &me = s.side[k], &they = s.side[1 - k];
        double *table = k == 0 ? tableA : tableB;
        const int L = min(Ls[k], Lmax);
        for (int c = tid; c < L; c += kCloseThreads) {
            const double *seg = me.ctable + (size_t)c * kOrderCols;
            const int *link = me.link + (size_t)c * 4;
            const int p = link[0], inter = link[1];
            const bool has = p >= 0;
            const double rows = seg[1], prows = has ? they.ctable[(size_t)p * kOrderCols + 1] : 0.0;
            const bool mutual = has && they.link[(size_t)p * 4] == c;
            double *row = table + (size_t)c * kCols;
            row[0] = seg[0], row[1] = rows, row[2] = (double)link[3], row[3] = (double)p;
            row[4] = has ? they.ctable[(size_t)p * kOrderCols] : 0.0;
            row[5] = (double)inter, row[6] = (double)link[2], row[7] = prows, row[8] = mutual ? 1.0 : 0.0;
            row[9] = has ? (double)inter / ((rows + prows) - (double)inter) : 0.0;
            if (k == 0 && link[3] != 0) atomicAdd(&tot[0], (unsigned long long)link[3]);   // (integers in LDS: no order)
            if (k == 0 && mutual) atomicAdd(&tot[1], 1ull);
            if (has) atomicAdd(&tot[2 + k], 1ull);
        }
    }
    __syncthreads();
    if (tid < kCounts) counts[tid] = tot[tid];
}

bool sizes_ok(int n, int Lmax) { return n >= 0 && n <= kMaxRows && Lmax >= 1 && Lmax <= kLmax; }

}  // namespace

namespace icpflow {
namespace overlap {

bool carve(Carver &ws, int n, int Lmax, Carve *c)
{
    size_t sortBytes = 0;
    if (cluster_table_workspace_bytes(n > 1 ? n : 1, Lmax, &sortBytes) != hipSuccess) return false;
    const size_t chunks = (size_t)segment_max_chunks(n, Lmax);
    for (int k = 0; k < 2; ++k) {
        Side &s = c->side[k];
        s.order = ws.take<int64_t>((size_t)n * sizeof(int64_t));
        s.ctable = ws.take<double>((size_t)Lmax * kOrderCols * sizeof(double));
        s.chunkStart = ws.take<int>(((size_t)Lmax + 1) * sizeof(int));
        s.segOf = ws.take<int32_t>((size_t)n * sizeof(int32_t));
        s.listCount = ws.take<int>(chunks * sizeof(int));
        s.list = ws.take<uint32_t>(chunks * kChunk * sizeof(uint32_t));
        s.link = ws.take<int>((size_t)Lmax * 4 * sizeof(int));
    }
    c->sort = ws.take<void>(sortBytes);
    c->sortBytes = sortBytes;
    return true;
}

hipError_t launch_links(const float *labelsA, const float *labelsB, int n, int Lmax, int32_t *numA, int32_t *numB, const Carve &c,
                        hipStream_t s)
{
    const float *labels[2] = {labelsA, labelsB};
    int32_t *num[2] = {numA, numB};
    Sides sides{};
    for (int k = 0; k < 2; ++k) {
        bool tooSmall = false;
        const hipError_t e = launch_label_order(labels[k], n, c.side[k].order, c.side[k].ctable, Lmax, num[k], c.sort, c.sortBytes, &tooSmall, s);
        if (e != hipSuccess) return e;
        if (tooSmall) return hipErrorInvalidValue;     // (cannot happen: the carve asked table.hip for the size)
        const hipError_t p = launch_segment_plan(c.side[k].ctable, num[k], c.side[k].chunkStart, s);
        if (p != hipSuccess) return p;
        sides.side[k] = c.side[k], sides.num[k] = num[k];
    }
    const int chunks = segment_max_chunks(n, Lmax);
    ov_rows_kernel<<<dim3(chunks, 2), kThreads, 0, s>>>(sides);
    ov_chunk_kernel<<<dim3(chunks, 2), kThreads, 0, s>>>(sides);
    ov_fold_kernel<<<dim3(Lmax, 2), kThreads, 0, s>>>(sides);
    return hipGetLastError();
}

hipError_t launch_tables(const Carve &c, const int32_t *numA, const int32_t *numB, int Lmax, double *tableA, double *tableB,
                         int64_t *counts, hipStream_t s)
{
    Sides sides{};
    sides.side[0] = c.side[0], sides.side[1] = c.side[1], sides.num[0] = numA, sides.num[1] = numB;
    ov_close_kernel<<<1, kCloseThreads, 0, s>>>(sides, Lmax, tableA, tableB, (unsigned long long *)counts);
    return hipGetLastError();
}

}  // namespace overlap
}  // namespace icpflow

extern "C" {

size_t icpflow_label_overlap_workspace_bytes(int n, int Lmax)
{
    if (!sizes_ok(n, Lmax)) return 0;
    icpflow::Carver ws(nullptr);
    Carve c{};
    return icpflow::overlap::carve(ws, n, Lmax, &c) ? ws.total() : 0;
}

int icpflow_label_overlap(const float *d_labels_a, const float *d_labels_b, int n, int Lmax, double *d_table_a, int32_t *d_num_a,
                          double *d_table_b, int32_t *d_num_b, int64_t *d_counts, void *d_ws, size_t ws_bytes, icpflow_stream_t stream)
{
    const char *fn = "icpflow_label_overlap";
    if (n < 0) return report_errorf(ICPFLOW_E_ARG, "icpflow_label_overlap: n = %d: a negative size", n);
    if (n > kMaxRows) return report_errorf(ICPFLOW_E_LIMIT, "icpflow_label_overlap: n = %d: at most %d rows", n, kMaxRows);
    if (Lmax < 1) return report_errorf(ICPFLOW_E_ARG, "icpflow_label_overlap: Lmax = %d: Lmax must be at least 1", Lmax);
    if (Lmax > kLmax) return report_errorf(ICPFLOW_E_LIMIT, "icpflow_label_overlap: Lmax = %d: at most %d segments", Lmax, kLmax);
    if (!d_table_a || !d_num_a || !d_table_b || !d_num_b || !d_counts || (n > 0 && (!d_labels_a || !d_labels_b))) return pointer_error(fn);
    icpflow::Carver ws(d_ws);
    Carve c{};
    if (!icpflow::overlap::carve(ws, n, Lmax, &c)) return report_error(ICPFLOW_E_ARG, "icpflow_label_overlap: no workspace layout for these sizes");
    if (!d_ws || ws_bytes < ws.total()) return workspace_error(fn, "icpflow_label_overlap_workspace_bytes", d_ws, ws_bytes, ws.total());
    if (((uintptr_t)d_ws & 15) != 0) return report_error(ICPFLOW_E_ARG, "icpflow_label_overlap: d_ws must be 16-byte aligned");

    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        ICPFLOW_TRY(hipMemsetAsync(d_num_a, 0, sizeof(int32_t), st));
        ICPFLOW_TRY(hipMemsetAsync(d_num_b, 0, sizeof(int32_t), st));
        ICPFLOW_TRY(hipMemsetAsync(d_counts, 0, kCounts * sizeof(int64_t), st));
        return ICPFLOW_OK;
    }
    ICPFLOW_TRY(icpflow::overlap::launch_links(d_labels_a, d_labels_b, n, Lmax, d_num_a, d_num_b, c, st));
    ICPFLOW_TRY(icpflow::overlap::launch_tables(c, d_num_a, d_num_b, Lmax, d_table_a, d_table_b, d_counts, st));
    return ICPFLOW_OK;
}

}  // extern "C"
