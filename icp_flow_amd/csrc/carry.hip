// carry.hip -- ids carried between two views of one sweep whose rows are not identical, and an id per row of one side of a
// frame pair (include/icpflow_hip.h, "8(l) object tracks across the files of a log": icpflow_rows_carry,
// icpflow_pair_row_ids).
//
// icpflow_rows_carry: the previous view's rows are moved by the pose in fp32 and become the targets of icpflow_nn_residual's
// exact search (nnresid.hpp: the same grid, the same scan, the same binned query -- none of it is copied); a row of the other
// view takes the id of its nearest moved row inside the radius.
//   1. carry_count_kernel    a thread per previous row: moved, its bucket counted (integer atomics: counts are order-free);
//                            the bad rows counted into d_counts[4] by ballot and popcount
//      nnr::scan_grid        the buckets' starts (nnresid.hip's tile / offsets / starts kernels)
//   2. carry_scatter_kernel  a thread per previous row: moved again by the same operations, (x', y', z', row) to its slot --
//                            the moved cloud is never stored row by row, the move costs no pass of its own
//      nnr::bin_cloud, nnr::launch_binned_query   the other view binned and searched: d2 and idx, word for word 8(g)'s
//   3. carry_gather_kernel   a thread per query: the id of the hit's previous row; hits, hits with an id and misses by ballot and
//                            popcount, one integer atomic per count and workgroup
//   4. carry_close_kernel    BROKEN = (double)hits < min_share * (double)n decided on the device; every id -1 then
// icpflow_pair_row_ids, shaped like trust.hip:
//   1. prid_table_kernel     a thread per pair: every pair's (key, id, weight) passes through LDS in tiles of 1024; the thread
//                            learns its rank in the stable order of the keys and the winner among the pairs of its key, and
//                            writes (key, winner) at its rank -- a sorted table with no sort and no atomic
//   2. prid_row_kernel       a workgroup of 256 threads per 1024 rows, the table staged in LDS, a row's key by binary search
// No floating-point atomic anywhere: every output is a function of the arguments alone.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.hpp"
#include "gridhash.hpp"
#include "host.hpp"
#include "labelkey.hpp"
#include "nnresid.hpp"
#include "trust.hpp"

using icpflow::Carver;
using icpflow::kWave;
using icpflow::pointer_error;
using icpflow::report_error;
using icpflow::report_errorf;
using icpflow::workspace_error;
using icpflow::nnr::cell_of;
using icpflow::nnr::Cloud;
using icpflow::nnr::good_coord;
using icpflow::nnr::Grid;
using icpflow::nnr::kMaxRadius;
using icpflow::nnr::kMaxRows;
using icpflow::nnr::kMinRadius;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kCarryCounts = ICPFLOW_CARRY_COUNTS;
constexpr int kRowIdCounts = ICPFLOW_PAIR_ROW_ID_COUNTS;
constexpr int kMaxPairs = ICPFLOW_PAIR_ROW_ID_MAX_PAIRS;
constexpr int kPairTile = 1024;
constexpr int kRowsBlock = 1024;
constexpr int kPerThread = kRowsBlock / kThreads;
static_assert(kCarryCounts == 6, "hits, hits with an id, misses, bad queries, bad previous rows, broken");
static_assert(kRowIdCounts == 3, "rows with an id, rows without, pairs whose label an earlier pair has");

// rows 0 .. 2 of the pose, narrowed to float on the host
struct Move {
    float m[12];
};

// previous row j moved: x' = ((m00 x + m01 y) + m02 z) + m03, every operation rounded by itself (-ffp-contract=off); false for a
// bad row -- a coordinate of the row or of the moved row not finite or beyond 1e6 m
__device__ __forceinline__ bool load_moved(const float *__restrict__ prev, const Move &mv, size_t j, float &x, float &y, float &z)
{
    const float px = prev[3 * j + 0], py = prev[3 * j + 1], pz = prev[3 * j + 2];
    x = ((mv.m[0] * px + mv.m[1] * py) + mv.m[2] * pz) + mv.m[3];
    y = ((mv.m[4] * px + mv.m[5] * py) + mv.m[6] * pz) + mv.m[7];
    z = ((mv.m[8] * px + mv.m[9] * py) + mv.m[10] * pz) + mv.m[11];
    return good_coord(px, py, pz) && good_coord(x, y, z);
}

__global__ __launch_bounds__(kThreads) void carry_count_kernel(const float *__restrict__ prev, int m, Move mv, double h, unsigned mask,
                                                               unsigned *__restrict__ cursor, unsigned long long *__restrict__ bad_rows)
{
    const size_t j = (size_t)blockIdx.x * kThreads + threadIdx.x;
    bool bad = false;
    if (j < (size_t)m) {
        float x, y, z;
        if (load_moved(prev, mv, j, x, y, z)) atomicAdd(cursor + icpflow::grid_hash(cell_of(x, h), cell_of(y, h), cell_of(z, h), mask), 1u);
        else bad = true;
    }
    const unsigned long long n_bad = __popcll(__ballot(bad));      // (every lane takes the ballot)
    if ((threadIdx.x & (kWave - 1)) == 0 && n_bad) atomicAdd(bad_rows, n_bad);
}

__global__ __launch_bounds__(kThreads) void carry_scatter_kernel(const float *__restrict__ prev, int m, Move mv, double h, unsigned mask,
                                                                 unsigned *__restrict__ cursor, float4 *__restrict__ records)
{
    const size_t j = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= (size_t)m) return;
    float x, y, z;
    if (!load_moved(prev, mv, j, x, y, z)) return;
    const unsigned slot = atomicAdd(cursor + icpflow::grid_hash(cell_of(x, h), cell_of(y, h), cell_of(z, h), mask), 1u);   // < good rows <= m: the counts' scan
    records[slot] = make_float4(x, y, z, __int_as_float((int)j));
}

// the workgroup's counts of K flags per thread into counts[first ...]: ballot and popcount per wave, the waves' words added in
// wave order, one integer atomic per count (all threads call it)
template <int K>
__device__ __forceinline__ void count_flags(const bool (&flag)[K], int (*sh)[K], unsigned long long *__restrict__ counts)
{
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int t = __popcll(__ballot(flag[k]));
        if ((threadIdx.x & (kWave - 1)) == 0) sh[wave][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        int t = 0;
        for (int w = 0; w < kWaves; ++w) t += sh[w][threadIdx.x];
        if (t != 0) atomicAdd(&counts[threadIdx.x], (unsigned long long)t);
    }
}

__global__ __launch_bounds__(kThreads) void carry_gather_kernel(const int32_t *__restrict__ idx, const int32_t *__restrict__ prev_id, int n,
                                                                int32_t *__restrict__ id_out, unsigned long long *__restrict__ counts)
{
    __shared__ int sh[kWaves][3];
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    bool hit = false, with = false, miss = false;
    if (i < (size_t)n) {
        const int at = idx[i];                          // a previous row, -1 (no hit) or -2 (a bad query)
        int id = -1;
        if (at >= 0) id = prev_id[at];
        hit = at >= 0, with = hit && id >= 0, miss = at == -1;
        id_out[i] = with ? id : -1;
    }
    const bool flag[3] = {hit, with, miss};
    count_flags<3>(flag, sh, counts);
}

__global__ __launch_bounds__(kThreads) void carry_close_kernel(int n, double min_share, int32_t *__restrict__ id_out,
                                                               unsigned long long *__restrict__ counts)
{
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const bool broken = (double)counts[0] < min_share * (double)n;    // one fp64 product; word 0 is final: the gather is over
    if (broken && i < (size_t)n) id_out[i] = -1;
    if (i == 0) counts[5] = broken ? 1ull : 0ull;
}

struct CarryCarve {
    Grid targets, queries;
    float *d2;
    int32_t *idx;
    size_t total;
};

CarryCarve carve_carry(void *base, int n, int m)
{
    CarryCarve c;
    Carver ws(base);
    c.targets = icpflow::nnr::carve_grid(ws, m);
    c.queries = icpflow::nnr::carve_grid(ws, n);
    c.d2 = ws.take<float>((size_t)n * sizeof(float));
    c.idx = ws.take<int32_t>((size_t)n * sizeof(int32_t));
    c.total = ws.total();
    return c;
}

inline unsigned blocks_for(int rows) { return (unsigned)(((size_t)rows + kThreads - 1) / kThreads); }

// ---------------------------------------------------------------------------------------------------------- icpflow_pair_row_ids

__device__ __forceinline__ uint32_t key_of(float label) { return icpflow::label_key(icpflow::trust::quieted(label)); }

struct RowIdCarve {
    uint32_t *key;     // [kMaxPairs] ascending
    int32_t *winner;   // [kMaxPairs] the id the rows of that key take
    size_t total;
};

RowIdCarve carve_row_ids(void *base)
{
    RowIdCarve c;
    Carver ws(base);
    c.key = ws.take<uint32_t>((size_t)kMaxPairs * sizeof(uint32_t));
    c.winner = ws.take<int32_t>((size_t)kMaxPairs * sizeof(int32_t));
    c.total = ws.total();
    return c;
}

__global__ __launch_bounds__(kThreads) void prid_table_kernel(const float *__restrict__ pairs, int P, int stride, int col,
                                                              const int32_t *__restrict__ pair_id, const double *__restrict__ weight,
                                                              int weight_stride, uint32_t *__restrict__ key_out, int32_t *__restrict__ winner_out,
                                                              unsigned long long *__restrict__ counts)
{
    __shared__ uint32_t tkey[kPairTile];
    __shared__ int32_t tid[kPairTile];
    __shared__ double tw[kPairTile];
    __shared__ int sh[kWaves][1];
    const int p = blockIdx.x * kThreads + (int)threadIdx.x;
    const bool mine = p < P;
    const uint32_t key = mine ? key_of(pairs[(size_t)p * stride + col]) : 0u;
    int rank = 0, winner = -1;
    double best = 0.0;
    bool shared = false;
    for (int p0 = 0; p0 < P; p0 += kPairTile) {        // (every thread takes every tile: the barriers see whole workgroups)
        const int rows = min(kPairTile, P - p0);
        for (int j = threadIdx.x; j < rows; j += kThreads) {
            const int q = p0 + j;
            const double w = weight != nullptr ? weight[(size_t)q * weight_stride] : 0.0;
            tkey[j] = key_of(pairs[(size_t)q * stride + col]);
            tid[j] = pair_id[q];
            tw[j] = w != w ? -__builtin_huge_val() : w;    // (a NaN weighs least)
        }
        __syncthreads();
        if (mine)
            for (int j = 0; j < rows; ++j) {           // pairs in ascending q: a later one wins by a LARGER weight only
                const int q = p0 + j;
                const uint32_t k = tkey[j];
                rank += (k < key || (k == key && q < p)) ? 1 : 0;
                if (k != key) continue;
                shared = shared || q < p;
                if (tid[j] >= 0 && (winner < 0 || tw[j] > best)) winner = tid[j], best = tw[j];
            }
        __syncthreads();
    }
    if (mine) key_out[rank] = key, winner_out[rank] = winner;    // (the ranks of the P pairs are 0 .. P - 1, each once)
    const bool flag[1] = {mine && shared};
    const int wave = threadIdx.x >> 6;
    const int t = __popcll(__ballot(flag[0]));
    if ((threadIdx.x & (kWave - 1)) == 0) sh[wave][0] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < kWaves; ++w) s += sh[w][0];
        if (s != 0) atomicAdd(&counts[2], (unsigned long long)s);
    }
}

__global__ __launch_bounds__(kThreads) void prid_row_kernel(const float *__restrict__ labels, int n, const uint32_t *__restrict__ key_in,
                                                            const int32_t *__restrict__ winner_in, int P, int32_t *__restrict__ row_id,
                                                            unsigned long long *__restrict__ counts)
{
    __shared__ uint32_t key[kMaxPairs];
    __shared__ int32_t winner[kMaxPairs];
    __shared__ int sh[kWaves][2];
    for (int c = threadIdx.x; c < P; c += kThreads) key[c] = key_in[c], winner[c] = winner_in[c];
    __syncthreads();
    int with = 0, without = 0;                          // the wave's counts (wave-uniform)
    const size_t base = (size_t)blockIdx.x * kRowsBlock;
#pragma unroll
    for (int u = 0; u < kPerThread; ++u) {              // (every lane takes every round: the ballots see whole waves)
        const size_t i = base + (size_t)(u * kThreads) + threadIdx.x;
        const bool live = i < (size_t)n;
        int id = -1;
        if (live) {
            const float label = labels[i];
            if (!(label < 0.0f)) {                      // (a NaN is no negative number, -0.0 neither)
                const uint32_t want = key_of(label);
                int lo = 0, hi = P;                     // the first entry whose key is not below `want`: all entries of a key agree
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (key[mid] < want) lo = mid + 1; else hi = mid;
                }
                if (lo < P && key[lo] == want) id = winner[lo];
            }
            row_id[i] = id;
        }
        with += __popcll(__ballot(live && id >= 0));
        without += __popcll(__ballot(live && id < 0));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & (kWave - 1)) == 0) sh[wave][0] = with, sh[wave][1] = without;
    __syncthreads();
    if (threadIdx.x < 2) {
        int t = 0;
        for (int w = 0; w < kWaves; ++w) t += sh[w][threadIdx.x];
        if (t != 0) atomicAdd(&counts[threadIdx.x], (unsigned long long)t);
    }
}

}  // namespace

extern "C" {

size_t icpflow_rows_carry_workspace_bytes(int n, int m)
{
    if (n < 0 || m < 0 || n > kMaxRows || m > kMaxRows) return 0;
    return carve_carry(nullptr, n, m).total;
}

int icpflow_rows_carry(const float *d_prev, const int32_t *d_prev_id, int m, const double *h_pose, const float *d_next, int n, double radius,
                       double min_share, int32_t *d_id, float *d_d2, int32_t *d_idx, int64_t *d_counts, void *d_ws, size_t ws_bytes,
                       icpflow_stream_t stream)
{
    const char *fn = "icpflow_rows_carry";
    if (n < 0 || m < 0) return report_errorf(ICPFLOW_E_ARG, "icpflow_rows_carry: n = %d, m = %d: a negative size", n, m);
    if (n > kMaxRows || m > kMaxRows)
        return report_errorf(ICPFLOW_E_LIMIT, "icpflow_rows_carry: n = %d, m = %d: at most %d rows a view", n, m, kMaxRows);
    if (!(radius >= kMinRadius && radius <= kMaxRadius))
        return report_errorf(ICPFLOW_E_ARG, "icpflow_rows_carry: radius = %g: the radius must lie in [1e-3, 1e3] metres", radius);
    if (!(min_share >= 0.0 && min_share <= 1.0))
        return report_errorf(ICPFLOW_E_ARG, "icpflow_rows_carry: min_share = %g: min_share must lie in [0, 1]", min_share);
    if (!h_pose || !d_counts || (m > 0 && (!d_prev || !d_prev_id)) || (n > 0 && (!d_next || !d_id))) return pointer_error(fn);
    Move mv;
    for (int k = 0; k < 16; ++k) {
        const float f = (float)h_pose[k];
        if (!std::isfinite(h_pose[k]) || !std::isfinite(f))
            return report_errorf(ICPFLOW_E_ARG, "icpflow_rows_carry: pose[%d] = %g: every entry of the pose must be finite, as a float too", k, h_pose[k]);
        if (k < 12) mv.m[k] = f;
    }
    const size_t need = icpflow_rows_carry_workspace_bytes(n, m);
    if (!d_ws || ws_bytes < need) return workspace_error(fn, "icpflow_rows_carry_workspace_bytes", d_ws, ws_bytes, need);
    if (((uintptr_t)d_ws & 15) != 0) return report_error(ICPFLOW_E_ARG, "icpflow_rows_carry: d_ws must be 16-byte aligned");

    hipStream_t st = (hipStream_t)stream;
    const CarryCarve c = carve_carry(d_ws, n, m);
    const float rf = (float)radius, r2 = rf * rf;
    const double h = 1.01 * radius;
    unsigned long long *counts = (unsigned long long *)d_counts;
    float *d2 = d_d2 ? d_d2 : c.d2;
    int32_t *idx = d_idx ? d_idx : c.idx;
    const unsigned mask = (unsigned)c.targets.H - 1u;

    ICPFLOW_TRY(hipMemsetAsync(counts, 0, kCarryCounts * sizeof(unsigned long long), st));
    ICPFLOW_TRY(hipMemsetAsync(c.targets.cursor, 0, (size_t)c.targets.H * sizeof(unsigned), st));
    if (m > 0) carry_count_kernel<<<blocks_for(m), kThreads, 0, st>>>(d_prev, m, mv, h, mask, c.targets.cursor, counts + 4);
    icpflow::nnr::scan_grid(c.targets, nullptr, st);
    if (m > 0) carry_scatter_kernel<<<blocks_for(m), kThreads, 0, st>>>(d_prev, m, mv, h, mask, c.targets.cursor, c.targets.records);
    ICPFLOW_TRY(hipGetLastError());
    const Cloud queries = {d_next, nullptr, nullptr, n, 1};
    ICPFLOW_TRY(icpflow::nnr::bin_cloud(queries, c.queries, h, counts + 3, nullptr, r2, d2, idx, st));
    ICPFLOW_TRY(icpflow::nnr::launch_binned_query(c.queries, c.targets, n, r2, h, d2, idx, st));
    if (n > 0) {
        carry_gather_kernel<<<blocks_for(n), kThreads, 0, st>>>(idx, d_prev_id, n, d_id, counts);
        ICPFLOW_TRY(hipGetLastError());
    }
    carry_close_kernel<<<n > 0 ? blocks_for(n) : 1u, kThreads, 0, st>>>(n, min_share, d_id, counts);
    ICPFLOW_TRY(hipGetLastError());
    return ICPFLOW_OK;
}

size_t icpflow_pair_row_ids_workspace_bytes(int P)
{
    if (P < 0 || P > kMaxPairs) return 0;
    return carve_row_ids(nullptr).total;
}

int icpflow_pair_row_ids(const float *d_labels, int n, const float *d_pair_rows, int P, int pair_stride, int col, const int32_t *d_pair_id,
                         const double *d_weight, int weight_stride, int32_t *d_row_id, int64_t *d_counts, void *d_ws, size_t ws_bytes,
                         icpflow_stream_t stream)
{
    const char *fn = "icpflow_pair_row_ids";
    if (n < 0 || P < 0) return report_errorf(ICPFLOW_E_ARG, "icpflow_pair_row_ids: n = %d, P = %d: a negative size", n, P);
    if (n > kMaxRows) return report_errorf(ICPFLOW_E_LIMIT, "icpflow_pair_row_ids: n = %d: at most %d rows", n, kMaxRows);
    if (P > kMaxPairs) return report_errorf(ICPFLOW_E_LIMIT, "icpflow_pair_row_ids: P = %d: at most %d pairs", P, kMaxPairs);
    if (col != 0 && col != 1) return report_errorf(ICPFLOW_E_ARG, "icpflow_pair_row_ids: col = %d: col is 0 (the source side) or 1 (the destination side)", col);
    if (pair_stride < 2) return report_errorf(ICPFLOW_E_ARG, "icpflow_pair_row_ids: pair_stride = %d: pair_stride must be at least 2", pair_stride);
    if (d_weight != nullptr && weight_stride < 1)
        return report_errorf(ICPFLOW_E_ARG, "icpflow_pair_row_ids: weight_stride = %d: weight_stride must be at least 1", weight_stride);
    if (!d_counts || (n > 0 && (!d_labels || !d_row_id)) || (P > 0 && (!d_pair_rows || !d_pair_id))) return pointer_error(fn);
    const RowIdCarve c = carve_row_ids(d_ws);
    if (!d_ws || ws_bytes < c.total) return workspace_error(fn, "icpflow_pair_row_ids_workspace_bytes", d_ws, ws_bytes, c.total);
    if (((uintptr_t)d_ws & 15) != 0) return report_error(ICPFLOW_E_ARG, "icpflow_pair_row_ids: d_ws must be 16-byte aligned");

    hipStream_t st = (hipStream_t)stream;
    unsigned long long *counts = (unsigned long long *)d_counts;
    ICPFLOW_TRY(hipMemsetAsync(counts, 0, kRowIdCounts * sizeof(unsigned long long), st));
    if (P > 0) {
        prid_table_kernel<<<(P + kThreads - 1) / kThreads, kThreads, 0, st>>>(d_pair_rows, P, pair_stride, col, d_pair_id, d_weight, weight_stride,
                                                                              c.key, c.winner, counts);
        ICPFLOW_TRY(hipGetLastError());
    }
    if (n > 0) {
        prid_row_kernel<<<(n + kRowsBlock - 1) / kRowsBlock, kThreads, 0, st>>>(d_labels, n, c.key, c.winner, P, d_row_id, counts);
        ICPFLOW_TRY(hipGetLastError());
    }
    return ICPFLOW_OK;
}

}  // extern "C"
