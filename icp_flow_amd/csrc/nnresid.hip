// nnresid.hip -- the truncated nearest-neighbour residual of one cloud against another on the GPU (include/icpflow_hip.h,
// "8(g) nearest-neighbour residual", icpflow_nn_residual): a hashed uniform grid over a WHOLE frame (60 - 130 k points), built by
// as many workgroups as the frame needs, an exact radius-bounded K = 1 query over it, and a small table of the distances per
// group of query rows.  icpflow_nn_batch is an all-pairs scan for B cluster pairs; the ICP's grid (gridhash.hpp, icp_prep.hip)
// is built per pair inside one workgroup; neither reaches a frame.
//
// The arithmetic, in the order it is done (the file is compiled with -ffp-contract=off, build.py: CFLAGS, so nothing below
// fuses; every operation is one correctly rounded IEEE operation):
//   q   = p + f                               one fp32 addition per coordinate (f absent: q = p)
//   r2  = (float)r * (float)r                 rounded once, on the host
//   dx  = q.x - t.x, dy, dz alike             fp32
//   d2  = (dx * dx + dy * dy) + dz * dz       fp32: three products, the x and y products added first, then z
//   hit = d2 <= r2
//   a query's d2_out is the smallest d2 among its hits and idx_out the LOWEST target row that attains it; without a hit
//   idx_out = -1 and d2_out = r2.  Both are functions of the arguments alone: the minimum over a set and the lowest row among
//   equals do not depend on the order in which the scatter left the records inside a bucket.
//   d   = sqrtf(d2_out)                       fp32, correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt), widened to
//                                             fp64 for the table; the table's second sum takes (double)d * (double)d, which is
//                                             exact in fp64
// A row is BAD when a coordinate is not finite or lies beyond +-1e6 m (for a query: a coordinate of q), or when its group is
// outside [0, G).  A bad target enters no bucket; a bad query gets idx_out = -2, d2_out = r2 and enters no cell of the table.
//
// The grid.  Cell edge h = 1.01 r in fp64; the cell of a coordinate v is floor((double)v / h), one IEEE fp64 division.
//   * the index fits: |v| <= 1e6 and r >= 1e-3 give |v / h| <= 1e6 / 1.01e-3 < 9.91e8 < 2^30, so the index and its two
//     neighbours are ints;
//   * every hit lies in the 27 cells around the query.  Let a, b be one coordinate of q and t with d2 <= r2.  The three
//     squares are non-negative, so fl(dx * dx) <= d2 up to the two additions' roundings, and with dx = fl(a - b):
//     |a - b| <= sqrt(r2) (1 + 2^-24)^(5/2) <= r (1 + 2^-24)^3 < 1.000001 r  (a product that underflows belongs to an
//     |a - b| below 1e-18, far inside the same bound).  In exact arithmetic |a / h - b / h| < 1.000001 / 1.01 < 0.9901; each
//     fp64 quotient is off by at most 2^-53 * 9.91e8 < 1.2e-7; so the two computed quotients differ by less than 1 and their
//     floors by at most one cell;
//   * the fp32 form of the ICP's grid, floorf((v - o) * invh), does not carry over to these magnitudes: an fp32 product of
//     magnitude c is rounded by up to c * 2^-24 cells, which is a sixteenth of a cell from 10^6 cells on and 64 whole cells at
//     the 10^9 cells this grid reaches (the ICP's clouds span a few hundred cells); the margin between r and h is one
//     hundredth of a cell.
// Buckets: H = 2^k >= 2 m, the bucket of a cell is gridhash.hpp's grid_hash.  Distinct cells may share a bucket: a record of a
// foreign cell is evaluated like any other (the hit test rejects it, or it is a legitimate hit), and a bucket that two of a
// query's 27 cells share is scanned once -- a cell whose bucket an earlier one of the 27 already named is left out.
//
// Kernels, all on the caller's stream:
//   1. nnr_count_kernel     a thread per target: the good targets counted per bucket (integer atomics: counts are order-free),
//                           the bad ones counted into d_info[1];
//   2. nnr_tile_kernel      a workgroup per tile of 1024 buckets: the tile's total, its occupied buckets, its longest bucket;
//   3. nnr_offsets_kernel   one workgroup: the exclusive scan of the tiles' totals (rounds of 256 with a carry), and d_info[2..3];
//   4. nnr_starts_kernel    a workgroup per tile: the exclusive scan inside the tile on top of the tile's offset -> where each
//                           bucket starts; the count word becomes the bucket's cursor;
//   5. nnr_scatter_kernel   a thread per target: (x, y, z, row) to the slot an atomic increment of the cursor hands out; after
//                           it the cursor is the bucket's end;
//      1 - 5 once more on the QUERIES (q = p + f, a table of H' = 2^k >= 2 n buckets of the same cells): the queries in the
//      order of their buckets; a bad query is counted into d_info[0] and gets its outputs from the scatter;
//   6. nnr_query_kernel     the BINNED form: a workgroup per 64 good queries in bucket order, so that its lanes sit in one cell
//                           or a few and walk the same buckets; a wave loads 64 target records at a time, coalesced, and hands
//                           them round by v_readlane; the workgroup's eight waves share each bucket's pieces and merge their
//                           candidates in LDS; every loop bound is wave-uniform.  (The first form, a lane per query in row
//                           order, is kept behind -DICPFLOW_NNR_LANE_QUERY for the timing tool: the same bits; on the demo
//                           frame at r = 2 m its waves wait for their lane in the densest cell and gather 64 scattered records
//                           per step -- COVERAGE.md row 13 has the figures of both.)
//   7. nnr_table_kernel, nnr_table_final_kernel   the table, by bucketeval.hip's scheme item by item: the grid follows from n
//                           alone, the waves walk 64-row tiles in rounds, the groups of a tile are taken in the order of their
//                           first row, counts by ballot and popcount, the two sums through one fixed butterfly (wave_sum), the
//                           round's records applied to the workgroup's LDS table in (wave, record) order, the workgroups'
//                           tables added in workgroup order by a thread per word.  No floating-point atomic anywhere.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.hpp"
#include "gridhash.hpp"
#include "host.hpp"
#include "nnresid.hpp"
#include "rowerr.hpp"

using icpflow::align256;
using icpflow::Carver;
using icpflow::kWave;
using icpflow::pointer_error;
using icpflow::report_error;
using icpflow::report_errorf;
using icpflow::workspace_error;
using icpflow::nnr::Cloud;
using icpflow::nnr::Edges;
using icpflow::nnr::Grid;
using icpflow::nnr::kMaxEdges;
using icpflow::nnr::kMaxRows;
using icpflow::nnr::kMaxRadius;
using icpflow::nnr::kMinRadius;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kTile = 1024;                         // buckets per scan tile: four per thread
constexpr int kPerThread = kTile / kThreads;
constexpr int kMaxGroups = ICPFLOW_NNR_MAX_GROUPS;  // (the limits both entry points share: nnresid.hpp)
using icpflow::nnr::good_coord;                     // (nnresid.hpp: a coordinate beyond 1e6 m is a bad row)

using icpflow::nnr::cell_of;                        // (nnresid.hpp: floor((double)v / h), one fp64 division)

// row j of the cloud -> its coordinates; false for a bad row
__device__ __forceinline__ bool load_row(const Cloud &c, size_t j, float &x, float &y, float &z)
{
    x = c.pts[3 * j + 0], y = c.pts[3 * j + 1], z = c.pts[3 * j + 2];
    if (c.flow) x = x + c.flow[3 * j + 0], y = y + c.flow[3 * j + 1], z = z + c.flow[3 * j + 2];
    const int g = c.group ? c.group[j] : 0;
    return good_coord(x, y, z) && g >= 0 && g < c.G;
}

__global__ __launch_bounds__(kThreads) void nnr_count_kernel(Cloud c, double h, unsigned mask, unsigned *__restrict__ cursor,
                                                             unsigned long long *__restrict__ bad_rows)
{
    const size_t j = (size_t)blockIdx.x * kThreads + threadIdx.x;
    bool bad = false;
    if (j < (size_t)c.rows) {
        float x, y, z;
        if (load_row(c, j, x, y, z)) atomicAdd(cursor + icpflow::grid_hash(cell_of(x, h), cell_of(y, h), cell_of(z, h), mask), 1u);
        else bad = true;
    }
    const unsigned long long n_bad = __popcll(__ballot(bad));
    if ((threadIdx.x & (kWave - 1)) == 0 && n_bad) atomicAdd(bad_rows, n_bad);
}

// the workgroup's sum of one unsigned per thread, wave by wave in wave order; every thread gets it (all threads call it)
__device__ __forceinline__ unsigned block_sum(unsigned v, unsigned *part)
{
    v = icpflow::wave_sum(v);
    __syncthreads();                                // (the previous use of part[] is over)
    if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned s = 0;
    for (int w = 0; w < kWaves; ++w) s += part[w];
    return s;
}

__device__ __forceinline__ unsigned block_max(unsigned v, unsigned *part)
{
    for (int o = kWave / 2; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, kWave));
    __syncthreads();
    if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned s = 0;
    for (int w = 0; w < kWaves; ++w) s = max(s, part[w]);
    return s;
}

// the exclusive prefix of one unsigned per thread in thread order, `total` the workgroup's sum (all threads call it)
__device__ __forceinline__ unsigned block_exclusive(unsigned v, unsigned *part, unsigned &total)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    unsigned inc = v;
    for (int o = 1; o < kWave; o <<= 1) {
        const unsigned up = (unsigned)__shfl_up((int)inc, o, kWave);
        if (lane >= o) inc += up;
    }
    __syncthreads();
    if (lane == kWave - 1) part[wave] = inc;
    __syncthreads();
    unsigned before = 0;
    total = 0;
    for (int w = 0; w < kWaves; ++w) {
        if (w < wave) before += part[w];
        total += part[w];
    }
    return before + inc - v;
}

__global__ __launch_bounds__(kThreads) void nnr_tile_kernel(const unsigned *__restrict__ cursor, int H, unsigned *__restrict__ tile_sum,
                                                            unsigned *__restrict__ tile_occupied, unsigned *__restrict__ tile_longest)
{
    __shared__ unsigned part[kWaves];
    const size_t b0 = (size_t)blockIdx.x * kTile + (size_t)threadIdx.x * kPerThread;
    unsigned sum = 0, occupied = 0, longest = 0;
    for (int k = 0; k < kPerThread; ++k) {
        const unsigned c = b0 + k < (size_t)H ? cursor[b0 + k] : 0u;
        sum += c, occupied += c ? 1u : 0u, longest = max(longest, c);
    }
    sum = block_sum(sum, part);
    occupied = block_sum(occupied, part);
    longest = block_max(longest, part);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = sum, tile_occupied[blockIdx.x] = occupied, tile_longest[blockIdx.x] = longest;
}

__global__ __launch_bounds__(kThreads) void nnr_offsets_kernel(const unsigned *__restrict__ tile_sum, const unsigned *__restrict__ tile_occupied,
                                                               const unsigned *__restrict__ tile_longest, int tiles,
                                                               unsigned *__restrict__ tile_offset, unsigned *__restrict__ total_rows,
                                                               unsigned long long *__restrict__ d_info)
{
    __shared__ unsigned part[kWaves];
    unsigned carry = 0, occupied = 0, longest = 0;
    for (int t0 = 0; t0 < tiles; t0 += kThreads) {              // (uniform over the workgroup)
        const int t = t0 + threadIdx.x;
        unsigned total;
        const unsigned before = block_exclusive(t < tiles ? tile_sum[t] : 0u, part, total);
        if (t < tiles) {
            tile_offset[t] = carry + before;
            occupied += tile_occupied[t];
            longest = max(longest, tile_longest[t]);
        }
        carry += total;
    }
    occupied = block_sum(occupied, part);
    longest = block_max(longest, part);
    if (threadIdx.x == 0) {
        *total_rows = carry;                                    // the rows in the table: the good ones
        if (d_info) d_info[2] = occupied, d_info[3] = longest;
    }
}

__global__ __launch_bounds__(kThreads) void nnr_starts_kernel(unsigned *__restrict__ cursor, int H, const unsigned *__restrict__ tile_offset,
                                                              unsigned *__restrict__ start)
{
    __shared__ unsigned part[kWaves];
    const size_t b0 = (size_t)blockIdx.x * kTile + (size_t)threadIdx.x * kPerThread;
    unsigned c[kPerThread], mine = 0;
    for (int k = 0; k < kPerThread; ++k) {
        c[k] = b0 + k < (size_t)H ? cursor[b0 + k] : 0u;
        mine += c[k];
    }
    unsigned total;
    unsigned at = tile_offset[blockIdx.x] + block_exclusive(mine, part, total);
    for (int k = 0; k < kPerThread; ++k) {
        if (b0 + k < (size_t)H) start[b0 + k] = at, cursor[b0 + k] = at;
        at += c[k];
    }
}

// (x, y, z, row) of every good row to its bucket; the queries' bad rows get their outputs here (d2_out NULL: the targets)
__global__ __launch_bounds__(kThreads) void nnr_scatter_kernel(Cloud c, double h, unsigned mask, unsigned *__restrict__ cursor,
                                                               float4 *__restrict__ records, float r2, float *__restrict__ d2_out,
                                                               int32_t *__restrict__ idx_out)
{
    const size_t j = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= (size_t)c.rows) return;
    float x, y, z;
    if (!load_row(c, j, x, y, z)) {
        if (d2_out) d2_out[j] = r2, idx_out[j] = -2;
        return;
    }
    const unsigned slot = atomicAdd(cursor + icpflow::grid_hash(cell_of(x, h), cell_of(y, h), cell_of(z, h), mask), 1u);   // < rows: the counts' scan
    records[slot] = make_float4(x, y, z, __int_as_float((int)j));
}

#ifndef ICPFLOW_NNR_LANE_QUERY
__device__ __forceinline__ float lane_value(float v, unsigned lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)lane)); }

// The query, BINNED: workgroup b takes the good queries 64 b ... 64 b + 63 in the order of their buckets (`queries`: the scatter
// above on the query cloud), one per lane, so the lanes sit in one cell or a few.  Cell by cell, in the order of the cells' first
// lanes: lanes 0 .. 26 name the buckets of the 27 cells around it (a bucket an earlier lane names is left out) and fetch their
// bounds, then a wave loads 64 records of a bucket at a time, one per lane and coalesced, and every lane of the cell weighs the
// 64 in turn (the record handed round by v_readlane).  Every loop bound is wave-uniform: no lane waits for another's longer
// bucket.  The kQueryWaves waves of the workgroup hold the SAME 64 queries and share every bucket's 64-record pieces round
// robin -- a frame has fewer 64-query groups than the device has SIMDs, and the groups of a crowded cell walk tens of thousands
// of records --; their (d2, row) candidates meet in LDS under the rule every step uses: smaller d2, then the lower row.
constexpr int kQueryWaves = 8;

__global__ __launch_bounds__(kQueryWaves * kWave) void nnr_query_kernel(const float4 *__restrict__ queries, const unsigned *__restrict__ good_queries,
                                                                        float r2, double h, unsigned mask, const unsigned *__restrict__ start,
                                                                        const unsigned *__restrict__ end, const float4 *__restrict__ records,
                                                                        float *__restrict__ d2_out, int32_t *__restrict__ idx_out)
{
    __shared__ float best_of[kQueryWaves][kWave];
    __shared__ int at_of[kQueryWaves][kWave];
    const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const size_t at_row = (size_t)blockIdx.x * kWave + lane;
    const bool active = at_row < (size_t)*good_queries;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    int row = 0, cx = 0, cy = 0, cz = 0;
    if (active) {
        const float4 q = queries[at_row];
        qx = q.x, qy = q.y, qz = q.z, row = __float_as_int(q.w);
        cx = cell_of(qx, h), cy = cell_of(qy, h), cz = cell_of(qz, h);
    }
    float best = r2;
    int at = -1;
    unsigned long long todo = __ballot(active);
    while (todo) {                                                 // the cells of the 64 queries, in the order of their first lanes
        const int leader = __ffsll((long long)todo) - 1;
        const int lx = __shfl(cx, leader, kWave), ly = __shfl(cy, leader, kWave), lz = __shfl(cz, leader, kWave);
        const bool mine = active && cx == lx && cy == ly && cz == lz;
        todo &= ~__ballot(mine);
        // lane k < 27: cell k of the 27 (x offset k / 9 - 1, y (k / 3) % 3 - 1, z k % 3 - 1), its bucket, and the bucket's bounds
        // unless an earlier lane names the same bucket
        const unsigned bucket = icpflow::grid_hash(lx + (int)lane / 9 - 1, ly + ((int)lane / 3) % 3 - 1, lz + (int)lane % 3 - 1, mask);
        bool first = lane < 27;
        for (unsigned j = 0; j < 26; ++j) {
            const unsigned other = (unsigned)__shfl((int)bucket, (int)j, kWave);
            first = first && !(j < lane && other == bucket);
        }
        unsigned lo = 0, hi = 0;
        if (first) lo = start[bucket], hi = end[bucket];
        for (int k = 0; k < 27; ++k) {
            const unsigned s = (unsigned)__builtin_amdgcn_readlane((int)lo, k), e = (unsigned)__builtin_amdgcn_readlane((int)hi, k);
            for (unsigned base = s + wave * kWave; base < e; base += kQueryWaves * kWave) {     // (wave-uniform) this wave's pieces
                const unsigned count = min((unsigned)kWave, e - base);
                float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
                if (lane < count) t = records[base + lane];
                for (unsigned j = 0; j < count; ++j) {
                    const float dx = qx - lane_value(t.x, j), dy = qy - lane_value(t.y, j), dz = qz - lane_value(t.z, j);
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    const int target = __float_as_int(lane_value(t.w, j));
                    if (mine && d2 <= r2 && (at < 0 || d2 < best || (d2 == best && target < at))) best = d2, at = target;
                }
            }
        }
    }
    best_of[wave][lane] = best, at_of[wave][lane] = at;
    __syncthreads();
    if (wave == 0 && active) {
        for (int w = 1; w < kQueryWaves; ++w) {
            const float d2 = best_of[w][lane];
            const int target = at_of[w][lane];
            if (target >= 0 && (at < 0 || d2 < best || (d2 == best && target < at))) best = d2, at = target;
        }
        d2_out[row] = best, idx_out[row] = at;
    }
}
#else
// A lane per query.  `start` and `end` (the cursors after the scatter) bound the records of a bucket.
__global__ __launch_bounds__(kThreads) void nnr_query_kernel(const float *__restrict__ qr, const float *__restrict__ flow, int n,
                                                             const int32_t *__restrict__ group, int G, float r2, double h, unsigned mask,
                                                             const unsigned *__restrict__ start, const unsigned *__restrict__ end,
                                                             const float4 *__restrict__ records, float *__restrict__ d2_out,
                                                             int32_t *__restrict__ idx_out, unsigned long long *__restrict__ d_info)
{
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    bool bad = false;
    if (i < (size_t)n) {
        float qx = qr[3 * i + 0], qy = qr[3 * i + 1], qz = qr[3 * i + 2];
        if (flow) qx = qx + flow[3 * i + 0], qy = qy + flow[3 * i + 1], qz = qz + flow[3 * i + 2];
        const int g = group ? group[i] : 0;
        bad = !good_coord(qx, qy, qz) || g < 0 || g >= G;
        float best = r2;
        int at = bad ? -2 : -1;
        if (!bad) {
            const int cx = cell_of(qx, h), cy = cell_of(qy, h), cz = cell_of(qz, h);
            // the cells of the 27 whose bucket no earlier one names (cell k: x offset k / 9 - 1, y (k / 3) % 3 - 1, z k % 3 - 1)
            unsigned bucket[27];
#pragma unroll
            for (int k = 0; k < 27; ++k) bucket[k] = icpflow::grid_hash(cx + k / 9 - 1, cy + (k / 3) % 3 - 1, cz + k % 3 - 1, mask);
            unsigned todo = 0;
#pragma unroll
            for (int k = 0; k < 27; ++k) {
                bool seen = false;
#pragma unroll
                for (int j = 0; j < k; ++j) seen |= bucket[j] == bucket[k];
                todo |= seen ? 0u : 1u << k;
            }
            while (todo) {
                const int k = __ffs((int)todo) - 1;
                todo &= todo - 1;
                const unsigned b = icpflow::grid_hash(cx + k / 9 - 1, cy + (k / 3) % 3 - 1, cz + k % 3 - 1, mask);
                const unsigned hi = end[b];
                for (unsigned s = start[b]; s < hi; ++s) {
                    const float4 t = records[s];
                    const float dx = qx - t.x, dy = qy - t.y, dz = qz - t.z;
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    const int row = __float_as_int(t.w);
                    if (d2 <= r2 && (at < 0 || d2 < best || (d2 == best && row < at))) best = d2, at = row;
                }
            }
        }
        d2_out[i] = best;
        idx_out[i] = at;
    }
    const unsigned long long n_bad = __popcll(__ballot(bad));
    if ((threadIdx.x & (kWave - 1)) == 0 && n_bad) atomicAdd(d_info + 0, n_bad);
}
#endif

__device__ __forceinline__ unsigned long long add_bits(unsigned long long bits, double v)
{
    return (unsigned long long)__double_as_longlong(__longlong_as_double((long long)bits) + v);
}

// The table of a workgroup: [group][rows, hits, E counts, bits of the sum of d, bits of the sum of d * d].
__global__ __launch_bounds__(kThreads) void nnr_table_kernel(const float *__restrict__ d2_in, const int32_t *__restrict__ idx_in,
                                                             const int32_t *__restrict__ group, int n, int G, Edges ed,
                                                             unsigned long long *__restrict__ partial)
{
    __shared__ unsigned long long table[kMaxGroups * (kMaxEdges + 4)];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int pitch = ed.E + 4, words = G * pitch;
    for (int k = threadIdx.x; k < words; k += kThreads) table[k] = 0;   // (the bits of +0.0 are zero too)
    __syncthreads();

    const size_t tiles = ((size_t)n + kWave - 1) / kWave;
    const size_t W = (size_t)gridDim.x * kWaves;
    const size_t rounds = (tiles + W - 1) / W;                    // uniform over the grid
    for (size_t round = 0; round < rounds; ++round) {
        const size_t tile = round * W + (size_t)blockIdx.x * kWaves + wave;
        int records = 0;                                          // wave-uniform
        int my_group = 0;                                         // lane k: record k of the tile
        unsigned long long my_n = 0, my_hits = 0, my_under[kMaxEdges] = {0, 0, 0, 0};
        double my_d = 0.0, my_dd = 0.0;
        if (tile < tiles) {                                       // (wave-uniform)
            const size_t i = tile * kWave + lane;
            bool counted = false, hit = false;
            int g = 0;
            double d = 0.0;
            if (i < (size_t)n) {
                const int at = idx_in[i];
                counted = at != -2;
                hit = at >= 0;
                if (counted) {
                    g = group ? group[i] : 0;
                    d = (double)sqrtf(d2_in[i]);
                }
            }
            unsigned long long todo = __ballot(counted);
            while (todo) {                                         // the groups of the tile, in the order of their first row
                const int leader = __ffsll((long long)todo) - 1;
                const int j = __shfl(g, leader, kWave);
                const bool mine = counted && g == j;
                const unsigned long long rows = __ballot(mine);
                todo &= ~rows;
                const unsigned long long hits = __popcll(__ballot(mine && hit));
                unsigned long long under[kMaxEdges];
#pragma unroll
                for (int e = 0; e < kMaxEdges; ++e) under[e] = __popcll(__ballot(mine && e < ed.E && d <= ed.edge[e]));
                const double sum_d = icpflow::wave_sum(mine ? d : 0.0), sum_dd = icpflow::wave_sum(mine ? d * d : 0.0);
                if (lane == records) {
                    my_group = j, my_n = __popcll(rows), my_hits = hits, my_d = sum_d, my_dd = sum_dd;
#pragma unroll
                    for (int e = 0; e < kMaxEdges; ++e) my_under[e] = under[e];
                }
                ++records;
            }
        }
        for (int w = 0; w < kWaves; ++w) {                        // the round's records in (wave, record) order
            if (wave == w && lane < records) {
                unsigned long long *v = table + (size_t)my_group * pitch;
                v[0] += my_n;
                v[1] += my_hits;
#pragma unroll
                for (int e = 0; e < kMaxEdges; ++e)
                    if (e < ed.E) v[2 + e] += my_under[e];
                v[2 + ed.E] = add_bits(v[2 + ed.E], my_d);
                v[3 + ed.E] = add_bits(v[3 + ed.E], my_dd);
            }
            __syncthreads();
        }
    }
    unsigned long long *mine = partial + (size_t)blockIdx.x * words;
    for (int k = threadIdx.x; k < words; k += kThreads) mine[k] = table[k];
}

// A thread per word: the partials of the word in workgroup order.
__global__ __launch_bounds__(kThreads) void nnr_table_final_kernel(const unsigned long long *__restrict__ partial, int grid, int words, int pitch,
                                                                   unsigned long long *__restrict__ table)
{
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= words) return;
    const bool is_sum = (k % pitch) >= pitch - 2;
    unsigned long long acc = 0;
    double accd = 0.0;
    for (int g = 0; g < grid; ++g) {
        const unsigned long long v = partial[(size_t)g * words + k];
        if (is_sum) accd += __longlong_as_double((long long)v);
        else acc += v;
    }
    table[k] = is_sum ? (unsigned long long)__double_as_longlong(accd) : acc;
}

int buckets_for(int m)   // H = 2^k >= 2 m (1 for an empty cloud)
{
    int H = 1;
    while (H < 2 * (long long)m) H <<= 1;
    return H;
}

inline unsigned blocks_for(int rows) { return (unsigned)(((size_t)rows + kThreads - 1) / kThreads); }

}  // namespace

// what segresid.hip calls as well (nnresid.hpp)
namespace icpflow {
namespace nnr {

Grid carve_grid(Carver &ws, int rows)
{
    Grid g;
    g.H = buckets_for(rows);
    g.tiles = (g.H + kTile - 1) / kTile;
    g.cursor = ws.take<unsigned>((size_t)g.H * sizeof(unsigned));
    g.start = ws.take<unsigned>((size_t)g.H * sizeof(unsigned));
    g.tile_sum = ws.take<unsigned>((size_t)g.tiles * sizeof(unsigned));
    g.tile_occupied = ws.take<unsigned>((size_t)g.tiles * sizeof(unsigned));
    g.tile_longest = ws.take<unsigned>((size_t)g.tiles * sizeof(unsigned));
    g.tile_offset = ws.take<unsigned>((size_t)g.tiles * sizeof(unsigned));
    g.rows = ws.take<unsigned>(sizeof(unsigned));
    g.records = ws.take<float4>((size_t)rows * sizeof(float4));
    return g;
}

void scan_grid(const Grid &g, unsigned long long *d_info, hipStream_t st)
{
    nnr_tile_kernel<<<g.tiles, kThreads, 0, st>>>(g.cursor, g.H, g.tile_sum, g.tile_occupied, g.tile_longest);
    nnr_offsets_kernel<<<1, kThreads, 0, st>>>(g.tile_sum, g.tile_occupied, g.tile_longest, g.tiles, g.tile_offset, g.rows, d_info);
    nnr_starts_kernel<<<g.tiles, kThreads, 0, st>>>(g.cursor, g.H, g.tile_offset, g.start);
}

hipError_t bin_cloud(const Cloud &cloud, const Grid &g, double h, unsigned long long *bad_rows, unsigned long long *d_info, float r2,
                     float *d2, int32_t *idx, hipStream_t st)
{
    const unsigned mask = (unsigned)g.H - 1u;
    hipError_t e = hipMemsetAsync(g.cursor, 0, (size_t)g.H * sizeof(unsigned), st);
    if (e != hipSuccess) return e;
    if (cloud.rows > 0) nnr_count_kernel<<<blocks_for(cloud.rows), kThreads, 0, st>>>(cloud, h, mask, g.cursor, bad_rows);
    scan_grid(g, d_info, st);
    if (cloud.rows > 0) nnr_scatter_kernel<<<blocks_for(cloud.rows), kThreads, 0, st>>>(cloud, h, mask, g.cursor, g.records, r2, d2, idx);
    return hipGetLastError();
}

// the queries binned by the same cells (a table of their own size), then a workgroup per 64 of them in bucket order
hipError_t launch_binned_query(const Grid &queries, const Grid &targets, int n, float r2, double h, float *d2, int32_t *idx, hipStream_t st)
{
#ifndef ICPFLOW_NNR_LANE_QUERY
    if (n <= 0) return hipSuccess;
    nnr_query_kernel<<<(unsigned)(((size_t)n + kWave - 1) / kWave), kQueryWaves * kWave, 0, st>>>(queries.records, queries.rows, r2, h, (unsigned)targets.H - 1u,
                                                                                             targets.start, targets.cursor, targets.records, d2, idx);
    return hipGetLastError();
#else
    return hipErrorNotSupported;                    // (the timing variant has the lane-per-query kernel only)
#endif
}

}  // namespace nnr
}  // namespace icpflow

namespace {

using icpflow::nnr::bin_cloud;
using icpflow::nnr::carve_grid;

// what the call carves out of its workspace, in this order (the size query runs it on a null base): the targets' grid, the
// queries' grid, the per-row outputs the caller did not take, the table's partials
struct Carve {
    Grid targets, queries;
    float *d2;
    int32_t *idx;
    unsigned long long *partial;
    int grid;
    size_t total;
};

Carve carve(void *base, int n, int m, int G, int E)
{
    Carve c;
    Carver ws(base);
    c.targets = carve_grid(ws, m);
    c.queries = carve_grid(ws, n);
    c.grid = icpflow::table_grid(n);
    c.d2 = ws.take<float>((size_t)n * sizeof(float));
    c.idx = ws.take<int32_t>((size_t)n * sizeof(int32_t));
    c.partial = ws.take<unsigned long long>((size_t)c.grid * G * (E + 4) * sizeof(unsigned long long));
    c.total = ws.total();
    return c;
}

bool sizes_ok(int n, int m, int G, int E) { return n >= 0 && m >= 0 && n <= kMaxRows && m <= kMaxRows && G >= 1 && G <= kMaxGroups && E >= 0 && E <= kMaxEdges; }

}  // namespace

extern "C" {

size_t icpflow_nn_residual_workspace_bytes(int n, int m, int G, int E)
{
    if (!sizes_ok(n, m, G, E)) return 0;
    return carve(nullptr, n, m, G, E).total;
}

int icpflow_nn_residual(const float *d_query, const float *d_flow, int n, const float *d_target, int m, double radius,
                        const int32_t *d_group, int G, const double *h_edges, int E, float *d_d2_out, int32_t *d_idx_out,
                        int64_t *d_table, int64_t *d_info, void *d_ws, size_t ws_bytes, icpflow_stream_t stream)
{
    const char *fn = "icpflow_nn_residual";
    if (n < 0 || m < 0) return report_error(ICPFLOW_E_ARG, "icpflow_nn_residual: n < 0 or m < 0");
    if (n > kMaxRows || m > kMaxRows)
        return report_errorf(ICPFLOW_E_LIMIT, "icpflow_nn_residual: n = %d, m = %d: at most %d rows a cloud (twice as many buckets are indexed by an int)", n, m, kMaxRows);
    if (!(radius >= kMinRadius && radius <= kMaxRadius))
        return report_errorf(ICPFLOW_E_ARG, "icpflow_nn_residual: radius = %g: the radius must lie in [1e-3, 1e3] metres", radius);
    if (G < 1 || G > kMaxGroups) return report_errorf(ICPFLOW_E_ARG, "icpflow_nn_residual: G = %d: G must lie in [1, %d]", G, kMaxGroups);
    if (E < 0 || E > kMaxEdges) return report_errorf(ICPFLOW_E_ARG, "icpflow_nn_residual: E = %d: E must lie in [0, %d]", E, kMaxEdges);
    if (!d_info || (E > 0 && !h_edges) || (n > 0 && !d_query) || (m > 0 && !d_target)) return pointer_error(fn);
    if (!d_d2_out && !d_idx_out && !d_table) return report_error(ICPFLOW_E_ARG, "icpflow_nn_residual: d_d2_out, d_idx_out and d_table are all NULL: nothing to compute");
    if (!icpflow::edges_ok(h_edges, E) || (E > 0 && (!(h_edges[0] > 0.0) || !(h_edges[E - 1] <= radius))))
        return report_error(ICPFLOW_E_ARG, "icpflow_nn_residual: the edges must be finite, positive, strictly ascending and at most the radius");
    const size_t need = icpflow_nn_residual_workspace_bytes(n, m, G, E);
    if (!d_ws || ws_bytes < need) return workspace_error(fn, "icpflow_nn_residual_workspace_bytes", d_ws, ws_bytes, need);
    if (((uintptr_t)d_ws & 15) != 0) return report_error(ICPFLOW_E_ARG, "icpflow_nn_residual: d_ws must be 16-byte aligned");

    hipStream_t st = (hipStream_t)stream;
    const Carve c = carve(d_ws, n, m, G, E);
    const float rf = (float)radius, r2 = rf * rf;
    const double h = 1.01 * radius;
#ifdef ICPFLOW_NNR_LANE_QUERY
    const unsigned mask = (unsigned)c.targets.H - 1u;
#endif
    unsigned long long *info = (unsigned long long *)d_info;
    float *d2 = d_d2_out ? d_d2_out : c.d2;
    int32_t *idx = d_idx_out ? d_idx_out : c.idx;
    const Cloud targets = {d_target, nullptr, nullptr, m, 1};
    const Cloud queries = {d_query, d_flow, d_group, n, G};

    ICPFLOW_TRY(hipMemsetAsync(info, 0, 4 * sizeof(unsigned long long), st));
    ICPFLOW_TRY(bin_cloud(targets, c.targets, h, info + 1, info, r2, nullptr, nullptr, st));
#ifndef ICPFLOW_NNR_LANE_QUERY
    ICPFLOW_TRY(bin_cloud(queries, c.queries, h, info + 0, nullptr, r2, d2, idx, st));
    ICPFLOW_TRY(icpflow::nnr::launch_binned_query(c.queries, c.targets, n, r2, h, d2, idx, st));
#else
    if (n > 0) {
        nnr_query_kernel<<<blocks_for(n), kThreads, 0, st>>>(d_query, d_flow, n, d_group, G, r2, h, mask, c.targets.start, c.targets.cursor,
                                                             c.targets.records, d2, idx, info);
        ICPFLOW_TRY(hipGetLastError());
    }
#endif
    if (d_table) {
        Edges ed;
        ed.E = E;
        for (int k = 0; k < kMaxEdges; ++k) ed.edge[k] = k < E ? h_edges[k] : 0.0;
        const int words = G * (E + 4);
        nnr_table_kernel<<<c.grid, kThreads, 0, st>>>(d2, idx, d_group, n, G, ed, c.partial);
        ICPFLOW_TRY(hipGetLastError());
        nnr_table_final_kernel<<<(words + kThreads - 1) / kThreads, kThreads, 0, st>>>(c.partial, c.grid, words, E + 4, (unsigned long long *)d_table);
        ICPFLOW_TRY(hipGetLastError());
    }
    return ICPFLOW_OK;
}

}  // extern "C"
