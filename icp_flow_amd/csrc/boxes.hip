// boxes.hip -- an oriented box per segment of a labelled cloud and one object row per matched pair (include/icpflow_hip.h,
// "8(j) object boxes": icpflow_segment_boxes, icpflow_pair_objects).  The box of a segment is the bounding rectangle, among
// the caller's A directions, that has the most rows within `delta` of one of its sides -- an exact integer, so the choice does
// not depend on the order of the rows; ties go to the smaller float32 area, then to the lower direction.
//
// icpflow_segment_boxes, five launches on the caller's stream, the segments cut into chunks of 1024 rows of the stable order
// (segeval.hip's scheme; the plan here skips the segments with a negative label and clips what a table claims to n):
//   1. box_plan_kernel     one workgroup: chunkStart[c] = the first chunk of segment c, chunkStart[L] = the number of chunks
//   2. box_extent_kernel   a workgroup of 256 per chunk, thread t rows t, t + 256, t + 512, t + 768, gathered once through
//                          d_order into registers; per direction the four extrema through a wave reduction and, across the
//                          four waves, through LDS -> partial[chunk][k]; z's extrema and the good rows beside them
//   3. box_fold_kernel     one thread per (segment, direction): the chunks of the segment folded; near[segment][k] = 0
//   4. box_near_kernel     the chunks again, the same gather, the same u and v: rows within delta of a side, by ballot and
//                          popcount, one integer atomic per (segment, direction) and wave
//   5. box_final_kernel    one thread per segment: the best direction, the row of d_boxes
// Minima, maxima and integer sums do not depend on their order, no floating-point atomic anywhere: every number is a function
// of the arguments alone.  Every partial a later kernel reads was written by an earlier one of the same call.
//
// icpflow_pair_objects: one thread per pair, a label's segment by binary search on label_key (labelkey.hpp), counts by ballot
// and popcount.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "boxes.hpp"
#include "common.hpp"
#include "host.hpp"

using icpflow::kInf;
using icpflow::kWave;
using icpflow::pointer_error;
using icpflow::report_error;
using icpflow::report_errorf;
using icpflow::workspace_error;
using icpflow::boxes::Dirs;
using icpflow::boxes::kBoxCols;
using icpflow::boxes::kChunk;
using icpflow::boxes::kCounts;
using icpflow::boxes::kLmax;
using icpflow::boxes::kMaxDirs;
using icpflow::boxes::kMaxRows;
using icpflow::boxes::kObjectCols;
using icpflow::boxes::kOrderCols;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kPerThread = kChunk / kThreads;
constexpr int kPlanThreads = 1024;
constexpr int kPlanEach = kLmax / kPlanThreads;

int max_chunks(int n, int Lmax) { return n / kChunk + (n < Lmax ? n : Lmax) + 1; }

// what the call carves out of its workspace, in this order (the size query runs it on a null base)
struct Carve {
    int *chunkStart;     // [Lmax + 1]
    float *partial;      // [max chunks][A][4]  umin, umax, vmin, vmax of a chunk
    float *partialZ;     // [max chunks][2]     zmin, zmax
    int *partialGood;    // [max chunks]
    float *extent;       // [Lmax][A][4]
    float *extentZ;      // [Lmax][2]
    int *good;           // [Lmax]
    int *near;           // [Lmax][A]
    size_t total;
};

void carve(void *base, int n, int Lmax, int A, Carve *c)
{
    const size_t chunks = (size_t)max_chunks(n, Lmax);
    icpflow::Carver ws(base);
    c->chunkStart = ws.take<int>(((size_t)Lmax + 1) * sizeof(int));
    c->partial = ws.take<float>(chunks * A * 4 * sizeof(float));
    c->partialZ = ws.take<float>(chunks * 2 * sizeof(float));
    c->partialGood = ws.take<int>(chunks * sizeof(int));
    c->extent = ws.take<float>((size_t)Lmax * A * 4 * sizeof(float));
    c->extentZ = ws.take<float>((size_t)Lmax * 2 * sizeof(float));
    c->good = ws.take<int>((size_t)Lmax * sizeof(int));
    c->near = ws.take<int>((size_t)Lmax * A * sizeof(int));
    c->total = ws.total();
}

// the number of segments every kernel works with: *d_num, nothing when it reports overflow, never beyond the table's rows
__device__ __forceinline__ int segments_of(const int32_t *__restrict__ num, int Lmax)
{
    const int L = *num;
    return L <= 0 ? 0 : min(L, Lmax);
}

// One workgroup of 1024, thread t segments 4 t .. 4 t + 3: the exclusive scan of the segments' chunk counts.  A segment with a
// negative label has no chunk (the cluster table computes no statistics for it either).
__global__ __launch_bounds__(kPlanThreads) void box_plan_kernel(const double *__restrict__ ctable, const int32_t *__restrict__ num, int Lmax,
                                                                int n, int *__restrict__ chunkStart)
{
    __shared__ int part[kPlanThreads / kWave];
    const int L = segments_of(num, Lmax), tid = threadIdx.x;
    if (L == 0) return;
    int v[kPlanEach], mine = 0;
#pragma unroll
    for (int e = 0; e < kPlanEach; ++e) {
        const int c = tid * kPlanEach + e;
        v[e] = 0;
        if (c < L && !(ctable[(size_t)c * kOrderCols] < 0.0)) {
            int start, count;
            icpflow::boxes::segment_rows(ctable + (size_t)c * kOrderCols, n, &start, &count);
            v[e] = (count + kChunk - 1) / kChunk;
        }
        mine += v[e];
    }
    int incl = mine;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int up = __shfl_up(incl, o, kWave);
        if ((tid & (kWave - 1)) >= o) incl += up;
    }
    if ((tid & (kWave - 1)) == kWave - 1) part[tid >> 6] = incl;
    __syncthreads();
    int before = incl - mine;
    for (int w = 0; w < (tid >> 6); ++w) before += part[w];
#pragma unroll
    for (int e = 0; e < kPlanEach; ++e) {
        const int c = tid * kPlanEach + e;
        if (c < L) chunkStart[c] = before;
        before += v[e];
    }
    if (tid == kPlanThreads - 1) chunkStart[L] = before;
}

// the rows of one chunk in a thread's registers, moved to the segment's reference point
struct Rows {
    float x[kPerThread], y[kPerThread], z[kPerThread];
    bool good[kPerThread];
    int seg;
};

// -> false when workgroup b has no chunk (workgroup-uniform)
__device__ __forceinline__ bool gather(const float *__restrict__ points, int n, const int64_t *__restrict__ order,
                                       const double *__restrict__ ctable, int L, const int *__restrict__ chunkStart, int b, Rows *r)
{
    if (L == 0 || b >= chunkStart[L]) return false;
    int lo = 0, hi = L - 1;                            // the segment of chunk b: the last one that starts at or before it
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (chunkStart[mid] <= b) lo = mid; else hi = mid - 1;
    }
    const double *seg = ctable + (size_t)lo * kOrderCols;
    int start, count;
    icpflow::boxes::segment_rows(seg, n, &start, &count);
    const float rx = (float)seg[3], ry = (float)seg[4];
    const int first = (b - chunkStart[lo]) * kChunk;
    const int rows = min(kChunk, count - first);
    r->seg = lo;
#pragma unroll
    for (int u = 0; u < kPerThread; ++u) {
        const int j = u * kThreads + (int)threadIdx.x;
        r->x[u] = r->y[u] = r->z[u] = 0.0f;
        r->good[u] = false;
        if (j < rows) {                                // (start + first + j < start + count <= n)
            const int64_t i = order[(size_t)start + first + j];
            if (i >= 0 && i < (int64_t)n) {            // an order entry outside the cloud is skipped
                const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
                r->good[u] = icpflow::boxes::finite3(x, y, z);
                r->x[u] = x - rx, r->y[u] = y - ry, r->z[u] = z;
            }
        }
    }
    return true;
}

__global__ __launch_bounds__(kThreads) void box_extent_kernel(const float *__restrict__ points, int n, const int64_t *__restrict__ order,
                                                              const double *__restrict__ ctable, const int32_t *__restrict__ num, int Lmax,
                                                              const int *__restrict__ chunkStart, Dirs dirs, int A,
                                                              float *__restrict__ partial, float *__restrict__ partialZ,
                                                              int *__restrict__ partialGood)
{
    __shared__ float sh[kWaves][kMaxDirs][4];
    __shared__ float shZ[kWaves][2];
    __shared__ int shGood[kWaves];
    const int L = segments_of(num, Lmax), b = blockIdx.x;
    Rows r;
    if (!gather(points, n, order, ctable, L, chunkStart, b, &r)) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
    for (int k = 0; k < A; ++k) {                      // (wave-uniform: the direction comes through scalar loads)
        const float c = dirs.cs[k][0], s = dirs.cs[k][1];
        float ulo = kInf, uhi = -kInf, vlo = kInf, vhi = -kInf;
#pragma unroll
        for (int u = 0; u < kPerThread; ++u) {
            if (r.good[u]) {
                const float pu = icpflow::boxes::proj_u(r.x[u], r.y[u], c, s), pv = icpflow::boxes::proj_v(r.x[u], r.y[u], c, s);
                ulo = fminf(ulo, pu), uhi = fmaxf(uhi, pu), vlo = fminf(vlo, pv), vhi = fmaxf(vhi, pv);
            }
        }
        ulo = icpflow::wave_min_uniform(ulo), uhi = icpflow::wave_max_uniform(uhi);
        vlo = icpflow::wave_min_uniform(vlo), vhi = icpflow::wave_max_uniform(vhi);
        if (lane == 0) sh[wave][k][0] = ulo, sh[wave][k][1] = uhi, sh[wave][k][2] = vlo, sh[wave][k][3] = vhi;
    }
    float zlo = kInf, zhi = -kInf;
    int good = 0;
#pragma unroll
    for (int u = 0; u < kPerThread; ++u) {             // (every lane takes every round: the ballots see whole waves)
        if (r.good[u]) zlo = fminf(zlo, r.z[u]), zhi = fmaxf(zhi, r.z[u]);
        good += __popcll(__ballot(r.good[u]));
    }
    zlo = icpflow::wave_min_uniform(zlo), zhi = icpflow::wave_max_uniform(zhi);
    if (lane == 0) shZ[wave][0] = zlo, shZ[wave][1] = zhi, shGood[wave] = good;
    __syncthreads();
    for (int k = threadIdx.x; k < A; k += kThreads) {
        float lo0 = sh[0][k][0], hi0 = sh[0][k][1], lo1 = sh[0][k][2], hi1 = sh[0][k][3];
        for (int w = 1; w < kWaves; ++w)
            lo0 = fminf(lo0, sh[w][k][0]), hi0 = fmaxf(hi0, sh[w][k][1]), lo1 = fminf(lo1, sh[w][k][2]), hi1 = fmaxf(hi1, sh[w][k][3]);
        float *out = partial + ((size_t)b * A + k) * 4;
        out[0] = lo0, out[1] = hi0, out[2] = lo1, out[3] = hi1;
    }
    if (threadIdx.x == 0) {
        float lo = shZ[0][0], hi = shZ[0][1];
        int g = shGood[0];
        for (int w = 1; w < kWaves; ++w) lo = fminf(lo, shZ[w][0]), hi = fmaxf(hi, shZ[w][1]), g += shGood[w];
        partialZ[(size_t)b * 2] = lo, partialZ[(size_t)b * 2 + 1] = hi;
        partialGood[b] = g;
    }
}

// One thread per (segment, direction); the thread of "direction" A folds z and the good rows.  `chunks`: the workgroups the
// chunk kernels were launched with -- a table that claims more than the cloud holds is cut there.
__global__ __launch_bounds__(kThreads) void box_fold_kernel(const int32_t *__restrict__ num, int Lmax, const int *__restrict__ chunkStart,
                                                            int chunks, int A, const float *__restrict__ partial,
                                                            const float *__restrict__ partialZ, const int *__restrict__ partialGood,
                                                            float *__restrict__ extent, float *__restrict__ extentZ, int *__restrict__ good,
                                                            int *__restrict__ near)
{
    const int L = segments_of(num, Lmax);
    const int at = blockIdx.x * kThreads + threadIdx.x, c = at / (A + 1), k = at % (A + 1);
    if (c >= L) return;
    const int c0 = min(chunkStart[c], chunks), c1 = min(chunkStart[c + 1], chunks);
    if (k < A) {
        float ulo = kInf, uhi = -kInf, vlo = kInf, vhi = -kInf;
        for (int q = c0; q < c1; ++q) {
            const float *p = partial + ((size_t)q * A + k) * 4;
            ulo = fminf(ulo, p[0]), uhi = fmaxf(uhi, p[1]), vlo = fminf(vlo, p[2]), vhi = fmaxf(vhi, p[3]);
        }
        float *out = extent + ((size_t)c * A + k) * 4;
        out[0] = ulo, out[1] = uhi, out[2] = vlo, out[3] = vhi;
        near[(size_t)c * A + k] = 0;
    } else {
        float lo = kInf, hi = -kInf;
        int g = 0;
        for (int q = c0; q < c1; ++q) lo = fminf(lo, partialZ[(size_t)q * 2]), hi = fmaxf(hi, partialZ[(size_t)q * 2 + 1]), g += partialGood[q];
        extentZ[(size_t)c * 2] = lo, extentZ[(size_t)c * 2 + 1] = hi;
        good[c] = g;
    }
}

__global__ __launch_bounds__(kThreads) void box_near_kernel(const float *__restrict__ points, int n, const int64_t *__restrict__ order,
                                                            const double *__restrict__ ctable, const int32_t *__restrict__ num, int Lmax,
                                                            const int *__restrict__ chunkStart, Dirs dirs, int A, float delta,
                                                            const float *__restrict__ extent, int *__restrict__ near)
{
    const int L = segments_of(num, Lmax), b = blockIdx.x;
    Rows r;
    if (!gather(points, n, order, ctable, L, chunkStart, b, &r)) return;
    const int lane = threadIdx.x & (kWave - 1);
    for (int k = 0; k < A; ++k) {                      // (every lane takes every round: the ballots see whole waves)
        const float c = dirs.cs[k][0], s = dirs.cs[k][1];
        const float *e = extent + ((size_t)r.seg * A + k) * 4;
        const float ulo = e[0], uhi = e[1], vlo = e[2], vhi = e[3];
        int count = 0;
#pragma unroll
        for (int u = 0; u < kPerThread; ++u) {
            const float pu = icpflow::boxes::proj_u(r.x[u], r.y[u], c, s), pv = icpflow::boxes::proj_v(r.x[u], r.y[u], c, s);
            const float side = fminf(fminf(uhi - pu, pu - ulo), fminf(vhi - pv, pv - vlo));
            count += __popcll(__ballot(r.good[u] && side <= delta));
        }
        if (lane == 0 && count != 0) atomicAdd(&near[(size_t)r.seg * A + k], count);
    }
}

__global__ __launch_bounds__(kThreads) void box_final_kernel(const double *__restrict__ ctable, const int32_t *__restrict__ num, int Lmax,
                                                             Dirs dirs, int A, const float *__restrict__ extent,
                                                             const float *__restrict__ extentZ, const int *__restrict__ good,
                                                             const int *__restrict__ near, double *__restrict__ boxes)
{
    const int L = segments_of(num, Lmax);
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= L) return;
    const double *seg = ctable + (size_t)c * kOrderCols;
    double *row = boxes + (size_t)c * kBoxCols;
    const int g = seg[0] < 0.0 ? 0 : good[c];
    row[0] = seg[0], row[1] = seg[1];
    if (g == 0) {
        for (int j = 2; j < kBoxCols; ++j) row[j] = j == 3 ? -1.0 : 0.0;
        return;
    }
    int best = 0, bestNear = 0;
    float bestArea = 0.0f;
    for (int k = 0; k < A; ++k) {
        const float *e = extent + ((size_t)c * A + k) * 4;
        const float area = (e[1] - e[0]) * (e[3] - e[2]);
        const int nr = near[(size_t)c * A + k];
        if (k == 0 || nr > bestNear || (nr == bestNear && area < bestArea)) best = k, bestNear = nr, bestArea = area;
    }
    const float *e = extent + ((size_t)c * A + best) * 4;
    const double ck = (double)dirs.cs[best][0], sk = (double)dirs.cs[best][1];
    const double um = ((double)e[0] + (double)e[1]) * 0.5, vm = ((double)e[2] + (double)e[3]) * 0.5;
    const double rx = (double)(float)seg[3], ry = (double)(float)seg[4];
    const double zlo = (double)extentZ[(size_t)c * 2], zhi = (double)extentZ[(size_t)c * 2 + 1];
    row[2] = (double)g, row[3] = (double)best, row[4] = (double)bestNear, row[5] = (double)bestArea;
    row[6] = rx + (ck * um - sk * vm);
    row[7] = ry + (sk * um + ck * vm);
    row[8] = (zlo + zhi) * 0.5;
    row[9] = (double)e[1] - (double)e[0];
    row[10] = (double)e[3] - (double)e[2];
    row[11] = zhi - zlo;
    row[12] = ck, row[13] = sk, row[14] = zlo, row[15] = zhi;
}

// the segment of a label in a box table (column 0, ascending by label_key), or -1
__device__ __forceinline__ int find_segment(const double *__restrict__ boxes, int L, float label)
{
    const uint32_t want = icpflow::label_key(icpflow::boxes::quieted(label));
    int lo = 0, hi = L;                                // the first segment whose key is not below `want`
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (icpflow::label_key(icpflow::boxes::quieted((float)boxes[(size_t)mid * kBoxCols])) < want) lo = mid + 1; else hi = mid;
    }
    return lo < L && icpflow::label_key(icpflow::boxes::quieted((float)boxes[(size_t)lo * kBoxCols])) == want ? lo : -1;
}

__global__ __launch_bounds__(kThreads) void pair_objects_kernel(const double *__restrict__ src, const int32_t *__restrict__ numSrc,
                                                                const double *__restrict__ dst, const int32_t *__restrict__ numDst, int Lmax,
                                                                const float *__restrict__ pairs, int P, int stride,
                                                                const float *__restrict__ T, double seconds, double minSpeed2,
                                                                double *__restrict__ objects, unsigned long long *__restrict__ counts)
{
    __shared__ int sh[kWaves][kCounts];
    const int p = blockIdx.x * kThreads + (int)threadIdx.x;
    const bool live = p < P;
    bool boxed = false, moving = false, noSrc = false, noDst = false;
    if (live) {
        const float ls = pairs[(size_t)p * stride], ld = pairs[(size_t)p * stride + 1];
        const int cs = find_segment(src, segments_of(numSrc, Lmax), ls);
        const int cd = dst != nullptr ? find_segment(dst, segments_of(numDst, Lmax), ld) : -1;
        noSrc = cs < 0, noDst = cd < 0;
        double *row = objects + (size_t)p * kObjectCols;
        row[0] = (double)ls, row[1] = (double)ld, row[2] = (double)cs, row[3] = (double)cd;
        const double *bs = cs >= 0 ? src + (size_t)cs * kBoxCols : nullptr;
        boxed = bs != nullptr && bs[3] >= 0.0 && bs[2] > 0.0;
        if (!boxed) {
            for (int j = 4; j < kObjectCols; ++j) row[j] = 0.0;
        } else {
            const float *m = T + (size_t)p * 16;
            const double cx = bs[6], cy = bs[7], cz = bs[8];
            double d[3];
#pragma unroll
            for (int a = 0; a < 3; ++a)
                d[a] = ((((double)m[4 * a] * cx + (double)m[4 * a + 1] * cy) + (double)m[4 * a + 2] * cz) + (double)m[4 * a + 3]) - (a == 0 ? cx : a == 1 ? cy : cz);
            const double vx = d[0] / seconds, vy = d[1] / seconds, vz = d[2] / seconds;
            const double speed2 = vx * vx + vy * vy;
            moving = speed2 >= minSpeed2;
            const double ck = bs[12], sk = bs[13], du = bs[9], dv = bs[10];
            const double ex[4] = {ck, -sk, -ck, sk}, ey[4] = {sk, ck, -sk, -ck};
            int mq = 0;
            if (moving) {
                double bestDot = ex[0] * d[0] + ey[0] * d[1];
#pragma unroll
                for (int q = 1; q < 4; ++q) {
                    const double dot = ex[q] * d[0] + ey[q] * d[1];
                    if (dot > bestDot) bestDot = dot, mq = q;
                }
            } else {
                mq = du >= dv ? 0 : 1;
            }
            row[4] = cx, row[5] = cy, row[6] = cz;
            row[7] = d[0], row[8] = d[1], row[9] = d[2];
            row[10] = vx, row[11] = vy, row[12] = vz;
            row[13] = speed2, row[14] = moving ? 1.0 : 0.0, row[15] = (double)mq;
            row[16] = (mq & 1) ? dv : du, row[17] = (mq & 1) ? du : dv, row[18] = bs[11];
            row[19] = ex[mq], row[20] = ey[mq];
            const double *bd = cd >= 0 ? dst + (size_t)cd * kBoxCols : nullptr;
            const bool target = bd != nullptr && bd[3] >= 0.0 && bd[2] > 0.0;
            double gap = -1.0;
            if (target) {
                const double gx = (cx + d[0]) - bd[6], gy = (cy + d[1]) - bd[7];
                gap = gx * gx + gy * gy;
            }
            row[21] = gap, row[22] = bs[2], row[23] = target ? bd[2] : 0.0;
        }
    }
    const bool flag[kCounts] = {boxed, moving, live && noSrc, live && noDst};
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kCounts; ++k) {                // (every lane takes every round: the ballots see whole waves)
        const int t = __popcll(__ballot(flag[k]));
        if ((threadIdx.x & (kWave - 1)) == 0) sh[wave][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < kCounts) {
        int t = 0;
        for (int w = 0; w < kWaves; ++w) t += sh[w][threadIdx.x];
        if (t != 0) atomicAdd(&counts[threadIdx.x], (unsigned long long)t);
    }
}

bool sizes_ok(int n, int Lmax, int A) { return n >= 0 && n <= kMaxRows && Lmax >= 1 && Lmax <= kLmax && A >= 1 && A <= kMaxDirs; }

}  // namespace

extern "C" {

size_t icpflow_segment_boxes_workspace_bytes(int n, int Lmax, int A)
{
    if (!sizes_ok(n, Lmax, A)) return 0;
    Carve c{};
    carve(nullptr, n, Lmax, A, &c);
    return c.total;
}

int icpflow_segment_boxes(const float *d_points, int n, const int64_t *d_order, const double *d_table, const int32_t *d_num, int Lmax,
                          const float *h_dirs, int A, double delta, double *d_boxes, void *d_ws, size_t ws_bytes, icpflow_stream_t stream)
{
    const char *fn = "icpflow_segment_boxes";
    if (n < 0) return report_errorf(ICPFLOW_E_ARG, "icpflow_segment_boxes: n = %d: a negative size", n);
    if (n > kMaxRows) return report_errorf(ICPFLOW_E_LIMIT, "icpflow_segment_boxes: n = %d: at most %d rows a cloud", n, kMaxRows);
    if (Lmax < 1) return report_errorf(ICPFLOW_E_ARG, "icpflow_segment_boxes: Lmax = %d: Lmax must be at least 1", Lmax);
    if (Lmax > kLmax) return report_errorf(ICPFLOW_E_LIMIT, "icpflow_segment_boxes: Lmax = %d: at most %d segments", Lmax, kLmax);
    if (A < 1 || A > kMaxDirs) return report_errorf(ICPFLOW_E_ARG, "icpflow_segment_boxes: A = %d: A must lie in [1, %d]", A, kMaxDirs);
    if (!(delta >= 0.0 && delta <= 1e3)) return report_errorf(ICPFLOW_E_ARG, "icpflow_segment_boxes: delta = %g: delta must lie in [0, 1e3] metres", delta);
    if (!d_table || !d_num || !h_dirs || !d_boxes || (n > 0 && (!d_points || !d_order))) return pointer_error(fn);
    Dirs dirs{};
    for (int k = 0; k < A; ++k) {
        const float c = h_dirs[2 * k], s = h_dirs[2 * k + 1];
        const double norm = (double)c * (double)c + (double)s * (double)s;
        if (!std::isfinite(c) || !std::isfinite(s) || !(std::fabs(norm - 1.0) <= 1e-3))
            return report_errorf(ICPFLOW_E_ARG, "icpflow_segment_boxes: direction %d = (%g, %g): a direction must be a finite unit vector", k, (double)c, (double)s);
        dirs.cs[k][0] = c, dirs.cs[k][1] = s;
    }
    Carve c{};
    carve(d_ws, n, Lmax, A, &c);
    if (!d_ws || ws_bytes < c.total) return workspace_error(fn, "icpflow_segment_boxes_workspace_bytes", d_ws, ws_bytes, c.total);
    if (((uintptr_t)d_ws & 15) != 0) return report_error(ICPFLOW_E_ARG, "icpflow_segment_boxes: d_ws must be 16-byte aligned");

    hipStream_t st = (hipStream_t)stream;
    const int chunks = max_chunks(n, Lmax);
    box_plan_kernel<<<1, kPlanThreads, 0, st>>>(d_table, d_num, Lmax, n, c.chunkStart);
    ICPFLOW_TRY(hipGetLastError());
    box_extent_kernel<<<chunks, kThreads, 0, st>>>(d_points, n, d_order, d_table, d_num, Lmax, c.chunkStart, dirs, A, c.partial, c.partialZ,
                                                   c.partialGood);
    ICPFLOW_TRY(hipGetLastError());
    box_fold_kernel<<<(Lmax * (A + 1) + kThreads - 1) / kThreads, kThreads, 0, st>>>(d_num, Lmax, c.chunkStart, chunks, A, c.partial, c.partialZ,
                                                                                    c.partialGood, c.extent, c.extentZ, c.good, c.near);
    ICPFLOW_TRY(hipGetLastError());
    box_near_kernel<<<chunks, kThreads, 0, st>>>(d_points, n, d_order, d_table, d_num, Lmax, c.chunkStart, dirs, A, (float)delta, c.extent, c.near);
    ICPFLOW_TRY(hipGetLastError());
    box_final_kernel<<<(Lmax + kThreads - 1) / kThreads, kThreads, 0, st>>>(d_table, d_num, Lmax, dirs, A, c.extent, c.extentZ, c.good, c.near, d_boxes);
    ICPFLOW_TRY(hipGetLastError());
    return ICPFLOW_OK;
}

int icpflow_pair_objects_default_params(icpflow_object_params_t *params)
{
    if (!params) return pointer_error("icpflow_pair_objects_default_params");
    params->struct_size = sizeof(icpflow_object_params_t);
    params->seconds = 0.1, params->min_speed = 0.5;
    return ICPFLOW_OK;
}

int icpflow_pair_objects(const double *d_boxes_src, const int32_t *d_num_src, const double *d_boxes_dst, const int32_t *d_num_dst, int Lmax,
                         const float *d_pair_rows, int P, int pair_stride, const float *d_T, const icpflow_object_params_t *params,
                         double *d_objects, int64_t *d_counts, icpflow_stream_t stream)
{
    const char *fn = "icpflow_pair_objects";
    if (P < 0) return report_errorf(ICPFLOW_E_ARG, "icpflow_pair_objects: P = %d: a negative size", P);
    if (Lmax < 1) return report_errorf(ICPFLOW_E_ARG, "icpflow_pair_objects: Lmax = %d: Lmax must be at least 1", Lmax);
    if (Lmax > kLmax) return report_errorf(ICPFLOW_E_LIMIT, "icpflow_pair_objects: Lmax = %d: at most %d segments", Lmax, kLmax);
    if (pair_stride < 2) return report_errorf(ICPFLOW_E_ARG, "icpflow_pair_objects: pair_stride = %d: pair_stride must be at least 2", pair_stride);
    if (!d_boxes_src || !d_num_src || !params || !d_counts || (P > 0 && !d_objects)) return pointer_error(fn);
    if ((d_boxes_dst == nullptr) != (d_num_dst == nullptr))
        return report_error(ICPFLOW_E_ARG, "icpflow_pair_objects: the destination's boxes and their number come together or not at all");
    if (P > 0 && (!d_pair_rows || !d_T)) return report_errorf(ICPFLOW_E_ARG, "icpflow_pair_objects: P = %d and no pair rows or no transforms", P);
    if (params->struct_size != sizeof(icpflow_object_params_t))
        return report_errorf(ICPFLOW_E_ARG, "icpflow_pair_objects: params->struct_size = %zu, this library's icpflow_object_params_t has %zu bytes",
                             params->struct_size, sizeof(icpflow_object_params_t));
    if (!(params->seconds > 0.0) || !std::isfinite(params->seconds))
        return report_errorf(ICPFLOW_E_ARG, "icpflow_pair_objects: seconds = %g: seconds must be positive and finite", params->seconds);
    if (!(params->min_speed >= 0.0) || !std::isfinite(params->min_speed))
        return report_errorf(ICPFLOW_E_ARG, "icpflow_pair_objects: min_speed = %g: min_speed must be finite and not negative", params->min_speed);

    hipStream_t st = (hipStream_t)stream;
    ICPFLOW_TRY(hipMemsetAsync(d_counts, 0, kCounts * sizeof(int64_t), st));
    if (P == 0) return ICPFLOW_OK;
    pair_objects_kernel<<<(P + kThreads - 1) / kThreads, kThreads, 0, st>>>(d_boxes_src, d_num_src, d_boxes_dst, d_num_dst, Lmax, d_pair_rows, P,
                                                                            pair_stride, d_T, params->seconds, params->min_speed * params->min_speed,
                                                                            d_objects, (unsigned long long *)d_counts);
    ICPFLOW_TRY(hipGetLastError());
    return ICPFLOW_OK;
}

}  // extern "C"
