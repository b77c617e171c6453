// ground.hip -- ground segmentation of one cloud on the GPU (include/icpflow_hip.h, "8(f) ground segmentation"): the method
// of Patchwork++ as the reference configures it (utils_ground.py:43-66, patchwork-plusplus/patchworkpp/src/patchworkpp.cpp),
// a fresh object per cloud, so the adaptive thresholds never act.
//
// Five launches on the caller's stream, nothing crosses to the host:
//   1. ground_bin_kernel      a patch id per row (fp64, pc2czm), every row labelled non-ground, and the rows of each patch
//                             counted per wave: a wave owns a contiguous range of rows;
//   2. ground_scan_kernel     one workgroup: per patch the exclusive scan of the waves' counts in wave order, then of the
//                             patches' totals -- where each wave's rows of each patch begin;
//   3. ground_scatter_kernel  the same waves over the same rows: a row's place is its patch's start + the rows of that patch
//                             before it, so a patch's rows lie together IN ROW ORDER, whatever the grid (a stable counting sort
//                             like table.hip's); the coordinates travel with them;
//   4. ground_patch_kernel    one workgroup per patch: R-VPF, R-GPF and the likelihood chain of its patch;
//   5. ground_revert_kernel   one workgroup: the temporal ground revert, ring by ring on one lane, then the candidates' rows.
// A point's state is one byte in the workspace (0 in the set, 1 non-ground, 2 ground part), read and written by the one
// thread that owns the point in every pass: a patch of 20 000 points runs the code a patch of 20 runs.
//
// Determinism.  The sets of a plane estimate are predicates evaluated per point (nothing is compacted).  The moments are
// two-pass (mean, then centred products) in fp64, added in a fixed order: a thread takes the points t, t + 256, ... of its
// patch in that order, a wave adds its lanes by one butterfly, the waves are added in wave order out of LDS
// (common.hpp block_sum).  The 3x3 eigen-solve is cyclic Jacobi in fp64 on one lane.  The lowest points come by selection:
// num_lpr times the smallest (z, place) key above the last one.  No floating-point atomics; integer atomics count rows.
// Compiled with -ffp-contract=off: a point-plane distance is ((nx x + ny y) + nz z) + d, each operation rounded by itself.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "common.hpp"
#include "host.hpp"

using icpflow::Carver;
using icpflow::kWave;
using icpflow::pointer_error;
using icpflow::report_error;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kPatches = ICPFLOW_GROUND_PATCHES;
constexpr int kCols = ICPFLOW_GROUND_TABLE_COLS;
constexpr int kNearPatches = 96;           // the patches of the 4 rings of interest: 2 x 16 + 2 x 32
constexpr int kNearRings = 4;
constexpr int kChunkMin = 512;             // rows a binning wave takes at least
constexpr int kMaxBinWaves = 1024;         // binning waves at most (a CU's workgroup each four)
constexpr int kScanThreads = 512;
constexpr unsigned long long kNoKey = ~0ull;

// the one layout: zones of {2, 4, 4, 4} rings and {16, 32, 54, 32} sectors
__host__ __device__ constexpr int rings_of(int k) { return k == 0 ? 2 : 4; }
__host__ __device__ constexpr int sectors_of(int k) { return k == 0 ? 16 : k == 2 ? 54 : 32; }
__host__ __device__ constexpr int patch_base(int k) { return k == 0 ? 0 : k == 1 ? 32 : k == 2 ? 160 : 376; }
__host__ __device__ constexpr int ring_base(int k) { return k == 0 ? 0 : k == 1 ? 2 : k == 2 ? 6 : 10; }

struct Geo {                               // patchworkpp.h:118-130, in double as there
    double min_range, max_range;
    double lo[4], ring_size[4], sector_size[4];
};

struct Par {
    double skip_below;                     // adaptive_seed_selection_margin * sensor_height
    double th_seeds, th_dist, th_seeds_v, th_dist_v, upright;
    int num_iter, num_lpr, num_min_pts;
};

struct Plane {
    double mean[3], normal[3], sv[3], d;
};

struct Carve {
    int waves, chunk;                      // binning waves and the rows of each
    size_t pid, order, points, state, wave_count, start, table, total;
};

Carve carve(int n)
{
    Carve c;
    const long long want = ((long long)n + kChunkMin - 1) / kChunkMin;
    c.waves = (int)(want < 1 ? 1 : want > kMaxBinWaves ? kMaxBinWaves : want);
    const long long per = ((long long)n + c.waves - 1) / c.waves;
    c.chunk = (int)((per + kWave - 1) / kWave * kWave);
    Carver mem;
    c.pid = mem.take((size_t)n * sizeof(int32_t));
    c.order = mem.take((size_t)n * sizeof(int32_t));
    c.points = mem.take((size_t)n * 3 * sizeof(float));
    c.state = mem.take((size_t)n);
    c.wave_count = mem.take((size_t)c.waves * kPatches * sizeof(int32_t));
    c.start = mem.take((size_t)(kPatches + 1) * sizeof(int32_t));
    c.table = mem.take((size_t)kPatches * kCols * sizeof(double));
    c.total = mem.total();
    return c;
}

// ---- binning (pc2czm, patchworkpp.cpp:561-605) -------------------------------------------------------------------------
__device__ __forceinline__ int patch_of(float x, float y, float z, const Geo &g)
{
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return -1;
    const double dx = x, dy = y;
    const double r = sqrt(dx * dx + dy * dy);
    if (!(r <= g.max_range && r > g.min_range)) return -1;
    double theta = atan2(dy, dx);
    if (!(theta > 0.0)) theta = 2.0 * M_PI + theta;          // (y = 0, x > 0: 2 pi, the last sector)
    const int k = r < g.lo[1] ? 0 : r < g.lo[2] ? 1 : r < g.lo[3] ? 2 : 3;
    const int ring = min((int)((r - g.lo[k]) / g.ring_size[k]), rings_of(k) - 1);
    const int sector = min((int)(theta / g.sector_size[k]), sectors_of(k) - 1);
    return patch_base(k) + ring * sectors_of(k) + sector;
}

__device__ __forceinline__ void wave_sync_lds()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kThreads) void ground_bin_kernel(const float *__restrict__ pts, int stride, int n, Geo geo, int waves, int chunk,
                                                              int32_t *__restrict__ pid, uint8_t *__restrict__ nonground,
                                                              int32_t *__restrict__ wave_count)
{
    __shared__ int cnt[kWaves][kPatches];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int gw = blockIdx.x * kWaves + wave;
    for (int b = lane; b < kPatches; b += kWave) cnt[wave][b] = 0;
    __syncthreads();
    if (gw < waves) {
        const long long lo = (long long)gw * chunk;
        const long long hi = lo + chunk < n ? lo + chunk : n;
        for (long long i = lo + lane; i < hi; i += kWave) {
            const float *p = pts + (size_t)i * stride;
            const int b = patch_of(p[0], p[1], p[2], geo);
            pid[i] = b;
            nonground[i] = 1;
            if (b >= 0) atomicAdd(&cnt[wave][b], 1);
        }
    }
    __syncthreads();
    if (gw < waves)
        for (int b = lane; b < kPatches; b += kWave) wave_count[(size_t)gw * kPatches + b] = cnt[wave][b];
}

__global__ __launch_bounds__(kScanThreads) void ground_scan_kernel(int32_t *__restrict__ wave_count, int waves, int32_t *__restrict__ start)
{
    __shared__ int total[kPatches];
    const int b = threadIdx.x;
    if (b < kPatches) {
        int run = 0;
        for (int w = 0; w < waves; ++w) {
            const int c = wave_count[(size_t)w * kPatches + b];
            wave_count[(size_t)w * kPatches + b] = run;
            run += c;
        }
        total[b] = run;
    }
    __syncthreads();
    if (b == 0) {
        int run = 0;
        for (int k = 0; k < kPatches; ++k) {
            start[k] = run;
            run += total[k];
        }
        start[kPatches] = run;
    }
}

__global__ __launch_bounds__(kThreads) void ground_scatter_kernel(const float *__restrict__ pts, int stride, int n, int waves, int chunk,
                                                                  const int32_t *__restrict__ pid, const int32_t *__restrict__ wave_count,
                                                                  const int32_t *__restrict__ start, int32_t *__restrict__ order,
                                                                  float *__restrict__ sorted)
{
    __shared__ int at[kWaves][kPatches];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int gw = blockIdx.x * kWaves + wave;
    if (gw >= waves) return;                                       // (no workgroup barrier below)
    for (int b = lane; b < kPatches; b += kWave) at[wave][b] = start[b] + wave_count[(size_t)gw * kPatches + b];
    wave_sync_lds();
    const long long lo = (long long)gw * chunk;
    const long long hi = lo + chunk < n ? lo + chunk : n;
    const unsigned long long below = (1ull << lane) - 1;
    for (long long tile = lo; tile < hi; tile += kWave) {
        const long long i = tile + lane;
        const int b = i < hi ? pid[i] : -1;
        unsigned long long todo = __ballot(b >= 0);
        while (todo) {                                             // the patches of the tile, in the order of their first row
            const int leader = __ffsll((long long)todo) - 1;
            const int lb = __shfl(b, leader, kWave);
            const bool mine = b == lb;
            const unsigned long long members = __ballot(mine);
            todo &= ~members;
            const int base = at[wave][lb];
            if (mine) {
                const int pos = base + __popcll(members & below);
                const float *p = pts + (size_t)i * stride;
                order[pos] = (int32_t)i;
                sorted[(size_t)pos * 3 + 0] = p[0], sorted[(size_t)pos * 3 + 1] = p[1], sorted[(size_t)pos * 3 + 2] = p[2];
            }
            wave_sync_lds();
            if (lane == leader) at[wave][lb] = base + __popcll(members);
            wave_sync_lds();
        }
    }
}

// ---- one patch ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double plane_dist(const Plane &pl, double x, double y, double z)
{
    return ((pl.normal[0] * x + pl.normal[1] * y) + pl.normal[2] * z) + pl.d;    // calc_point_to_plane_d, patchworkpp.cpp:534-537
}

__device__ __forceinline__ void jacobi_rotate(double (&a)[3][3], double (&v)[3][3], int p, int q, int r, int sweep)
{
    const double g = 100.0 * fabs(a[p][q]);
    if (sweep > 3 && fabs(a[p][p]) + g == fabs(a[p][p]) && fabs(a[q][q]) + g == fabs(a[q][q])) {
        a[p][q] = a[q][p] = 0.0;
        return;
    }
    if (a[p][q] == 0.0) return;
    double h = a[q][q] - a[p][p], t;
    if (fabs(h) + g == fabs(h)) {
        t = a[p][q] / h;
    } else {
        const double theta = 0.5 * h / a[p][q];
        t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
        if (theta < 0.0) t = -t;
    }
    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c);
    h = t * a[p][q];
    a[p][p] -= h, a[q][q] += h, a[p][q] = a[q][p] = 0.0;
    const double arp = a[r][p], arq = a[r][q];
    a[r][p] = a[p][r] = arp - s * (arq + arp * tau);
    a[r][q] = a[q][r] = arq + s * (arp - arq * tau);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double vp = v[j][p], vq = v[j][q];
        v[j][p] = vp - s * (vq + vp * tau);
        v[j][q] = vq + s * (vp - vq * tau);
    }
}

// The plane of a mean and a covariance (xx xy xz yy yz zz): singular values descending, the normal the singular vector of the
// smallest with normal_z >= 0, d = -normal . mean (estimate_plane, patchworkpp.cpp:37-65).  A covariance that is not finite
// (the 0 / 0 of a single point) gives a NaN plane.
__device__ void plane_from_moments(const double (&mean)[3], const double (&c)[6], Plane &pl)
{
    pl.mean[0] = mean[0], pl.mean[1] = mean[1], pl.mean[2] = mean[2];
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) finite = finite && isfinite(c[k]);
    if (!finite) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        pl.normal[0] = pl.normal[1] = pl.normal[2] = pl.sv[0] = pl.sv[1] = pl.sv[2] = pl.d = nan;
        return;
    }
    double a[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < 50; ++sweep) {
        if (fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]) == 0.0) break;
        jacobi_rotate(a, v, 0, 1, 2, sweep);
        jacobi_rotate(a, v, 0, 2, 1, sweep);
        jacobi_rotate(a, v, 1, 2, 0, sweep);
    }
    double s[3] = {fabs(a[0][0]), fabs(a[1][1]), fabs(a[2][2])};
    int o[3] = {0, 1, 2};
#define GROUND_SWAP(i, j) \
    if (s[o[i]] < s[o[j]]) { const int t_ = o[i]; o[i] = o[j]; o[j] = t_; }
    GROUND_SWAP(0, 1) GROUND_SWAP(1, 2) GROUND_SWAP(0, 1)
#undef GROUND_SWAP
    pl.sv[0] = s[o[0]], pl.sv[1] = s[o[1]], pl.sv[2] = s[o[2]];
    double nx = 0.0, ny = 0.0, nz = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (o[2] == k) nx = v[0][k], ny = v[1][k], nz = v[2][k];
    if (nz < 0.0) nx = -nx, ny = -ny, nz = -nz;
    pl.normal[0] = nx, pl.normal[1] = ny, pl.normal[2] = nz;
    pl.d = -((nx * mean[0] + ny * mean[1]) + nz * mean[2]);
}

struct Lds {
    double red[kWaves * 6];
    double plane[10];
    unsigned long long low[2][kWaves];
};

// The plane of the points of the current set that satisfy `in`; an empty set leaves `pl` as it was.  -> the set's size.
// All threads of the workgroup call it; `pl` and the result are the same in every thread.
template <typename In>
__device__ int estimate_plane(const float *__restrict__ xyz, const uint8_t *__restrict__ state, int cnt, In in, Plane &pl, Lds &lds)
{
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < cnt; i += kThreads) {
        if (state[i] != 0) continue;
        const double x = xyz[3 * (size_t)i + 0], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
        if (in(x, y, z)) s[0] += x, s[1] += y, s[2] += z, s[3] += 1.0;
    }
    icpflow::block_sum<4>(s, lds.red);
    const int m = (int)s[3];
    if (m == 0) return 0;
    const double mean[3] = {s[0] / m, s[1] / m, s[2] / m};
    double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < cnt; i += kThreads) {
        if (state[i] != 0) continue;
        const double x = xyz[3 * (size_t)i + 0], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
        if (in(x, y, z)) {
            const double dx = x - mean[0], dy = y - mean[1], dz = z - mean[2];
            c[0] += dx * dx, c[1] += dx * dy, c[2] += dx * dz, c[3] += dy * dy, c[4] += dy * dz, c[5] += dz * dz;
        }
    }
    icpflow::block_sum<6>(c, lds.red);
    if (threadIdx.x == 0) {
        const double over = (double)(m - 1);
        const double cov[6] = {c[0] / over, c[1] / over, c[2] / over, c[3] / over, c[4] / over, c[5] / over};
        Plane q;
        plane_from_moments(mean, cov, q);
        for (int k = 0; k < 3; ++k) lds.plane[k] = q.normal[k], lds.plane[3 + k] = q.sv[k];
        lds.plane[6] = q.d;
    }
    __syncthreads();
    for (int k = 0; k < 3; ++k) pl.mean[k] = mean[k], pl.normal[k] = lds.plane[k], pl.sv[k] = lds.plane[3 + k];
    pl.d = lds.plane[6];
    return m;
}

// lpr + th of extract_initial_seeds (patchworkpp.cpp:67-102): the mean of the up to num_lpr lowest z of the current set,
// in zone 0 after the points below skip_below; 0 when there is none.  Selection: the smallest (z, place) key above the last.
__device__ double seed_threshold(const float *__restrict__ xyz, const uint8_t *__restrict__ state, int cnt, bool zone0, const Par &par,
                                 double th, Lds &lds)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    unsigned long long last = 0;
    double sum = 0.0;
    int taken = 0;
    for (int r = 0; r < par.num_lpr; ++r) {
        unsigned long long best = kNoKey;
        for (int i = threadIdx.x; i < cnt; i += kThreads) {
            if (state[i] != 0) continue;
            const float z = xyz[3 * (size_t)i + 2];
            if (zone0 && (double)z < par.skip_below) continue;
            const unsigned long long key = icpflow::sort_pack(z, i);
            if ((r == 0 || key > last) && key < best) best = key;
        }
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            const unsigned long long w = __shfl_xor(best, o, kWave);
            best = w < best ? w : best;
        }
        if (lane == 0) lds.low[r & 1][wave] = best;
        __syncthreads();
        for (int w = 0; w < kWaves; ++w) best = lds.low[r & 1][w] < best ? lds.low[r & 1][w] : best;
        if (best == kNoKey) break;
        sum += (double)icpflow::sort_key_of(best);
        ++taken, last = best;
    }
    __syncthreads();
    const double lpr = taken != 0 ? sum / taken : 0.0;
    return lpr + th;
}

__global__ __launch_bounds__(kThreads) void ground_patch_kernel(const float *__restrict__ sorted, const int32_t *__restrict__ order,
                                                                const int32_t *__restrict__ start, Par par, uint8_t *__restrict__ state_all,
                                                                uint8_t *__restrict__ nonground, double *__restrict__ table)
{
    __shared__ Lds lds;
    const int patch = blockIdx.x;
    const int zone = patch < patch_base(1) ? 0 : patch < patch_base(2) ? 1 : patch < patch_base(3) ? 2 : 3;
    const int ring = ring_base(zone) + (patch - patch_base(zone)) / sectors_of(zone);
    const int first = start[patch], cnt = start[patch + 1] - first;
    double *row = table + (size_t)patch * kCols;
    if (cnt < par.num_min_pts) {                                   // its rows stay non-ground (patchworkpp.cpp:181-185)
        if (threadIdx.x < kCols) row[threadIdx.x] = threadIdx.x == 0 ? (double)cnt : 0.0;
        return;
    }
    const float *xyz = sorted + (size_t)first * 3;
    uint8_t *state = state_all + first;
    const int32_t *rows = order + first;
    for (int i = threadIdx.x; i < cnt; i += kThreads) state[i] = 0;
    const bool zone0 = zone == 0;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    Plane pl;
    for (int k = 0; k < 3; ++k) pl.mean[k] = pl.normal[k] = pl.sv[k] = nan;
    pl.d = nan;

    // R-VPF (patchworkpp.cpp:465-491)
    double removed[1] = {0.0};
    for (int it = 0; it < par.num_iter; ++it) {
        const double thr = seed_threshold(xyz, state, cnt, zone0, par, par.th_seeds_v, lds);
        estimate_plane(xyz, state, cnt, [thr](double, double, double z) { return z < thr; }, pl, lds);
        if (!(zone0 && pl.normal[2] < par.upright)) break;
        for (int i = threadIdx.x; i < cnt; i += kThreads) {
            if (state[i] != 0) continue;
            const double x = xyz[3 * (size_t)i + 0], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
            if (fabs(plane_dist(pl, x, y, z)) < par.th_dist_v) state[i] = 1, removed[0] += 1.0;
        }
    }
    icpflow::block_sum<1>(removed, lds.red);

    // R-GPF (patchworkpp.cpp:496-526)
    {
        const double thr = seed_threshold(xyz, state, cnt, zone0, par, par.th_seeds, lds);
        estimate_plane(xyz, state, cnt, [thr](double, double, double z) { return z < thr; }, pl, lds);
    }
    Plane by = pl;
    int ground = 0;
    for (int it = 0; it < par.num_iter; ++it) {
        by = pl;                                                   // the plane that decides this round's set
        const double th = par.th_dist;
        ground = estimate_plane(xyz, state, cnt, [by, th](double x, double y, double z) { return plane_dist(by, x, y, z) < th; }, pl, lds);
    }

    // the likelihood chain with thresholds 0 (patchworkpp.cpp:207-265)
    const bool upright = pl.normal[2] > par.upright;
    const bool not_elevated = pl.mean[2] < 0.0;
    const bool flat = pl.sv[2] < 0.0;
    const bool near = ring < kNearRings;
    double heading = 0.0;
    for (int k = 0; k < 3; ++k) heading += pl.mean[k] * pl.normal[k];
    const int code = !upright ? ICPFLOW_GROUND_NOT_UPRIGHT : !near ? ICPFLOW_GROUND_FAR : !(heading < 0.0) ? ICPFLOW_GROUND_HEADING
                     : (not_elevated || flat) ? ICPFLOW_GROUND_ACCEPTED : ICPFLOW_GROUND_CANDIDATE;
    const bool accept = code == ICPFLOW_GROUND_FAR || code == ICPFLOW_GROUND_ACCEPTED;
    for (int i = threadIdx.x; i < cnt; i += kThreads) {
        bool g = false;
        if (state[i] == 0) {
            const double x = xyz[3 * (size_t)i + 0], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
            g = plane_dist(by, x, y, z) < par.th_dist;
        }
        state[i] = g ? 2 : 1;
        if (g && accept) nonground[rows[i]] = 0;
    }
    if (threadIdx.x == 0) {
        row[0] = (double)cnt, row[1] = (double)ground;
        for (int k = 0; k < 3; ++k) row[2 + k] = pl.mean[k], row[5 + k] = pl.normal[k], row[8 + k] = pl.sv[k];
        row[11] = pl.d, row[12] = (double)code, row[13] = (double)ICPFLOW_GROUND_TGR_NONE, row[14] = removed[0], row[15] = 0.0;
    }
}

// ---- temporal ground revert (patchworkpp.cpp:236-242, 275-287, 385-447, 540-549) ------------------------------------------
__global__ __launch_bounds__(kThreads) void ground_revert_kernel(const int32_t *__restrict__ order, const int32_t *__restrict__ start,
                                                                 const uint8_t *__restrict__ state, Par par, double *__restrict__ table,
                                                                 uint8_t *__restrict__ nonground, double *__restrict__ table_out)
{
    __shared__ double flatness[kNearPatches];
    __shared__ int candidate[64];
    __shared__ int revert[kNearPatches];
    for (int p = threadIdx.x; p < kNearPatches; p += kThreads) revert[p] = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        int listed = 0;                                            // cleared only after a ring that had candidates
        for (int ring = 0; ring < kNearRings; ++ring) {
            const int zone = ring < ring_base(1) ? 0 : 1;
            const int base = patch_base(zone) + (ring - ring_base(zone)) * sectors_of(zone);
            int candidates = 0;
            for (int j = 0; j < sectors_of(zone); ++j) {
                const double *row = table + (size_t)(base + j) * kCols;
                if (row[0] < (double)par.num_min_pts) continue;
                if (row[7] > par.upright && row[4] < 0.0) flatness[listed++] = row[10];
                if ((int)row[12] == ICPFLOW_GROUND_CANDIDATE) candidate[candidates++] = base + j;
            }
            if (candidates == 0) continue;
            double mean = 0.0, stdev = 0.0;                        // calc_mean_stdev: left 0 for at most one value
            if (listed > 1) {
                double sum = 0.0;
                for (int k = 0; k < listed; ++k) sum += flatness[k];
                mean = sum / listed;
                for (int k = 0; k < listed; ++k) stdev += (flatness[k] - mean) * (flatness[k] - mean);
                stdev /= listed - 1;
                stdev = sqrt(stdev);
            }
            const double mu = mean + 1.5 * stdev;
            for (int k = 0; k < candidates; ++k) {
                double *row = table + (size_t)candidate[k] * kCols;
                const double f = row[10];
                double prob = 1.0 / (1.0 + exp((f - mu) / (mu / 10.0)));
                if (row[1] > 1500.0 && f < par.th_dist * par.th_dist) prob = 1.0;
                const double line = row[9] != 0.0 ? row[8] / row[9] : DBL_MAX;
                const double prob_line = line > 8.0 ? 0.0 : 1.0;
                const bool back = prob_line * prob > 0.5;
                row[13] = (double)(back ? ICPFLOW_GROUND_TGR_REVERTED : ICPFLOW_GROUND_TGR_REJECTED);
                revert[candidate[k]] = back ? 1 : 0;
            }
            listed = 0;
        }
    }
    __syncthreads();
    for (int p = 0; p < kNearPatches; ++p) {
        if (!revert[p]) continue;
        const int lo = start[p], hi = start[p + 1];
        for (int i = lo + threadIdx.x; i < hi; i += kThreads)
            if (state[i] == 2) nonground[order[i]] = 0;
    }
    if (table_out)
        for (int k = threadIdx.x; k < kPatches * kCols; k += kThreads) table_out[k] = table[k];
}

const int kRingsWanted[4] = {2, 4, 4, 4}, kSectorsWanted[4] = {16, 32, 54, 32};

// nullptr = fine
const char *check_params(const icpflow_ground_params_t *p, const char *fn, char *msg, size_t len)
{
    if (p->struct_size != sizeof(*p)) {
        snprintf(msg, len, "%s: params->struct_size is %zu, this library's icpflow_ground_params_t has %zu bytes", fn, p->struct_size, sizeof(*p));
        return msg;
    }
    for (int k = 0; k < 4; ++k)
        if (p->num_rings_each_zone[k] != kRingsWanted[k] || p->num_sectors_each_zone[k] != kSectorsWanted[k] || p->num_rings_of_interest != kNearRings) {
            snprintf(msg, len, "%s: zone layout other than rings {2,4,4,4}, sectors {16,32,54,32}, 4 rings of interest", fn);
            return msg;
        }
    if (!(p->min_range > 0.0) || !(p->max_range > p->min_range) || !std::isfinite(p->max_range)) {
        snprintf(msg, len, "%s: need 0 < min_range < max_range", fn);
        return msg;
    }
    if (p->num_iter < 1 || p->num_lpr < 1 || p->num_min_pts < 1) {
        snprintf(msg, len, "%s: num_iter, num_lpr and num_min_pts must be >= 1", fn);
        return msg;
    }
    return nullptr;
}

}  // namespace

extern "C" {

int icpflow_ground_default_params(icpflow_ground_params_t *p)
{
    if (!p) return pointer_error("icpflow_ground_default_params");
    std::memset(p, 0, sizeof(*p));
    p->struct_size = sizeof(*p);
    p->sensor_height = 1.723, p->min_range = 1.0, p->max_range = 64.0;                  // utils_ground.py:52-57
    p->th_seeds = 0.125, p->th_dist = 0.125, p->th_seeds_v = 0.25, p->th_dist_v = 0.1;  // patchworkpp.h:90-98
    p->uprightness_thr = 0.707, p->adaptive_seed_selection_margin = -1.2;
    p->num_iter = 3, p->num_lpr = 20, p->num_min_pts = 10, p->num_rings_of_interest = kNearRings;
    for (int k = 0; k < 4; ++k) p->num_rings_each_zone[k] = kRingsWanted[k], p->num_sectors_each_zone[k] = kSectorsWanted[k];
    return ICPFLOW_OK;
}

size_t icpflow_ground_workspace_bytes(int n, const icpflow_ground_params_t *params)
{
    char msg[192];
    if (n <= 0 || !params || check_params(params, "icpflow_ground_workspace_bytes", msg, sizeof(msg))) return 0;
    return carve(n).total;
}

int icpflow_ground_segment(const float *d_points, int stride, int n, const icpflow_ground_params_t *params, uint8_t *d_nonground,
                           double *d_patch_table, void *d_ws, size_t ws_bytes, icpflow_stream_t stream)
{
    const char *fn = "icpflow_ground_segment";
    char msg[192];
    if (n < 0) return report_error(ICPFLOW_E_ARG, "icpflow_ground_segment: n < 0");
    if (!params || (n > 0 && (!d_points || !d_nonground))) return pointer_error(fn);
    if (const char *why = check_params(params, fn, msg, sizeof(msg))) return report_error(ICPFLOW_E_ARG, why);
    if (stride < 3) return report_error(ICPFLOW_E_ARG, "icpflow_ground_segment: stride must be >= 3 floats");
    if (n == 0) return ICPFLOW_OK;
    const Carve c = carve(n);
    if (!d_ws || ws_bytes < c.total) return icpflow::workspace_error(fn, "icpflow_ground_workspace_bytes", d_ws, ws_bytes, c.total);
    if (((uintptr_t)d_ws & 7) != 0) return report_error(ICPFLOW_E_ARG, "icpflow_ground_segment: d_ws must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)d_ws;
    int32_t *pid = (int32_t *)(ws + c.pid), *order = (int32_t *)(ws + c.order), *wave_count = (int32_t *)(ws + c.wave_count);
    int32_t *start = (int32_t *)(ws + c.start);
    float *sorted = (float *)(ws + c.points);
    uint8_t *state = (uint8_t *)(ws + c.state);
    double *table = (double *)(ws + c.table);

    Geo g;                                                          // patchworkpp.h:118-130
    const double lo = params->min_range, hi = params->max_range;
    g.min_range = lo, g.max_range = hi;
    g.lo[0] = lo, g.lo[1] = (7 * lo + hi) / 8.0, g.lo[2] = (3 * lo + hi) / 4.0, g.lo[3] = (lo + hi) / 2.0;
    for (int k = 0; k < 4; ++k) {
        g.ring_size[k] = ((k < 3 ? g.lo[k + 1] : hi) - g.lo[k]) / rings_of(k);
        g.sector_size[k] = 2 * M_PI / sectors_of(k);
    }
    Par par;
    par.skip_below = params->adaptive_seed_selection_margin * params->sensor_height;
    par.th_seeds = params->th_seeds, par.th_dist = params->th_dist, par.th_seeds_v = params->th_seeds_v, par.th_dist_v = params->th_dist_v;
    par.upright = params->uprightness_thr;
    par.num_iter = params->num_iter, par.num_lpr = params->num_lpr, par.num_min_pts = params->num_min_pts;

    const int blocks = (c.waves + kWaves - 1) / kWaves;
    ground_bin_kernel<<<blocks, kThreads, 0, st>>>(d_points, stride, n, g, c.waves, c.chunk, pid, d_nonground, wave_count);
    ICPFLOW_TRY(hipGetLastError());
    ground_scan_kernel<<<1, kScanThreads, 0, st>>>(wave_count, c.waves, start);
    ICPFLOW_TRY(hipGetLastError());
    ground_scatter_kernel<<<blocks, kThreads, 0, st>>>(d_points, stride, n, c.waves, c.chunk, pid, wave_count, start, order, sorted);
    ICPFLOW_TRY(hipGetLastError());
    ground_patch_kernel<<<kPatches, kThreads, 0, st>>>(sorted, order, start, par, state, d_nonground, table);
    ICPFLOW_TRY(hipGetLastError());
    ground_revert_kernel<<<1, kThreads, 0, st>>>(order, start, state, par, table, d_nonground, d_patch_table);
    ICPFLOW_TRY(hipGetLastError());
    return ICPFLOW_OK;
}

}  // extern "C"
