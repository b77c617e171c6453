// ego.hip -- ego motion of a LiDAR sequence without poses: scan-to-map odometry resident on the GPU (include/icpflow_hip.h,
// "8(f) ego motion"; the reference's utils_ego_motion.py:21-111 hands this to the kiss_icp package).
//
// The map is an open-addressing table of voxels (key, count, up to 20 float32 points) in caller memory; a second table of
// the same size receives the voxels that survive the range prune of every frame, so a table never holds a deleted slot and
// a lookup ends at the first empty one.  Every decision that picks a point is by input index, never by arrival: the point
// kept by a down-sampling is its voxel's atomicMin over indices, a frame's points enter a voxel at (points already there +
// number of lower-indexed points of the frame in the same voxel).  Which SLOT a voxel lands in depends on arrival, what the
// voxel holds does not, and nothing reads a slot number.
//
// The registration is ONE workgroup for all iterations of a frame (source is a few hundred to a few thousand points: a
// launch per iteration, or a grid-wide exchange, would cost more than the iteration): a thread per source point walks the
// 27 voxels around it, the 27 fp64 sums + the count go through a fixed shuffle tree and a fixed LDS order, thread 0 solves
// the 6 x 6 system, steps the pose and raises the stop flag the others read after the barrier.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "host.hpp"

using icpflow::Carver;
using icpflow::pointer_error;
using icpflow::report_error;

namespace {

constexpr int kVoxelPoints = 20;          // storage per voxel (params.max_points_per_voxel <= 20)
constexpr int kRegThreads = 512;
constexpr int kRegWaves = kRegThreads / 64;
constexpr int kSums = 28;                 // 21 of J^T J (upper triangle), 6 of J^T r, the correspondence count
constexpr unsigned long long kEmpty = ~0ull;
constexpr int kCoordBias = 1 << 20;       // voxel coordinates are kept in 21 bits each
constexpr int kInfoWords = 8;

// flags[]: what the kernels report next to their results
enum { kFlagTableFull = 0, kFlagCoordRange = 1, kFlagLive = 2, kFlagExport = 3, kNumFlags = 4 };

struct MapTable {
    unsigned long long *keys;   // [C]
    int32_t *count;             // [C]
    float *pts;                 // [C][kVoxelPoints][3]
};

__device__ __forceinline__ unsigned hash_key(unsigned long long key, unsigned mask)
{
    return (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 32) & mask;
}

// floor(x / size) per axis, fp64; false when a coordinate leaves the 21 bits of a key
__device__ __forceinline__ bool voxel_key(double x, double y, double z, double size, unsigned long long *key)
{
    const double fx = floor(x / size), fy = floor(y / size), fz = floor(z / size);
    const double lim = (double)(kCoordBias - 2);
    if (!(fabs(fx) < lim && fabs(fy) < lim && fabs(fz) < lim)) return false;   // (NaN fails too)
    const long long ix = (long long)fx + kCoordBias, iy = (long long)fy + kCoordBias, iz = (long long)fz + kCoordBias;
    *key = ((unsigned long long)ix << 42) | ((unsigned long long)iy << 21) | (unsigned long long)iz;
    return true;
}

__device__ __forceinline__ unsigned long long pack_key(long long ix, long long iy, long long iz)
{
    return ((unsigned long long)(ix + kCoordBias) << 42) | ((unsigned long long)(iy + kCoordBias) << 21) |
           (unsigned long long)(iz + kCoordBias);
}

// the slot of `key`, claimed when absent; -1 when the table is full
__device__ int find_or_insert(unsigned long long *keys, unsigned mask, unsigned long long key)
{
    unsigned h = hash_key(key, mask);
    for (unsigned probe = 0; probe <= mask; ++probe) {
        unsigned long long k = keys[h];
        if (k == kEmpty) k = atomicCAS(&keys[h], kEmpty, key), k = (k == kEmpty) ? key : k;
        if (k == key) return (int)h;
        h = (h + 1) & mask;
    }
    return -1;
}

__device__ __forceinline__ int find_slot(const unsigned long long *__restrict__ keys, unsigned mask, unsigned long long key)
{
    unsigned h = hash_key(key, mask);
    for (unsigned probe = 0; probe <= mask; ++probe) {
        const unsigned long long k = keys[h];
        if (k == key) return (int)h;
        if (k == kEmpty) return -1;
        h = (h + 1) & mask;
    }
    return -1;
}

// ---- step 0 (optional): motion compensation by per-point stamps ------------------------------------------------------------
// The twist of the last motion, xi = log(inv(P[-2]) P[-1]) = (rho, omega), split on the host into the angle per unit stamp
// w = |omega| and the unit axis a; K = [a]_x, K2 = K K.  With phi = d w (signed) the closed forms of exp(d xi) become
//   R = I + sin(phi) K + (1 - cos(phi)) K2,   V = I + ((1 - cos(phi)) / phi) K + ((phi - sin(phi)) / phi) K2,   t = V (d rho)
// and only the two coefficients of V divide by phi: below kSeriesBelow they come from their series.
struct DeskewArgs {
    double mid, w;
    double rho[3], K[9], K2[9];
};

constexpr double kSeriesBelow = 0x1p-13;   // |phi| below which V's coefficients are series (include/icpflow_hip.h, 8(f) step 0)

// one thread per point; a wave reads 768 consecutive bytes of rows and 256 of stamps, and writes 768: every fetched line
// is used whole, whatever the alignment of the caller's buffers (12-byte rows leave nothing wider to rely on)
__global__ __launch_bounds__(256) void ego_deskew_kernel(const float *__restrict__ pts, const float *__restrict__ stamps, int n,
                                                         DeskewArgs a, float *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double p[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
    const double d = (double)stamps[i] - a.mid;
    const double phi = d * a.w;
    double sh, ch;
    sincos(0.5 * phi, &sh, &ch);
    const double a1 = 2.0 * (sh * ch), a2 = 2.0 * (sh * sh);   // sin(phi), 1 - cos(phi) without the cancellation
    double v1, v2;
    if (fabs(phi) < kSeriesBelow) {
        const double q = phi * phi;
        v1 = phi * (0.5 - q / 24.0), v2 = q * (1.0 / 6.0 - q / 120.0);
    } else {   // (a stamp that is not finite lands here: phi is NaN and so is the row)
        v1 = a2 / phi, v2 = 1.0 - a1 / phi;
    }
    const double u[3] = {d * a.rho[0], d * a.rho[1], d * a.rho[2]};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double kp = (a.K[3 * r] * p[0] + a.K[3 * r + 1] * p[1]) + a.K[3 * r + 2] * p[2];
        const double k2p = (a.K2[3 * r] * p[0] + a.K2[3 * r + 1] * p[1]) + a.K2[3 * r + 2] * p[2];
        const double ku = (a.K[3 * r] * u[0] + a.K[3 * r + 1] * u[1]) + a.K[3 * r + 2] * u[2];
        const double k2u = (a.K2[3 * r] * u[0] + a.K2[3 * r + 1] * u[1]) + a.K2[3 * r + 2] * u[2];
        out[3 * (size_t)i + r] = (float)((p[r] + (a1 * kp + a2 * k2p)) + (u[r] + (v1 * ku + v2 * k2u)));
    }
}

// ---- steps 1-2: crop + voxel key + lowest index ----------------------------------------------------------------------------
// pass 1: every candidate claims its voxel in the scratch table and lowers the voxel's index to its own
__global__ void ds_vote_kernel(const float *__restrict__ pts, const int32_t *__restrict__ rows, const int32_t *__restrict__ d_n,
                               int n_max, double size, int crop, double min2, double max2, unsigned long long *tkeys,
                               int32_t *tmin, unsigned tmask, int32_t *__restrict__ slotOf, int32_t *flags)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = d_n ? min(*d_n, n_max) : n_max;
    if (i >= n) return;
    const int row = rows ? rows[i] : i;
    const double x = pts[3 * (size_t)row], y = pts[3 * (size_t)row + 1], z = pts[3 * (size_t)row + 2];
    int slot = -1;
    const double r2 = x * x + y * y + z * z;
    if (!crop || (r2 > min2 && r2 < max2)) {
        unsigned long long key;
        if (voxel_key(x, y, z, size, &key)) {
            slot = find_or_insert(tkeys, tmask, key);
            if (slot >= 0) atomicMin(&tmin[slot], i);
            else atomicExch(&flags[kFlagTableFull], 1);
        } else if (r2 == r2) {
            atomicExch(&flags[kFlagCoordRange], 1);
        }
    }
    slotOf[i] = slot;
}

// pass 2: the winners, compacted in ascending index by ONE workgroup (a chunk of consecutive candidates per thread)
__global__ __launch_bounds__(1024) void ds_compact_kernel(const int32_t *__restrict__ rows, const int32_t *__restrict__ d_n, int n_max,
                                                          const int32_t *__restrict__ tmin, const int32_t *__restrict__ slotOf,
                                                          int32_t *__restrict__ out, int32_t *__restrict__ d_count)
{
    __shared__ int part[1024];
    const int n = d_n ? min(*d_n, n_max) : n_max;
    const int t = threadIdx.x, chunk = (n + 1023) / 1024;
    const int lo = min(t * chunk, n), hi = min(lo + chunk, n);
    int c = 0;
    for (int i = lo; i < hi; ++i) {
        const int s = slotOf[i];
        c += (s >= 0 && tmin[s] == i) ? 1 : 0;
    }
    part[t] = c;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {   // inclusive scan
        const int v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int w = part[t] - c;
    for (int i = lo; i < hi; ++i) {
        const int s = slotOf[i];
        if (s >= 0 && tmin[s] == i) out[w++] = rows ? rows[i] : i;
    }
    if (t == 1023) *d_count = part[1023];
}

// ---- step 5: the registration loop ------------------------------------------------------------------------------------------
struct RegArgs {
    double guess[16];
    double sigma, voxel, convergence;
    int max_iterations, per_voxel;
};

// exp of the twist (v, w) applied from the left: T <- exp(dx) T  (T: rows 0..2 of the 4 x 4, row-major [3][4])
__device__ void step_pose(const double *dx, double *T)
{
    const double wx = dx[3], wy = dx[4], wz = dx[5];
    const double th2 = wx * wx + wy * wy + wz * wz, th = sqrt(th2);
    double A, B, C;
    if (th < 1e-4) {
        A = 1.0 - th2 / 6.0, B = 0.5 - th2 / 24.0, C = 1.0 / 6.0 - th2 / 120.0;
    } else {
        A = sin(th) / th, B = (1.0 - cos(th)) / th2, C = (th - sin(th)) / (th2 * th);
    }
    const double K[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
    double K2[9], R[9], V[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) K2[3 * r + c] = K[3 * r] * K[c] + K[3 * r + 1] * K[3 + c] + K[3 * r + 2] * K[6 + c];
    for (int k = 0; k < 9; ++k) {
        const double I = (k % 4 == 0) ? 1.0 : 0.0;
        R[k] = I + A * K[k] + B * K2[k];
        V[k] = I + B * K[k] + C * K2[k];
    }
    double t[3], N[12];
    for (int r = 0; r < 3; ++r) t[r] = V[3 * r] * dx[0] + V[3 * r + 1] * dx[1] + V[3 * r + 2] * dx[2];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c)
            N[4 * r + c] = R[3 * r] * T[c] + R[3 * r + 1] * T[4 + c] + R[3 * r + 2] * T[8 + c] + (c == 3 ? t[r] : 0.0);
    for (int k = 0; k < 12; ++k) T[k] = N[k];
}

// A dx = b, 6 x 6 symmetric from its upper triangle, Gaussian elimination with partial pivoting; false when singular
__device__ bool solve6(const double *S, double *dx)
{
    double M[6][7];
    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b, ++k) M[a][b] = M[b][a] = S[k];
    for (int a = 0; a < 6; ++a) M[a][6] = -S[21 + a];
    for (int c = 0; c < 6; ++c) {
        int p = c;
        for (int r = c + 1; r < 6; ++r)
            if (fabs(M[r][c]) > fabs(M[p][c])) p = r;
        if (!(fabs(M[p][c]) > 0.0)) return false;
        if (p != c)
            for (int j = 0; j < 7; ++j) { const double s = M[c][j]; M[c][j] = M[p][j]; M[p][j] = s; }
        for (int r = c + 1; r < 6; ++r) {
            const double f = M[r][c] / M[c][c];
            for (int j = c; j < 7; ++j) M[r][j] -= f * M[c][j];
        }
    }
    for (int r = 5; r >= 0; --r) {
        double s = M[r][6];
        for (int j = r + 1; j < 6; ++j) s -= M[r][j] * dx[j];
        dx[r] = s / M[r][r];
    }
    return true;
}

__global__ __launch_bounds__(kRegThreads) void ego_register_kernel(const float *__restrict__ pts, const int32_t *__restrict__ rows,
                                                                   const int32_t *__restrict__ d_m, int m_max, MapTable map,
                                                                   unsigned mask, RegArgs a, double *__restrict__ result)
{
    __shared__ double Tsh[12];
    __shared__ double wsum[kRegWaves][kSums];
    __shared__ double total[kSums];
    __shared__ int stop;
    __shared__ int itersDone;
    __shared__ double lastDx;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m = d_m ? min(*d_m, m_max) : m_max;
    if (t < 12) Tsh[t] = a.guess[t];
    if (t == 0) stop = 0, itersDone = 0, lastDx = 0.0;
    __syncthreads();
    const double gate2 = (3.0 * a.sigma) * (3.0 * a.sigma), kern = a.sigma / 3.0;
    double corr = 0.0;
    for (int it = 0; it < a.max_iterations; ++it) {
        double T[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = Tsh[k];
        double acc[kSums];
#pragma unroll
        for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
        for (int i = t; i < m; i += kRegThreads) {
            const size_t row = rows ? (size_t)rows[i] : (size_t)i;
            const double px = pts[3 * row], py = pts[3 * row + 1], pz = pts[3 * row + 2];
            const double x = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
            const double y = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
            const double z = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
            const double fx = floor(x / a.voxel), fy = floor(y / a.voxel), fz = floor(z / a.voxel);
            const double lim = (double)(kCoordBias - 2);
            if (!(fabs(fx) < lim && fabs(fy) < lim && fabs(fz) < lim)) continue;
            const long long ix = (long long)fx, iy = (long long)fy, iz = (long long)fz;
            double best = INFINITY, qx = 0.0, qy = 0.0, qz = 0.0;
            for (int ox = -1; ox <= 1; ++ox)
                for (int oy = -1; oy <= 1; ++oy)
                    for (int oz = -1; oz <= 1; ++oz) {
                        const int s = find_slot(map.keys, mask, pack_key(ix + ox, iy + oy, iz + oz));
                        if (s < 0) continue;
                        const int c = min(map.count[s], a.per_voxel);
                        const float *q = map.pts + (size_t)s * (kVoxelPoints * 3);
                        for (int j = 0; j < c; ++j) {
                            const double ax = q[3 * j], ay = q[3 * j + 1], az = q[3 * j + 2];
                            const double ex = x - ax, ey = y - ay, ez = z - az;
                            const double d2 = (ex * ex + ey * ey) + ez * ez;
                            if (d2 < best) best = d2, qx = ax, qy = ay, qz = az;
                        }
                    }
            if (!(best < gate2)) continue;
            const double r[3] = {x - qx, y - qy, z - qz};
            const double wq = kern / (kern + best), w = wq * wq;
            const double J[3][6] = {{1.0, 0.0, 0.0, 0.0, z, -y}, {0.0, 1.0, 0.0, -z, 0.0, x}, {0.0, 0.0, 1.0, y, -x, 0.0}};
            int k = 0;
#pragma unroll
            for (int p = 0; p < 6; ++p)
#pragma unroll
                for (int q2 = p; q2 < 6; ++q2, ++k) acc[k] += w * ((J[0][p] * J[0][q2] + J[1][p] * J[1][q2]) + J[2][p] * J[2][q2]);
#pragma unroll
            for (int p = 0; p < 6; ++p) acc[21 + p] += w * ((J[0][p] * r[0] + J[1][p] * r[1]) + J[2][p] * r[2]);
            acc[27] += 1.0;
        }
#pragma unroll
        for (int k = 0; k < kSums; ++k) {
            double v = acc[k];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if (lane == 0) wsum[wave][k] = v;
        }
        __syncthreads();
        if (t < kSums) {
            double v = 0.0;
            for (int w = 0; w < kRegWaves; ++w) v += wsum[w][t];
            total[t] = v;
        }
        __syncthreads();
        if (t == 0) {
            double S[kSums], dx[6], Tn[12];
            for (int k = 0; k < kSums; ++k) S[k] = total[k];
            corr = S[27];
            bool ok = S[27] >= 3.0 && solve6(S, dx);
            double nrm = 0.0;
            if (ok) {
                for (int k = 0; k < 6; ++k) nrm += dx[k] * dx[k];
                nrm = sqrt(nrm);
                ok = nrm == nrm && nrm < INFINITY;
            }
            itersDone = it + 1;
            if (ok) {
                for (int k = 0; k < 12; ++k) Tn[k] = Tsh[k];
                step_pose(dx, Tn);
                for (int k = 0; k < 12; ++k) Tsh[k] = Tn[k];
                lastDx = nrm;
                if (nrm < a.convergence) stop = 1;
            } else {
                stop = 1;
            }
        }
        __syncthreads();
        if (stop) break;
    }
    if (t == 0) {
        for (int k = 0; k < 12; ++k) result[k] = Tsh[k];
        result[12] = result[13] = result[14] = 0.0;
        result[15] = 1.0;
        result[16] = (double)itersDone;
        result[17] = lastDx;
        result[18] = corr;
        result[19] = 0.0;
    }
}

// with a map that has received no frame since the state was created or reset (frame 0) the result is the guess
__global__ void ego_guess_kernel(RegArgs a, double *__restrict__ result)
{
    const int t = threadIdx.x;
    if (t < 16) result[t] = a.guess[t];
    if (t >= 16 && t < 20) result[t] = 0.0;
}

// ---- step 6: the map ----------------------------------------------------------------------------------------------------------
// pass 1: move the frame's points by the pose (device memory: the registration's result), claim their voxels
__global__ void map_claim_kernel(const float *__restrict__ pts, const int32_t *__restrict__ rows, const int32_t *__restrict__ d_n,
                                 int n_max, const double *__restrict__ pose, double voxel, MapTable map, unsigned mask,
                                 float *__restrict__ moved, int32_t *__restrict__ slotOf, int32_t *flags)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = d_n ? min(*d_n, n_max) : n_max;
    if (i >= n) return;
    const size_t row = rows ? (size_t)rows[i] : (size_t)i;
    const double px = pts[3 * row], py = pts[3 * row + 1], pz = pts[3 * row + 2];
    const float x = (float)(((pose[0] * px + pose[1] * py) + pose[2] * pz) + pose[3]);
    const float y = (float)(((pose[4] * px + pose[5] * py) + pose[6] * pz) + pose[7]);
    const float z = (float)(((pose[8] * px + pose[9] * py) + pose[10] * pz) + pose[11]);
    moved[3 * (size_t)i] = x, moved[3 * (size_t)i + 1] = y, moved[3 * (size_t)i + 2] = z;
    unsigned long long key;
    int slot = -1;
    if (voxel_key((double)x, (double)y, (double)z, voxel, &key)) {
        slot = find_or_insert(map.keys, mask, key);
        if (slot < 0) atomicExch(&flags[kFlagTableFull], 1);
    } else if (x == x && y == y && z == z) {
        atomicExch(&flags[kFlagCoordRange], 1);
    }
    slotOf[i] = slot;
}

// pass 2: point i enters its voxel behind the points already there and the frame's lower-indexed points of the same voxel
// (a tiled all-pairs count: a frame_ds is a few thousand points); the voxel's count is NOT touched here, every thread reads it
__global__ __launch_bounds__(256) void map_append_kernel(const int32_t *__restrict__ d_n, int n_max, const float *__restrict__ moved,
                                                         const int32_t *__restrict__ slotOf, MapTable map, int per_voxel,
                                                         int32_t *__restrict__ sameTotal)
{
    __shared__ int tile[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = d_n ? min(*d_n, n_max) : n_max;
    if (blockIdx.x * 256 >= n) return;   // (whole block)
    const int mine = i < n ? slotOf[i] : -1;
    int before = 0, all = 0;
    for (int base = 0; base < n; base += 256) {
        const int j = base + threadIdx.x;
        tile[threadIdx.x] = j < n ? slotOf[j] : -2;
        __syncthreads();
        if (mine >= 0) {
            const int lim = min(256, n - base);
            for (int k = 0; k < lim; ++k) {
                const int same = tile[k] == mine ? 1 : 0;
                all += same;
                before += (base + k < i) ? same : 0;
            }
        }
        __syncthreads();
    }
    if (i >= n) return;
    sameTotal[i] = before == 0 ? all : 0;   // the voxel's first point of this frame carries the frame's total
    if (mine < 0) return;
    const int at = map.count[mine] + before;
    if (at < per_voxel) {
        float *q = map.pts + (size_t)mine * (kVoxelPoints * 3) + 3 * at;
        q[0] = moved[3 * (size_t)i], q[1] = moved[3 * (size_t)i + 1], q[2] = moved[3 * (size_t)i + 2];
    }
}

// pass 3: the counts
__global__ void map_count_kernel(const int32_t *__restrict__ d_n, int n_max, const int32_t *__restrict__ slotOf,
                                 const int32_t *__restrict__ sameTotal, MapTable map, int per_voxel)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = d_n ? min(*d_n, n_max) : n_max;
    if (i >= n) return;
    const int s = slotOf[i], add = sameTotal[i];
    if (s >= 0 && add > 0) map.count[s] = min(map.count[s] + add, per_voxel);
}

// the prune: the voxels whose first point is within range of the new position move to the other (cleared) table
__global__ void map_prune_kernel(MapTable from, MapTable to, unsigned mask, const double *__restrict__ pose, double max2,
                                 int32_t *flags)
{
    const unsigned s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s > mask) return;
    const unsigned long long key = from.keys[s];
    if (key == kEmpty) return;
    const int c = from.count[s];
    if (c <= 0) return;
    const float *q = from.pts + (size_t)s * (kVoxelPoints * 3);
    const double ex = (double)q[0] - pose[3], ey = (double)q[1] - pose[7], ez = (double)q[2] - pose[11];
    if ((ex * ex + ey * ey) + ez * ez > max2) return;
    const int d = find_or_insert(to.keys, mask, key);
    if (d < 0) {
        atomicExch(&flags[kFlagTableFull], 1);
        return;
    }
    to.count[d] = c;
    float *o = to.pts + (size_t)d * (kVoxelPoints * 3);
    for (int k = 0; k < 3 * c; ++k) o[k] = q[k];
    atomicAdd(&flags[kFlagLive], 1);
}

__global__ void map_export_kernel(MapTable map, unsigned mask, int per_voxel, long long *__restrict__ keys,
                                  int32_t *__restrict__ counts, float *__restrict__ pts, int capacity, int32_t *d_num)
{
    const unsigned s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s > mask) return;
    const unsigned long long key = map.keys[s];
    if (key == kEmpty || map.count[s] <= 0) return;
    const int at = atomicAdd(d_num, 1);
    if (at >= capacity) return;
    keys[at] = (long long)key;
    const int c = min(map.count[s], per_voxel);
    counts[at] = c;
    const float *q = map.pts + (size_t)s * (kVoxelPoints * 3);
    for (int k = 0; k < 3 * per_voxel; ++k) pts[(size_t)at * (3 * per_voxel) + k] = k < 3 * c ? q[k] : 0.0f;
}

// ---- host -------------------------------------------------------------------------------------------------------------------
struct Carve {
    size_t keys[2], count[2], pts[2], tkeys, tmin, slotOf, idxDs, idxSrc, moved, sameTotal, counts, result, flags, total;
    unsigned tcap;
};

Carve carve(const icpflow_ego_params_t &p)
{
    Carve c{};
    Carver mem;
    const size_t C = (size_t)p.map_capacity, n = (size_t)p.max_points;
    for (int k = 0; k < 2; ++k) {
        c.keys[k] = mem.take(C * 8);
        c.count[k] = mem.take(C * 4);
        c.pts[k] = mem.take(C * kVoxelPoints * 3 * 4);
    }
    unsigned tcap = 1024;
    while ((size_t)tcap < 2 * n) tcap <<= 1;
    c.tcap = tcap;
    c.tkeys = mem.take((size_t)tcap * 8);
    c.tmin = mem.take((size_t)tcap * 4);
    c.slotOf = mem.take(n * 4);
    c.idxDs = mem.take(n * 4);
    c.idxSrc = mem.take(n * 4);
    c.moved = mem.take(n * 12);
    c.sameTotal = mem.take(n * 4);
    c.counts = mem.take(4 * 4);
    c.result = mem.take(20 * 8);
    c.flags = mem.take(kNumFlags * 4);
    c.total = mem.total();
    return c;
}

const char *check_params(const icpflow_ego_params_t *p)
{
    if (!p) return "icpflow_ego: null pointer (params)";
    if (p->struct_size != sizeof(icpflow_ego_params_t)) return "icpflow_ego: params.struct_size is not sizeof(icpflow_ego_params_t)";
    if (!(p->max_range > 0.0) || !(p->min_range >= 0.0) || !(p->min_range < p->max_range)) return "icpflow_ego: need 0 <= min_range < max_range";
    if (!(p->voxel_size >= 0.0)) return "icpflow_ego: voxel_size must be >= 0 (0 = max_range / 100)";
    if (!(p->min_motion_th >= 0.0) || !(p->initial_threshold > 0.0) || !(p->convergence > 0.0))
        return "icpflow_ego: need min_motion_th >= 0, initial_threshold > 0, convergence > 0";
    if (p->max_points_per_voxel < 1 || p->max_points_per_voxel > kVoxelPoints) return "icpflow_ego: max_points_per_voxel must be 1 .. 20";
    if (p->max_iterations < 1) return "icpflow_ego: max_iterations must be >= 1";
    if (p->max_points < 1 || p->max_points > (1 << 24)) return "icpflow_ego: max_points must be 1 .. 2^24";
    if (p->map_capacity < 1024 || p->map_capacity > (1 << 26) || (p->map_capacity & (p->map_capacity - 1)))
        return "icpflow_ego: map_capacity must be a power of two, 1024 .. 2^26";
    return nullptr;
}

struct Mat4 {
    double v[16];
};

Mat4 identity()
{
    Mat4 m{};
    m.v[0] = m.v[5] = m.v[10] = m.v[15] = 1.0;
    return m;
}

Mat4 mul(const Mat4 &a, const Mat4 &b)
{
    Mat4 o{};
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += a.v[4 * r + k] * b.v[4 * k + c];
            o.v[4 * r + c] = s;
        }
    return o;
}

Mat4 rigid_inverse(const Mat4 &a)
{
    Mat4 o = identity();
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) o.v[4 * r + c] = a.v[4 * c + r];
    for (int r = 0; r < 3; ++r) o.v[4 * r + 3] = -(o.v[4 * r] * a.v[3] + o.v[4 * r + 1] * a.v[7] + o.v[4 * r + 2] * a.v[11]);
    return o;
}

}  // namespace

struct icpflow_ego {
    icpflow_ego_params_t par;
    double voxel;
    char *mem;
    Carve c;
    int cur;                  // the live map table
    bool mapEmpty;
    std::vector<Mat4> poses;
    double sse;
    int numSamples;
    double *h_back;           // pinned: result [20] + flags + counts
    double info[kInfoWords];
    icpflow_ego_motion_params_t motion;   // host only; kept across a reset

    MapTable table(int k) const
    {
        return MapTable{(unsigned long long *)(mem + c.keys[k]), (int32_t *)(mem + c.count[k]), (float *)(mem + c.pts[k])};
    }
    template <class T> T *at(size_t off) const { return (T *)(mem + off); }
};

namespace {

constexpr int kBackDoubles = 20 + 4;   // result, then (as int32) flags [4] + counts [4]

int clear_scratch_table(icpflow_ego *e, hipStream_t st)
{
    ICPFLOW_TRY(hipMemsetAsync(e->mem + e->c.tkeys, 0xFF, (size_t)e->c.tcap * 8, st));
    ICPFLOW_TRY(hipMemsetAsync(e->mem + e->c.tmin, 0x7F, (size_t)e->c.tcap * 4, st));
    return 0;
}

// steps 1-2 into the state's own lists (idxDs, idxSrc, counts[0..1])
int enqueue_downsample(icpflow_ego *e, const float *d_points, int n, hipStream_t st)
{
    const icpflow_ego_params_t &p = e->par;
    int32_t *counts = e->at<int32_t>(e->c.counts), *slotOf = e->at<int32_t>(e->c.slotOf), *flags = e->at<int32_t>(e->c.flags);
    unsigned long long *tkeys = e->at<unsigned long long>(e->c.tkeys);
    int32_t *tmin = e->at<int32_t>(e->c.tmin);
    const int blocks = (n + 255) / 256;
    if (int rc = clear_scratch_table(e, st)) return rc;
    ds_vote_kernel<<<blocks, 256, 0, st>>>(d_points, nullptr, nullptr, n, 0.5 * e->voxel, 1, p.min_range * p.min_range,
                                           p.max_range * p.max_range, tkeys, tmin, e->c.tcap - 1, slotOf, flags);
    ds_compact_kernel<<<1, 1024, 0, st>>>(nullptr, nullptr, n, tmin, slotOf, e->at<int32_t>(e->c.idxDs), counts);
    if (int rc = clear_scratch_table(e, st)) return rc;
    ds_vote_kernel<<<blocks, 256, 0, st>>>(d_points, e->at<int32_t>(e->c.idxDs), counts, n, 1.5 * e->voxel, 0, 0.0, 0.0, tkeys, tmin,
                                           e->c.tcap - 1, slotOf, flags);
    ds_compact_kernel<<<1, 1024, 0, st>>>(e->at<int32_t>(e->c.idxDs), counts, n, tmin, slotOf, e->at<int32_t>(e->c.idxSrc), counts + 1);
    ICPFLOW_TRY(hipGetLastError());
    return 0;
}

RegArgs reg_args(const icpflow_ego *e, const double *guess, double sigma)
{
    RegArgs a;
    std::memcpy(a.guess, guess, sizeof(a.guess));
    a.sigma = sigma, a.voxel = e->voxel, a.convergence = e->par.convergence;
    a.max_iterations = e->par.max_iterations, a.per_voxel = e->par.max_points_per_voxel;
    return a;
}

int enqueue_register(icpflow_ego *e, const float *pts, const int32_t *rows, const int32_t *d_m, int m_max, const double *guess,
                     double sigma, double *d_result, hipStream_t st)
{
    const RegArgs a = reg_args(e, guess, sigma);
    // (a source of no points is no short cut: the loop runs once, finds fewer than 3 correspondences and stops -- the same
    // result whether the count is known here (m_max) or only on the device (d_m); a null `pts` is never read then)
    if (e->mapEmpty)
        ego_guess_kernel<<<1, 64, 0, st>>>(a, d_result);
    else
        ego_register_kernel<<<1, kRegThreads, 0, st>>>(pts, rows, d_m, m_max, e->table(e->cur), (unsigned)e->par.map_capacity - 1, a, d_result);
    ICPFLOW_TRY(hipGetLastError());
    return 0;
}

// the map half of step 6; d_pose: 16 doubles in device memory
int enqueue_map_add(icpflow_ego *e, const float *pts, const int32_t *rows, const int32_t *d_n, int n_max, const double *d_pose,
                    hipStream_t st)
{
    const icpflow_ego_params_t &p = e->par;
    const unsigned mask = (unsigned)p.map_capacity - 1;
    int32_t *slotOf = e->at<int32_t>(e->c.slotOf), *same = e->at<int32_t>(e->c.sameTotal), *flags = e->at<int32_t>(e->c.flags);
    float *moved = e->at<float>(e->c.moved);
    const MapTable cur = e->table(e->cur), nxt = e->table(e->cur ^ 1);
    if (n_max > 0) {
        const int blocks = (n_max + 255) / 256;
        map_claim_kernel<<<blocks, 256, 0, st>>>(pts, rows, d_n, n_max, d_pose, e->voxel, cur, mask, moved, slotOf, flags);
        map_append_kernel<<<blocks, 256, 0, st>>>(d_n, n_max, moved, slotOf, cur, p.max_points_per_voxel, same);
        map_count_kernel<<<blocks, 256, 0, st>>>(d_n, n_max, slotOf, same, cur, p.max_points_per_voxel);
    }
    ICPFLOW_TRY(hipMemsetAsync(nxt.keys, 0xFF, (size_t)p.map_capacity * 8, st));
    ICPFLOW_TRY(hipMemsetAsync(nxt.count, 0, (size_t)p.map_capacity * 4, st));
    ICPFLOW_TRY(hipMemsetAsync(flags + kFlagLive, 0, 4, st));
    map_prune_kernel<<<(p.map_capacity + 255) / 256, 256, 0, st>>>(cur, nxt, mask, d_pose, p.max_range * p.max_range, flags);
    ICPFLOW_TRY(hipGetLastError());
    e->cur ^= 1;
    e->mapEmpty = false;
    return 0;
}

int enqueue_reset(icpflow_ego *e, hipStream_t st)
{
    const MapTable t = e->table(e->cur);
    ICPFLOW_TRY(hipMemsetAsync(t.keys, 0xFF, (size_t)e->par.map_capacity * 8, st));
    ICPFLOW_TRY(hipMemsetAsync(t.count, 0, (size_t)e->par.map_capacity * 4, st));
    ICPFLOW_TRY(hipMemsetAsync(e->mem + e->c.flags, 0, kNumFlags * 4, st));
    ICPFLOW_TRY(hipMemsetAsync(e->mem + e->c.counts, 0, 16, st));
    e->mapEmpty = true;
    e->poses.clear();
    e->sse = 0.0, e->numSamples = 0;
    std::memset(e->info, 0, sizeof(e->info));
    return 0;
}

void default_motion(icpflow_ego_motion_params_t *p)
{
    std::memset(p, 0, sizeof(*p));
    p->struct_size = sizeof(*p);
    p->deskew = 0, p->mid_stamp = 0.5, p->fixed_threshold = 0.0;
}

// the log of the rigid motion D in the kernel's terms: angle w, K = [axis]_x, K2 = K K, rho = V^-1 t with
// V^-1 = I - (w / 2) K + (1 - (w / 2) cot(w / 2)) K2; false for a half turn, which has no axis to read off the skew part
bool twist_of(const Mat4 &D, double mid, DeskewArgs *a)
{
    std::memset(a, 0, sizeof(*a));
    a->mid = mid;
    const double v[3] = {0.5 * (D.v[9] - D.v[6]), 0.5 * (D.v[2] - D.v[8]), 0.5 * (D.v[4] - D.v[1])};
    const double s = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]), c = 0.5 * (((D.v[0] + D.v[5]) + D.v[10]) - 1.0);
    const double t[3] = {D.v[3], D.v[7], D.v[11]};
    if (!(s > 0.0)) {
        if (!(c > 0.0)) return false;
        for (int k = 0; k < 3; ++k) a->rho[k] = t[k];   // no rotation: w = 0, K = K2 = 0
        return true;
    }
    const double w = std::atan2(s, c), ax[3] = {v[0] / s, v[1] / s, v[2] / s};
    const double K[9] = {0.0, -ax[2], ax[1], ax[2], 0.0, -ax[0], -ax[1], ax[0], 0.0};
    a->w = w;
    for (int r = 0; r < 3; ++r)
        for (int cc = 0; cc < 3; ++cc) {
            a->K[3 * r + cc] = K[3 * r + cc];
            a->K2[3 * r + cc] = (K[3 * r] * K[cc] + K[3 * r + 1] * K[3 + cc]) + K[3 * r + 2] * K[6 + cc];
        }
    const double h = 0.5 * w;
    const double g = w < kSeriesBelow ? (w * w) * (1.0 / 12.0 + (w * w) / 720.0) : 1.0 - h * std::cos(h) / std::sin(h);
    for (int r = 0; r < 3; ++r) {
        const double kt = (a->K[3 * r] * t[0] + a->K[3 * r + 1] * t[1]) + a->K[3 * r + 2] * t[2];
        const double k2t = (a->K2[3 * r] * t[0] + a->K2[3 * r + 1] * t[1]) + a->K2[3 * r + 2] * t[2];
        a->rho[r] = t[r] + (g * k2t - h * kt);
    }
    return true;
}

// step 0 into d_out: the points moved by exp((stamp - mid_stamp) xi), xi from h_poses [2][16] or the state's last two
// poses; a copy with fewer than two poses
int enqueue_deskew(icpflow_ego *e, const char *fn, const float *d_points, const float *d_stamps, int n, const double *h_poses,
                   float *d_out, hipStream_t st)
{
    if (n == 0) return 0;
    const size_t np = e->poses.size();
    if (!h_poses && np < 2) {
        if (d_out != d_points) ICPFLOW_TRY(hipMemcpyAsync(d_out, d_points, (size_t)n * 12, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    Mat4 prev, last;
    if (h_poses) {
        std::memcpy(prev.v, h_poses, sizeof(prev.v));
        std::memcpy(last.v, h_poses + 16, sizeof(last.v));
    } else {
        prev = e->poses[np - 2], last = e->poses[np - 1];
    }
    DeskewArgs a;
    if (!twist_of(mul(rigid_inverse(prev), last), e->motion.mid_stamp, &a))
        return icpflow::report_errorf(ICPFLOW_E_ARG, "%s: the two poses differ by a half turn (or are not finite): no twist to interpolate", fn);
    ego_deskew_kernel<<<(n + 255) / 256, 256, 0, st>>>(d_points, d_stamps, n, a, d_out);
    ICPFLOW_TRY(hipGetLastError());
    return 0;
}

double model_error(const Mat4 &dev, double max_range)
{
    const double tr = dev.v[0] + dev.v[5] + dev.v[10];
    const double cs = std::fmin(1.0, std::fmax(-1.0, 0.5 * (tr - 1.0)));
    const double theta = std::acos(cs);
    const double dt = std::sqrt(dev.v[3] * dev.v[3] + dev.v[7] * dev.v[7] + dev.v[11] * dev.v[11]);
    return dt + 2.0 * max_range * std::sin(0.5 * theta);
}

}  // namespace

extern "C" {

int icpflow_ego_default_params(icpflow_ego_params_t *p)
{
    if (!p) return pointer_error("icpflow_ego_default_params");
    std::memset(p, 0, sizeof(*p));
    p->struct_size = sizeof(*p);
    p->max_range = 100.0, p->min_range = 1.0, p->voxel_size = 0.0, p->min_motion_th = 0.1, p->initial_threshold = 10.0;
    p->convergence = 1e-4, p->max_points_per_voxel = 20, p->max_iterations = 500;
    p->max_points = 1 << 18, p->map_capacity = 1 << 19;
    return ICPFLOW_OK;
}

size_t icpflow_ego_state_bytes(const icpflow_ego_params_t *params)
{
    if (check_params(params)) return 0;
    return carve(*params).total;
}

int icpflow_ego_create(const icpflow_ego_params_t *params, void *d_mem, size_t mem_bytes, icpflow_stream_t stream, icpflow_ego_t **out)
{
    if (const char *why = check_params(params)) return report_error(ICPFLOW_E_ARG, why);
    if (!out) return pointer_error("icpflow_ego_create");
    *out = nullptr;
    const Carve c = carve(*params);
    if (!d_mem || mem_bytes < c.total) return icpflow::workspace_error("icpflow_ego_create", "icpflow_ego_state_bytes", d_mem, mem_bytes, c.total);
    if (((uintptr_t)d_mem & 7) != 0) return report_error(ICPFLOW_E_ARG, "icpflow_ego_create: d_mem must be 8-byte aligned");
    icpflow_ego *e = new (std::nothrow) icpflow_ego();
    if (!e) return report_error(ICPFLOW_E_HOSTMEM, "icpflow_ego_create: out of host memory");
    e->par = *params;
    e->voxel = params->voxel_size > 0.0 ? params->voxel_size : params->max_range / 100.0;
    e->mem = (char *)d_mem;
    e->c = c;
    e->cur = 0;
    e->h_back = nullptr;
    default_motion(&e->motion);
    if (hipHostMalloc((void **)&e->h_back, kBackDoubles * sizeof(double), hipHostMallocDefault) != hipSuccess) {
        delete e;
        return report_error(ICPFLOW_E_HOSTMEM, "icpflow_ego_create: pinned host memory could not be allocated");
    }
    if (int rc = enqueue_reset(e, (hipStream_t)stream)) {
        (void)hipHostFree(e->h_back);
        delete e;
        return rc;
    }
    *out = e;
    return ICPFLOW_OK;
}

int icpflow_ego_destroy(icpflow_ego_t *e)
{
    if (!e) return ICPFLOW_OK;
    if (e->h_back) (void)hipHostFree(e->h_back);
    delete e;
    return ICPFLOW_OK;
}

int icpflow_ego_reset(icpflow_ego_t *e, icpflow_stream_t stream)
{
    if (!e) return pointer_error("icpflow_ego_reset");
    return enqueue_reset(e, (hipStream_t)stream);
}

int icpflow_ego_downsample(icpflow_ego_t *e, const float *d_points, int n, int32_t *d_idx_ds, int32_t *d_idx_source, int32_t *d_counts,
                           icpflow_stream_t stream)
{
    if (!e || !d_idx_ds || !d_idx_source || !d_counts || (n > 0 && !d_points)) return pointer_error("icpflow_ego_downsample");
    if (n < 0) return report_error(ICPFLOW_E_ARG, "icpflow_ego_downsample: n < 0");
    if (n > e->par.max_points) return report_error(ICPFLOW_E_LIMIT, "icpflow_ego_downsample: n beyond the state's max_points");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        ICPFLOW_TRY(hipMemsetAsync(d_counts, 0, 8, st));
        return ICPFLOW_OK;
    }
    if (int rc = enqueue_downsample(e, d_points, n, st)) return rc;
    ICPFLOW_TRY(hipMemcpyAsync(d_idx_ds, e->mem + e->c.idxDs, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    ICPFLOW_TRY(hipMemcpyAsync(d_idx_source, e->mem + e->c.idxSrc, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    ICPFLOW_TRY(hipMemcpyAsync(d_counts, e->mem + e->c.counts, 8, hipMemcpyDeviceToDevice, st));
    return ICPFLOW_OK;
}

int icpflow_ego_register_step(icpflow_ego_t *e, const float *d_source, int m, const double *h_guess, double sigma, double *d_result,
                              icpflow_stream_t stream)
{
    if (!e || !h_guess || !d_result || (m > 0 && !d_source)) return pointer_error("icpflow_ego_register_step");
    if (m < 0) return report_error(ICPFLOW_E_ARG, "icpflow_ego_register_step: m < 0");
    if (!(sigma > 0.0)) return report_error(ICPFLOW_E_ARG, "icpflow_ego_register_step: sigma must be > 0");
    return enqueue_register(e, d_source, nullptr, nullptr, m, h_guess, sigma, d_result, (hipStream_t)stream);
}

int icpflow_ego_map_add(icpflow_ego_t *e, const float *d_points, int n, const double *h_pose, icpflow_stream_t stream)
{
    if (!e || !h_pose || (n > 0 && !d_points)) return pointer_error("icpflow_ego_map_add");
    if (n < 0) return report_error(ICPFLOW_E_ARG, "icpflow_ego_map_add: n < 0");
    if (n > e->par.max_points) return report_error(ICPFLOW_E_LIMIT, "icpflow_ego_map_add: n beyond the state's max_points");
    hipStream_t st = (hipStream_t)stream;
    RegArgs a = reg_args(e, h_pose, 1.0);
    double *d_pose = e->at<double>(e->c.result);
    ego_guess_kernel<<<1, 64, 0, st>>>(a, d_pose);   // the pose travels as a kernel argument: no host buffer to keep alive
    return enqueue_map_add(e, d_points, nullptr, nullptr, n, d_pose, st);
}

int icpflow_ego_map_export(icpflow_ego_t *e, int64_t *d_keys, int32_t *d_counts, float *d_points, int capacity, int32_t *d_num,
                           icpflow_stream_t stream)
{
    if (!e || !d_num || (capacity > 0 && (!d_keys || !d_counts || !d_points))) return pointer_error("icpflow_ego_map_export");
    if (capacity < 0) return report_error(ICPFLOW_E_ARG, "icpflow_ego_map_export: capacity < 0");
    hipStream_t st = (hipStream_t)stream;
    ICPFLOW_TRY(hipMemsetAsync(d_num, 0, 4, st));
    map_export_kernel<<<(e->par.map_capacity + 255) / 256, 256, 0, st>>>(e->table(e->cur), (unsigned)e->par.map_capacity - 1,
                                                                         e->par.max_points_per_voxel, (long long *)d_keys, d_counts,
                                                                         d_points, capacity, d_num);
    ICPFLOW_TRY(hipGetLastError());
    return ICPFLOW_OK;
}

int icpflow_ego_register_frame(icpflow_ego_t *e, const float *d_points, int n, double *h_pose_out, icpflow_stream_t stream)
{
    if (!e || !h_pose_out || (n > 0 && !d_points)) return pointer_error("icpflow_ego_register_frame");
    if (n < 0) return report_error(ICPFLOW_E_ARG, "icpflow_ego_register_frame: n < 0");
    if (n > e->par.max_points) return report_error(ICPFLOW_E_LIMIT, "icpflow_ego_register_frame: n beyond the state's max_points");
    hipStream_t st = (hipStream_t)stream;
    const icpflow_ego_params_t &p = e->par;
    // steps 3-4 need nothing from the device
    const size_t np = e->poses.size();
    const Mat4 last = np ? e->poses[np - 1] : identity();
    const Mat4 guess = np >= 2 ? mul(last, mul(rigid_inverse(e->poses[np - 2]), last)) : last;
    const double moved = std::sqrt(last.v[3] * last.v[3] + last.v[7] * last.v[7] + last.v[11] * last.v[11]);
    const bool adaptive = moved > 5.0 * p.min_motion_th && e->numSamples > 0;
    const double sigma = e->motion.fixed_threshold > 0.0 ? e->motion.fixed_threshold
                         : adaptive                      ? std::sqrt(e->sse / e->numSamples)
                                                         : p.initial_threshold;
    int32_t *counts = e->at<int32_t>(e->c.counts);
    double *d_result = e->at<double>(e->c.result);
    if (n > 0) {
        if (int rc = enqueue_downsample(e, d_points, n, st)) return rc;
    } else {
        ICPFLOW_TRY(hipMemsetAsync(counts, 0, 8, st));
    }
    if (int rc = enqueue_register(e, d_points, e->at<int32_t>(e->c.idxSrc), counts + 1, n, guess.v, sigma, d_result, st)) return rc;
    if (int rc = enqueue_map_add(e, d_points, e->at<int32_t>(e->c.idxDs), counts, n, d_result, st)) return rc;
    // the frame's one read-back
    ICPFLOW_TRY(hipMemcpyAsync(e->h_back, d_result, 20 * 8, hipMemcpyDeviceToHost, st));
    ICPFLOW_TRY(hipMemcpyAsync(e->h_back + 20, e->mem + e->c.flags, kNumFlags * 4, hipMemcpyDeviceToHost, st));
    ICPFLOW_TRY(hipMemcpyAsync(e->h_back + 22, counts, 16, hipMemcpyDeviceToHost, st));
    ICPFLOW_TRY(hipStreamSynchronize(st));
    const int32_t *hflags = (const int32_t *)(e->h_back + 20), *hcounts = (const int32_t *)(e->h_back + 22);
    Mat4 pose;
    std::memcpy(pose.v, e->h_back, sizeof(pose.v));
    e->info[0] = hcounts[0], e->info[1] = hcounts[1], e->info[2] = e->h_back[16], e->info[3] = e->h_back[17];
    e->info[4] = e->h_back[18], e->info[5] = sigma, e->info[6] = hflags[kFlagLive], e->info[7] = 0.0;
    if (hflags[kFlagTableFull] || hflags[kFlagCoordRange]) {
        (void)hipMemsetAsync(e->mem + e->c.flags, 0, kNumFlags * 4, st);
        return report_error(ICPFLOW_E_LIMIT, hflags[kFlagTableFull]
                                                 ? "icpflow_ego_register_frame: a voxel table is full (map_capacity / max_points too small); reset the state"
                                                 : "icpflow_ego_register_frame: a coordinate leaves the 2^20 voxels a key holds; reset the state");
    }
    for (int k = 0; k < 16; ++k)
        if (!(pose.v[k] == pose.v[k])) return report_error(ICPFLOW_E_ARG, "icpflow_ego_register_frame: the pose is not finite (NaN input?); reset the state");
    // step 6, the odometry's half
    const double err = model_error(mul(rigid_inverse(guess), pose), p.max_range);
    if (err > p.min_motion_th) e->sse += err * err, e->numSamples += 1;
    e->poses.push_back(pose);
    std::memcpy(h_pose_out, pose.v, sizeof(pose.v));
    return ICPFLOW_OK;
}

int icpflow_ego_poses(const icpflow_ego_t *e, double *h_poses, int capacity, int *h_count)
{
    if (!e || !h_count || (capacity > 0 && !h_poses)) return pointer_error("icpflow_ego_poses");
    if (capacity < 0) return report_error(ICPFLOW_E_ARG, "icpflow_ego_poses: capacity < 0");
    *h_count = (int)e->poses.size();
    const size_t k = std::min((size_t)capacity, e->poses.size());
    for (size_t j = 0; j < k; ++j) std::memcpy(h_poses + 16 * j, e->poses[j].v, 16 * sizeof(double));
    return ICPFLOW_OK;
}

int icpflow_ego_frame_info(const icpflow_ego_t *e, double *h_info)
{
    if (!e || !h_info) return pointer_error("icpflow_ego_frame_info");
    std::memcpy(h_info, e->info, sizeof(e->info));
    return ICPFLOW_OK;
}

// ---- motion compensation and the fixed threshold (the estimator's second configuration) --------------------------------------
int icpflow_egomotion_default_params(icpflow_ego_motion_params_t *p)
{
    if (!p) return pointer_error("icpflow_egomotion_default_params");
    default_motion(p);
    return ICPFLOW_OK;
}

int icpflow_egomotion_set_params(icpflow_ego_t *e, const icpflow_ego_motion_params_t *p)
{
    if (!e || !p) return pointer_error("icpflow_egomotion_set_params");
    if (p->struct_size != sizeof(icpflow_ego_motion_params_t))
        return icpflow::report_errorf(ICPFLOW_E_ARG, "icpflow_egomotion_set_params: struct_size is %zu, sizeof(icpflow_ego_motion_params_t) is %zu",
                                      p->struct_size, sizeof(icpflow_ego_motion_params_t));
    if (p->deskew != 0 && p->deskew != 1) return icpflow::report_errorf(ICPFLOW_E_ARG, "icpflow_egomotion_set_params: deskew is %d, not 0 or 1", p->deskew);
    if (!std::isfinite(p->mid_stamp) || p->mid_stamp < 0.0)
        return icpflow::report_errorf(ICPFLOW_E_ARG, "icpflow_egomotion_set_params: mid_stamp is %g, need a finite value >= 0", p->mid_stamp);
    if (!std::isfinite(p->fixed_threshold) || p->fixed_threshold < 0.0)
        return icpflow::report_errorf(ICPFLOW_E_ARG, "icpflow_egomotion_set_params: fixed_threshold is %g, need a finite value >= 0 (0 = adaptive)",
                                      p->fixed_threshold);
    e->motion = *p;
    e->motion.reserved = 0;
    return ICPFLOW_OK;
}

int icpflow_egomotion_deskew(icpflow_ego_t *e, const float *d_points, const float *d_stamps, int n, const double *h_poses, float *d_out,
                             icpflow_stream_t stream)
{
    if (!e || (n > 0 && (!d_points || !d_stamps || !d_out))) return pointer_error("icpflow_egomotion_deskew");
    if (n < 0) return report_error(ICPFLOW_E_ARG, "icpflow_egomotion_deskew: n < 0");
    if (n > e->par.max_points) return report_error(ICPFLOW_E_LIMIT, "icpflow_egomotion_deskew: n beyond the state's max_points");
    return enqueue_deskew(e, "icpflow_egomotion_deskew", d_points, d_stamps, n, h_poses, d_out, (hipStream_t)stream);
}

int icpflow_egomotion_register_frame_stamped(icpflow_ego_t *e, const float *d_points, const float *d_stamps, int n, float *d_corrected,
                                             double *h_pose_out, icpflow_stream_t stream)
{
    if (!e) return pointer_error("icpflow_egomotion_register_frame_stamped");
    if (!e->motion.deskew || !d_stamps) return icpflow_ego_register_frame(e, d_points, n, h_pose_out, stream);
    if (!h_pose_out || (n > 0 && (!d_points || !d_corrected))) return pointer_error("icpflow_egomotion_register_frame_stamped");
    if (n < 0) return report_error(ICPFLOW_E_ARG, "icpflow_egomotion_register_frame_stamped: n < 0");
    if (n > e->par.max_points) return report_error(ICPFLOW_E_LIMIT, "icpflow_egomotion_register_frame_stamped: n beyond the state's max_points");
    if (int rc = enqueue_deskew(e, "icpflow_egomotion_register_frame_stamped", d_points, d_stamps, n, nullptr, d_corrected, (hipStream_t)stream))
        return rc;
    return icpflow_ego_register_frame(e, d_corrected, n, h_pose_out, stream);
}

}  // extern "C"
