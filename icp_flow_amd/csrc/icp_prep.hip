// icp_prep.hip -- what a registration prepares once, before its first iteration (launch_icp, icp.hip): the fixed cloud
// binned into the hashed grid (grid_build_kernel), or both clouds sorted along the fixed cloud's key for the sorted sweep
// (sort_clouds_kernel up to kChunkSortMinN points, sort.hip's chunked sort beyond).  The scoring sweep (nn.hip) takes the
// same sort, without a pre-pose and with the moving cloud's structure-of-arrays image.
//
// (sort_clouds_kernel is not in sort.hip: beside it, sort.hip's own kernels compile to other code.)
#include "scan.hpp"
#include "sortdir.hpp"
#include "kernels.hpp"
#include "gridhash.hpp"

namespace icpflow {

constexpr int kGridBlock = 256;

int grid_buckets(int N)
{
    int H = 64;
    while (H < 2 * N) H <<= 1;
    return H;
}

// One workgroup per pair.  counts/starts live in global scratch (L2 resident).
__global__ __launch_bounds__(kGridBlock) void grid_build_kernel(
    const float *__restrict__ X, const float *__restrict__ Y, const int32_t *__restrict__ lenX,
    const int32_t *__restrict__ lenY, const uint8_t *__restrict__ swap, int N, int H, float invh,
    float *__restrict__ origin, int32_t *__restrict__ start, int32_t *__restrict__ cursor,
    float4 *__restrict__ pts)
{
    __shared__ int part[kGridBlock];
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool sw = swap != nullptr && swap[b] != 0;
    const float4 *yb = reinterpret_cast<const float4 *>(sw ? X : Y) + (size_t)b * N;
    const int n = (sw ? lenX : lenY)[b];
    int32_t *st = start + (size_t)b * (H + 1);
    int32_t *cu = cursor + (size_t)b * H;
    float4 *out = pts + (size_t)b * N;
    const unsigned mask = (unsigned)H - 1u;
    float4 o4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n > 0) o4 = yb[0];
    if (tid == 0) { origin[b * 4 + 0] = o4.x; origin[b * 4 + 1] = o4.y; origin[b * 4 + 2] = o4.z; origin[b * 4 + 3] = 0.f; }
    for (int k = tid; k <= H; k += kGridBlock) st[k] = 0;
    __syncthreads();
    for (int j = tid; j < n; j += kGridBlock) {
        const float4 q = yb[j];
        const unsigned h = grid_hash(grid_cell(q.x, o4.x, invh), grid_cell(q.y, o4.y, invh),
                                     grid_cell(q.z, o4.z, invh), mask);
        atomicAdd(&st[h + 1], 1);
    }
    __syncthreads();
    // exclusive scan of st[1..H] in place: thread t owns a contiguous slice
    const int per = (H + kGridBlock - 1) / kGridBlock;
    const int lo = 1 + tid * per, hi = min(1 + (tid + 1) * per, H + 1);
    int sum = 0;
    for (int k = lo; k < hi; ++k) sum += st[k];
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int k = 0; k < kGridBlock; ++k) { const int v = part[k]; part[k] = run; run += v; }
    }
    __syncthreads();
    int run = part[tid];
    for (int k = lo; k < hi; ++k) { run += st[k]; st[k] = run; }   // st[k] = #points in buckets < k
    __syncthreads();
    for (int k = tid; k < H; k += kGridBlock) cu[k] = st[k];
    __syncthreads();
    for (int j = tid; j < n; j += kGridBlock) {
        const float4 q = yb[j];
        const unsigned h = grid_hash(grid_cell(q.x, o4.x, invh), grid_cell(q.y, o4.y, invh),
                                     grid_cell(q.z, o4.z, invh), mask);
        const int pos = atomicAdd(&cu[h], 1);
        out[pos] = make_float4(q.x, q.y, q.z, __int_as_float(j));
    }
}

// the fixed cloud of every pair binned once per registration (cells of edge 1 / invh)
void launch_grid_build(const float *X, const float *Y, const int32_t *lenX, const int32_t *lenY, const uint8_t *swap, int B,
                       int N, float invh, const GridScratch *grid, hipStream_t s)
{
    hipLaunchKernelGGL(grid_build_kernel, dim3(B), dim3(kGridBlock), 0, s, X, Y, lenX, lenY, swap, N,
                       grid->H, invh, grid->origin, grid->start, grid->cursor, (float4 *)grid->pts);
}

// ---------------------------------------------------------------------------------
// Sorted sweep: exact gated nearest neighbour with BROADCAST target reads.
//
// Both clouds are sorted once per registration along the longest axis a of the fixed cloud.
// In every iteration a wave (64 consecutive sorted queries) computes the span [lo, hi] of its
// CURRENT query coordinates along a (exact, from the moved points) and scans only the fixed
// points with coordinate in [lo - m, hi + m], m = 1.01 * thres: a contiguous range of the sorted
// array, read through LDS at one address for the whole wave (the same broadcast scan core as the
// all-pairs search, just over ~1/10 of the targets).  A point outside that window is farther than
// the gate radius from every query of the wave, so gate decisions and gated neighbours are the
// ones of the all-pairs search; equal-distance ties are resolved to the lowest ORIGINAL index.
// ---------------------------------------------------------------------------------
constexpr int kSortBlock = 1024;
static std::atomic<unsigned long long> g_sortAttr{0ull};   // devices on which sort_clouds_kernel has its dynamic-LDS opt-in

// grid (B, 2): blockIdx.y == 0 sorts the fixed cloud, 1 the moving cloud (pre-pose applied)
__global__ __launch_bounds__(kSortBlock) void sort_clouds_kernel(
    const float *__restrict__ X, const float *__restrict__ Y, const int32_t *__restrict__ lenX,
    const int32_t *__restrict__ lenY, const uint8_t *__restrict__ swap, const float *__restrict__ prePose,
    int N, int NP2, int32_t *__restrict__ axisOut, float4 *__restrict__ Xs, float4 *__restrict__ Ys,
    float *__restrict__ Ysoa, float *__restrict__ Xsoa, int selfCount, int dirKeys)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dynLds[];
    unsigned long long *kv = reinterpret_cast<unsigned long long *>(dynLds);   // (sort key, row) pairs, NP2 of them
    __shared__ float bb[6 * (kSortBlock / kWave)];
    __shared__ int axisSh;
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool moving = blockIdx.y == 1;
    int cX, cY;
    bool sw;
    if (selfCount) {
        // hist_icp on the side stream, forked before anything has counted: the lengths (rows with a positive flag) and
        // the smaller-cloud-first flag exactly as count_pair_kernel / zsort_kernel form them; lenX / lenY / swap unread
        __shared__ int cntScratch[2 * (kSortBlock / kWave)];
        const float4 *px = reinterpret_cast<const float4 *>(X) + (size_t)b * N;
        const float4 *py = reinterpret_cast<const float4 *>(Y) + (size_t)b * N;
        int c[2] = {0, 0};
        for (int i = tid; i < N; i += kSortBlock) {
            c[0] += (px[i].w > 0.0f) ? 1 : 0;
            c[1] += (py[i].w > 0.0f) ? 1 : 0;
        }
        block_sum<2, int>(c, cntScratch);
        cX = c[0]; cY = c[1];
        sw = selfCount == 2 && cX > cY;
    } else {
        cX = lenX[b]; cY = lenY[b];
        sw = swap != nullptr && swap[b] != 0;
    }
    const float4 *xb = reinterpret_cast<const float4 *>(sw ? Y : X) + (size_t)b * N;  // moving role
    const float4 *yb = reinterpret_cast<const float4 *>(sw ? X : Y) + (size_t)b * N;  // fixed role
    const int nx = sw ? cY : cX, ny = sw ? cX : cY;
    // axis of largest extent of the fixed cloud (both blocks compute it the same way)
    float mn[3] = {kInf, kInf, kInf}, mx[3] = {-kInf, -kInf, -kInf};
    for (int j = tid; j < ny; j += kSortBlock) {
        const float4 q = yb[j];
        mn[0] = fminf(mn[0], q.x); mn[1] = fminf(mn[1], q.y); mn[2] = fminf(mn[2], q.z);
        mx[0] = fmaxf(mx[0], q.x); mx[1] = fmaxf(mx[1], q.y); mx[2] = fmaxf(mx[2], q.z);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            mn[k] = fminf(mn[k], __shfl_xor(mn[k], o, kWave));
            mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o, kWave));
        }
    if ((tid & (kWave - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { bb[(tid >> 6) * 6 + k] = mn[k]; bb[(tid >> 6) * 6 + 3 + k] = mx[k]; }
    }
    __syncthreads();
    __shared__ float boxSh[6];
    if (tid == 0) {
        float e[3];
        for (int k = 0; k < 3; ++k) {
            float lo = bb[k], hi = bb[3 + k];
            for (int w = 1; w < kSortBlock / kWave; ++w) { lo = fminf(lo, bb[w * 6 + k]); hi = fmaxf(hi, bb[w * 6 + 3 + k]); }
            e[k] = hi - lo;
            boxSh[k] = lo; boxSh[3 + k] = hi;
        }
        const int a = (e[0] >= e[1] && e[0] >= e[2]) ? 0 : (e[1] >= e[2] ? 1 : 2);
        axisSh = a;
    }
    __syncthreads();
    // The key that spreads the fixed cloud best (sortdir.hpp): among the three axes and kSortDirs horizontal directions, the one
    // with the smallest sum of squared populations of 0.1 m key bins -- the longest axis, as before, unless another key is at
    // least a tenth better (clouds of a thousand points and more: below that every window is short anyway).  Integer counts,
    // the same on both blocks of the pair.
    if (dirKeys && ny >= kSortDirMinN && nx >= kSortDirMinMoving) {
        __shared__ unsigned int scoreSh[kSortCodes];
        // (the sort has not started: its key array -- NP2 >= 2048 entries of 8 bytes here -- holds the counters)
        (void)choose_sort_code<kSortBlock>(yb, ny, boxSh, axisSh, reinterpret_cast<unsigned int *>(dynLds), scoreSh, &axisSh);
    }
    if (tid == 0 && !moving) axisOut[b] = axisSh;
    const int axis = axisSh;
    float dirX = 0.f, dirY = 0.f;
    if (axis >= 3) sort_dir(axis, dirX, dirY);
    const int n = moving ? nx : ny;
    const float4 *cloud = moving ? xb : yb;
    PointXf pre;
    pre.kind = (moving && prePose) ? XF_AFFINE : XF_NONE;
    pre.a = (moving && prePose) ? affine_from_pose(prePose + (size_t)b * 16) : affine_identity();
    // the sorting network only has to hold THIS cloud: next power of two >= n (ragged batches are
    // padded to the largest cluster, most clusters are far smaller)
    int np2 = kWave;
    while (np2 < n) np2 <<= 1;
    np2 = min(np2, NP2);
    for (int j = tid; j < np2; j += kSortBlock) {
        float k = kInf;
        if (j < n) {
            const float4 q = cloud[j];
            float px, py, pz;
            xf_apply(pre, q.x, q.y, q.z, px, py, pz);
            k = sort_key_of(axis, dirX, dirY, px, py, pz);
        }
        kv[j] = sort_pack(k, j);
    }
    __syncthreads();
    bitonic_sort_lds(kv, np2);
    float4 *out = (moving ? Xs : Ys) + (size_t)b * N;
    const int NP16 = (N + kChunk - 1) / kChunk * kChunk;
    // structure-of-arrays image (x[], y[], z[], padded with +inf to a multiple of 16): always for the
    // fixed cloud, for the moving cloud when the caller wants to sweep in both directions (Xsoa)
    float *soa = moving ? (Xsoa ? Xsoa + (size_t)b * 3 * NP16 : nullptr) : Ysoa + (size_t)b * 3 * NP16;
    for (int r = tid; r < (soa ? NP16 : n); r += kSortBlock) {
        float px = kInf, py = kInf, pz = kInf;
        if (r < n) {
            const int j = sort_index_of(kv[r]);
            const float4 q = cloud[j];
            xf_apply(pre, q.x, q.y, q.z, px, py, pz);
            out[r] = make_float4(px, py, pz, __int_as_float(j));
        }
        if (soa) { soa[r] = px; soa[NP16 + r] = py; soa[2 * NP16 + r] = pz; }
    }
}

// long clouds, where the scratch has the chunk arrays: several workgroups per sort (sort.hip)
static bool sort_is_chunked(int N, const GridScratch *grid) { return N > kChunkSortMinN && grid->ckey != nullptr; }

// Both clouds of every pair sorted along the fixed cloud's key into grid->sortX / pts / sortYsoa / axis: one workgroup per
// cloud up to kChunkSortMinN points, several beyond (sort.hip, where the scratch has its chunk arrays).
// prePose: applied to the moving cloud, or NULL.  wantXsoa: also the moving cloud's structure-of-arrays image (grid->sortXsoa).
// boxes: count_pair's boxes for the chunked sort, or NULL.  selfCount (single-workgroup sorts only): 1 = the kernel counts
// the valid rows itself, 2 = and forms the smaller-cloud-first flag itself (X = src); lenX / lenY / swap are then not read.
hipError_t launch_sort_clouds(const float *X, const float *Y, const int32_t *lenX, const int32_t *lenY, const uint8_t *swap,
                              const float *prePose, int B, int N, const GridScratch *grid, bool wantXsoa, const float *boxes,
                              int selfCount, hipStream_t s)
{
    if (selfCount != 0 && N > kChunkSortMinN) return hipErrorInvalidValue;
    float *Xsoa = wantXsoa ? grid->sortXsoa : nullptr;
    int NP2 = 64;
    while (NP2 < N) NP2 <<= 1;
    if ((size_t)NP2 * 8 > 64 * 1024)   // dynamic LDS above 64 KiB needs the attribute (N > 8192)
        ensure_dynamic_lds(reinterpret_cast<const void *>(&sort_clouds_kernel), 128 * 1024, &g_sortAttr);
    if (sort_is_chunked(N, grid))
        return launch_sort_clouds_chunked(X, Y, lenX, lenY, swap, prePose, B, N, grid->axis, grid->sortX, grid->pts,
                                          grid->sortYsoa, Xsoa, grid->ckey, grid->cidx, s, boxes, grid->dirKeys);
    hipLaunchKernelGGL(sort_clouds_kernel, dim3(B, 2), dim3(kSortBlock), (size_t)NP2 * 8, s, X, Y, lenX, lenY, swap,
                       prePose, N, NP2, grid->axis, (float4 *)grid->sortX, (float4 *)grid->pts, grid->sortYsoa, Xsoa,
                       selfCount, grid->dirKeys);
    return hipSuccess;   // (a launch error is the caller's to fetch: launch_icp reads it after its last launch)
}

// ... without a pre-pose, with the images of BOTH clouds and count_pair's boxes: input of the scoring sweep (nn.hip)
hipError_t launch_sort_clouds_soa(const float *X, const float *Y, const int32_t *lenX, const int32_t *lenY,
                                  const uint8_t *swap, int B, int N, const GridScratch *grid, hipStream_t s, int selfCount)
{
    const hipError_t e = launch_sort_clouds(X, Y, lenX, lenY, swap, nullptr, B, N, grid, true, grid->pairBox, selfCount, s);
    return (e != hipSuccess || sort_is_chunked(N, grid)) ? e : hipGetLastError();   // (the chunked sort has asked itself)
}

}  // namespace icpflow
