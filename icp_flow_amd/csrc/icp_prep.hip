// icp_prep.hip -- what a registration prepares once, before its first iteration (launch_icp, icp.hip): the fixed cloud
// binned into the hashed grid (grid_build_kernel), or both clouds sorted along the fixed cloud's key for the sorted sweep
// (sort_clouds_kernel up to kChunkSortMinN points, sort.hip's chunked sort beyond).  The scoring sweep (nn.hip) takes the
// same sort, without a pre-pose and with the moving cloud's structure-of-arrays image.
//
// (sort_clouds_kernel is not in sort.hip: beside it, sort.hip's own kernels compile to other code.)
#include "scan.hpp"
#include "sortdir.hpp"
#include "sortclouds.hpp"
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

// grid (B, 2): blockIdx.y == 0 sorts the fixed cloud, 1 the moving cloud (pre-pose applied); the body: sortclouds.hpp
__global__ __launch_bounds__(kSortBlock) void sort_clouds_kernel(
    const float *__restrict__ X, const float *__restrict__ Y, const int32_t *__restrict__ lenX,
    const int32_t *__restrict__ lenY, const uint8_t *__restrict__ swap, const float *__restrict__ prePose,
    int N, int NP2, int32_t *__restrict__ axisOut, float4 *__restrict__ Xs, float4 *__restrict__ Ys,
    float *__restrict__ Ysoa, float *__restrict__ Xsoa, int selfCount, int dirKeys)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dynLds[];
    __shared__ float bb[6 * (kSortBlock / kWave)];
    __shared__ float boxSh[6];
    __shared__ int axisSh;
    __shared__ unsigned int scoreSh[kSortCodes];
    __shared__ int cntScratch[2 * (kSortBlock / kWave)];
    const SortLds lds{reinterpret_cast<unsigned long long *>(dynLds), bb, boxSh, &axisSh, scoreSh, cntScratch};
    sort_clouds_body<kSortBlock>(lds, blockIdx.x, blockIdx.y == 1, threadIdx.x, X, Y, lenX, lenY, swap, prePose, N, NP2, axisOut, Xs,
                                 Ys, Ysoa, Xsoa, selfCount, dirKeys);
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
