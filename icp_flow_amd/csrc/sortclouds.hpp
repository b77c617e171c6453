// sortclouds.hpp -- both clouds of a pair sorted along the fixed cloud's key (the sorted sweeps' input: icp_prep.hip), as the body
// of ONE workgroup of BLOCK threads per cloud: sort_clouds_kernel (icp_prep.hip) runs it with 1024 threads on a grid of its own,
// the vote launch's sort workgroups (hist.hip: front_roles_kernel) with 512 -- the network of a 1024-point cloud has 512
// exchanges per step.  The caller owns the LDS.
#pragma once
#include "scan.hpp"
#include "sortdir.hpp"

namespace icpflow {

struct SortLds {
    unsigned long long *kv;   // NP2 (key, row) pairs; at least 3 * kSortDirBins counters where direction keys are chosen
    float *bb;                // 6 * (BLOCK / kWave)
    float *box;               // 6
    int *axis;                // 1
    unsigned int *score;      // kSortCodes
    int *cnt;                 // 2 * (BLOCK / kWave), or NULL with selfCount == 0
};
// bytes behind the keys that the small arrays of a BLOCK-thread workgroup take (without the counting scratch)
constexpr int sort_lds_small_bytes(int block) { return (6 * (block / kWave) + 6 + 1 + kSortCodes) * 4; }

// All BLOCK threads of the workgroup call it for pair b; moving: the moving role's cloud (pre-pose applied), else the fixed
// role's.  Contains barriers.
template <int BLOCK>
__device__ __forceinline__ void sort_clouds_body(
    const SortLds &lds, int b, bool moving, int tid, const float *__restrict__ X, const float *__restrict__ Y,
    const int32_t *__restrict__ lenX, const int32_t *__restrict__ lenY, const uint8_t *__restrict__ swap,
    const float *__restrict__ prePose, int N, int NP2, int32_t *__restrict__ axisOut, float4 *__restrict__ Xs,
    float4 *__restrict__ Ys, float *__restrict__ Ysoa, float *__restrict__ Xsoa, int selfCount, int dirKeys)
{
    unsigned long long *const kv = lds.kv;   // (sort key, row) pairs, NP2 of them
    float *const bb = lds.bb;
    int &axisSh = *lds.axis;
    int cX, cY;
    bool sw;
    if (selfCount) {
        // hist_icp on the side stream, forked before anything has counted: the lengths (rows with a positive flag) and
        // the smaller-cloud-first flag exactly as count_pair_kernel / zsort_kernel form them; lenX / lenY / swap unread
        int *const cntScratch = lds.cnt;
        const float4 *px = reinterpret_cast<const float4 *>(X) + (size_t)b * N;
        const float4 *py = reinterpret_cast<const float4 *>(Y) + (size_t)b * N;
        int c[2] = {0, 0};
        for (int i = tid; i < N; i += BLOCK) {
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
    for (int j = tid; j < ny; j += BLOCK) {
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
    float *const boxSh = lds.box;
    if (tid == 0) {
        float e[3];
        for (int k = 0; k < 3; ++k) {
            float lo = bb[k], hi = bb[3 + k];
            for (int w = 1; w < BLOCK / kWave; ++w) { lo = fminf(lo, bb[w * 6 + k]); hi = fmaxf(hi, bb[w * 6 + 3 + k]); }
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
        unsigned int *const scoreSh = lds.score;
        // (the sort has not started: its key array -- NP2 >= 2048 entries of 8 bytes here -- holds the counters)
        (void)choose_sort_code<BLOCK>(yb, ny, boxSh, axisSh, reinterpret_cast<unsigned int *>(kv), scoreSh, &axisSh);
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
    for (int j = tid; j < np2; j += BLOCK) {
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
    for (int r = tid; r < (soa ? NP16 : n); r += BLOCK) {
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

}  // namespace icpflow
