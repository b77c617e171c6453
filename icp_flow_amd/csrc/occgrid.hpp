// occgrid.hpp -- the dilated occupancy grid of one cloud (the scoring sweeps' pre-bound, nn.hip), as the body of a workgroup of
// kOccBlock threads: occ_build_kernel (nn.hip) runs it on a grid of its own, the vote launch's grid workgroups (hist.hip:
// front_roles_kernel) run it twice, in their two halves of four waves.  The caller owns the LDS: two bit arrays of kOccWords words, the reduction
// arrays, and -- only where the body counts the rows itself (selfCount) -- the counting scratch.
#pragma once
#include "common.hpp"
#include "kernels.hpp"

namespace icpflow {

// Dilated occupancy grid of one sorted cloud (SoA image of launch_sort_clouds_soa: valid rows first, +inf behind them), grid (B, 2):
// y = 0 the src role's cloud, 1 the dst role's.  Cell edge h = 0.125 m, grown by a quarter at a time until the box of the cloud --
// plus one cell of margin all round -- fits kOccWords * 32 cells.  A point sets the bits of its cell and of the 26 around it.
constexpr int kOccBlock = 256;
// The whole bit array moved by `sh` bits towards higher (up) or lower cell numbers; bits moved in from outside are zero.
__device__ __forceinline__ uint32_t occ_shifted(const uint32_t *in, int w, int sh, bool up)
{
    const int q = sh >> 5, r = sh & 31;
    if (up) {
        const int a = w - q;
        const uint32_t lo = a >= 0 ? in[a] : 0u, lo1 = a - 1 >= 0 ? in[a - 1] : 0u;
        return r == 0 ? lo : ((lo << r) | (lo1 >> (32 - r)));
    }
    const int a = w + q;
    const uint32_t hi = a < kOccWords ? in[a] : 0u, hi1 = a + 1 < kOccWords ? in[a + 1] : 0u;
    return r == 0 ? hi : ((hi >> r) | (hi1 << (32 - r)));
}

//
// RAW: the same grids from the clouds as they come in ([B, N, 4] rows, X the src and Y the dst cloud), for a launch that must not wait
// for the sort: the rows the sort takes (the first n of the role's cloud: sort_clouds_kernel, lengths and roles formed the same way,
// selfCount as there) are the points of its image, and the grid is a function of the SET of points -- minima, maxima and bits set
// by atomicOr -- so it is the same grid, bit for bit.
struct OccLds {
    uint32_t *bitsA, *bitsB;   // kOccWords words each
    float *red;                // 6 * (kOccBlock / kWave)
    float *hd;                 // 8
    int *cnt;                  // 2 * (kOccBlock / kWave), or NULL with selfCount == 0
};
constexpr int kOccLdsBytes = 2 * kOccWords * 4 + (6 * (kOccBlock / kWave) + 8) * 4;   // without the counting scratch

// All kOccBlock threads of the workgroup (tid = 0 .. kOccBlock - 1) call it for pair b, role `which`; contains barriers.
template <bool RAW>
__device__ __forceinline__ void occ_build_body(const OccLds &lds, int b, int which, int tid, const float *__restrict__ Xsoa,
                                               const float *__restrict__ Ysoa, int NP16, float *__restrict__ hdrOut,
                                               uint32_t *__restrict__ bitsOut, const int32_t *__restrict__ lenX,
                                               const int32_t *__restrict__ lenY, const uint8_t *__restrict__ swap, int selfCount)
{
    uint32_t *const bitsA = lds.bitsA, *const bitsB = lds.bitsB;
    float *const red = lds.red, *const hd = lds.hd;
    const int lane = tid & (kWave - 1), wave = tid >> 6;
    // SoA image: NP16 rows per coordinate; raw rows: the first `rows` float4 of the role's cloud (NP16 is N then), 4 floats apart
    const float *px, *py, *pz;
    int rows = NP16;
    constexpr int kStep = RAW ? 4 : 1;
    if (RAW) {
        int cX, cY;
        bool sw;
        if (selfCount) {
            int *const cntScratch = lds.cnt;
            const float4 *qx = reinterpret_cast<const float4 *>(Xsoa) + (size_t)b * NP16;
            const float4 *qy = reinterpret_cast<const float4 *>(Ysoa) + (size_t)b * NP16;
            int c[2] = {0, 0};
            for (int i = tid; i < NP16; i += kOccBlock) {
                c[0] += (qx[i].w > 0.0f) ? 1 : 0;
                c[1] += (qy[i].w > 0.0f) ? 1 : 0;
            }
            block_sum<2, int>(c, cntScratch);
            cX = c[0]; cY = c[1];
            sw = selfCount == 2 && cX > cY;
        } else {
            cX = lenX[b]; cY = lenY[b];
            sw = swap != nullptr && swap[b] != 0;
        }
        const bool fromY = (which == 0) == sw;   // which 0: the moving role's cloud (X unless swapped), 1: the fixed role's
        px = (fromY ? Ysoa : Xsoa) + (size_t)b * NP16 * 4; py = px + 1; pz = px + 2;
        rows = fromY ? cY : cX;
    } else {
        px = (which == 0 ? Xsoa : Ysoa) + (size_t)b * 3 * NP16; py = px + NP16; pz = py + NP16;
    }
    for (int k = tid; k < kOccWords; k += kOccBlock) bitsA[k] = 0u;
    float mn[3] = {kInf, kInf, kInf}, mx[3] = {-kInf, -kInf, -kInf};
    for (int i = tid; i < rows; i += kOccBlock) {
        const float x = px[i * kStep], y = py[i * kStep], z = pz[i * kStep];
        if (fabsf(x) < 1e30f && fabsf(y) < 1e30f && fabsf(z) < 1e30f) {   // (pads are +inf; NaN rows fail too: they are no target anybody is near)
            mn[0] = fminf(mn[0], x); mn[1] = fminf(mn[1], y); mn[2] = fminf(mn[2], z);
            mx[0] = fmaxf(mx[0], x); mx[1] = fmaxf(mx[1], y); mx[2] = fmaxf(mx[2], z);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            mn[a] = fminf(mn[a], __shfl_xor(mn[a], o, kWave));
            mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o, kWave));
        }
        if (lane == 0) { red[wave * 6 + a] = mn[a]; red[wave * 6 + 3 + a] = mx[a]; }
    }
    __syncthreads();
    if (tid == 0) {
        float lo[3], hi[3];
        for (int a = 0; a < 3; ++a) {
            lo[a] = kInf; hi[a] = -kInf;
            for (int w = 0; w < kOccBlock / kWave; ++w) { lo[a] = fminf(lo[a], red[w * 6 + a]); hi[a] = fmaxf(hi[a], red[w * 6 + 3 + a]); }
        }
        int n[3] = {0, 0, 0};
        float h = 0.125f;
        if (lo[0] <= hi[0]) {   // a cloud with points
            for (int grow = 0; grow < 64; ++grow) {
                bool fits = true;
                long long cells = 1;
                for (int a = 0; a < 3; ++a) {
                    const float e = (hi[a] - lo[a]) / h;
                    if (!(e < 30000.f)) { fits = false; break; }
                    n[a] = (int)e + 2 + 2 * kOccRings;   // kOccRings cells of margin below the lowest point, the points' cells, as many above, one of slack
                    cells *= n[a];
                }
                if (fits && cells <= (long long)kOccWords * 32) break;
                h *= 1.25f; n[0] = 0;
            }
        }
        if (n[0] <= 0) n[0] = n[1] = n[2] = 0;   // empty cloud (or one no grid holds): no bound
        hd[0] = lo[0] - kOccRings * h; hd[1] = lo[1] - kOccRings * h; hd[2] = lo[2] - kOccRings * h;   // the lowest point falls into cell kOccRings
        // rounding of the cell arithmetic: two ulps of the largest coordinate, in cells -- below 0.5 % of a cell or no grid at all
        // (coordinates of kilometres against a 12.5 cm cell); the bound itself keeps 2 % in hand (0.98 h)
        float big = 0.f;
        for (int a = 0; a < 3; ++a) big = fmaxf(big, fmaxf(fabsf(lo[a]), fabsf(hi[a])));
        if (!(big * 2.4e-7f / h < 0.005f)) n[0] = n[1] = n[2] = 0;
        hd[3] = 1.0f / h; hd[4] = 0.98f * h;
        hd[5] = __int_as_float(n[0]); hd[6] = __int_as_float(n[1]); hd[7] = __int_as_float(n[2]);
    }
    __syncthreads();
    const float gox = hd[0], goy = hd[1], goz = hd[2], ginv = hd[3];
    const int gnx = __float_as_int(hd[5]), gny = __float_as_int(hd[6]), gnz = __float_as_int(hd[7]);
    if (gnx > 0) {
        for (int i = tid; i < rows; i += kOccBlock) {
            const float x = px[i * kStep], y = py[i * kStep], z = pz[i * kStep];
            if (!(fabsf(x) < 1e30f && fabsf(y) < 1e30f && fabsf(z) < 1e30f)) continue;
            // the cell, kept kOccRings cells inside the grid (rounding at the box's faces): every dilation stays inside, and a
            // shift of the bit array by one cell along any axis never carries a bit across a face
            const int cx = min(max((int)floorf((x - gox) * ginv), kOccRings), gnx - 1 - kOccRings);
            const int cy = min(max((int)floorf((y - goy) * ginv), kOccRings), gny - 1 - kOccRings);
            const int cz = min(max((int)floorf((z - goz) * ginv), kOccRings), gnz - 1 - kOccRings);
            const int c = (cx * gny + cy) * gnz + cz;
            atomicOr(&bitsA[c >> 5], 1u << (c & 31));
        }
    }
    __syncthreads();
    // dilation by one cell along z, y, x in turn (separable: the 27-neighbourhood), each a shift of the whole bit array by 1, nz,
    // ny * nz bits up and down
    // Plane k (k = 0 .. kOccRings - 1) is the cloud dilated k + 1 times: a cell that is empty there has no point within k + 1 cells.
    const int strides[3] = {1, gnz, gny * gnz};
    uint32_t *in = bitsA, *outb = bitsB;
    uint32_t *bo = bitsOut + ((size_t)b * 2 + which) * kOccRings * kOccWords;
    for (int ring = 0; ring < kOccRings; ++ring) {
        for (int a = 0; a < 3; ++a) {
            if (gnx > 0)
                for (int w = tid; w < kOccWords; w += kOccBlock) outb[w] = in[w] | occ_shifted(in, w, strides[a], true) | occ_shifted(in, w, strides[a], false);
            __syncthreads();
            uint32_t *t = in; in = outb; outb = t;
        }
        for (int k = tid; k < kOccWords; k += kOccBlock) bo[ring * kOccWords + k] = gnx > 0 ? in[k] : 0u;
    }
    if (tid < 8) hdrOut[((size_t)b * 2 + which) * 8 + tid] = hd[tid];
}

}  // namespace icpflow
