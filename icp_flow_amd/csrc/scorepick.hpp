// scorepick.hpp -- the pick of a pair's initial pose among its scored candidates (utils_hist.py:101-106, :121-122), as ONE wave
// does it: the only copy of that arithmetic.  Its callers: score_pick_kernel (pose.hip), one wave per pair in a launch of its own,
// and the ICP loop's prologue (icp.hip), where wave 0 of the pair's workgroup picks the pose the pair starts from.
#pragma once
#include "common.hpp"
#include "kernels.hpp"

namespace icpflow {

// sum of a job's per-block records, in block order.  Eight loads in flight at a time (unconditional, from clamped
// addresses), then eight ordered adds: as a plain loop every record is a dependent round trip -- 40 of them on a
// 10000-point batch, where this was most of select_kernel's 19 us.
__device__ __forceinline__ double partial_total(const double *partial, int job, int qblocks, int k)
{
    double s = 0.0;
    const double *base = partial + (size_t)job * qblocks * kPartial + k;
    if (qblocks <= 4) {   // (config 2: four blocks -- no point in eight loads)
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = base[(size_t)min(u, qblocks - 1) * kPartial];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (u < qblocks) s += v[u];
        return s;
    }
    for (int q0 = 0; q0 < qblocks; q0 += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = base[(size_t)min(q0 + u, qblocks - 1) * kPartial];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (q0 + u < qblocks) s += v[u];
    }
    return s;
}

// score_k = min(mean fwd, mean bwd); first arg-min; T = I with that translation
// (utils_hist.py:101-106, :121-122)
// one wave for pair b (all 64 lanes call it together): lane j < 12 totals job j (candidate j / 2, direction j % 2) over the
// query blocks.  Writes Tinit[b] (16 floats) and, where wanted, initSum[b]; -> lane l < 16: word l of that pose (0 elsewhere).
__device__ __forceinline__ float score_pick_wave(const double *partial, int qblocks, const int32_t *lenA, const int32_t *lenC,
                                                 const uint8_t *swap, const float *cand, int b, int lane, float *Tinit,
                                                 double *initSum)
{
    const bool sw = swap != nullptr && swap[b] != 0;
    const float na = (float)(sw ? lenC[b] : lenA[b]);
    const float nc = (float)(sw ? lenA[b] : lenC[b]);
    float mean = 0.f;
    double total = 0.0;
    if (lane < 2 * kCand) {
        total = partial_total(partial, b * 12 + lane, qblocks, 0);
        mean = (float)total / ((lane & 1) ? nc : na);
    }
    int pick = 0;
    float best = 0.f;
    for (int k = 0; k < kCand; ++k) {
        const float sc = fminf(__shfl(mean, 2 * k, kWave), __shfl(mean, 2 * k + 1, kWave));
        if (k == 0 || sc < best) { best = sc; pick = k; }
    }
    // The forward total of the picked candidate IS the roll-back check's sum under the initial pose (utils_icp.py:28-29 on
    // src + t, the points utils_hist.py:86-89 has just scored: same queries in the same sorted order, same targets, same
    // block records) -- kept for the check sweep of the same call, which then scans under the final pose only.  A scan
    // that was pruned reports +inf (the pick can still fall on it through its backward mean): the check scans for itself.
    if (initSum != nullptr && lane == 2 * pick) initSum[b] = total;
    float v = 0.f;
    if (lane < 16) {
        const float *t = cand + ((size_t)b * kCand + pick) * 3;
        v = (lane % 5 == 0) ? 1.f : 0.f;
        if (lane == 3) v = t[0];
        if (lane == 7) v = t[1];
        if (lane == 11) v = t[2];
        Tinit[(size_t)b * 16 + lane] = v;
    }
    return v;
}

}  // namespace icpflow
