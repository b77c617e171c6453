// icp_epilogue.hip -- the kernels around the ICP loop that read only what it leaves behind (IcpState, IcpCtrl, the
// per-iteration history): the history epilogue of the speculative launch, the export to the caller's arrays, the list of
// pairs between the two launches of a drained grid, and the batch rule re-tallied over a subset of the pairs.
#include "common.hpp"
#include "kernels.hpp"

namespace icpflow {

// speculative mode epilogue: the reference's stopping iteration is the first one at which every
// pair had arrived and none was unconverged; every pair's state is taken from its history there.
__global__ void icp_resolve_history_kernel(IcpState *__restrict__ st, IcpCtrl *__restrict__ ctrl,
                                           const float *__restrict__ history, int B, int maxIter)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int n = maxIter;
    for (int s = 0; s < maxIter; ++s) {
        const unsigned long long t = ctrl->tally[s];
        if ((int)(t & 0xffffffffull) == B && (t >> 32) == 0ull) { n = s + 1; break; }
    }
    const float *h = history + ((size_t)(n - 1) * B + b) * kHistStride;
    for (int k = 0; k < 9; ++k) st[b].R[k] = h[k];
    for (int k = 0; k < 3; ++k) st[b].T[k] = h[9 + k];
    st[b].rmse = h[12];
    st[b].s = h[13];
#ifdef ICPFLOW_DEBUG_EXECUTED
    st[b].rmse = (float)st[b].iters;   // developer builds: iterations this pair actually executed
#endif
    st[b].iters = n;
    if (ctrl->error) st[b].R[0] = __int_as_float(0x7fc00000);   // a team gave up waiting: poison
    if (b == 0) {
        ctrl->iters = n;
        // same convention as the per-iteration path: notconv[n-1] == 0 <=> converged
        ctrl->notconv[n - 1] = (int)(ctrl->tally[n - 1] >> 32);
    }
}

hipError_t launch_icp_resolve_history(IcpState *state, IcpCtrl *ctrl, const float *history, int B, int maxIter,
                                      hipStream_t s)
{
    hipLaunchKernelGGL(icp_resolve_history_kernel, dim3((B + 127) / 128), dim3(128), 0, s, state, ctrl, history, B,
                       maxIter);
    return hipGetLastError();
}

__global__ void icp_export_kernel(const IcpState *__restrict__ st, const IcpCtrl *__restrict__ ctrl,
                                  int B, int stopMode, float *__restrict__ R, float *__restrict__ T,
                                  float *__restrict__ rmse, int32_t *__restrict__ iters,
                                  int32_t *__restrict__ converged, float *__restrict__ scale)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) {
        if (R) for (int k = 0; k < 9; ++k) R[(size_t)b * 9 + k] = ctrl->error ? __int_as_float(0x7fc00000) : st[b].R[k];
        if (T) for (int k = 0; k < 3; ++k) T[(size_t)b * 3 + k] = st[b].T[k];
        if (rmse) rmse[b] = st[b].rmse;
        if (scale) scale[b] = st[b].s;
    }
    if (b == 0) {
        const int n = ctrl->iters;
        if (iters) *iters = ctrl->error ? -1 : n;
        if (converged) {
            if (stopMode == ICPFLOW_STOP_REFERENCE_) *converged = (n > 0 && ctrl->notconv[n - 1] == 0) ? 1 : 0;
            else *converged = (ctrl->notconv[0] == 0) ? 1 : 0;
        }
    }
}

hipError_t launch_icp_export(IcpState *state, IcpCtrl *ctrl, int B, int stopMode, float *R,
                             float *T, float *rmse, int32_t *iters, int32_t *converged, hipStream_t s, float *scale)
{
    hipLaunchKernelGGL(icp_export_kernel, dim3((B + 127) / 128), dim3(128), 0, s, state, ctrl, B,
                       stopMode, R, T, rmse, iters, converged, scale);
    return hipGetLastError();
}

// Two launches for batches of a few rounds (round 6).  A persistent grid deals its pairs in index order, and which pairs
// are the long ones is not known beforehand (tools/dbg/order_predictor.py): config 4's shard (1024 pairs x 2048 points, two
// 512-thread workgroups per CU) keeps its 512 slots full for the first half of the launch and spends the second half on a
// thinning set of long pairs, each on HALF a CU (tools/dbg/help_timeline.py: 498 owners at 50 % of the span, 227 at 70 %, 55 at
// 85 %; 30-40 us per iteration while the CU is shared, ~20 us with helpers once it is not).  So the launch is DRAINED as soon as
// at most `drainAt` (the number of CUs) pairs are unfinished: every pair still iterating leaves behind its current iteration,
// still moving (IcpState: state, rmse, iterations; its history rows and tallies are in place).  This kernel, between the two
// launches, looks for the batch rule among the tallies (found: nobody goes on), finds the first iteration some pair has not
// reached yet (the floor of the second launch's search for the rule) and lists the pairs that left still moving; the SECOND launch
// gives each of them a whole CU -- one 1024-thread workgroup, two passes instead of four -- and resumes it at ITS iteration.
// What makes that bit-identical (ICPFLOW_OPT_TWO_LAUNCH against the default; tests/test_gpu_fullsize.py): the first launch keeps its moment sums
// per (pass, wave) and adds them in that order (redPasses, the helpers' bookkeeping) -- i.e. in the order of the UNITS of 64
// consecutive sorted queries, which is the same order whether 8 waves take 4 passes or 16 waves take 2; everything else of an
// iteration is a function of (R, T).  The neighbour certificates are rebuilt in a pair's first iteration of the second launch,
// the cycle detection and the own-convergence bits are restored from the pair's history rows (icp_pair).
__global__ __launch_bounds__(1024) void icp_split_kernel(const IcpCtrl *__restrict__ ctrl, const IcpState *__restrict__ st, int B, int maxIter,
                                                         int32_t *__restrict__ list, int32_t *__restrict__ meta)
{
    __shared__ int foundSh, floorSh, waveCnt[16];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    if (tid == 0) { foundSh = 0; floorSh = maxIter; }
    __syncthreads();
    for (int s0 = tid; s0 < maxIter; s0 += 1024) {
        const unsigned long long t = ctrl->tally[s0];
        if ((int)(t & 0xffffffffull) >= B) { if ((t >> 32) == 0ull) foundSh = 1; }
        else atomicMin(&floorSh, s0);
    }
    __syncthreads();
    if (foundSh) {   // the batch rule holds at an iteration every pair has reached: nobody goes on
        if (tid == 0) { meta[0] = 0; meta[1] = 0; }
        return;
    }
    int total = 0;   // (workgroup-uniform)
    for (int b0 = 0; b0 < B; b0 += 1024) {
        const int b = b0 + tid;
        const bool on = b < B && st[b].active != 0 && st[b].iters < maxIter;
        const unsigned long long m = __ballot(on);
        if (lane == 0) waveCnt[wave] = __builtin_popcountll(m);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) { const int c = waveCnt[w]; before += w < wave ? c : 0; all += c; }
        if (on) list[total + before + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = b;
        total += all;
        __syncthreads();
    }
    if (tid == 0) { meta[0] = total; meta[1] = floorSh; }
}

void launch_icp_split(const IcpCtrl *ctrl, const IcpState *state, int B, int maxIter, int32_t *list, int32_t *meta, hipStream_t s)
{
    hipLaunchKernelGGL(icp_split_kernel, dim3(1), dim3(1024), 0, s, ctrl, state, B, maxIter, list, meta);
}

// The batch rule over a SUBSET of the pairs, after the fact (round 5: a frame pair's stage 2 iterates all the candidates of its
// superset beside stage 1, before it is known which of them are in the batch).  The speculative launch has left every pair's
// (R, T, rmse) of every iteration in the history and the tallies of the rule over ALL pairs; every pair has rows up to the first
// iteration s_all at which that rule held (a pair leaves only when it has seen such an iteration, when its trajectory is
// periodic -- it then writes all remaining rows -- or at the cap), and the rule over a subset holds no later.  This kernel
// recomputes, per iteration s <= s_all, "every ACTIVE pair converged" from the history's rmse values with the loop's own test
// (:195-198, :209: rel = (prev - rmse) / prev <= thr, false at iteration 0 and on a NaN) and REWRITES the tallies so that their
// readers (posefuse.hpp) find the subset's stopping iteration: exactly what a launch with options.d_pair_active would have left.
__global__ __launch_bounds__(1024) void icp_retally_kernel(IcpCtrl *__restrict__ ctrl, const float *__restrict__ history,
                                                           const uint8_t *__restrict__ active, int B, int maxIter, float relThr)
{
    __shared__ unsigned int bad[4];       // bit s: some active pair is not converged at iteration s
    __shared__ int limitSh;
    const int tid = threadIdx.x;
    if (tid < 4) bad[tid] = tid == 0 ? 1u : 0u;      // (iteration 0: rel = 1, nobody is converged)
    if (tid < kWave) {                               // the first iteration at which the rule over ALL pairs held (wave 0, 64 tallies a round)
        int lim = maxIter - 1;
        for (int s0 = 0; s0 < maxIter; s0 += kWave) {
            const int s = s0 + tid;
            bool hit = false;
            if (s < maxIter) {
                const unsigned long long t = ctrl->tally[s];
                hit = (int)(t & 0xffffffffull) == B && (t >> 32) == 0ull;
            }
            const unsigned long long m = __ballot(hit);
            if (m != 0ull) { lim = s0 + __builtin_ctzll(m); break; }
        }
        if (tid == 0) limitSh = lim;
    }
    __syncthreads();
    const int lim = limitSh;
    // one (pair, iteration) per thread and round, pairs fastest (neighbouring threads read neighbouring rows): every test reads
    // the two rmse values it compares -- no chain through the iterations
    for (int i = tid; i < B * lim; i += 1024) {
        const int b = i % B, s = i / B + 1;
        if (active[b] == 0) continue;
        const float prev = history[((size_t)(s - 1) * B + b) * kHistStride + 12];
        const float rm = history[((size_t)s * B + b) * kHistStride + 12];
        const float rel = (prev - rm) / prev;
        if (!(rel <= relThr)) atomicOr(&bad[s >> 5], 1u << (s & 31));
    }
    __syncthreads();
    for (int s = tid; s < maxIter; s += 1024) {
        unsigned long long t = 0ull;                              // beyond s_all: "not everybody has arrived"
        if (s <= lim) t = (unsigned long long)(unsigned)B | (((bad[s >> 5] >> (s & 31)) & 1u) ? (1ull << 32) : 0ull);
        ctrl->tally[s] = t;
    }
}

hipError_t launch_icp_retally(IcpCtrl *ctrl, const float *history, const uint8_t *active, int B, int maxIter, double relThr,
                              hipStream_t s)
{
    if (maxIter > kHistIters) return hipErrorInvalidValue;
    hipLaunchKernelGGL(icp_retally_kernel, dim3(1), dim3(1024), 0, s, ctrl, history, active, B, maxIter, (float)relThr);
    return hipGetLastError();
}

}  // namespace icpflow
