// icp_plan.hip -- teams (IcpTeam, kernels.hpp): which workgroup of a team launch serves which pair, decided on the
// device from the batch's lengths alone, and the host's figures of such a launch (workgroups, LDS room, shared scans).
#include "scan.hpp"   // kChunk: the padding of the LDS image
#include "kernels.hpp"

namespace icpflow {

// Team plan for one launch (one block of 256 threads; B <= 256).  Round 4: sizes by PASS BOUNDARIES.
//
// A member's waves take one unit (64 consecutive sorted queries) per pass, so an iteration of a member lasts
// passes x (its slowest unit), passes = ceil(units per member / 12) for the 768-thread team kernel: a fifth workgroup on
// a pair of 73 units (19 -> 15 units per member) shortens nothing, the seventh (11 units: one pass) halves the iteration.
// So team sizes move from one level of "units per member" to the next -- ..., 36, 24, 12 (passes 3, 2, 1), then 8 and 4
// (fewer waves sharing a SIMD: the early iterations, where every unit scans its window, are VALU issue) -- and the spare
// workgroups go, one level at a time, to the pair whose estimated iteration is the longest (levels x a weight that grows
// with the length of the fixed cloud: what a unit costs follows the targets in its window).
//   * A pair first gets the team that lets its members keep the per-query RECORDS (neighbour certificates: a member's
//     share of the queries must fit `recCap`): a 2200-query pair served by ONE workgroup of a batch padded to 10000
//     searched every window in every iteration (90 k clocks per iteration against 25 k; ragged real-shape batch).
//   * Pairs of a single pass (<= 768 queries) are CHAINED: up to kTeamChain of them are served one after the other by one
//     workgroup (t.next), when the large pairs can use the workgroups that frees.  They finish within a few per cent
//     of the launch (nobody waits for anybody under the speculative batch rule; a chained pair only arrives later at
//     the tallies), and a workgroup that has finished its one small pair would idle for the rest of the launch.
// The sums of a team are added in member order: the plan decides the rounding of a registration's moment sums, so it
// depends on the batch's lengths alone (never on timing).
#ifndef ICPFLOW_TEAM_CHAIN
#define ICPFLOW_TEAM_CHAIN 4
#endif
constexpr int kTeamChain = ICPFLOW_TEAM_CHAIN;
#ifndef ICPFLOW_TEAM_MIN_SHARE
#define ICPFLOW_TEAM_MIN_SHARE 256
#endif
constexpr int kTeamMinShare = ICPFLOW_TEAM_MIN_SHARE;   // queries per member, at least
constexpr int kTeamWaves = 768 / kWave;   // units per pass of a member

// units per member at the level below `u`
__device__ __forceinline__ int team_next_level(int u)
{
    if (u > kTeamWaves) return (u - 1) / kTeamWaves * kTeamWaves;   // one pass fewer
    return u > 8 ? 8 : (u > 4 ? 4 : 0);
}
// relative length of an iteration at u units per member
__device__ __forceinline__ float team_level_cost(int u)
{
    if (u >= kTeamWaves) return (float)((u + kTeamWaves - 1) / kTeamWaves);
    return u > 8 ? 1.0f : (u > 4 ? 0.85f : 0.7f);
}

__global__ __launch_bounds__(256) void icp_team_plan_kernel(const int32_t *__restrict__ lenX,
                                                            const int32_t *__restrict__ lenY,
                                                            const uint8_t *__restrict__ swap, int B, IcpTeam t, int recCap,
                                                            const uint8_t *__restrict__ active)
{
    __shared__ int size[256];
    __shared__ int first[257];
    __shared__ int part[4];
    __shared__ int sh[8];        // [0] small pairs, [1] sum of minimum teams, [2] sum of wishes, [3] chain length, [4] slots for the large pairs
    __shared__ int teamList[256];
    __shared__ int xcdUsed[8];
    const int b = threadIdx.x, lane = b & (kWave - 1), wv = b >> 6;
    int n = 0, nf = 0;
    if (b < B) {
        const bool sw = swap != nullptr && swap[b] != 0;
        n = sw ? lenY[b] : lenX[b];
        nf = sw ? lenX[b] : lenY[b];
        // a pair that is not in the batch (options.d_pair_active) counts as the two EMPTY clouds a caller who knew the mask
        // beforehand hands over: the plan -- hence the order of every team's sums -- is the same whether the pair's clouds are
        // there or not (a frame pair's stage 2 on the whole superset, api.hip, against the serial path's empty clouds)
        if (active != nullptr && active[b] == 0) { n = 0; nf = 0; }
    }
    const int units = (n + kWave - 1) / kWave;
    const bool small = b < B && units <= kTeamWaves;
    const bool big = b < B && !small;
    // smallest team whose members keep their records; the team of one pass
    int gMin = 1;
    if (big && recCap > 0) {
        const int capUnits = max(recCap / kWave, 1);
        gMin = min(kMaxTeam, (units + capUnits - 1) / capUnits);
    }
    const int gWish = small ? 1 : min(kMaxTeam, (units + kTeamWaves - 1) / kTeamWaves);
    // (the square root: between no weight and the full ratio of the fixed clouds' lengths, measured in round 3)
    const float weight = big ? sqrtf((float)max(nf, 1024) / 1024.0f) : 0.f;
    for (int w = threadIdx.x; w < t.maxWG; w += blockDim.x) { t.wgPair[w] = -1; t.wgRank[w] = 0; }
    if (b < 8) sh[b] = 0;
    __syncthreads();
    // block-wide sum of one int per thread (all threads call it)
    auto block_sum_int = [&](int v) -> int {
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
        __syncthreads();
        if (lane == 0) part[wv] = v;
        __syncthreads();
        return part[0] + part[1] + part[2] + part[3];
    };
    // block-wide exclusive prefix sum of one int per thread, in thread order (all threads call it)
    auto block_prefix_int = [&](int v) -> int {
        int inc = v;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const int up = __shfl_up(inc, o, kWave);
            if (lane >= o) inc += up;
        }
        __syncthreads();
        if (lane == kWave - 1) part[wv] = inc;
        __syncthreads();
        int base = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) base += (k < wv) ? part[k] : 0;
        return base + inc - v;
    };
    const int nSmall = block_sum_int(small ? 1 : 0), nBig = B - nSmall;
    const int sumMin = block_sum_int(big ? gMin : 0);
    const int sumWish = block_sum_int(big ? max(gWish, gMin) : 0);
    // chain the single-pass pairs only as far as the large pairs can use the workgroups: chain length c frees
    // nSmall - ceil(nSmall / c) of them
    int chain = 1;
    while (chain < kTeamChain && nBig > 0 && t.maxWG - (nSmall + chain - 1) / chain < sumWish) ++chain;
    int slots = t.maxWG - (nSmall + chain - 1) / chain;     // workgroups for the large pairs
    const bool fits = slots >= sumMin;       // not even the minimum teams: every pair one workgroup, no chains (B <= maxWG)
    if (!fits) { chain = 1; slots = t.maxWG - nSmall; }
    // The levels this pair's team can take: (workgroups, estimated length of an iteration), from its minimum team down the
    // levels of units per member.  The spare workgroups go where they shorten the LONGEST estimated iteration: the
    // smallest bound tau such that every pair brought down to tau (or as far as it can go) still fits, by bisection
    // over the levels' costs (a block-wide sum per step), then what is left over to the pairs just above, in pair order.
    constexpr int kLevels = 8;
    int lvG[kLevels];          // (every loop over the levels is fully unrolled: the tables stay in registers)
    float lvC[kLevels];
    int gLast = 0;
    {
        int G = fits ? gMin : 1;
        int u = (units + G - 1) / G;
        bool open = big;
#pragma unroll
        for (int k = 0; k < kLevels; ++k) {
            lvG[k] = G; lvC[k] = open ? team_level_cost(u) * weight : 3.0e38f;
            if (open) gLast = G;
            const int uNext = team_next_level(u);
            const int gNext = uNext > 0 ? (units + uNext - 1) / uNext : 0;
            open = open && uNext > 0 && gNext <= kMaxTeam && gNext > G && n / max(gNext, 1) >= kTeamMinShare;
            if (open) { G = gNext; u = (units + G - 1) / G; }
        }
    }
    auto teams_at = [&](float tau) -> int {      // this pair's team under the bound tau: the first level that meets it, or its last
        int G = gLast;
#pragma unroll
        for (int k = kLevels - 1; k >= 0; --k)
            if (lvC[k] <= tau) G = lvG[k];
        return big ? G : 0;
    };
    int G = b < B ? 1 : 0;
    if (nBig > 0) {
        // bisection on tau between 0 (everybody at its last level) and the largest first-level cost
        float hiC = big ? lvC[0] : 0.f;
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) hiC = fmaxf(hiC, __shfl_xor(hiC, o, kWave));
        __syncthreads();
        if (lane == 0) part[wv] = __float_as_int(hiC);
        __syncthreads();
        float hi = fmaxf(fmaxf(__int_as_float(part[0]), __int_as_float(part[1])), fmaxf(__int_as_float(part[2]), __int_as_float(part[3])));
        float lo = 0.f;
        // (hi always fits: every pair at its first level is sumMin <= slots, or one workgroup each)
        for (int step = 0; step < 14; ++step) {
            const float mid = 0.5f * (lo + hi);
            if (block_sum_int(teams_at(mid)) <= slots) hi = mid; else lo = mid;
        }
        G = big ? teams_at(hi) : G;
        // left-over workgroups: one more level for the pairs that can take one, in pair order
        int left = slots - block_sum_int(big ? G : 0);
        if (left > 0) {
            int want = 0;
#pragma unroll
            for (int k = 0; k + 1 < kLevels; ++k)
                if (big && lvG[k] == G && lvC[k + 1] < 3.0e38f && want == 0) want = lvG[k + 1] - G;
            const int before = block_prefix_int(want);
            if (want > 0 && before + want <= left) G += want;
        }
    }
    // a chain of single-pass pairs is one workgroup: its first pair carries the slot, the others hang on t.next
    {
        const int seq = block_prefix_int(small ? 1 : 0);   // this small pair's number among the small pairs (in pair order)
        if (small) first[seq] = b;      // (first[] is scratch here: small pair number -> pair)
        __syncthreads();
        const bool head = small && (seq % chain) == 0;
        if (b < B) t.next[b] = (small && seq + 1 < nSmall && (seq + 1) % chain != 0) ? first[seq + 1] : -1;
        __syncthreads();
        size[b] = (b < B) ? (small ? (head ? 1 : 0) : G) : 0;
    }
    __syncthreads();
    // Workgroup w is dispatched to XCD w % 8, so slot k = (w % 8) * per + w / 8 enumerates the
    // workgroups XCD by XCD (per = maxWG / 8 of them each).  A team takes consecutive slots of ONE
    // XCD (its exchange stays inside one L2); teams go to the XCD with the most free slots, which
    // spreads the launch over all eight L2s.  Only the teams of several members go through that (serial) loop; the
    // single workgroups then fill what is left, XCD by XCD.
    const int per = (t.maxWG % 8 == 0) ? t.maxWG / 8 : t.maxWG;
    const int nx = (per == t.maxWG) ? 1 : 8;
    // this pair's number among the teams / the single workgroups (in pair order; both counts in one word)
    const int numbers = block_prefix_int((b < B && size[b] > 1 ? 1 << 16 : 0) + (b < B && size[b] == 1 ? 1 : 0));
    const int teamNo = numbers >> 16, singleNo = numbers & 0xffff;
    if (b < B && size[b] > 1) teamList[teamNo] = b;
    const int nTeams = block_sum_int((b < B && size[b] > 1) ? 1 : 0);
    if (b == 0) {
        int used[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        bool ok = true;
        for (int k = 0; k < nTeams && ok; ++k) {
            // (the least-used XCD, first one on ties; the counters stay in registers: no indexing by a variable)
            int x = 0, ux = used[0];
#pragma unroll
            for (int c = 1; c < 8; ++c)
                if (c < nx && used[c] < ux) { x = c; ux = used[c]; }
            const int sz = size[teamList[k]];
            if (ux + sz > per) ok = false;
            first[teamList[k]] = x * per + ux;
#pragma unroll
            for (int c = 0; c < 8; ++c) used[c] += (c == x) ? sz : 0;
        }
        if (!ok) {   // does not fit XCD by XCD: plain packing (teams may span two XCDs)
            int acc = 0;
            for (int k = 0; k < nTeams; ++k) { first[teamList[k]] = acc; acc += size[teamList[k]]; }
#pragma unroll
            for (int c = 0; c < 8; ++c) used[c] = 0;
            for (int c = 0; c < 8; ++c) { const int take = min(max(acc - c * per, 0), per); xcdUsed[c] = (c < nx) ? take : per; }
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) xcdUsed[c] = (c < nx) ? used[c] : per;
        }
    }
    __syncthreads();
    if (b < B && size[b] == 1) {
        // the singleNo-th single workgroup: the singleNo-th free slot, XCD by XCD
        int skip = singleNo, slot = -1;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int freeC = per - xcdUsed[c];
            if (slot < 0 && c < nx) {
                if (skip < freeC) slot = c * per + xcdUsed[c] + skip;
                else skip -= freeC;
            }
        }
        first[b] = slot;    // (>= 0: the plan never hands out more workgroups than there are)
    }
    __syncthreads();
    if (b < B) {
        t.teamSize[b] = G;
        t.arrived[b] = 0u;
        for (int r = 0; r < size[b]; ++r) {
            const int k = first[b] + r;
            const int w = (per == t.maxWG) ? k : (k % per) * 8 + k / per;
            if (first[b] >= 0 && w < t.maxWG) { t.wgPair[w] = b; t.wgRank[w] = r; }
        }
    }
}

// Shared window scans (icp_pair, SHAREK): from this padded width on -- below, windows of 256 targets are rare.
#ifndef ICPFLOW_SHARE_LAUNCH_MIN_N
#define ICPFLOW_SHARE_LAUNCH_MIN_N 5000
#endif
bool icp_team_shares(const IcpOpts &opts, int N) { return opts.sharedScans && opts.adaptiveWindows && N >= ICPFLOW_SHARE_LAUNCH_MIN_N && N <= 12288; }
// dynamic LDS of a team member with the LDS image (image + records): the CU's 160 KiB less the team kernel's static LDS
// (~16 KiB with the accumulators of the shared window scans: 143 KiB; ~6.7 KiB without: 152 KiB)
size_t icp_team_room(const IcpOpts &opts, int N) { return icp_team_shares(opts, N) ? (size_t)143 * 1024 : (size_t)152 * 1024; }
// workgroups of a team launch: one per CU, or one per CU of HALF the GPU (a multiple of the eight XCDs either way)
int icp_team_workgroups(const IcpOpts &opts)
{
    const int cus = device_cus();
    return opts.teamsHalfGpu ? max(8, cus / 2 / 8 * 8) : cus;
}

// the plan of a team launch (icp_team_plan_kernel): depends on the pairs' lengths and roles only
void launch_icp_team_plan(const IcpTeam *team, const int32_t *lenX, const int32_t *lenY, const uint8_t *swap, int B, int N,
                          const IcpOpts &opts, hipStream_t s)
{
    IcpTeam t = *team;
    t.maxWG = min(icp_team_workgroups(opts), team->maxWG);
    // (records behind the LDS image of the padded length: what a member's share of the queries has to fit, see launch_icp)
    const size_t imgT = (size_t)((N + kChunk - 1) / kChunk * kChunk) * 12;
    const size_t roomT = icp_team_room(opts, N);
    const int recCapT = (opts.adaptiveWindows && N <= 12288 && imgT + 64 * 20 <= roomT) ? (int)((roomT - imgT) / 20 / 64 * 64) : 0;
    hipLaunchKernelGGL(icp_team_plan_kernel, dim3(1), dim3(256), 0, s, lenX, lenY, swap, B, t, recCapT, opts.pairActive);
}

}  // namespace icpflow
