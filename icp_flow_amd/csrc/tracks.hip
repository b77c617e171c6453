// tracks.hip -- the clusters of a sample's shared sweep linked across its gaps, and a constant velocity per track
// (include/icpflow_hip.h, "8(k) object tracks": icpflow_object_tracks_extend, icpflow_object_tracks_fit); the same extension
// on the SOURCE side of a pair and one row per track over a log ("8(l)": icpflow_object_tracks_extend_side,
// icpflow_object_tracks_path -- trk_path_kernel, a thread per track like the fit); which observation breaks its track
// ("8(m) track repair": icpflow_object_tracks_suspects -- trk_suspects_kernel, a thread per OBSERVATION, the fit leave-one-out;
// repair.hip registers the named pairs again); which segment of the shared sweep lacks a pair in its gap ("8(n) track fill":
// icpflow_object_tracks_missing -- trk_missing_kernel, a thread per (gap slot, segment), the suspects' two walks through one
// device function; repair.hip finds the source cluster and registers the pair).
//
// icpflow_object_tracks_extend, one gap:
//   1. trk_labels_kernel    "track id per row" as a float32 labelling (an id is its own label, no track is -1)
//   2. overlap.hip's chain  this gap's labels (side A) against it (side B): partner, mutual and IoU per segment of A
//   3. trk_assign_kernel    ONE workgroup of 1024, thread t segments 4 t .. 4 t + 3: inherit or fresh, the fresh ids by an
//                           exclusive scan in ascending label order; the rows of d_segments, the counts, overflow, *d_next_id
//   4. trk_relabel_kernel   a thread per row: the rows of linkable segments take their segment's id
//   5. trk_obs_kernel       a thread per object row: the id of its destination label's segment (binary search on label_key);
//                           side 0: of its source label's
// The state is written by kernels 3 (its last statement) and 4 only, behind everything that reads it, and not at all on
// overflow.  icpflow_object_tracks_fit: one thread per track walks all observations in row order -- T * M is a few thousand
// tracks times a few thousand rows at most (a sample has at most 15 gaps of at most 4096 pairs), far below what a segmented
// reduction would pay for; the order of the sums is then the order of the rows, and the numbers a function of the arguments.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "boxes.hpp"
#include "common.hpp"
#include "host.hpp"
#include "overlap.hpp"

using icpflow::kWave;
using icpflow::pointer_error;
using icpflow::report_error;
using icpflow::report_errorf;
using icpflow::workspace_error;
using icpflow::overlap::kLmax;
using icpflow::overlap::kMaxRows;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kAssignThreads = 1024;
constexpr int kAssignEach = kLmax / kAssignThreads;
constexpr int kOvCols = ICPFLOW_OVERLAP_COLS, kSegCols = ICPFLOW_TRACK_SEGMENT_COLS, kObsCols = ICPFLOW_TRACK_OBS_COLS;
constexpr int kTrackCols = ICPFLOW_TRACK_COLS, kObjectCols = ICPFLOW_OBJECT_COLS;
constexpr int kFitCounts = ICPFLOW_TRACK_FIT_COUNTS;
static_assert(ICPFLOW_TRACK_EXTEND_COUNTS == 6, "segments, inherited, fresh, observations with and without an id, overflow");
constexpr int kMaxId = 1 << 24;                        // ids travel as float32 labels: exact up to here
constexpr int kMaxFitRows = 1 << 24;
constexpr int kMaxSuspectRows = 1 << 16;               // the plan's walk is quadratic in the observations

// what an extension carves out of its workspace, in this order (the size query runs it on a null base)
struct Carve {
    icpflow::overlap::Carve ov;
    float *trackLabel;       // [n]
    double *table[2];        // [Lmax][kOvCols] each: the overlap's tables, A = this gap's labels, B = the tracks
    int32_t *num;            // [2]
    int64_t *ovCounts;       // [4]
    int32_t *segId;          // [Lmax] the id of every segment of A, -1 when it is not linkable
    int32_t *state;          // [2] 1 iff the extension went through; the segments of A
    size_t total;
};

bool carve(void *base, int n, int Lmax, Carve *c)
{
    icpflow::Carver ws(base);
    if (!icpflow::overlap::carve(ws, n, Lmax, &c->ov)) return false;
    c->trackLabel = ws.take<float>((size_t)n * sizeof(float));
    for (int k = 0; k < 2; ++k) c->table[k] = ws.take<double>((size_t)Lmax * kOvCols * sizeof(double));
    c->num = ws.take<int32_t>(2 * sizeof(int32_t));
    c->ovCounts = ws.take<int64_t>(ICPFLOW_OVERLAP_COUNTS * sizeof(int64_t));
    c->segId = ws.take<int32_t>((size_t)Lmax * sizeof(int32_t));
    c->state = ws.take<int32_t>(2 * sizeof(int32_t));
    c->total = ws.total();
    return true;
}

__global__ __launch_bounds__(kThreads) void trk_labels_kernel(const int32_t *__restrict__ trackOfRow, int n, float *__restrict__ label)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int t = trackOfRow[i];
    label[i] = t < 0 ? -1.0f : (float)t;               // (an id beyond 2^24 never enters the state: overflow below)
}

__global__ __launch_bounds__(kAssignThreads) void trk_assign_kernel(const int32_t *__restrict__ num, const double *__restrict__ tableA, int Lmax,
                                                                    double minIou, int32_t *__restrict__ nextId, int32_t *__restrict__ segId,
                                                                    int32_t *__restrict__ state, double *__restrict__ segments,
                                                                    int32_t *__restrict__ dNum, unsigned long long *__restrict__ counts)
{
    __shared__ int part[3][kAssignThreads / kWave];
    const int La = num[0], Lb = num[1], tid = threadIdx.x, wave = tid >> 6, lane = tid & (kWave - 1);
    const bool tooMany = La < 0 || Lb < 0;
    const int L = tooMany ? 0 : min(La, Lmax);
    const int next = *nextId;
    bool link[kAssignEach], inherit[kAssignEach];
    int fresh = 0, linked = 0, kept = 0;
#pragma unroll
    for (int e = 0; e < kAssignEach; ++e) {
        const int c = tid * kAssignEach + e;
        link[e] = inherit[e] = false;
        if (c < L) {
            const double *row = tableA + (size_t)c * kOvCols;
            link[e] = icpflow::overlap::linkable(row[0]);
            inherit[e] = link[e] && row[3] >= 0.0 && row[8] != 0.0 && row[9] >= minIou;
        }
        linked += link[e] ? 1 : 0, kept += inherit[e] ? 1 : 0, fresh += (link[e] && !inherit[e]) ? 1 : 0;
    }
    int incl = fresh;                                  // the fresh segments before this thread's, in ascending label order
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int up = __shfl_up(incl, o, kWave);
        if (lane >= o) incl += up;
    }
    const int linkedW = icpflow::wave_sum(linked), keptW = icpflow::wave_sum(kept);
    if (lane == kWave - 1) part[0][wave] = incl;
    if (lane == 0) part[1][wave] = linkedW, part[2][wave] = keptW;
    __syncthreads();
    int before = incl - fresh, allFresh = 0, allLinked = 0, allKept = 0;
    for (int w = 0; w < kAssignThreads / kWave; ++w) {
        if (w < wave) before += part[0][w];
        allFresh += part[0][w], allLinked += part[1][w], allKept += part[2][w];
    }
    const bool overflow = tooMany || next < 0 || next > kMaxId - allFresh;
    if (tid == 0) {
        state[0] = overflow ? 0 : 1, state[1] = L;
        *dNum = La < 0 ? La : Lb < 0 ? Lb : overflow ? -max(La, 1) : La;
        counts[0] = overflow ? 0ull : (unsigned long long)allLinked;
        counts[1] = overflow ? 0ull : (unsigned long long)allKept;
        counts[2] = overflow ? 0ull : (unsigned long long)allFresh;
        counts[3] = 0ull, counts[4] = 0ull, counts[5] = overflow ? 1ull : 0ull;
    }
    if (overflow) return;                              // (workgroup-uniform) the state keeps every bit
#pragma unroll
    for (int e = 0; e < kAssignEach; ++e) {
        const int c = tid * kAssignEach + e;
        if (c >= L) continue;
        const double *row = tableA + (size_t)c * kOvCols;
        const int id = !link[e] ? -1 : inherit[e] ? (int)row[4] : next + before;
        if (link[e] && !inherit[e]) ++before;
        segId[c] = id;
        double *out = segments + (size_t)c * kSegCols;
        out[0] = row[0], out[1] = row[1], out[2] = (double)id, out[3] = inherit[e] ? 1.0 : 0.0, out[4] = row[5], out[5] = row[9];
    }
    if (tid == 0) *nextId = next + allFresh;           // (read into `next` by every thread before the barrier above)
}

__global__ __launch_bounds__(kThreads) void trk_relabel_kernel(const int32_t *__restrict__ state, const int32_t *__restrict__ segOf,
                                                               const int32_t *__restrict__ segId, int n, int32_t *__restrict__ trackOfRow)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n || state[0] == 0) return;
    const int s = segOf[i];
    if (s >= 0 && s < state[1]) {
        const int id = segId[s];
        if (id >= 0) trackOfRow[i] = id;
    }
}

// the segment of a label in the overlap's table of side A (column 0, ascending by label_key), or -1
__device__ __forceinline__ int find_segment(const double *__restrict__ table, int L, float label)
{
    const uint32_t want = icpflow::label_key(icpflow::boxes::quieted(label));
    int lo = 0, hi = L;                                // the first segment whose key is not below `want`
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (icpflow::label_key(icpflow::boxes::quieted((float)table[(size_t)mid * kOvCols])) < want) lo = mid + 1; else hi = mid;
    }
    return lo < L && icpflow::label_key(icpflow::boxes::quieted((float)table[(size_t)lo * kOvCols])) == want ? lo : -1;
}

__global__ __launch_bounds__(kThreads) void trk_obs_kernel(const int32_t *__restrict__ state, const double *__restrict__ tableA,
                                                           const int32_t *__restrict__ segId, const double *__restrict__ objects, int P,
                                                           int side, double gap, double seconds, double *__restrict__ obs,
                                                           unsigned long long *__restrict__ counts)
{
    __shared__ int sh[kWaves][2];
    const int p = blockIdx.x * kThreads + (int)threadIdx.x;
    const bool live = p < P;
    bool with = false;
    if (live) {
        const double *o = objects + (size_t)p * kObjectCols;
        int id = -1;
        if (state[0] != 0 && o[22] > 0.0) {
            const int c = find_segment(tableA, state[1], (float)o[side]);   // (side 1: the destination label, side 0: the source label)
            if (c >= 0) id = segId[c];
        }
        with = id >= 0;
        const double len = o[16], wid = o[17];
        double *row = obs + (size_t)p * kObsCols;
        row[0] = (double)id, row[1] = gap, row[2] = seconds;
        row[3] = o[7], row[4] = o[8], row[5] = o[9];
        row[6] = len >= wid ? len : wid, row[7] = len >= wid ? wid : len, row[8] = o[18];
        row[9] = o[22], row[10] = o[4], row[11] = o[5], row[12] = o[6];
    }
    const bool flag[2] = {with, live && !with};
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 2; ++k) {                      // (every lane takes every round: the ballots see whole waves)
        const int t = __popcll(__ballot(flag[k]));
        if ((threadIdx.x & (kWave - 1)) == 0) sh[wave][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        int t = 0;
        for (int w = 0; w < kWaves; ++w) t += sh[w][threadIdx.x];
        if (t != 0) atomicAdd(&counts[3 + threadIdx.x], (unsigned long long)t);
    }
}

__global__ __launch_bounds__(kThreads) void trk_fit_kernel(const double *__restrict__ obs, int M, int T, double maxResidual, double minSpeed,
                                                           double *__restrict__ tracks, unsigned long long *__restrict__ counts)
{
    __shared__ int sh[kWaves][kFitCounts];
    const int t = blockIdx.x * kThreads + (int)threadIdx.x;
    const bool live = t < T;
    bool observed = false, judged = false, consistent = false, moving = false;
    if (live) {
        const double id = (double)t;
        int seen = 0;
        unsigned long long mask = 0ull;
        double num[3] = {0.0, 0.0, 0.0}, den = 0.0, longest = 0.0, shortest = 0.0, height = 0.0, points = 0.0;
        for (int k = 0; k < M; ++k) {
            const double *o = obs + (size_t)k * kObsCols;
            if (o[0] != id) continue;
            const double s = o[2];
            num[0] += s * o[3], num[1] += s * o[4], num[2] += s * o[5];
            den += s * s;
            ++seen;
            if (o[1] >= 0.0 && o[1] < 64.0) mask |= 1ull << (int)o[1];
            longest = o[6] > longest ? o[6] : longest, shortest = o[7] > shortest ? o[7] : shortest;
            height = o[8] > height ? o[8] : height, points = o[9] > points ? o[9] : points;
        }
        double v[3] = {0.0, 0.0, 0.0}, worst = 0.0, sum = 0.0;
        if (seen > 0) {
            v[0] = num[0] / den, v[1] = num[1] / den, v[2] = num[2] / den;
            for (int k = 0; k < M; ++k) {
                const double *o = obs + (size_t)k * kObsCols;
                if (o[0] != id) continue;
                const double rx = o[3] - o[2] * v[0], ry = o[4] - o[2] * v[1];
                const double r2 = rx * rx + ry * ry;
                worst = r2 > worst ? r2 : worst;
                sum += r2;
            }
        }
        const double speed = sqrt(v[0] * v[0] + v[1] * v[1]);
        const double largest = sqrt(worst), rms = seen > 0 ? sqrt(sum / (double)seen) : 0.0;
        observed = seen > 0;
        moving = observed && speed >= minSpeed;
        judged = __popcll(mask) >= 2;
        consistent = judged && largest <= maxResidual;
        double *row = tracks + (size_t)t * kTrackCols;
        row[0] = id, row[1] = (double)seen, row[2] = (double)mask;
        row[3] = v[0], row[4] = v[1], row[5] = v[2], row[6] = speed, row[7] = largest, row[8] = rms;
        row[9] = moving ? 1.0 : 0.0, row[10] = judged ? 1.0 : 0.0, row[11] = consistent ? 1.0 : 0.0;
        row[12] = longest, row[13] = shortest, row[14] = height, row[15] = points;
    }
    const bool flag[kFitCounts] = {live, observed, judged, consistent, moving};
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kFitCounts; ++k) {             // (every lane takes every round: the ballots see whole waves)
        const int c = __popcll(__ballot(flag[k]));
        if ((threadIdx.x & (kWave - 1)) == 0) sh[wave][k] = c;
    }
    __syncthreads();
    if (threadIdx.x < kFitCounts) {
        int c = 0;
        for (int w = 0; w < kWaves; ++w) c += sh[w][threadIdx.x];
        if (c != 0) atomicAdd(&counts[threadIdx.x], (unsigned long long)c);
    }
}

// The two walks that 8(m) and 8(n) share: the rows of track `id` in ascending order, fp64, every operation written out.  Row
// `skipRow` is left out (8(m): the observation itself; -1 leaves none out); a row whose gap equals `skipGap` is COUNTED as
// observed and enters nothing else (8(n): the slot's own gap; a NaN equals none).
struct OthersWalk {
    int others = 0, observed = 0;
    unsigned long long mask = 0ull;
    double num[3] = {0.0, 0.0, 0.0}, den = 0.0, land[3] = {0.0, 0.0, 0.0};   // sum s d, sum s s, sum (c + d)
};

__device__ __forceinline__ void walk_others(const double *__restrict__ obs, int M, double id, int skipRow, double skipGap, OthersWalk &w)
{
    for (int k = 0; k < M; ++k) {
        const double *o = obs + (size_t)k * kObsCols;
        if (k == skipRow || o[0] != id) continue;
        if (o[1] == skipGap) {
            ++w.observed;
            continue;
        }
        const double s = o[2];
        w.den += s * s;
        w.num[0] += s * o[3], w.num[1] += s * o[4], w.num[2] += s * o[5];
        w.land[0] += o[10] + o[3], w.land[1] += o[11] + o[4], w.land[2] += o[12] + o[5];
        if (o[1] >= 0.0 && o[1] < 64.0) w.mask |= 1ull << (int)o[1];
        ++w.others;
    }
}

// the largest squared xy residual of the same rows against d = s v
__device__ __forceinline__ double walk_inner(const double *__restrict__ obs, int M, double id, int skipRow, double skipGap, const double *v)
{
    double inner = 0.0;
    for (int k = 0; k < M; ++k) {
        const double *o = obs + (size_t)k * kObsCols;
        if (k == skipRow || o[0] != id || o[1] == skipGap) continue;
        const double rx = o[3] - o[2] * v[0], ry = o[4] - o[2] * v[1];
        const double r2 = rx * rx + ry * ry;
        inner = r2 > inner ? r2 : inner;
    }
    return inner;
}

// Which observation breaks its track (8(m)): a thread per observation j fits the OTHER observations of its track and asks
// whether they agree among themselves and j does not agree with them.  Two walks over the M rows in ascending order, fp64,
// every operation written out -- the fit's style, leave-one-out.
__global__ __launch_bounds__(kThreads) void trk_suspects_kernel(const double *__restrict__ obs, int M, int T, double maxResidual,
                                                                double *__restrict__ plan, unsigned long long *__restrict__ counts)
{
    constexpr int kCols = ICPFLOW_TRACK_PLAN_COLS, kCounts = ICPFLOW_TRACK_PLAN_COUNTS;
    __shared__ int sh[kWaves][kCounts];
    const int j = blockIdx.x * kThreads + (int)threadIdx.x;
    const bool live = j < M;
    bool withId = false, eligible = false, agreed = false, suspect = false;
    if (live) {
        const double *me = obs + (size_t)j * kObsCols;
        const double id = me[0];
        double row[kCols] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        withId = id >= 0.0 && id < (double)T;           // (a NaN is outside)
        if (withId) {
            const double none = __longlong_as_double(0x7ff8000000000000ll);   // no gap equals a NaN: every other row enters
            OthersWalk w;
            walk_others(obs, M, id, j, none, w);
            const int gaps = __popcll(w.mask);
            row[1] = (double)w.others, row[2] = (double)gaps;
            eligible = gaps >= 2 && w.den > 0.0;
            if (eligible) {
                const double v[3] = {w.num[0] / w.den, w.num[1] / w.den, w.num[2] / w.den};
                const double inner = walk_inner(obs, M, id, j, none, v);
                const double s = me[2];
                const double p[3] = {s * v[0], s * v[1], s * v[2]};
                const double rx = me[3] - p[0], ry = me[4] - p[1];
                const double r2 = rx * rx + ry * ry, m2 = maxResidual * maxResidual;
                agreed = inner <= m2;
                suspect = agreed && r2 > m2;
                row[0] = suspect ? 1.0 : 0.0, row[3] = p[0], row[4] = p[1], row[5] = p[2], row[6] = sqrt(r2), row[7] = sqrt(inner);
            }
        }
        double *out = plan + (size_t)j * kCols;
#pragma unroll
        for (int c = 0; c < kCols; ++c) out[c] = row[c];
    }
    const bool flag[kCounts] = {withId, eligible, agreed, suspect};
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kCounts; ++k) {                // (every lane takes every round: the ballots see whole waves)
        const int c = __popcll(__ballot(flag[k]));
        if ((threadIdx.x & (kWave - 1)) == 0) sh[wave][k] = c;
    }
    __syncthreads();
    if (threadIdx.x < kCounts) {
        int c = 0;
        for (int w = 0; w < kWaves; ++w) c += sh[w][threadIdx.x];
        if (c != 0) atomicAdd(&counts[threadIdx.x], (unsigned long long)c);
    }
}

// Which segment of the shared sweep lacks a pair in its gap, and what the other gaps predict for it (8(n)): a thread per
// (slot g = blockIdx.y, segment c) walks the observations of the segment's track as the suspects' threads do -- the rows of the
// slot's own gap say OBSERVED and enter nothing else.  The slots' gaps and seconds travel in the kernel arguments.
struct MissingSlots {
    int32_t gap[ICPFLOW_TRACK_MISSING_MAX_SLOTS];
    double seconds[ICPFLOW_TRACK_MISSING_MAX_SLOTS];
};

__global__ __launch_bounds__(kThreads) void trk_missing_kernel(const double *__restrict__ obs, int M, int T, const double *__restrict__ segments,
                                                               const int32_t *__restrict__ num, int Lmax, MissingSlots slots, double maxResidual,
                                                               double *__restrict__ plan, unsigned long long *__restrict__ counts)
{
    constexpr int kCols = ICPFLOW_TRACK_MISSING_COLS, kCounts = ICPFLOW_TRACK_MISSING_COUNTS;
    __shared__ int sh[kWaves][kCounts];
    const int g = blockIdx.y, c = blockIdx.x * kThreads + (int)threadIdx.x;
    const int L = min(num[g], Lmax);                    // (negative: no row of this slot)
    const bool live = c < L;
    bool withId = false, unseen = false, eligible = false, missing = false;
    if (live) {
        const double *seg = segments + ((size_t)g * Lmax + c) * kSegCols;
        const double id = seg[2];
        double row[kCols] = {0.0, id, seg[0], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, seg[1]};
        withId = id >= 0.0 && id < (double)T;           // (a NaN is outside)
        if (withId) {
            const double gap = (double)slots.gap[g];
            OthersWalk w;
            walk_others(obs, M, id, -1, gap, w);
            const int gaps = __popcll(w.mask);
            row[3] = (double)w.observed, row[4] = (double)w.others, row[5] = (double)gaps;
            unseen = w.observed == 0;
            eligible = unseen && gaps >= 2 && w.den > 0.0;
            if (eligible) {
                const double v[3] = {w.num[0] / w.den, w.num[1] / w.den, w.num[2] / w.den};
                const double inner = walk_inner(obs, M, id, -1, gap, v);
                const double s = slots.seconds[g], n = (double)w.others;
                const double p[3] = {s * v[0], s * v[1], s * v[2]};
                missing = inner <= maxResidual * maxResidual;
                row[0] = missing ? 1.0 : 0.0, row[6] = p[0], row[7] = p[1], row[8] = p[2];
                row[9] = w.land[0] / n - p[0], row[10] = w.land[1] / n - p[1], row[11] = w.land[2] / n - p[2], row[12] = sqrt(inner);
            }
        }
        double *out = plan + ((size_t)g * Lmax + c) * kCols;
#pragma unroll
        for (int k = 0; k < kCols; ++k) out[k] = row[k];
    }
    const bool flag[kCounts] = {withId, withId && unseen, eligible, missing};
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
        if (t != 0) atomicAdd(&counts[(size_t)g * kCounts + threadIdx.x], (unsigned long long)t);
    }
}

// One row per track over a log (8(l)): a thread per track walks the M observations in row order; of the observations of one
// step the one with the most source points is COUNTED (the lower row on a tie) -- a step's rows are contiguous, the steps are
// non-decreasing, so the walk keeps one candidate and counts it when the step changes.  fp64, every operation written out.
struct PathWalk {
    int seen = 0, first = 0, last = 0, pairs = 0;
    double seconds = 0.0, length = 0.0, sum[3] = {0.0, 0.0, 0.0}, dv = 0.0, jump = 0.0;
    double longest = 0.0, shortest = 0.0, height = 0.0, points = 0.0, start[3] = {0.0, 0.0, 0.0};
    double pc[3], pd[3], pv[3];                        // the previous counted observation: centre, displacement, velocity
};

__device__ __forceinline__ void path_count(PathWalk &w, const double *__restrict__ o, const double *__restrict__ f, int step)
{
    const double cx = o[10], cy = o[11], cz = o[12], dx = o[3], dy = o[4], dz = o[5], s = o[2];
    const double c[3] = {((f[0] * cx + f[1] * cy) + f[2] * cz) + f[9], ((f[3] * cx + f[4] * cy) + f[5] * cz) + f[10],
                         ((f[6] * cx + f[7] * cy) + f[8] * cz) + f[11]};
    const double d[3] = {(f[0] * dx + f[1] * dy) + f[2] * dz, (f[3] * dx + f[4] * dy) + f[5] * dz, (f[6] * dx + f[7] * dy) + f[8] * dz};
    const double v[3] = {d[0] / s, d[1] / s, d[2] / s};
    if (w.seen == 0) w.first = step, w.start[0] = c[0], w.start[1] = c[1], w.start[2] = c[2];
    else if (step == w.last + 1) {                     // ADJACENT steps only
        const double ax = v[0] - w.pv[0], ay = v[1] - w.pv[1];
        const double dv = sqrt(ax * ax + ay * ay);
        const double jx = (w.pc[0] + w.pd[0]) - c[0], jy = (w.pc[1] + w.pd[1]) - c[1];
        const double jump = sqrt(jx * jx + jy * jy);
        w.dv = dv > w.dv ? dv : w.dv, w.jump = jump > w.jump ? jump : w.jump;
        ++w.pairs;
    }
    ++w.seen;
    w.last = step;
    w.seconds += s;
    w.length += sqrt(d[0] * d[0] + d[1] * d[1]);
#pragma unroll
    for (int a = 0; a < 3; ++a) w.sum[a] += d[a], w.pc[a] = c[a], w.pd[a] = d[a], w.pv[a] = v[a];
    w.longest = o[6] > w.longest ? o[6] : w.longest, w.shortest = o[7] > w.shortest ? o[7] : w.shortest;
    w.height = o[8] > w.height ? o[8] : w.height, w.points = o[9] > w.points ? o[9] : w.points;
}

__global__ __launch_bounds__(kThreads) void trk_path_kernel(const double *__restrict__ obs, const int32_t *__restrict__ stepOf, int M,
                                                            const double *__restrict__ frames, int F, int T, double maxDv, double minSpeed,
                                                            double *__restrict__ paths, unsigned long long *__restrict__ counts)
{
    constexpr int kCols = ICPFLOW_TRACK_PATH_COLS, kCounts = ICPFLOW_TRACK_PATH_COUNTS;
    __shared__ int sh[kWaves][kCounts];
    const int t = blockIdx.x * kThreads + (int)threadIdx.x;
    const bool live = t < T;
    bool observed = false, judged = false, smooth = false, moving = false;
    if (live) {
        const double id = (double)t;
        PathWalk w;
        int cand = -1, candStep = 0;                    // the row that stands for candStep so far
        for (int k = 0; k < M; ++k) {
            const double *o = obs + (size_t)k * kObsCols;
            if (o[0] != id) continue;
            const int s = stepOf[k];
            if (s < 0 || s >= F) continue;              // a step outside [0, F): not counted
            if (cand >= 0 && s == candStep) {
                if (o[9] > obs[(size_t)cand * kObsCols + 9]) cand = k;
                continue;
            }
            if (cand >= 0) path_count(w, obs + (size_t)cand * kObsCols, frames + (size_t)candStep * 12, candStep);
            cand = k, candStep = s;
        }
        if (cand >= 0) path_count(w, obs + (size_t)cand * kObsCols, frames + (size_t)candStep * 12, candStep);
        double v[3] = {0.0, 0.0, 0.0};
        if (w.seen > 0) v[0] = w.sum[0] / w.seconds, v[1] = w.sum[1] / w.seconds, v[2] = w.sum[2] / w.seconds;
        const double speed = sqrt(v[0] * v[0] + v[1] * v[1]);
        observed = w.seen > 0;
        moving = observed && speed >= minSpeed;
        judged = w.pairs >= 1;
        smooth = judged && w.dv <= maxDv;
        double *row = paths + (size_t)t * kCols;
        row[0] = id, row[1] = (double)w.seen, row[2] = (double)w.first, row[3] = (double)w.last;
        row[4] = observed ? (double)((w.last - w.first + 1) - w.seen) : 0.0;
        row[5] = w.seconds, row[6] = w.length, row[7] = v[0], row[8] = v[1], row[9] = v[2], row[10] = speed;
        row[11] = w.dv, row[12] = (double)w.pairs, row[13] = w.jump;
        row[14] = moving ? 1.0 : 0.0, row[15] = judged ? 1.0 : 0.0, row[16] = smooth ? 1.0 : 0.0;
        row[17] = w.longest, row[18] = w.shortest, row[19] = w.height, row[20] = w.points;
        row[21] = w.start[0], row[22] = w.start[1], row[23] = w.start[2];
    }
    const bool flag[kCounts] = {live, observed, judged, smooth, moving};
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kCounts; ++k) {                // (every lane takes every round: the ballots see whole waves)
        const int c = __popcll(__ballot(flag[k]));
        if ((threadIdx.x & (kWave - 1)) == 0) sh[wave][k] = c;
    }
    __syncthreads();
    if (threadIdx.x < kCounts) {
        int c = 0;
        for (int w = 0; w < kWaves; ++w) c += sh[w][threadIdx.x];
        if (c != 0) atomicAdd(&counts[threadIdx.x], (unsigned long long)c);
    }
}

bool sizes_ok(int n, int Lmax) { return n >= 0 && n <= kMaxRows && Lmax >= 1 && Lmax <= kLmax; }

// -> 0, or the status of a refused parameter block
int check_params(const char *fn, const icpflow_track_params_t *p)
{
    if (p->struct_size != sizeof(icpflow_track_params_t))
        return report_errorf(ICPFLOW_E_ARG, "%s: params->struct_size = %zu, this library's icpflow_track_params_t has %zu bytes", fn, p->struct_size,
                             sizeof(icpflow_track_params_t));
    if (!(p->min_iou > 0.0 && p->min_iou <= 1.0)) return report_errorf(ICPFLOW_E_ARG, "%s: min_iou = %g: min_iou must lie in (0, 1]", fn, p->min_iou);
    if (!(p->max_residual >= 0.0) || !std::isfinite(p->max_residual))
        return report_errorf(ICPFLOW_E_ARG, "%s: max_residual = %g: max_residual must be finite and not negative", fn, p->max_residual);
    if (!(p->min_speed >= 0.0) || !std::isfinite(p->min_speed))
        return report_errorf(ICPFLOW_E_ARG, "%s: min_speed = %g: min_speed must be finite and not negative", fn, p->min_speed);
    return ICPFLOW_OK;
}

// both entry points of the extension; `fn` names the one that was called in every message
int extend(const char *fn, const float *d_labels, int n, int Lmax, int32_t *d_track_of_row, int32_t *d_next_id, const double *d_objects, int P,
           int side, int gap, double seconds, const icpflow_track_params_t *params, double *d_segments, int32_t *d_num, double *d_obs,
           int64_t *d_counts, void *d_ws, size_t ws_bytes, icpflow_stream_t stream)
{
    if (n < 0 || P < 0) return report_errorf(ICPFLOW_E_ARG, "%s: n = %d, P = %d: a negative size", fn, n, P);
    if (n > kMaxRows) return report_errorf(ICPFLOW_E_LIMIT, "%s: n = %d: at most %d rows", fn, n, kMaxRows);
    if (Lmax < 1) return report_errorf(ICPFLOW_E_ARG, "%s: Lmax = %d: Lmax must be at least 1", fn, Lmax);
    if (Lmax > kLmax) return report_errorf(ICPFLOW_E_LIMIT, "%s: Lmax = %d: at most %d segments", fn, Lmax, kLmax);
    if (side != 0 && side != 1) return report_errorf(ICPFLOW_E_ARG, "%s: side = %d: side is 0 (the source labels) or 1 (the destination labels)", fn, side);
    if (gap < 0 || gap > 63) return report_errorf(ICPFLOW_E_ARG, "%s: gap = %d: gap must lie in [0, 63]", fn, gap);
    if (!(seconds > 0.0) || !std::isfinite(seconds))
        return report_errorf(ICPFLOW_E_ARG, "%s: seconds = %g: seconds must be positive and finite", fn, seconds);
    if (!d_next_id || !params || !d_segments || !d_num || !d_counts || (n > 0 && (!d_labels || !d_track_of_row)) || (P > 0 && (!d_objects || !d_obs)))
        return pointer_error(fn);
    if (const int rc = check_params(fn, params)) return rc;
    Carve c{};
    if (!carve(d_ws, n, Lmax, &c)) return report_errorf(ICPFLOW_E_ARG, "%s: no workspace layout for these sizes", fn);
    if (!d_ws || ws_bytes < c.total) return workspace_error(fn, "icpflow_object_tracks_extend_workspace_bytes", d_ws, ws_bytes, c.total);
    if (((uintptr_t)d_ws & 15) != 0) return report_errorf(ICPFLOW_E_ARG, "%s: d_ws must be 16-byte aligned", fn);

    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        ICPFLOW_TRY(hipMemsetAsync(c.num, 0, 2 * sizeof(int32_t), st));
    } else {
        trk_labels_kernel<<<(n + kThreads - 1) / kThreads, kThreads, 0, st>>>(d_track_of_row, n, c.trackLabel);
        ICPFLOW_TRY(hipGetLastError());
        ICPFLOW_TRY(icpflow::overlap::launch_links(d_labels, c.trackLabel, n, Lmax, c.num, c.num + 1, c.ov, st));
        ICPFLOW_TRY(icpflow::overlap::launch_tables(c.ov, c.num, c.num + 1, Lmax, c.table[0], c.table[1], c.ovCounts, st));
    }
    trk_assign_kernel<<<1, kAssignThreads, 0, st>>>(c.num, c.table[0], Lmax, params->min_iou, d_next_id, c.segId, c.state, d_segments, d_num,
                                                    (unsigned long long *)d_counts);
    ICPFLOW_TRY(hipGetLastError());
    if (n > 0) {
        trk_relabel_kernel<<<(n + kThreads - 1) / kThreads, kThreads, 0, st>>>(c.state, c.ov.side[0].segOf, c.segId, n, d_track_of_row);
        ICPFLOW_TRY(hipGetLastError());
    }
    if (P > 0) {
        trk_obs_kernel<<<(P + kThreads - 1) / kThreads, kThreads, 0, st>>>(c.state, c.table[0], c.segId, d_objects, P, side, (double)gap, seconds, d_obs,
                                                                           (unsigned long long *)d_counts);
        ICPFLOW_TRY(hipGetLastError());
    }
    return ICPFLOW_OK;
}

}  // namespace

extern "C" {

int icpflow_object_tracks_default_params(icpflow_track_params_t *params)
{
    if (!params) return pointer_error("icpflow_object_tracks_default_params");
    params->struct_size = sizeof(icpflow_track_params_t);
    params->min_iou = 0.5, params->max_residual = 0.2, params->min_speed = 0.5;
    return ICPFLOW_OK;
}

size_t icpflow_object_tracks_extend_workspace_bytes(int n, int Lmax)
{
    if (!sizes_ok(n, Lmax)) return 0;
    Carve c{};
    return carve(nullptr, n, Lmax, &c) ? c.total : 0;
}

int icpflow_object_tracks_extend(const float *d_labels, int n, int Lmax, int32_t *d_track_of_row, int32_t *d_next_id, const double *d_objects,
                                 int P, int gap, double seconds, const icpflow_track_params_t *params, double *d_segments, int32_t *d_num,
                                 double *d_obs, int64_t *d_counts, void *d_ws, size_t ws_bytes, icpflow_stream_t stream)
{
    return extend("icpflow_object_tracks_extend", d_labels, n, Lmax, d_track_of_row, d_next_id, d_objects, P, 1, gap, seconds, params, d_segments,
                  d_num, d_obs, d_counts, d_ws, ws_bytes, stream);
}

int icpflow_object_tracks_extend_side(const float *d_labels, int n, int Lmax, int32_t *d_track_of_row, int32_t *d_next_id,
                                      const double *d_objects, int P, int side, int gap, double seconds, const icpflow_track_params_t *params,
                                      double *d_segments, int32_t *d_num, double *d_obs, int64_t *d_counts, void *d_ws, size_t ws_bytes,
                                      icpflow_stream_t stream)
{
    return extend("icpflow_object_tracks_extend_side", d_labels, n, Lmax, d_track_of_row, d_next_id, d_objects, P, side, gap, seconds, params,
                  d_segments, d_num, d_obs, d_counts, d_ws, ws_bytes, stream);
}

int icpflow_object_tracks_fit(const double *d_obs, int M, int T, const icpflow_track_params_t *params, double *d_tracks, int64_t *d_counts,
                              icpflow_stream_t stream)
{
    const char *fn = "icpflow_object_tracks_fit";
    if (M < 0 || T < 0) return report_errorf(ICPFLOW_E_ARG, "icpflow_object_tracks_fit: M = %d, T = %d: a negative size", M, T);
    if (M > kMaxFitRows || T > kMaxFitRows)
        return report_errorf(ICPFLOW_E_LIMIT, "icpflow_object_tracks_fit: M = %d, T = %d: at most %d observations and tracks", M, T, kMaxFitRows);
    if (!params || !d_counts || (M > 0 && !d_obs) || (T > 0 && !d_tracks)) return pointer_error(fn);
    if (const int rc = check_params(fn, params)) return rc;

    hipStream_t st = (hipStream_t)stream;
    ICPFLOW_TRY(hipMemsetAsync(d_counts, 0, kFitCounts * sizeof(int64_t), st));
    if (T == 0) return ICPFLOW_OK;
    trk_fit_kernel<<<(T + kThreads - 1) / kThreads, kThreads, 0, st>>>(d_obs, M, T, params->max_residual, params->min_speed, d_tracks,
                                                                       (unsigned long long *)d_counts);
    ICPFLOW_TRY(hipGetLastError());
    return ICPFLOW_OK;
}

int icpflow_object_tracks_suspects(const double *d_obs, int M, int T, const icpflow_track_params_t *params, double *d_plan, int64_t *d_counts,
                                   icpflow_stream_t stream)
{
    const char *fn = "icpflow_object_tracks_suspects";
    if (M < 0 || T < 0) return report_errorf(ICPFLOW_E_ARG, "icpflow_object_tracks_suspects: M = %d, T = %d: a negative size", M, T);
    if (M > kMaxSuspectRows || T > kMaxFitRows)
        return report_errorf(ICPFLOW_E_LIMIT, "icpflow_object_tracks_suspects: M = %d, T = %d: at most %d observations (the walk is quadratic) and %d tracks",
                             M, T, kMaxSuspectRows, kMaxFitRows);
    if (!params || !d_counts || (M > 0 && (!d_obs || !d_plan))) return pointer_error(fn);
    if (params->struct_size != sizeof(icpflow_track_params_t))
        return report_errorf(ICPFLOW_E_ARG, "%s: params->struct_size = %zu, this library's icpflow_track_params_t has %zu bytes", fn, params->struct_size,
                             sizeof(icpflow_track_params_t));
    if (!(params->max_residual >= 0.0) || !std::isfinite(params->max_residual))
        return report_errorf(ICPFLOW_E_ARG, "%s: max_residual = %g: max_residual must be finite and not negative", fn, params->max_residual);

    hipStream_t st = (hipStream_t)stream;
    ICPFLOW_TRY(hipMemsetAsync(d_counts, 0, ICPFLOW_TRACK_PLAN_COUNTS * sizeof(int64_t), st));
    if (M == 0) return ICPFLOW_OK;
    trk_suspects_kernel<<<(M + kThreads - 1) / kThreads, kThreads, 0, st>>>(d_obs, M, T, params->max_residual, d_plan, (unsigned long long *)d_counts);
    ICPFLOW_TRY(hipGetLastError());
    return ICPFLOW_OK;
}

int icpflow_object_tracks_missing(const double *d_obs, int M, int T, const double *d_segments, const int32_t *d_num, int G, int Lmax,
                                  const int32_t *h_gap, const double *h_seconds, const icpflow_track_params_t *params, double *d_plan,
                                  int64_t *d_counts, icpflow_stream_t stream)
{
    const char *fn = "icpflow_object_tracks_missing";
    constexpr int kSlots = ICPFLOW_TRACK_MISSING_MAX_SLOTS;
    if (M < 0 || T < 0) return report_errorf(ICPFLOW_E_ARG, "icpflow_object_tracks_missing: M = %d, T = %d: a negative size", M, T);
    if (G < 1 || G > kSlots) return report_errorf(ICPFLOW_E_ARG, "icpflow_object_tracks_missing: G = %d: G must lie in [1, %d]", G, kSlots);
    if (Lmax < 1) return report_errorf(ICPFLOW_E_ARG, "icpflow_object_tracks_missing: Lmax = %d: Lmax must be at least 1", Lmax);
    if (M > kMaxSuspectRows || T > kMaxFitRows)
        return report_errorf(ICPFLOW_E_LIMIT, "icpflow_object_tracks_missing: M = %d, T = %d: at most %d observations (every segment walks them) and %d tracks",
                             M, T, kMaxSuspectRows, kMaxFitRows);
    if (Lmax > kLmax) return report_errorf(ICPFLOW_E_LIMIT, "icpflow_object_tracks_missing: Lmax = %d: at most %d segments", Lmax, kLmax);
    if (!params || !d_segments || !d_num || !h_gap || !h_seconds || !d_plan || !d_counts || (M > 0 && !d_obs)) return pointer_error(fn);
    if (params->struct_size != sizeof(icpflow_track_params_t))
        return report_errorf(ICPFLOW_E_ARG, "%s: params->struct_size = %zu, this library's icpflow_track_params_t has %zu bytes", fn, params->struct_size,
                             sizeof(icpflow_track_params_t));
    if (!(params->max_residual >= 0.0) || !std::isfinite(params->max_residual))
        return report_errorf(ICPFLOW_E_ARG, "%s: max_residual = %g: max_residual must be finite and not negative", fn, params->max_residual);
    MissingSlots slots{};
    unsigned long long seen = 0ull;
    for (int g = 0; g < G; ++g) {
        if (h_gap[g] < 0 || h_gap[g] > 63) return report_errorf(ICPFLOW_E_ARG, "%s: h_gap[%d] = %d: a gap must lie in [0, 63]", fn, g, h_gap[g]);
        if (seen >> h_gap[g] & 1ull) return report_errorf(ICPFLOW_E_ARG, "%s: h_gap[%d] = %d: the gaps must be distinct", fn, g, h_gap[g]);
        if (!(h_seconds[g] > 0.0) || !std::isfinite(h_seconds[g]))
            return report_errorf(ICPFLOW_E_ARG, "%s: h_seconds[%d] = %g: seconds must be positive and finite", fn, g, h_seconds[g]);
        seen |= 1ull << h_gap[g];
        slots.gap[g] = h_gap[g], slots.seconds[g] = h_seconds[g];
    }

    hipStream_t st = (hipStream_t)stream;
    ICPFLOW_TRY(hipMemsetAsync(d_counts, 0, (size_t)G * ICPFLOW_TRACK_MISSING_COUNTS * sizeof(int64_t), st));
    trk_missing_kernel<<<dim3((Lmax + kThreads - 1) / kThreads, G), kThreads, 0, st>>>(d_obs, M, T, d_segments, d_num, Lmax, slots, params->max_residual,
                                                                                       d_plan, (unsigned long long *)d_counts);
    ICPFLOW_TRY(hipGetLastError());
    return ICPFLOW_OK;
}

int icpflow_object_tracks_path_default_params(icpflow_track_path_params_t *params)
{
    if (!params) return pointer_error("icpflow_object_tracks_path_default_params");
    params->struct_size = sizeof(icpflow_track_path_params_t);
    params->max_dv = 1.0, params->min_speed = 0.5;
    return ICPFLOW_OK;
}

int icpflow_object_tracks_path(const double *d_obs, const int32_t *d_step, int M, const double *d_frames, int F, int T,
                               const icpflow_track_path_params_t *params, double *d_paths, int64_t *d_counts, icpflow_stream_t stream)
{
    const char *fn = "icpflow_object_tracks_path";
    if (M < 0 || T < 0 || F < 0) return report_errorf(ICPFLOW_E_ARG, "icpflow_object_tracks_path: M = %d, T = %d, F = %d: a negative size", M, T, F);
    if (M > kMaxFitRows || T > kMaxFitRows || F > kMaxFitRows)
        return report_errorf(ICPFLOW_E_LIMIT, "icpflow_object_tracks_path: M = %d, T = %d, F = %d: at most %d observations, tracks and files", M, T, F,
                             kMaxFitRows);
    if (M > 0 && F < 1) return report_errorf(ICPFLOW_E_ARG, "icpflow_object_tracks_path: M = %d observations and F = %d files", M, F);
    if (!params || !d_counts || (M > 0 && (!d_obs || !d_step)) || (F > 0 && !d_frames) || (T > 0 && !d_paths)) return pointer_error(fn);
    if (params->struct_size != sizeof(icpflow_track_path_params_t))
        return report_errorf(ICPFLOW_E_ARG, "%s: params->struct_size = %zu, this library's icpflow_track_path_params_t has %zu bytes", fn, params->struct_size,
                             sizeof(icpflow_track_path_params_t));
    if (!(params->max_dv >= 0.0) || !std::isfinite(params->max_dv))
        return report_errorf(ICPFLOW_E_ARG, "%s: max_dv = %g: max_dv must be finite and not negative", fn, params->max_dv);
    if (!(params->min_speed >= 0.0) || !std::isfinite(params->min_speed))
        return report_errorf(ICPFLOW_E_ARG, "%s: min_speed = %g: min_speed must be finite and not negative", fn, params->min_speed);

    hipStream_t st = (hipStream_t)stream;
    ICPFLOW_TRY(hipMemsetAsync(d_counts, 0, ICPFLOW_TRACK_PATH_COUNTS * sizeof(int64_t), st));
    if (T == 0) return ICPFLOW_OK;
    trk_path_kernel<<<(T + kThreads - 1) / kThreads, kThreads, 0, st>>>(d_obs, d_step, M, d_frames, F, T, params->max_dv, params->min_speed, d_paths,
                                                                        (unsigned long long *)d_counts);
    ICPFLOW_TRY(hipGetLastError());
    return ICPFLOW_OK;
}

}  // extern "C"
