// trust.hpp -- the trust byte of include/icpflow_hip.h, "8(i) trust byte", as the two kernels of trust.hip compose it: the
// layout of the byte, the columns of the two segment tables it reads, and the three decisions (a segment's bits, a row's class,
// KEEP) as device functions of plain numbers, so that each is stated once.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "labelkey.hpp"
#include "nnresid.hpp"
#include "../../include/icpflow_hip.h"

namespace icpflow {
namespace trust {

constexpr int kLmax = 4096;
constexpr int kCounts = ICPFLOW_TRUST_COUNTS;
constexpr int kResidCols = ICPFLOW_NNRS_COLS, kSightCols = ICPFLOW_SIGHT_COLS;
constexpr int kGoodAfter = 10, kSumAfter = 16;      // icpflow_nn_residual_segments' table: AFTER good rows, AFTER sum of d
constexpr int kFarAfter = 15;                       // icpflow_sight_segments' table: AFTER far rows of code k at kFarAfter + 2 k

constexpr int kRowMask = 7, kFitShift = 3, kFitMask = 3;
constexpr unsigned kMatched = 1u << 5, kSkipped = 1u << 6, kKeep = 1u << 7;
constexpr int kRowBad = 0, kRowNear = 1, kRowNoCode = 7;
constexpr int kFitSeenThrough = 1, kFitLostFromView = 2, kFitUndecided = 3;

struct Params {
    double above, share;
    float far2;
    float skip[2];
};

// a NaN label as the tables' float64 column holds it: widening a float quiets a signalling NaN, its payload kept
__device__ __forceinline__ float quieted(float f)
{
    return f != f ? __uint_as_float(__float_as_uint(f) | 0x00400000u) : f;
}

// bits 3 - 6 of the byte from one row of the residual table and (or NULL) of the sight table
__device__ __forceinline__ unsigned segment_bits(const Params &p, const double *__restrict__ resid, const double *__restrict__ sight, bool matched)
{
    const double label = resid[0];
    const bool skipped = label == (double)p.skip[0] || label == (double)p.skip[1];
    unsigned fit = 0;
    const double good = resid[kGoodAfter];
    // SegmentResidual.worst: no good row, no mean, not listed; else listed iff the mean EXCEEDS `above`
    if (!skipped && good != 0.0 && resid[kSumAfter] / good > p.above) {
        fit = kFitUndecided;
        if (sight != nullptr) {                     // SegmentSight.annotate
            double far = 0.0;
            for (int k = 0; k < 5; ++k) far += sight[kFarAfter + 2 * k];
            const double seen = sight[kFarAfter + 2 * ICPFLOW_SIGHT_SEEN_THROUGH];
            const double excused = sight[kFarAfter + 2 * ICPFLOW_SIGHT_OUTSIDE] + sight[kFarAfter + 2 * ICPFLOW_SIGHT_NO_RETURN] +
                                   sight[kFarAfter + 2 * ICPFLOW_SIGHT_BEHIND];
            const double bar = p.share * far;
            fit = seen > bar ? kFitSeenThrough : excused > bar ? kFitLostFromView : kFitUndecided;
        }
    }
    return (fit << kFitShift) | (matched ? kMatched : 0u) | (skipped ? kSkipped : 0u);
}

// bits 0 - 2: the class of one row of the source cloud (has_code false: no line-of-sight codes were given)
__device__ __forceinline__ int row_class(bool good, float d2, float far2, bool has_code, int code)
{
    if (!good) return kRowBad;
    if (d2 <= far2) return kRowNear;
    if (!has_code) return kRowNoCode;
    switch (code) {
    case ICPFLOW_SIGHT_SEEN_THROUGH: return 2;
    case ICPFLOW_SIGHT_AT_FIRST_RETURN: return 3;
    case ICPFLOW_SIGHT_BEHIND: return 4;
    case ICPFLOW_SIGHT_NO_RETURN: return 5;
    case ICPFLOW_SIGHT_OUTSIDE: return 6;
    default: return kRowNoCode;                     // (no code of icpflow_sight_query)
    }
}

// the whole byte of a row that has a segment
__device__ __forceinline__ unsigned trust_byte(unsigned segment, int row)
{
    const int fit = (int)(segment >> kFitShift) & kFitMask;
    const bool keep = row != kRowBad && row != 2 && (fit == 0 || fit == kFitLostFromView);
    return (segment & ~(unsigned)kRowMask & 0x7fu) | (unsigned)row | (keep ? kKeep : 0u);
}

}  // namespace trust
}  // namespace icpflow
