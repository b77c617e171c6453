// rejecttest.hpp -- check_transformation (utils_check.py:51-66) of one registered pair from its metrics as icpflow_match_eval
// leaves them, on the device.  ONE copy for the association's stages (assoc.hip) and for the repair's select (repair.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace icpflow {

struct RejectTest {
    float nrm;     // sqrt((t0 t0 + t1 t1) + t2 t2)
    float iou;     // Python's builtin min(iou) on the two-element tensor
    float angle;   // fmaxf(|rot_1|, |rot_2|): the angle that is tested when neither is a NaN
    float err;     // min(error_src, error_dst), NaN if either is
    bool keep;
};

// The fp32 arithmetic of the numpy mirror (utils_check.py of this package): ~(sqrt((t0*t0 + t1*t1) + t2*t2) > tf) &
// ~(min(iou) < thres_iou) & ~(max(|rot_1|, |rot_2|) > thres_rot * 90).  numpy's minimum / maximum PROPAGATE a NaN and every
// comparison with a NaN is false, i.e. a NaN passes the test it sits in; fminf / fmaxf drop a NaN, so the NaN cases are spelled
// out.  errors, ious [.,2], tr, rot [.,3]: the arrays of a batch; k: the pair.
__device__ __forceinline__ RejectTest reject_test(const float *__restrict__ errors, const float *__restrict__ ious, const float *__restrict__ tr,
                                                  const float *__restrict__ rot, int k, float tf, float iouMin, float rotMax)
{
    RejectTest t;
    const float t0 = tr[3 * k], t1 = tr[3 * k + 1], t2 = tr[3 * k + 2];
    t.nrm = sqrtf((t0 * t0 + t1 * t1) + t2 * t2);
    const float i0 = ious[2 * k], i1 = ious[2 * k + 1];
    const float r1 = rot[3 * k + 1], r2 = rot[3 * k + 2];
    const float e0 = errors[2 * k], e1 = errors[2 * k + 1];
    t.err = (e0 != e0 || e1 != e1) ? __int_as_float(0x7fc00000) : fminf(e0, e1);
    const bool farOff = t.nrm > tf;                                                   // (NaN: false)
    // (Python's builtin min(iou) on the two-element tensor, utils_match.py:99: iou[1] if iou[1] < iou[0] else iou[0] -- a NaN in
    // iou[1] leaves iou[0] to be tested, a NaN in iou[0] is the result and passes the comparison)
    t.iou = (i1 < i0) ? i1 : i0;
    const bool lowIou = t.iou < iouMin;
    t.angle = fmaxf(fabsf(r1), fabsf(r2));
    const bool turned = (r1 == r1 && r2 == r2) && t.angle > rotMax;
    t.keep = !farOff && !lowIou && !turned;
    return t;
}

}  // namespace icpflow
