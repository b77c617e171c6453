// labelkey.hpp -- the order of float labels that table.hip's dictionary sorts by and trust.hip searches by: one definition, so
// that a segment found by its key is the segment the cluster table made.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace icpflow {

constexpr uint32_t kEmpty = 0xffffffffu;

// float -> uint32 whose unsigned order is the float order.  As bit patterns -0.0 < +0.0, where torch.argsort and
// torch.unique -- and every `==` on labels downstream -- see one label: label_key below maps -0.0 to +0.0 first, so
// the two are ONE cluster, reported as 0.0, its rows in original order.
__device__ __forceinline__ uint32_t sortable(float f)
{
    const uint32_t u = (uint32_t)__float_as_int(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ uint32_t label_key(float f)
{
    // both zeros are one label (a select, not sort_pack's f + 0.0f: an add would quiet a signalling NaN, and NaN labels are
    // kept apart by their bits)
    const uint32_t k = sortable(f == 0.0f ? 0.0f : f);
    return k == kEmpty ? kEmpty - 1u : k;    // (one NaN payload shares the empty mark's pattern)
}

}  // namespace icpflow
