// host.hpp -- the host side that every file with entry points shares: how an error reaches icpflow_last_error, the
// try-macro around HIP calls, the workspace carver.  Host code only: no kernel, no __device__ function, no launch helper.
#pragma once
#include "carver.hpp"

#include <algorithm>
#include <cmath>

#include <hip/hip_runtime.h>

#include "../../include/icpflow_hip.h"

namespace icpflow {

// api.hip, beside the thread's message buffer: sets what icpflow_last_error returns, -> code
int report_error(int code, const char *message);
// ... from a printf format
int report_errorf(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// "<what>: <HIP's text>", -> the HIP error as the status
inline int hip_error(hipError_t e, const char *what) { return report_errorf((int)e, "%s: %s", what, hipGetErrorString(e)); }

inline int pointer_error(const char *fn) { return report_errorf(ICPFLOW_E_ARG, "%s: null pointer", fn); }

// the workspace is missing or smaller than `query` (the name of the size function) says
inline int workspace_error(const char *fn, const char *query, const void *ws, size_t have, size_t need)
{
    return report_errorf(ICPFLOW_E_WORKSPACE, "%s: workspace of %zu bytes, %s says %zu", fn, ws ? have : (size_t)0, query, need);
}

// n interior edges of a list of buckets (HOST memory): finite and strictly ascending
inline bool edges_ok(const double *h, int n)
{
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(h[k]) || (k > 0 && !(h[k] > h[k - 1]))) return false;
    return true;
}

// (frame.hip's staging and read-backs, clusterpcd.hip's download and upload: one per host thread each, thread_local)
struct Pinned {   // a pinned host buffer that grows (read in place by the kernels / target of the read-backs)
    void *ptr = nullptr;
    size_t bytes = 0;
    int device = -1;
    Pinned() = default;
    Pinned(const Pinned &) = delete;
    Pinned &operator=(const Pinned &) = delete;
    ~Pinned() { if (ptr != nullptr) (void)hipHostFree(ptr); }   // (thread_local: freed when the host thread ends)
    char *need(size_t want)
    {
        int dev = -1;
        (void)hipGetDevice(&dev);
        if (ptr == nullptr || bytes < want || device != dev) {
            if (ptr != nullptr) (void)hipHostFree(ptr);
            ptr = nullptr;
            bytes = std::max(want, (size_t)1 << 20);
            if (hipHostMalloc(&ptr, bytes, hipHostMallocDefault) != hipSuccess) { ptr = nullptr; bytes = 0; }
            device = dev;
        }
        return static_cast<char *>(ptr);
    }
};

}  // namespace icpflow

// a HIP call that fails ends the entry point with hip_error, the expression as its text
#define ICPFLOW_TRY(expr)                                             \
    do {                                                              \
        const hipError_t e__ = (expr);                                \
        if (e__ != hipSuccess) return icpflow::hip_error(e__, #expr); \
    } while (0)
