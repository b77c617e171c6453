// device.hip -- host utilities every launcher may use: per-device caches (CU count, a kernel's opt-in to more dynamic LDS
// than the default) and the HIP-event recorder behind icpflow_profile_t.
#include <atomic>
#include <vector>

#include "kernels.hpp"

namespace icpflow {

int device_cus()
{
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 1;
    int c = cache[dev].load(std::memory_order_relaxed);
    if (c == 0) {
        if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 1;
        cache[dev].store(c, std::memory_order_relaxed);
    }
    return c;
}

void ensure_dynamic_lds(const void *func, int bytes, std::atomic<unsigned long long> *mask)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return;
    const unsigned long long bit = 1ull << (dev & 63);
    if (dev < 64 && (mask->load(std::memory_order_acquire) & bit)) return;
    // never more than the CU's 160 KiB less the kernel's static LDS (the request fails as a whole otherwise)
    hipFuncAttributes fa{};
    if (hipFuncGetAttributes(&fa, func) == hipSuccess) bytes = min(bytes, 160 * 1024 - (int)fa.sharedSizeBytes);
    (void)hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (dev < 64) mask->fetch_or(bit, std::memory_order_release);
}

// ---- optional per-launch timing of this (dominant) kernel with HIP events ---------------------
// bench.py needs the average launch duration of the dominant kernel measured on the stream it
// runs on; the events are recorded by the library because only it sees the individual launches.
// The recorder is an object the caller owns (icpflow_profile_t) and passes with the call's options.
struct LaunchProfile {
    std::vector<hipEvent_t> start, stop;
    int used = 0;
};

// -> true: the recorder has a slot left and the launch's start is recorded on `s`; profile_stop then closes the slot
bool profile_start(LaunchProfile *p, hipStream_t s)
{
    const bool timed = p != nullptr && p->used < (int)p->start.size();
    if (timed) (void)hipEventRecord(p->start[p->used], s);
    return timed;
}

void profile_stop(LaunchProfile *p, hipStream_t s)
{
    (void)hipEventRecord(p->stop[p->used++], s);
}

LaunchProfile *profile_create(int capacity, hipError_t *err)
{
    LaunchProfile *p = new LaunchProfile;
    *err = hipSuccess;
    for (int i = 0; i < capacity; ++i) {
        hipEvent_t a, b;
        hipError_t e = hipEventCreate(&a);
        if (e == hipSuccess) {
            e = hipEventCreate(&b);
            if (e != hipSuccess) (void)hipEventDestroy(a);
        }
        if (e != hipSuccess) { *err = e; profile_destroy(p); return nullptr; }
        p->start.push_back(a); p->stop.push_back(b);
    }
    return p;
}

void profile_destroy(LaunchProfile *p)
{
    if (p == nullptr) return;
    for (hipEvent_t e : p->start) (void)hipEventDestroy(e);
    for (hipEvent_t e : p->stop) (void)hipEventDestroy(e);
    delete p;
}

hipError_t profile_collect(LaunchProfile *p, double *total_ms, int *launches)
{
    double sum = 0.0;
    for (int i = 0; i < p->used; ++i) {
        hipError_t e = hipEventSynchronize(p->stop[i]);
        if (e != hipSuccess) return e;
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, p->start[i], p->stop[i]);
        if (e != hipSuccess) return e;
        sum += ms;
    }
    if (total_ms) *total_ms = sum;
    if (launches) *launches = p->used;
    p->used = 0;
    return hipSuccess;
}

}  // namespace icpflow
