// Test infrastructure: the HIP runtime calls of rpt_amd/csrc/rpt_capi.cpp backed by malloc / memcpy, so that the
// host half of the library (scene store, flattening, tree builds, box shell, instancing, error paths) runs on a CPU,
// under sanitizers and at different optimisation levels.  Kernel launches are no-ops.  Never part of the product.
// Events are 1-byte allocations, so that LeakSanitizer sees one that is never destroyed; hipMalloc fails above
// g_stub_malloc_limit bytes, as a device out of memory would.
// A harness that wants to know what the host code does with streams, events and device memory (sequence_harness.cpp) sets
// g_stub_observer: every stub then reports the call before it acts.  Null (the default): nothing is reported.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <hip/hip_runtime_api.h>
inline size_t g_stub_malloc_limit = SIZE_MAX;
struct StubObserver {
    virtual void allocated(void* p, size_t n) = 0;
    virtual void freed(void* p) = 0;                                                        // hipFree: synchronises the device first
    virtual void copied(const char* what, void* dst, const void* src, size_t n, hipStream_t st, bool blocking) = 0;   // src null: a memset
    virtual void stream_synchronized(hipStream_t st) = 0;
    virtual void device_synchronized() = 0;
    virtual void event_recorded(hipEvent_t e, hipStream_t st) = 0;
    virtual void event_waited(hipStream_t st, hipEvent_t e) = 0;
    virtual void event_synchronized(hipEvent_t e) = 0;
    virtual void event_destroyed(hipEvent_t e) = 0;
    virtual ~StubObserver() = default;
};
inline StubObserver* g_stub_observer = nullptr;
extern "C" {
hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_tR0600* p, int) {
    std::memset(p, 0, sizeof(*p));
    std::strcpy(p->gcnArchName, "gfx950");
    p->multiProcessorCount = 256;
    return hipSuccess;
}
hipError_t hipMalloc(void** p, size_t n) {
    if (n > g_stub_malloc_limit) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = std::calloc(n ? n : 1, 1);
    if (g_stub_observer) g_stub_observer->allocated(*p, n ? n : 1);
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    if (g_stub_observer && p) g_stub_observer->freed(p);
    std::free(p);
    return hipSuccess;
}
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) {
    if (g_stub_observer) g_stub_observer->copied("hipMemcpy", d, s, n, nullptr, true);
    std::memcpy(d, s, n);
    return hipSuccess;
}
hipError_t hipMemset(void* d, int v, size_t n) {
    if (g_stub_observer) g_stub_observer->copied("hipMemset", d, nullptr, n, nullptr, true);
    std::memset(d, v, n);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t st) {
    if (g_stub_observer) g_stub_observer->copied("hipMemsetAsync", d, nullptr, n, st, false);
    std::memset(d, v, n);
    return hipSuccess;
}
hipError_t hipMemsetD32Async(hipDeviceptr_t d, int v, size_t n, hipStream_t st) {
    if (g_stub_observer) g_stub_observer->copied("hipMemsetD32Async", d, nullptr, 4 * n, st, false);
    for (size_t i = 0; i < n; i++) std::memcpy(static_cast<char*>(d) + 4 * i, &v, 4);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t st) {
    if (g_stub_observer) g_stub_observer->stream_synchronized(st);
    return hipSuccess;
}
hipError_t hipDeviceSynchronize() {
    if (g_stub_observer) g_stub_observer->device_synchronized();
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) { *e = static_cast<hipEvent_t>(std::malloc(1)); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipEventCreate(e); }
hipError_t hipStreamWaitEvent(hipStream_t st, hipEvent_t e, unsigned) {
    if (g_stub_observer) g_stub_observer->event_waited(st, e);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
    if (g_stub_observer) g_stub_observer->event_destroyed(e);
    std::free(e);
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t st) {
    if (g_stub_observer) g_stub_observer->event_recorded(e, st);
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) {
    if (g_stub_observer) g_stub_observer->event_synchronized(e);
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float* f, hipEvent_t, hipEvent_t) { *f = 0; return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
}
