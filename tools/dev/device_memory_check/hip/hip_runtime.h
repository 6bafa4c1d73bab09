// A host-only stand-in for the HIP runtime, for tools/dev/device_memory_check/main.cpp alone: device memory is host memory, so that
// AddressSanitizer sees every block that is freed twice, freed by the wrong owner or never freed.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>

typedef int hipError_t;
constexpr hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2;
typedef struct stub_stream *hipStream_t;
typedef struct stub_event *hipEvent_t;

inline int stub_live = 0;           // blocks handed out and not yet freed
inline int stub_fail_after = -1;    // >= 0: that many hipMalloc calls succeed, the next ones fail

inline hipError_t hipMalloc(void **p, size_t size)
{
    if (stub_fail_after == 0) { *p = nullptr; return hipErrorOutOfMemory; }
    if (stub_fail_after > 0) --stub_fail_after;
    *p = malloc(size ? size : 1);
    memset(*p, 0xA5, size);
    ++stub_live;
    return hipSuccess;
}
inline hipError_t hipFree(void *p) { if (p) --stub_live; free(p); return hipSuccess; }
inline hipError_t hipMemsetAsync(void *p, int v, size_t size, hipStream_t) { memset(p, v, size); return hipSuccess; }
inline const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "out of memory"; }
inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
inline hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 1.f; return hipSuccess; }
