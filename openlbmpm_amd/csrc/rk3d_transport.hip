// rk3d_transport.hip -- the kernels of the slab transports (rk3d_transport.h: two one-lane ones, the probe's pair), in one translation unit: both slab models
// (rk3d.hip, rk3d_csf.hip) include the transport, and a kernel defined in the header would be defined twice.
#include "lbmpm_common.h"

namespace slabtx {

__global__ void flag_store(unsigned long long *f, unsigned long long v) { __hip_atomic_store(f, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }
__global__ void flag_wait(unsigned long long *f, unsigned long long v)
{
    while (__hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < v) __builtin_amdgcn_s_sleep(32);
}

void launch_flag_store(hipStream_t st, unsigned long long *f, unsigned long long v) { flag_store<<<1, 1, 0, st>>>(f, v); }
void launch_flag_wait(hipStream_t st, unsigned long long *f, unsigned long long v) { flag_wait<<<1, 1, 0, st>>>(f, v); }

__global__ void tx_fill(double *p, size_t n, double v) { const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; if (i < n) p[i] = v + (double)i; }
__global__ void tx_check(const double *p, size_t n, double v, unsigned long long *bad)
{
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n && p[i] != v + (double)i) atomicAdd(bad, 1ull);
}

void launch_probe_fill(hipStream_t st, double *p, size_t n, double v) { tx_fill<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(p, n, v); }
void launch_probe_check(hipStream_t st, const double *p, size_t n, double v, unsigned long long *bad)
{
    tx_check<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(p, n, v, bad);
}

}  // namespace slabtx
