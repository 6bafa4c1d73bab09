// device_memory.h -- who owns the device memory of a solver context (host code only; included from lbmpm_common.h, which brings the HIP
// runtime, set_error and the status codes).
//   DeviceBlocks   the blocks a context keeps beyond a call: counted in bytes() -- what lbmpm_*_device_bytes reports -- and freed by
//                  release() or release_all(), so that a destroy function names no pointer and a block cannot be forgotten there
//   DeviceTemp<T>  a staging buffer for the length of a call: freed on every return path, never counted
//   step_timed()   the body of the four lbmpm_*_step_timed entry points
#pragma once

namespace lbmpm {

class DeviceBlocks {
public:
    DeviceBlocks() = default;
    DeviceBlocks(const DeviceBlocks &) = delete;
    DeviceBlocks &operator=(const DeviceBlocks &) = delete;

    // count elements of T.  zero_on != null: zeroed on that stream -- the context's own: a null-stream memset is not ordered against
    // a non-blocking solver stream and could land after a kernel that already wrote the block.  zero_on == null: left as it comes.
    template <typename T>
    int alloc(T **ptr, size_t count, hipStream_t zero_on)
    {
        void *v = nullptr;
        const size_t size = count * sizeof(T);
        hipError_t e = hipMalloc(&v, size);
        if (e != hipSuccess) { set_error("hipMalloc(%zu bytes) failed: %s", size, hipGetErrorString(e)); return LBMPM_ERR_NOMEM; }
        if (zero_on && (e = hipMemsetAsync(v, 0, size, zero_on)) != hipSuccess) {
            (void)hipFree(v);
            set_error("hipMemsetAsync failed: %s", hipGetErrorString(e));
            return LBMPM_ERR_HIP;
        }
        blocks.push_back({v, size});
        total += (int64_t)size;
        *ptr = static_cast<T *>(v);
        return LBMPM_OK;
    }

    // one block given back and forgotten (a null pointer: nothing); the caller orders the free against the work that uses the block
    template <typename T>
    void release(T **ptr)
    {
        for (size_t k = 0; k < blocks.size() && *ptr; ++k)
            if (blocks[k].ptr == *ptr) {
                (void)hipFree(blocks[k].ptr);
                total -= (int64_t)blocks[k].size;
                blocks.erase(blocks.begin() + (std::ptrdiff_t)k);
                break;
            }
        *ptr = nullptr;
    }

    void release_all()
    {
        for (const Block &b : blocks) (void)hipFree(b.ptr);
        blocks.clear();
        total = 0;
    }

    int64_t bytes() const { return total; }

private:
    struct Block { void *ptr; size_t size; };
    std::vector<Block> blocks;
    int64_t total = 0;
};

template <typename T>
class DeviceTemp {
public:
    DeviceTemp() = default;
    DeviceTemp(const DeviceTemp &) = delete;
    DeviceTemp &operator=(const DeviceTemp &) = delete;
    // (hipFree waits for the device; where a call synchronises its stream before the buffer goes, it still says so itself)
    ~DeviceTemp() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t count) { return hipMalloc(reinterpret_cast<void **>(&p), count * sizeof(T)); }
    T *get() const { return p; }

private:
    T *p = nullptr;
};

// nsteps time steps between two events on `stream`, with one (start, stop) pair of `pool` around launches of the dominant kernel:
// run() enqueues the steps and records the inner pairs it takes from the pool (the first pair is the outer one), divisor() -- asked after
// run() -- says what the inner pairs cover: launches or time steps.  ms_dominant is their sum scaled to all nsteps.
template <typename Run, typename Divisor>
int step_timed(hipStream_t stream, EventPool &pool, int64_t nsteps, double *ms_total, double *ms_dominant, Run run, Divisor divisor)
{
    const size_t pairs = (size_t)(nsteps < 4096 ? nsteps : 4096);
    if (pool.reserve(pairs + 1) != LBMPM_OK) { set_error("hipEventCreate failed"); return LBMPM_ERR_HIP; }
    pool.reset();
    hipEvent_t t0, t1;
    pool.take(&t0, &t1);
    LBMPM_HIP_TRY(hipEventRecord(t0, stream));
    const int rc = run();
    if (rc != LBMPM_OK) return rc;
    LBMPM_HIP_TRY(hipEventRecord(t1, stream));
    LBMPM_HIP_TRY(hipStreamSynchronize(stream));
    float ms = 0.f;
    LBMPM_HIP_TRY(hipEventElapsedTime(&ms, t0, t1));
    if (ms_total) *ms_total = ms;
    if (ms_dominant) {
        double s = 0.0;
        for (size_t k = 2; k + 1 < pool.used; k += 2) {
            float m = 0.f;
            LBMPM_HIP_TRY(hipEventElapsedTime(&m, pool.ev[k], pool.ev[k + 1]));
            s += m;
        }
        const double d = (double)divisor();
        *ms_dominant = d != 0.0 ? s * (double)nsteps / d : 0.0;
    }
    return LBMPM_OK;
}

}  // namespace lbmpm
