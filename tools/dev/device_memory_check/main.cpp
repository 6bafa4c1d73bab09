// Host-side check of csrc/device_memory.h (DeviceBlocks, DeviceTemp) under AddressSanitizer and UBSan, without a GPU: hip/hip_runtime.h
// beside this file stands in for the runtime.  From the repository root:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Itools/dev/device_memory_check
//       tools/dev/device_memory_check/main.cpp -o /tmp/device_memory_check && /tmp/device_memory_check
#include "../../../openlbmpm_amd/csrc/lbmpm_common.h"

#include <cstdio>
#include <cstdlib>

namespace lbmpm {
static char last_error[256];
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof(last_error), fmt, ap);
    va_end(ap);
}
}  // namespace lbmpm

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static hipStream_t const STREAM = reinterpret_cast<hipStream_t>(0x10);

// a call that stages two buffers and leaves early, by either macro or at its end
static int staged_call(int leave_at)
{
    lbmpm::DeviceTemp<double> a;
    LBMPM_HIP_TRY(a.alloc(100));
    a.get()[99] = 1.0;
    LBMPM_REQUIRE(leave_at != 1, "left at %d", leave_at);
    lbmpm::DeviceTemp<unsigned> b;
    LBMPM_HIP_TRY(b.alloc(7));                     // (fails when the stand-in is told to)
    b.get()[6] = 1u;
    CHECK(stub_live >= 2);
    LBMPM_HIP_TRY(leave_at == 2 ? hipErrorOutOfMemory : hipSuccess);
    return LBMPM_OK;
}

// the all-or-nothing allocation of a tracer configure: what was handed out before the failure goes back
static int all_or_nothing(lbmpm::DeviceBlocks &mem, double **g, double **h, unsigned **t)
{
    int rc = mem.alloc(g, 50, nullptr);
    if (rc == LBMPM_OK) rc = mem.alloc(h, 50, nullptr);
    if (rc == LBMPM_OK) rc = mem.alloc(t, 10, nullptr);
    if (rc != LBMPM_OK) { mem.release(g); mem.release(h); mem.release(t); }
    return rc;
}

int main()
{
    {
        lbmpm::DeviceBlocks mem;
        CHECK(mem.bytes() == 0);
        double *f = nullptr, *diag = nullptr, *obs = nullptr;
        unsigned char *flags = nullptr;
        unsigned *rows = nullptr;
        CHECK(mem.alloc(&flags, 33, STREAM) == LBMPM_OK && mem.alloc(&f, 18 * 33, STREAM) == LBMPM_OK && mem.alloc(&diag, 3 * 33, STREAM) == LBMPM_OK);
        CHECK(mem.alloc(&rows, 5, nullptr) == LBMPM_OK && mem.alloc(&obs, 22 * 33, STREAM) == LBMPM_OK);
        const int64_t all = 33 + 8 * (18 + 3 + 22) * 33 + 4 * 5;
        CHECK(mem.bytes() == all && stub_live == 5);
        CHECK(flags[32] == 0 && f[18 * 33 - 1] == 0.0 && diag[0] == 0.0);      // zeroed on a stream ...
        CHECK(rows[4] == 0xA5A5A5A5u);                                          // ... and left alone without one
        mem.release(&diag);                                                     // one in the middle
        CHECK(diag == nullptr && mem.bytes() == all - 8 * 3 * 33 && stub_live == 4);
        mem.release(&diag);                                                     // a null pointer: nothing
        CHECK(mem.bytes() == all - 8 * 3 * 33 && stub_live == 4);
        f[0] = obs[22 * 33 - 1] = 2.0; rows[0] = 1u; flags[0] = 1;               // the neighbours are still there
        CHECK(mem.alloc(&diag, 3 * 33, STREAM) == LBMPM_OK && mem.bytes() == all);   // on again
        mem.release(&flags);                                                    // the first
        mem.release(&obs);                                                      // the last but one
        CHECK(mem.bytes() == all - 33 - 8 * 22 * 33 && stub_live == 3);

        stub_fail_after = 0;                                                    // out of memory: nothing counted, nothing kept
        double *more = nullptr;
        CHECK(mem.alloc(&more, 1000, STREAM) == LBMPM_ERR_NOMEM && more == nullptr && mem.bytes() == all - 33 - 8 * 22 * 33 && stub_live == 3);
        stub_fail_after = 2;
        double *g = nullptr, *h = nullptr;
        unsigned *t = nullptr;
        const int64_t before = mem.bytes();
        CHECK(all_or_nothing(mem, &g, &h, &t) == LBMPM_ERR_NOMEM && !g && !h && !t && mem.bytes() == before && stub_live == 3);
        stub_fail_after = -1;
        CHECK(all_or_nothing(mem, &g, &h, &t) == LBMPM_OK && mem.bytes() == before + 840 && stub_live == 6);

        mem.release_all();
        CHECK(mem.bytes() == 0 && stub_live == 0);
        mem.release_all();                                                      // (a destroy after a failed create)
        CHECK(mem.alloc(&more, 4, nullptr) == LBMPM_OK && mem.bytes() == 32);  // the owner is usable again
        mem.release_all();
        CHECK(stub_live == 0);
    }
    CHECK(staged_call(0) == LBMPM_OK && stub_live == 0);
    CHECK(staged_call(1) == LBMPM_ERR_INVALID && stub_live == 0);               // LBMPM_REQUIRE with one buffer alive
    CHECK(staged_call(2) == LBMPM_ERR_HIP && stub_live == 0);                   // LBMPM_HIP_TRY with both alive
    stub_fail_after = 1;
    CHECK(staged_call(0) == LBMPM_ERR_HIP && stub_live == 0);                   // the second allocation fails
    stub_fail_after = -1;
    {
        lbmpm::DeviceTemp<double> never;                                        // never allocated: nothing to free
        CHECK(never.get() == nullptr);
    }
    printf("device_memory_check: ok\n");
    return 0;
}
