// rk3d_transport.h -- the slab exchange's transports inside the library (include/lbmpm.h, "Transport of the slab exchange"):
// IPC landing areas filled by copy-engine transfers and stream value operations, or ncclSend / ncclRecv of a librccl opened at run
// time.  Included by rk3d.hip (the perturbation model's slabs) and rk3d_csf.hip (the CSF model's slabs): host code only.  What both
// models share lives here, once:
//   * the blob, its check and the mapping of the neighbours' landing areas (ipc_alloc / ipc_open / ipc_share / unmap), under the
//     identity -- API prefix of the error messages and blob magic -- the owning context gives its Transport once;
//   * the communicator of the RCCL transport, for the chain or the ring of slabs (rccl_connect);
//   * the per-step exchange (exchange) and the heartbeat its steps write (beat_ready / beat);
//   * the probe of a connected transport (probe_begin / probe_round / probe_result);
//   * the watchdog (release_waits / ipc_release_waits / sync_deadline) and the clean-up (disconnect / destroy).
// The model files keep their argument checks, their message sizes and loops, and what a failure voids of their own state.  The
// kernels -- two one-lane ones (the fallback of devices without stream value operations, and the heartbeat) and the probe's pair --
// live in rk3d_transport.hip, ONE translation unit, and are launched through the functions below.
#include <dlfcn.h>
#include <unistd.h>
#include <time.h>
#include <stdio.h>

namespace slabtx {

using lbmpm::set_error;

// flag_store<<<1, 1, 0, st>>>(f, v) / flag_wait<<<1, 1, 0, st>>>(f, v) (rk3d_transport.hip); the caller checks hipGetLastError
void launch_flag_store(hipStream_t st, unsigned long long *f, unsigned long long v);
void launch_flag_wait(hipStream_t st, unsigned long long *f, unsigned long long v);
// the probe's pattern p[i] = v + i written / compared (mismatches counted in *bad), n doubles; n > 0
void launch_probe_fill(hipStream_t st, double *p, size_t n, double v);
void launch_probe_check(hipStream_t st, const double *p, size_t n, double v, unsigned long long *bad);

// what a rank tells its neighbours (LBMPM_IPC_BLOB_BYTES)
struct IpcBlob {
    uint32_t magic, version;
    int32_t pid, device;
    uint64_t slot_bytes;                  // bytes between the four slots of the landing area: [from below | from above][parity]
    uint64_t bytes_from_below, bytes_from_above;      // message sizes this rank expects (0: no neighbour there)
    uint64_t land_ptr, flags_ptr;         // addresses in the owner's process (used by slabs of the same process)
    hipIpcMemHandle_t land, flags;
    uint64_t nonce;                       // drawn once per process: "same pid" alone does not mean "same process" (ranks in separate
                                          // containers or pid namespaces of one node commonly share a pid, e.g. 1)
};
static_assert(sizeof(IpcBlob) <= LBMPM_IPC_BLOB_BYTES, "blob size is part of the ABI");
constexpr uint32_t BLOB_MAGIC = 0x4c424d50u;     // "LBMP": the perturbation model's blobs
constexpr uint32_t BLOB_MAGIC_CSF = 0x4c424d43u; // "LBMC": the CSF model's (a CsfBlob around the IpcBlob)
constexpr uint32_t BLOB_VERSION = 2;

// one random 64-bit value per process (from /dev/urandom; pid, clock and an address as the fallback)
inline uint64_t process_nonce()
{
    static uint64_t n = 0;
    if (n) return n;
    uint64_t v = 0;
    if (FILE *f = fopen("/dev/urandom", "rb")) { if (fread(&v, sizeof v, 1, f) != 1) v = 0; fclose(f); }
    if (!v) {
        struct timespec ts;
        clock_gettime(CLOCK_REALTIME, &ts);
        v = ((uint64_t)getpid() << 32) ^ (uint64_t)ts.tv_nsec ^ ((uint64_t)ts.tv_sec << 20) ^ reinterpret_cast<uint64_t>(&n);
    }
    n = v | 1ull;
    return n;
}

// the part of librccl this file calls (types as in rccl.h: opaque communicator, 128-byte id, int enums)
struct Rccl {
    void *dl = nullptr;
    typedef struct { char internal[LBMPM_RCCL_ID_BYTES]; } UniqueId;
    int (*GetUniqueId)(UniqueId *) = nullptr;
    int (*CommInitRank)(void **, int, UniqueId, int) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*CommAbort)(void *) = nullptr;          // optional (present in every RCCL since 2.4): tears a communicator down without its peers
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*Recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    static constexpr int kFloat64 = 8;        // ncclFloat64 / ncclDouble
    int open(const char *path)
    {
        const char *names[] = {path, "librccl.so.1", "librccl.so"};
        for (const char *n : names) {
            if (!n || !*n) continue;
            dl = dlopen(n, RTLD_NOW | RTLD_LOCAL);
            if (dl) break;
        }
        if (!dl) { set_error("RCCL transport: cannot open librccl (%s)", dlerror()); return LBMPM_ERR_UNSUPPORTED; }
        bool ok = true;
        auto sym = [&](const char *n) { void *s = dlsym(dl, n); if (!s) ok = false; return s; };
        GetUniqueId = reinterpret_cast<decltype(GetUniqueId)>(sym("ncclGetUniqueId"));
        CommInitRank = reinterpret_cast<decltype(CommInitRank)>(sym("ncclCommInitRank"));
        CommDestroy = reinterpret_cast<decltype(CommDestroy)>(sym("ncclCommDestroy"));
        GroupStart = reinterpret_cast<decltype(GroupStart)>(sym("ncclGroupStart"));
        GroupEnd = reinterpret_cast<decltype(GroupEnd)>(sym("ncclGroupEnd"));
        Send = reinterpret_cast<decltype(Send)>(sym("ncclSend"));
        Recv = reinterpret_cast<decltype(Recv)>(sym("ncclRecv"));
        GetErrorString = reinterpret_cast<decltype(GetErrorString)>(sym("ncclGetErrorString"));
        CommAbort = reinterpret_cast<decltype(CommAbort)>(dlsym(dl, "ncclCommAbort"));
        if (!ok) { set_error("RCCL transport: librccl lacks ncclSend / ncclRecv / ncclCommInitRank"); close(); return LBMPM_ERR_UNSUPPORTED; }
        return LBMPM_OK;
    }
    void close() { if (dl) dlclose(dl); dl = nullptr; }
};

struct Transport {
    // ---- identity, given once where the owner is made: Transport tx{"lbmpm_rk3d", BLOB_MAGIC}
    const char *api = nullptr;                // the owner's API prefix: every error message names the caller's own functions
    uint32_t magic = 0;                       // of the owner's blobs
    int kind = LBMPM_TRANSPORT_NONE;
    int device = 0;
    bool has_below = false, has_above = false;
    size_t bytes_up = 0, bytes_dn = 0;        // message to the rank above (this rank's top plane) / below (its bottom plane)
    size_t bytes_from_below = 0, bytes_from_above = 0;     // messages from there (their face planes = this rank's halo planes)
    unsigned long long seq = 0;               // messages exchanged so far (all ranks count alike)
    // ---- IPC
    char *land = nullptr;                     // own landing area, 4 slots
    size_t slot = 0;
    bool land_fine = false;                   // the landing area is fine-grained memory
    unsigned long long *flags = nullptr;      // own, fine-grained: [face 0 from below | 1 from above][parity]
    char *peer_land[2] = {nullptr, nullptr};  // [0] landing area of the rank below (we fill its "from above" slots), [1] of the rank above
    unsigned long long *peer_flags[2] = {nullptr, nullptr};
    size_t peer_slot[2] = {0, 0};             // the neighbours' slot sizes (their halo planes differ from ours)
    bool mapped[2] = {false, false};          // peer_* came from hipIpcOpenMemHandle (to be closed)
    bool value_ops = false;
    bool connected = false;
    bool dead = false;                        // the steady-state watchdog gave up on a neighbour (sync_deadline)
    // ---- watchdog and probe (kept over disconnect, freed by destroy)
    hipStream_t wd_stream = nullptr;          // the watchdog's own copies
    unsigned long long *beat_host = nullptr, *beat_dev = nullptr;     // heartbeat: a pinned host word the slab steps write their number into
    unsigned long long *probe_bad = nullptr;  // mismatch counter of the probe
    // ---- RCCL
    Rccl rccl;
    void *comm = nullptr;
    int rank = 0, nranks = 1;
    int peer_up = -1, peer_dn = -1;           // RCCL ranks of the neighbours (rank + 1, rank - 1; the self-test talks to itself)
    bool ring = false;                        // the CSF model's ring of slabs: with two ranks both neighbours are ONE peer, whose messages
                                              // pair with ours in the order posted -- send low, send high, receive high, receive low

    char *slot_ptr(char *base, int face, unsigned par) const { return base + ((size_t)face * 2 + par) * slot; }
    char *peer_slot_ptr(int side, int face, unsigned par) const { return peer_land[side] + ((size_t)face * 2 + par) * peer_slot[side]; }

    int set_shape(int dev, bool below, bool above, size_t up, size_t dn, size_t from_below, size_t from_above)
    {
        if (kind != LBMPM_TRANSPORT_NONE) { set_error("a transport is connected already: %s_transport_disconnect first", api); return LBMPM_ERR_STATE; }
        device = dev; has_below = below; has_above = above; bytes_up = up; bytes_dn = dn; bytes_from_below = from_below; bytes_from_above = from_above;
        const size_t m = from_below > from_above ? from_below : from_above;
        slot = (m + 4095) / 4096 * 4096;
        LBMPM_HIP_TRY(hipSetDevice(dev));
        if (land) { (void)hipFree(land); land = nullptr; }          // (a connect that failed half way and is tried again)
        // The landing area is FINE-GRAINED memory where the device offers it: with the IPC transport a neighbour GPU's copy engine writes it
        // over xGMI, past this GPU's L2, and ordinary (coarse-grained) memory is coherent at kernel boundaries only -- a slot is reused
        // every second step, and a line of it left in L2 by the previous unpack would be served stale.  (The probe at set-up would catch
        // that and the selection would fall back to RCCL; this keeps the copy-engine path.  LBMPM_IPC_LAND=coarse: ordinary memory.)
#ifdef LBMPM_DEV
        const char *lk = getenv("LBMPM_IPC_LAND");
#else
        const char *lk = nullptr;
#endif
        land_fine = !(lk && !strcmp(lk, "coarse")) &&
                    hipExtMallocWithFlags(reinterpret_cast<void **>(&land), 4 * slot, hipDeviceMallocFinegrained) == hipSuccess;
        if (!land_fine) {
            (void)hipGetLastError();
            LBMPM_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&land), 4 * slot));
        }
        return LBMPM_OK;
    }

    int ipc_alloc(IpcBlob *blob)
    {
        const int dev = device;
        const bool below = has_below, above = has_above;
        if (hipExtMallocWithFlags(reinterpret_cast<void **>(&flags), 4096, hipDeviceMallocFinegrained) != hipSuccess) {
            (void)hipGetLastError();
            LBMPM_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&flags), 4096));
        }
        LBMPM_HIP_TRY(hipMemset(flags, 0, 4096));
        LBMPM_HIP_TRY(hipDeviceSynchronize());
        int can = 0;
        (void)hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, dev);
        value_ops = can != 0 && !getenv("LBMPM_IPC_FLAG_KERNELS");      // (the variable forces the one-lane kernels: test coverage of the fallback)
        memset(blob, 0, sizeof *blob);
        blob->magic = magic; blob->version = BLOB_VERSION; blob->pid = (int32_t)getpid(); blob->device = dev;
        blob->nonce = process_nonce();
        blob->slot_bytes = slot; blob->bytes_from_below = below ? bytes_from_below : 0; blob->bytes_from_above = above ? bytes_from_above : 0;
        blob->land_ptr = reinterpret_cast<uint64_t>(land); blob->flags_ptr = reinterpret_cast<uint64_t>(flags);
        LBMPM_HIP_TRY(hipIpcGetMemHandle(&blob->land, land));
        LBMPM_HIP_TRY(hipIpcGetMemHandle(&blob->flags, flags));
        kind = LBMPM_TRANSPORT_IPC; seq = 0; connected = false;
        return LBMPM_OK;
    }

    int ipc_open(int side, const IpcBlob *b, size_t my_bytes)
    {
        if (b->magic != magic || b->version != BLOB_VERSION) { set_error("%s_ipc_connect: not a blob of %s_ipc_init", api, api); return LBMPM_ERR_INVALID; }
        const uint64_t theirs = side == 0 ? b->bytes_from_above : b->bytes_from_below;     // the rank below receives "from above"
        if (theirs != my_bytes) {
            set_error("%s_ipc_connect: the rank %s expects %llu bytes per message, this rank sends %llu (different cuts or lattices)", api,
                      side == 0 ? "below" : "above", (unsigned long long)theirs, (unsigned long long)my_bytes);
            return LBMPM_ERR_INVALID;
        }
        if (b->slot_bytes < my_bytes) { set_error("%s_ipc_connect: the neighbour's slots are smaller than the message", api); return LBMPM_ERR_INVALID; }
        peer_slot[side] = (size_t)b->slot_bytes;
        if (b->pid == (int32_t)getpid() && b->nonce == process_nonce()) {      // a slab of this very process: plain pointers (peer access if it lives on another GPU)
            if (b->device != device) {
                const hipError_t e = hipDeviceEnablePeerAccess(b->device, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { set_error("hipDeviceEnablePeerAccess(%d): %s", b->device, hipGetErrorString(e)); return LBMPM_ERR_HIP; }
                (void)hipGetLastError();
            }
            peer_land[side] = reinterpret_cast<char *>(b->land_ptr);
            peer_flags[side] = reinterpret_cast<unsigned long long *>(b->flags_ptr);
            mapped[side] = false;
            return LBMPM_OK;
        }
        void *pl = nullptr, *pf = nullptr;
        hipError_t e = hipIpcOpenMemHandle(&pl, b->land, hipIpcMemLazyEnablePeerAccess);
        if (e == hipSuccess) e = hipIpcOpenMemHandle(&pf, b->flags, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) {
            if (pl) (void)hipIpcCloseMemHandle(pl);
            set_error("hipIpcOpenMemHandle (rank %s, pid %d, device %d): %s", side == 0 ? "below" : "above", b->pid, b->device, hipGetErrorString(e));
            (void)hipGetLastError();
            return LBMPM_ERR_HIP;
        }
        peer_land[side] = static_cast<char *>(pl); peer_flags[side] = static_cast<unsigned long long *>(pf); mapped[side] = true;
        return LBMPM_OK;
    }

    // both neighbours are one rank (a ring of two): side `to` uses the mapping of side `from` (a handle is opened once, closed once)
    void ipc_share(int to, int from)
    {
        peer_land[to] = peer_land[from]; peer_flags[to] = peer_flags[from]; peer_slot[to] = peer_slot[from]; mapped[to] = false;
    }

    // closes what ipc_open mapped (a connect that failed half way can be tried again; disconnect)
    void unmap()
    {
        for (int s = 0; s < 2; ++s) {
            if (mapped[s]) { (void)hipIpcCloseMemHandle(peer_land[s]); (void)hipIpcCloseMemHandle(peer_flags[s]); }
            peer_land[s] = nullptr; peer_flags[s] = nullptr; mapped[s] = false;
        }
    }

    // librccl opened, ncclCommInitRank (a blocking collective over the nranks ranks), the neighbours' ranks: rank -+ 1 in the chain of
    // slabs, modulo nranks in the ring.  After set_shape; a failure leaves the clean-up (disconnect) to the caller.
    int rccl_connect(const void *id, int rank_, int nranks_, const char *librccl_path, bool ring_)
    {
        const int rc = rccl.open(librccl_path);
        if (rc != LBMPM_OK) return rc;
        Rccl::UniqueId uid;
        memcpy(&uid, id, sizeof uid);
        if (hipSetDevice(device) != hipSuccess) { set_error("hipSetDevice(%d) failed", device); return LBMPM_ERR_HIP; }
        const int e = rccl.CommInitRank(&comm, nranks_, uid, rank_);
        if (e != 0) { set_error("ncclCommInitRank(rank %d of %d): %s", rank_, nranks_, rccl.GetErrorString(e)); return LBMPM_ERR_HIP; }
        rank = rank_; nranks = nranks_; ring = ring_;
        peer_up = ring ? (rank + 1) % nranks : rank + 1; peer_dn = ring ? (rank + nranks - 1) % nranks : rank - 1;
        kind = LBMPM_TRANSPORT_RCCL; connected = true; seq = 0;
        return LBMPM_OK;
    }

    // what lbmpm_*_transport_kind answers
    int kind_for_caller(int *value_ops_out) const
    {
        if (value_ops_out) *value_ops_out = kind == LBMPM_TRANSPORT_IPC && value_ops ? 1 : 0;
        return connected ? kind : LBMPM_TRANSPORT_NONE;
    }

    // One message each way, enqueued on `st`: send_up -> the rank above, send_dn -> the rank below; *from_below / *from_above = where
    // this rank's incoming messages will have landed when the stream gets past the waits enqueued here.
    int exchange(hipStream_t st, const double *send_up, const double *send_dn, const double **from_below, const double **from_above)
    {
        return exchange(st, send_up, send_dn, bytes_up, bytes_dn, bytes_from_below, bytes_from_above, from_below, from_above);
    }

    // The same for one of several message kinds of different sizes (the CSF model: phi, n, populations after the three stages of a step;
    // every size within the slots set_shape made).  The sequence number counts messages, whatever their kind: the two-parity argument
    // holds as long as every exchange's waits are enqueued before the stream goes on to produce the next message.
    int exchange(hipStream_t st, const double *send_up, const double *send_dn, size_t up, size_t dn, size_t in_below, size_t in_above,
                 const double **from_below, const double **from_above)
    {
        if (!connected) { set_error("the slab's transport is not connected"); return LBMPM_ERR_STATE; }
        if (dead) { set_error("the slab's transport was given up by the watchdog (a neighbour did not answer): disconnect and set up the run again"); return LBMPM_ERR_TIMEOUT; }
        seq += 1;
        const unsigned par = (unsigned)(seq & 1ull);
        if (kind == LBMPM_TRANSPORT_IPC) {
            *from_below = reinterpret_cast<const double *>(slot_ptr(land, 0, par));
            *from_above = reinterpret_cast<const double *>(slot_ptr(land, 1, par));
            if (has_above) LBMPM_HIP_TRY(hipMemcpyAsync(peer_slot_ptr(1, 0, par), send_up, up, hipMemcpyDeviceToDevice, st));
            if (has_below) LBMPM_HIP_TRY(hipMemcpyAsync(peer_slot_ptr(0, 1, par), send_dn, dn, hipMemcpyDeviceToDevice, st));
            auto post = [&](unsigned long long *f) -> hipError_t {
                if (value_ops) return hipStreamWriteValue64(st, f, seq, 0);
                launch_flag_store(st, f, seq);
                return hipGetLastError();
            };
            auto await = [&](unsigned long long *f) -> hipError_t {
                if (value_ops) return hipStreamWaitValue64(st, f, seq, hipStreamWaitValueGte, ~0ull);
                launch_flag_wait(st, f, seq);
                return hipGetLastError();
            };
            if (has_above) LBMPM_HIP_TRY(post(peer_flags[1] + 0 * 2 + par));
            if (has_below) LBMPM_HIP_TRY(post(peer_flags[0] + 1 * 2 + par));
            if (has_below) LBMPM_HIP_TRY(await(flags + 0 * 2 + par));
            if (has_above) LBMPM_HIP_TRY(await(flags + 1 * 2 + par));
            return LBMPM_OK;
        }
        if (kind == LBMPM_TRANSPORT_RCCL) {
            *from_below = reinterpret_cast<const double *>(slot_ptr(land, 0, 0));
            *from_above = reinterpret_cast<const double *>(slot_ptr(land, 1, 0));
            int rc = rccl.GroupStart();
            if (ring) {
                if (rc == 0 && has_below) rc = rccl.Send(send_dn, dn / 8, Rccl::kFloat64, peer_dn, comm, st);
                if (rc == 0 && has_above) rc = rccl.Send(send_up, up / 8, Rccl::kFloat64, peer_up, comm, st);
                if (rc == 0 && has_above) rc = rccl.Recv(slot_ptr(land, 1, 0), in_above / 8, Rccl::kFloat64, peer_up, comm, st);
                if (rc == 0 && has_below) rc = rccl.Recv(slot_ptr(land, 0, 0), in_below / 8, Rccl::kFloat64, peer_dn, comm, st);
            } else {
                if (rc == 0 && has_above) rc = rccl.Send(send_up, up / 8, Rccl::kFloat64, peer_up, comm, st);
                if (rc == 0 && has_above) rc = rccl.Recv(slot_ptr(land, 1, 0), in_above / 8, Rccl::kFloat64, peer_up, comm, st);
                if (rc == 0 && has_below) rc = rccl.Send(send_dn, dn / 8, Rccl::kFloat64, peer_dn, comm, st);
                if (rc == 0 && has_below) rc = rccl.Recv(slot_ptr(land, 0, 0), in_below / 8, Rccl::kFloat64, peer_dn, comm, st);
            }
            const int rc2 = rccl.GroupEnd();
            if (rc == 0) rc = rc2;
            if (rc != 0) { set_error("RCCL transport: %s", rccl.GetErrorString ? rccl.GetErrorString(rc) : "ncclSend / ncclRecv failed"); return LBMPM_ERR_HIP; }
            return LBMPM_OK;
        }
        set_error("no transport");
        return LBMPM_ERR_STATE;
    }

    // ---- the heartbeat: every slab step's exchange chain ends by writing its step number into a pinned host word (sync_deadline reads it)
    hipError_t beat_ready()
    {
        if (beat_dev) return hipSuccess;
        if (!beat_host) {
            const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&beat_host), 64, hipHostMallocMapped);
            if (e != hipSuccess) { beat_host = nullptr; return e; }
            *beat_host = 0ull;
        }
        return hipHostGetDevicePointer(reinterpret_cast<void **>(&beat_dev), beat_host, 0);
    }
    void beat(hipStream_t st, unsigned long long v) { launch_flag_store(st, beat_dev, v); }      // after beat_ready; the caller checks hipGetLastError

    // ---- Probe of the CONNECTED transport between the real neighbours, enqueued on `st` (the caller polls the stream under a deadline,
    // then reads the verdict): probe_begin, then rounds of one patterned message each way -- written into the (still unused) send
    // buffers, exchanged, and compared on the receiving side by a kernel launched behind the transport's waits.
    int probe_begin(hipStream_t st)
    {
        if (!probe_bad) LBMPM_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&probe_bad), sizeof(unsigned long long)));
        LBMPM_HIP_TRY(hipMemsetAsync(probe_bad, 0, sizeof(unsigned long long), st));
        return LBMPM_OK;
    }
    // nu / nd doubles go up / down as value + i / -value + i, nb / na doubles arrive from below / above (0: no message that way)
    int probe_round(hipStream_t st, double *send_up, double *send_dn, size_t nu, size_t nd, size_t nb, size_t na, double value)
    {
        if (nu) launch_probe_fill(st, send_up, nu, value);
        if (nd) launch_probe_fill(st, send_dn, nd, -value);
        const double *fb = nullptr, *fa = nullptr;
        const int rc = exchange(st, send_up, send_dn, 8 * nu, 8 * nd, 8 * nb, 8 * na, &fb, &fa);
        if (rc != LBMPM_OK) return rc;
        if (nb) launch_probe_check(st, fb, nb, value, probe_bad);        // what the rank below sent up
        if (na) launch_probe_check(st, fa, na, -value, probe_bad);       // what the rank above sent down
        LBMPM_HIP_TRY(hipGetLastError());
        return LBMPM_OK;
    }
    // verdict of the last probe: doubles that arrived different from what the neighbour sent (synchronises `st`)
    int probe_result(hipStream_t st, int64_t *mismatches)
    {
        if (!mismatches || !probe_bad) { set_error("%s_transport_probe_result: no probe was run", api); return LBMPM_ERR_INVALID; }
        unsigned long long v = 0;
        LBMPM_HIP_TRY(hipMemcpyAsync(&v, probe_bad, sizeof v, hipMemcpyDeviceToHost, st));
        LBMPM_HIP_TRY(hipStreamSynchronize(st));
        *mismatches = (int64_t)v;
        return LBMPM_OK;
    }

    // ---- The steady-state watchdog (include/lbmpm.h): host-side polling, so that a stream stuck in hipStreamWaitValue64 / flag_wait / an
    // ncclRecv on a neighbour that died does not hang this process for good.
    // every IPC wait of this slab returns: the flags say "arrived" for every message to come
    int release_waits()
    {
        // from a private non-blocking stream: a copy on the legacy null stream would queue behind the very wait it is to release when the
        // context runs on a blocking stream, and one on a stream that sits in the wait would never run
        static const unsigned long long big[4] = {~0ull, ~0ull, ~0ull, ~0ull};
        if (!wd_stream) LBMPM_HIP_TRY(hipStreamCreateWithFlags(&wd_stream, hipStreamNonBlocking));
        LBMPM_HIP_TRY(hipMemcpyAsync(flags, big, sizeof big, hipMemcpyHostToDevice, wd_stream));
        LBMPM_HIP_TRY(hipStreamSynchronize(wd_stream));
        return LBMPM_OK;
    }
    int ipc_release_waits()         // lbmpm_*_ipc_release_waits
    {
        if (kind != LBMPM_TRANSPORT_IPC || !flags) { set_error("%s_ipc_release_waits: no IPC transport", api); return LBMPM_ERR_INVALID; }
        return release_waits();
    }

    // Waits until the n (1 or 2) streams are idle -> LBMPM_OK, or until no heartbeat came for `seconds` -> LBMPM_ERR_TIMEOUT.  The
    // deadline counts from the last PROGRESS, not from the call: while the heartbeat word moves, the neighbours answer and the queued
    // steps drain, however many there are and however slow a neighbour is (an absolute deadline voided healthy long queues).  On a
    // time-out the connected transport is given up -- IPC: the waits released, RCCL: the communicator aborted; dead, the streams
    // synchronised -- and *gave_up names its kind; LBMPM_TRANSPORT_NONE: nothing was released, the work is still running and the
    // caller's state stays what it is.  Else the caller voids its state.  `where`: the slab's planes, the tail of the message.
    int sync_deadline(const hipStream_t *streams, int n, double seconds, const char *where, int *gave_up)
    {
        struct timespec t0, t;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        volatile unsigned long long *hb = beat_host;
        unsigned long long last = hb ? *hb : 0ull;
        for (unsigned spins = 0;;) {
            hipError_t e = hipSuccess;
            for (int i = 0; i < n && e == hipSuccess; ++i) e = hipStreamQuery(streams[i]);
            if (e == hipSuccess) return LBMPM_OK;
            if (e != hipErrorNotReady) { set_error("%s_sync_deadline: %s", api, hipGetErrorString(e)); return LBMPM_ERR_HIP; }
            (void)hipGetLastError();
            clock_gettime(CLOCK_MONOTONIC, &t);
            if (hb && *hb != last) { last = *hb; t0 = t; }
            if ((double)(t.tv_sec - t0.tv_sec) + 1e-9 * (double)(t.tv_nsec - t0.tv_nsec) > seconds) break;
            if (++spins > 2000) { struct timespec nap = {0, 200000}; nanosleep(&nap, nullptr); }       // busy for the first moments, then 0.2 ms naps
        }
        *gave_up = connected ? kind : LBMPM_TRANSPORT_NONE;
        if (*gave_up == LBMPM_TRANSPORT_IPC) {
            const int rc = release_waits();
            if (rc != LBMPM_OK) return rc;
        } else if (*gave_up == LBMPM_TRANSPORT_RCCL && comm && rccl.CommAbort) { (void)rccl.CommAbort(comm); comm = nullptr; }
        if (*gave_up != LBMPM_TRANSPORT_NONE) {
            dead = true;
            for (int i = 0; i < n; ++i) (void)hipStreamSynchronize(streams[i]);
        }
        set_error("%s_sync_deadline: the slab's streams were busy and no step's face messages came through for %.1f s -- %s (%s)", api, seconds,
                  *gave_up == LBMPM_TRANSPORT_IPC ? "a neighbour's face message did not arrive; the waits were released, the lattice state is void" :
                  *gave_up == LBMPM_TRANSPORT_RCCL ? "a neighbour did not answer; the communicator was aborted, the lattice state is void" :
                                                     "no in-library transport is connected: nothing was released", where);
        return LBMPM_ERR_TIMEOUT;
    }

    void disconnect()
    {
        unmap();
        if (comm) {         // dead: a peer is known not to answer (the watchdog fired) -- ncclCommDestroy would wait for it
            if (dead && rccl.CommAbort) (void)rccl.CommAbort(comm); else if (!dead) (void)rccl.CommDestroy(comm);
            comm = nullptr;
        }
        rccl.close();
        if (land) (void)hipFree(land);
        if (flags) (void)hipFree(flags);
        land = nullptr; flags = nullptr;
        kind = LBMPM_TRANSPORT_NONE; connected = false; seq = 0; dead = false; ring = false;
        (void)hipGetLastError();
    }

    // the end of the owning context: the transport and what outlives a disconnect
    void destroy()
    {
        disconnect();
        if (probe_bad) (void)hipFree(probe_bad);
        if (beat_host) (void)hipHostFree(beat_host);
        if (wd_stream) (void)hipStreamDestroy(wd_stream);
        probe_bad = nullptr; beat_host = beat_dev = nullptr; wd_stream = nullptr;
    }
};

}  // namespace slabtx
