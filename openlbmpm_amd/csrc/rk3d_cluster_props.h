// Per-cluster properties of the 3-D solvers (lbmpm_rk3d_cluster_props* / lbmpm_rk3dcsf_cluster_props*; the definition is in
// include/lbmpm.h): beside the cluster table of the last lbmpm_*_clusters call one row of int64 per cluster -- the faces towards the other
// phase and towards the solid, the pairs, squares and cubes of morphology credited to the cluster of their anchor, the sum of the plane
// numbers, and mass and momentum as fixed-point sums.  Included by rk3d.hip and rk3d_csf.hip inside their unnamed namespaces, after
// rk3d_clusters.h and rk3d_morphology.h, and templated over the flow's loader of rk3d_integrals.h (IntCell) as rk3d_morphology.h is.
// It reads what the clusters left on the device: the class bytes (0 / 1 / 2), the flattened global labels, the sorted label rows.
// Three launches (the face: one), whatever the state:
//   1 classify     one byte per own cell into [planes + 2][ny][nx] bytes: LBMPM_MORPH_R / _B exactly where the clusters' class is 1 / 2,
//                  _S where the flow's loader says solid, _N for every other fluid cell.  Plane 0 is the caller's `below`, plane
//                  planes + 1 the caller's `above`, or MORPH_NOTHING throughout: no face, pair, square or cube reaches into it.
//   2 zero         [CP_ACC][count] int64 (hipMemsetAsync)
//   3 accumulate   one workgroup per chunk of CP_CHUNK consecutive cells, CP_THREADS at a time.  A lane brings its cell's eleven
//                  contributions from the eleven class bytes around it (own, x -+ 1, y -+ 1, (x + 1, y + 1), the cell below, four above;
//                  from cache) and, through the flow's loader, rho and rho u in fixed point.  The wave joins the runs of equal labels (a
//                  ballot of "a run begins here", a segmented __shfl_down sum); a run's first lane adds the run to a label-keyed table of
//                  CP_SLOTS rows in LDS (64-bit LDS integer atomics) or, when its CP_PROBES slots are taken by other labels, to global
//                  memory.  At the end the workgroup finds the row of every slot by bisection of the sorted labels and issues one 64-bit
//                  global integer atomicAdd per non-zero (slot, column): a cluster that fills the lattice costs a workgroup at most eleven
//                  global atomics, not one chain per run.
// Every sum is an integer sum: the same bits under every order, launch and cut.  No kernel waits for another workgroup.  Every loop is
// finite by construction: the probes and the shuffle steps are counted, the bisection halves an interval (at most 32 turns).
// Memory: (planes + 2) * ny * nx bytes with the first call of either function; 88 bytes per cluster of the largest count seen with the
// first lbmpm_*_cluster_props call that meets it (a checkerboard has as many clusters as cells).
#pragma once

constexpr unsigned CP_CHUNK = 1024;              // cells per workgroup
constexpr unsigned CP_THREADS = 256;
constexpr unsigned CP_SLOTS = 32;                // labels a workgroup combines in LDS
constexpr unsigned CP_PROBES = 4;
constexpr int CP_ACC = 11;                       // the accumulated columns: all but LABEL, CLASS and CELLS, in the table's order
constexpr int CP_FIRST = LBMPM_CP_FACES_FLUID;   // column of accumulator 0
static_assert(LBMPM_CLUSTER_PROP_COLS == 14 && LBMPM_CP_LABEL == 0 && LBMPM_CP_CLASS == 1 && LBMPM_CP_CELLS == 2 && LBMPM_CP_FACES_FLUID == 3 &&
              LBMPM_CP_FACES_SOLID == 4 && LBMPM_CP_PAIRS == 5 && LBMPM_CP_SQUARES == 6 && LBMPM_CP_CUBES == 7 && LBMPM_CP_SUM_Z == 8 &&
              LBMPM_CP_MASS == 9 && LBMPM_CP_MOM_X == 10 && LBMPM_CP_MOM_Y == 11 && LBMPM_CP_MOM_Z == 12 && LBMPM_CP_CLIPPED == 13,
              "the columns of rk3d_cluster_props.h");
static_assert(CP_CHUNK % CP_THREADS == 0 && CP_THREADS % 64 == 0 && (CP_SLOTS & (CP_SLOTS - 1u)) == 0 && CP_SLOTS <= CP_THREADS, "whole waves; a slot per thread");
static_assert(LBMPM_MORPH_R == 1 && LBMPM_MORPH_B == 2, "the clusters' classes 1 and 2 are the morphology's R and B");

// the cells [first, first + n) of the own planes; pcls: the first own plane of the class array
template <typename Flow>
__global__ __launch_bounds__(CP_THREADS) void cluster_props_classify(const Flow flow, unsigned first, unsigned n, unsigned plane_cells, const uint8_t *cls, uint8_t *pcls)
{
    const unsigned t = blockIdx.x * CP_THREADS + threadIdx.x;
    if (t >= n) return;
    const unsigned i = first + t;
    unsigned c = cls[i];
    if (!c) {
        const unsigned plane = i / plane_cells;
        IntCell f;
        c = flow(0u, plane, i - plane * plane_cells, f) ? LBMPM_MORPH_N : LBMPM_MORPH_S;
    }
    pcls[i] = (uint8_t)c;
}

// the row whose label is key (the labels ascend), CL_NONE when there is none
__device__ __forceinline__ unsigned cp_row(const unsigned *rows, unsigned count, unsigned key)
{
    unsigned lo = 0, hi = count;
    for (int turn = 0; turn < 32 && lo + 1u < hi; ++turn) {
        const unsigned mid = lo + (hi - lo) / 2u;
        if (rows[mid] <= key) lo = mid; else hi = mid;
    }
    return lo < count && rows[lo] == key ? lo : CL_NONE;
}

__device__ __forceinline__ void cp_add(unsigned long long *p, unsigned long long v)
{
    if (v) atomicAdd(p, v);
}

// the six small counts of a cell share a word, ten bits each: a wave's run holds at most 6 * 64 of any
constexpr unsigned CP_PACK_BITS = 10;
static_assert(6u * 64u < (1u << CP_PACK_BITS), "the faces of a wave's cells fit a field");

// the run (packed small counts, then five sums) into eleven accumulators that lie `stride` apart
__device__ __forceinline__ void cp_add_run(unsigned long long *a, size_t stride, unsigned long long packed, const unsigned long long (&v)[5])
{
    constexpr int SLOT[6] = {LBMPM_CP_FACES_FLUID - CP_FIRST, LBMPM_CP_FACES_SOLID - CP_FIRST, LBMPM_CP_PAIRS - CP_FIRST,
                             LBMPM_CP_SQUARES - CP_FIRST, LBMPM_CP_CUBES - CP_FIRST, LBMPM_CP_CLIPPED - CP_FIRST};
#pragma unroll
    for (int k = 0; k < 6; ++k) cp_add(a + SLOT[k] * stride, (packed >> (CP_PACK_BITS * k)) & ((1ull << CP_PACK_BITS) - 1ull));
#pragma unroll
    for (int k = 0; k < 5; ++k) cp_add(a + (LBMPM_CP_SUM_Z - CP_FIRST + k) * stride, v[k]);
}

// pcls: [planes + 2][ny][nx]; lab: the global labels; rows: the sorted labels; acc: [CP_ACC][count]
template <typename Flow>
__global__ __launch_bounds__(CP_THREADS) void cluster_props_accumulate(const Flow flow, ClGeom g, const uint8_t *cls, const uint8_t *pcls, const unsigned *lab,
                                                                       const unsigned *rows, unsigned count, unsigned long long *acc)
{
    __shared__ unsigned keys[CP_SLOTS], slot_row[CP_SLOTS];
    __shared__ unsigned long long sums[CP_SLOTS][CP_ACC];
    for (unsigned t = threadIdx.x; t < CP_SLOTS * CP_ACC; t += CP_THREADS) sums[t / CP_ACC][t % CP_ACC] = 0ull;
    if (threadIdx.x < CP_SLOTS) keys[threadIdx.x] = CL_NONE;
    __syncthreads();
    const unsigned lane = threadIdx.x & 63u;
    const unsigned begin = blockIdx.x * CP_CHUNK;
    for (unsigned part = 0; part < CP_CHUNK; part += CP_THREADS) {
        const unsigned i = begin + part + threadIdx.x;             // (as in rk3d_clusters.h: a lattice that fits a device ends far below 2^32 - CP_CHUNK)
        const unsigned c = i < g.n ? cls[i] : 0u;
        const unsigned l = c ? lab[i] : CL_NONE;
        unsigned long long packed = 0ull, v[5] = {0ull, 0ull, 0ull, 0ull, 0ull};      // SUM_Z, MASS, MOM_X, MOM_Y, MOM_Z
        if (c) {
            const unsigned plane = i / g.plane_cells, k = i - plane * g.plane_cells, y = k / g.nx, x = k - y * g.nx;
            const unsigned xp = x + 1u < g.nx ? x + 1u : 0u, xm = x ? x - 1u : g.nx - 1u;
            const unsigned yp = y + 1u < g.ny ? y + 1u : 0u, ym = y ? y - 1u : g.ny - 1u;
            const uint8_t *own = pcls + (size_t)(plane + 1u) * g.plane_cells, *dn = own - g.plane_cells, *up = own + g.plane_cells;
            const unsigned other = 3u - c;
            const unsigned nxp = own[y * g.nx + xp], nxm = own[y * g.nx + xm], nyp = own[yp * g.nx + x], nym = own[ym * g.nx + x];
            const unsigned nxy = own[yp * g.nx + xp], ndn = dn[k];
            const unsigned u00 = up[k], u10 = up[y * g.nx + xp], u01 = up[yp * g.nx + x], u11 = up[yp * g.nx + xp];
            const unsigned ff = (nxp == other) + (nxm == other) + (nyp == other) + (nym == other) + (ndn == other) + (u00 == other);
            const unsigned fs = (nxp == LBMPM_MORPH_S) + (nxm == LBMPM_MORPH_S) + (nyp == LBMPM_MORPH_S) + (nym == LBMPM_MORPH_S) +
                                (ndn == LBMPM_MORPH_S) + (u00 == LBMPM_MORPH_S);
            const bool px = nxp == c, py = nyp == c, pz = u00 == c;
            const bool sxy = px && py && nxy == c, sxz = px && pz && u10 == c, syz = py && pz && u01 == c;
            const bool cube = sxy && sxz && syz && u11 == c;
            const unsigned pairs = (unsigned)px + (unsigned)py + (unsigned)pz, squares = (unsigned)sxy + (unsigned)sxz + (unsigned)syz;
            v[0] = (unsigned long long)(g.z0 + plane);
            IntCell f;
            bool good = flow(0u, plane, k, f) && integral_finite(f.rR) && integral_finite(f.rB) && integral_finite(f.ux) && integral_finite(f.uy) &&
                        integral_finite(f.uz);
            if (good) {
                const double rho = f.rR + f.rB;
                const double mx = rho * f.ux, my = rho * f.uy, mz = rho * f.uz;
                good = fabs(rho) < 64. && fabs(mx) < 1. && fabs(my) < 1. && fabs(mz) < 1.;
                if (good) {
                    v[1] = (unsigned long long)__double2ll_rn(rho * (double)(1ll << LBMPM_CP_MASS_BITS));
                    v[2] = (unsigned long long)__double2ll_rn(mx * (double)(1ll << LBMPM_CP_MOM_BITS));
                    v[3] = (unsigned long long)__double2ll_rn(my * (double)(1ll << LBMPM_CP_MOM_BITS));
                    v[4] = (unsigned long long)__double2ll_rn(mz * (double)(1ll << LBMPM_CP_MOM_BITS));
                }
            }
            packed = (unsigned long long)ff | (unsigned long long)fs << CP_PACK_BITS | (unsigned long long)pairs << (2 * CP_PACK_BITS) |
                     (unsigned long long)squares << (3 * CP_PACK_BITS) | (unsigned long long)cube << (4 * CP_PACK_BITS) |
                     (unsigned long long)!good << (5 * CP_PACK_BITS);
        }
        // the runs of equal labels of the wave (idle lanes: runs of CL_NONE that carry nothing)
        const unsigned prev = __shfl_up(l, 1, 64);
        const bool head = lane == 0 || prev != l;
        const unsigned long long heads = __ballot(head);
        const unsigned long long above = lane == 63u ? 0ull : heads >> (lane + 1u);
        const unsigned end = above ? lane + (unsigned)__ffsll((long long)above) : 64u;       // the lane after the run's last
#pragma unroll
        for (unsigned off = 1; off < 64u; off <<= 1) {
            const bool in = lane + off < end;
            const unsigned long long tp = __shfl_down(packed, off, 64);
            if (in) packed += tp;
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const unsigned long long tv = __shfl_down(v[q], off, 64);
                if (in) v[q] += tv;
            }
        }
        if (head && c) {
            const unsigned h = (l * 2654435761u) >> 16;
            int slot = -1;
            for (unsigned t = 0; t < CP_PROBES && slot < 0; ++t) {
                const unsigned s = (h + t) & (CP_SLOTS - 1u);
                const unsigned old = atomicCAS(&keys[s], CL_NONE, l);
                if (old == CL_NONE || old == l) slot = (int)s;
            }
            if (slot >= 0) cp_add_run(&sums[slot][0], 1, packed, v);
            else {
                const unsigned r = cp_row(rows, count, l);
                if (r != CL_NONE) cp_add_run(acc + r, count, packed, v);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < CP_SLOTS) slot_row[threadIdx.x] = keys[threadIdx.x] != CL_NONE ? cp_row(rows, count, keys[threadIdx.x]) : CL_NONE;
    __syncthreads();
    for (unsigned t = threadIdx.x; t < CP_SLOTS * CP_ACC; t += CP_THREADS) {
        const unsigned s = t % CP_SLOTS, a = t / CP_SLOTS;         // consecutive lanes: consecutive slots of one column
        if (slot_row[s] != CL_NONE) cp_add(acc + (size_t)a * count + slot_row[s], sums[s][a]);
    }
}

// ---- host side
struct CpState {
    uint8_t *cls = nullptr;                  // [planes + 2][ny][nx]
    unsigned long long *acc = nullptr;       // [CP_ACC][cap]
    size_t cap = 0;
};

inline int cluster_props_classes(lbmpm::DeviceBlocks &mem, CpState &p, const ClGeom &g, hipStream_t zero_on)
{
    return p.cls ? LBMPM_OK : mem.alloc(&p.cls, ((size_t)g.planes + 2u) * g.plane_cells, zero_on);
}

template <typename Flow>
void cluster_props_classify_range(const Flow &flow, const ClState &s, CpState &p, unsigned first, unsigned n, hipStream_t stream)
{
    cluster_props_classify<Flow><<<dim3((n + CP_THREADS - 1u) / CP_THREADS), dim3(CP_THREADS), 0, stream>>>(flow, first, n, s.g.plane_cells, s.cls,
                                                                                                          p.cls + s.g.plane_cells);
}

// The body of the lbmpm_*_cluster_props_face entry points (`who`) behind their null checks: the classes of the lowest and the highest
// own plane, host [2][ny][nx].  One synchronisation, 2 * ny * nx bytes.
template <typename Flow>
int cluster_props_face(const char *who, const Flow &flow, const ClState &s, CpState &p, int64_t steps, int device, lbmpm::DeviceBlocks &mem, hipStream_t zero_on,
                       hipStream_t stream, uint8_t *host_out)
{
    { const int rc = clusters_current(who, s, steps, device); if (rc) return rc; }
    { const int rc = cluster_props_classes(mem, p, s.g, zero_on); if (rc) return rc; }
    const unsigned pc = s.g.plane_cells, top = (s.g.planes - 1u) * pc;
    cluster_props_classify_range(flow, s, p, 0u, pc, stream);
    if (top) cluster_props_classify_range(flow, s, p, top, pc, stream);
    LBMPM_HIP_TRY(hipGetLastError());
    LBMPM_HIP_TRY(hipMemcpyAsync(host_out, p.cls + pc, pc, hipMemcpyDeviceToHost, stream));
    LBMPM_HIP_TRY(hipMemcpyAsync(host_out + pc, p.cls + pc + top, pc, hipMemcpyDeviceToHost, stream));
    LBMPM_HIP_TRY(hipStreamSynchronize(stream));
    return LBMPM_OK;
}

// The body of the lbmpm_*_cluster_props entry points (`who`) behind their null checks.  below, above: host [ny][nx] or null; host_out:
// [count][LBMPM_CLUSTER_PROP_COLS].  One synchronisation, count * (12 + 88) bytes.
template <typename Flow>
int cluster_props_run(const char *who, const Flow &flow, const ClState &s, CpState &p, int64_t steps, int device, lbmpm::DeviceBlocks &mem, hipStream_t zero_on,
                      hipStream_t stream, const uint8_t *below, const uint8_t *above, int64_t *host_out)
{
    { const int rc = clusters_current(who, s, steps, device); if (rc) return rc; }
    const ClGeom &g = s.g;
    const unsigned pc = g.plane_cells;
    const uint8_t *given[2] = {below, above};
    for (int side = 0; side < 2; ++side)
        for (unsigned k = 0; given[side] && k < pc; ++k)
            if (given[side][k] > 3) {
                set_error("%s: %s[%u] = %u (a class is 0 .. 3)", who, side ? "above" : "below", k, (unsigned)given[side][k]);
                return LBMPM_ERR_INVALID;
            }
    const size_t m = (size_t)s.count;
    if (!m) return LBMPM_OK;
    { const int rc = cluster_props_classes(mem, p, g, zero_on); if (rc) return rc; }
    if (m > p.cap) {                         // grows only; the last call that used the block has synchronised
        mem.release(&p.acc);
        p.cap = 0;
        { const int rc = mem.alloc(&p.acc, (size_t)CP_ACC * m, zero_on); if (rc) return rc; }
        p.cap = m;
    }
    uint8_t *ends[2] = {p.cls, p.cls + (size_t)(g.planes + 1u) * pc};
    for (int side = 0; side < 2; ++side) {
        if (given[side]) LBMPM_HIP_TRY(hipMemcpyAsync(ends[side], given[side], pc, hipMemcpyHostToDevice, stream));
        else LBMPM_HIP_TRY(hipMemsetAsync(ends[side], (int)MORPH_NOTHING, pc, stream));
    }
    cluster_props_classify_range(flow, s, p, 0u, g.n, stream);
    LBMPM_HIP_TRY(hipGetLastError());
    LBMPM_HIP_TRY(hipMemsetAsync(p.acc, 0, (size_t)CP_ACC * m * sizeof(unsigned long long), stream));
    cluster_props_accumulate<Flow><<<dim3((g.n + CP_CHUNK - 1u) / CP_CHUNK), dim3(CP_THREADS), 0, stream>>>(flow, g, s.cls, p.cls, s.lab, s.rows, (unsigned)m, p.acc);
    LBMPM_HIP_TRY(hipGetLastError());
    std::vector<unsigned> h(3 * m);
    std::vector<long long> a((size_t)CP_ACC * m);
    for (int col = 0; col < 3; ++col)
        LBMPM_HIP_TRY(hipMemcpyAsync(h.data() + col * m, s.rows + (size_t)col * g.n, m * sizeof(unsigned), hipMemcpyDeviceToHost, stream));
    LBMPM_HIP_TRY(hipMemcpyAsync(a.data(), p.acc, a.size() * sizeof(long long), hipMemcpyDeviceToHost, stream));
    LBMPM_HIP_TRY(hipStreamSynchronize(stream));
    for (size_t r = 0; r < m; ++r) {
        int64_t *row = host_out + r * LBMPM_CLUSTER_PROP_COLS;
        row[LBMPM_CP_LABEL] = h[r];
        row[LBMPM_CP_CLASS] = h[2 * m + r] >> 30;
        row[LBMPM_CP_CELLS] = h[m + r];
        for (int k = 0; k < CP_ACC; ++k) row[CP_FIRST + k] = (int64_t)a[(size_t)k * m + r];
    }
    return LBMPM_OK;
}
