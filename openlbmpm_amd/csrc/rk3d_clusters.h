// Phase clusters of the 3-D solvers (lbmpm_rk3d_clusters* / lbmpm_rk3dcsf_clusters*; the definition is in include/lbmpm.h): the connected
// components of the cells of each phase, labelled on the device by label-equivalence union-find.  Included by rk3d.hip and rk3d_csf.hip
// inside their unnamed namespaces, after rk3d_integrals.h.  Templated over a
//   Loader   bool operator()(unsigned plane, unsigned k, double &phi) const -- the cell k = y * nx + x of the context's own plane `plane`
//            (0: its first own plane); false for a solid cell.
// Everything works on the slab's own cell numbers i = (plane * ny + y) * nx + x; the label a caller sees is i + base, the global cell
// number (base = first own plane * nx * ny), added once at the end.  A label array L is a forest: L[i] <= i for every cell of a class,
// L[i] == i at a root, and a cluster's root is its smallest cell.  Seven launches, whatever the state:
//   1 classify   one byte per cell from the loader's phi; nothing reads phi afterwards
//   2 tiles      a workgroup labels a tile of CL_TX x CL_TY x CL_TZ cells in LDS: one wave per row, the runs along x from a ballot of
//                "a run begins here", the unions between the rows and planes of the tile in LDS; the tile's roots go out as cell numbers
//   3 merge      the links that leave a tile (its faces, the x and y wrap): unions on the global array, atomicMin on roots
//   4 flatten    every cell's label becomes its root; the roots of every chunk of CL_CHUNK cells are counted
//   5 scan       the chunk counts become offsets (one workgroup)
//   6 rows       the roots in cell order = label order: one table row each {label, cells = 0, class << 30 | zmax = 0}
//   7 sizes      a wave joins its runs of equal labels; a run's first lane finds the row by bisection of the sorted labels and adds the
//                run's length (integer atomicAdd) and its last plane (atomicMax).  ZMIN needs no column: it is the plane of the label.
// No kernel waits for another workgroup.  Every loop is finite by construction: cl_find walks strictly decreasing cell numbers, cl_union
// goes round again only with a strictly smaller cell, the bisection halves an interval.  A wrong forest gives a wrong table, not a hang.
// Memory per own cell: 1 (class) + 4 (label) + 12 (rows: a checkerboard has as many clusters as cells) = 17 bytes, + 4 per chunk.
#pragma once

constexpr unsigned CL_NONE = 0xFFFFFFFFu;
constexpr unsigned CL_TX = 64, CL_TY = 4, CL_TZ = 4;          // a tile: CL_TY waves, each a row of 64 cells, marching over CL_TZ planes
constexpr unsigned CL_TILE = CL_TX * CL_TY * CL_TZ;
constexpr unsigned CL_TILE_THREADS = CL_TX * CL_TY;
constexpr unsigned CL_CHUNK = 1024;                           // cells per workgroup of the stages 4 and 6
constexpr unsigned CL_THREADS = 256;
static_assert(CL_TX == 64 && CL_CHUNK % 64 == 0 && CL_CHUNK <= 1024, "one wave per row; a chunk is one workgroup");

struct ClGeom {
    unsigned nx, ny, planes, plane_cells;
    unsigned n;                  // planes * plane_cells
    unsigned z0, base;           // the first own plane in the undivided lattice; z0 * plane_cells
    int nlink;                   // 3: faces, 9: the D3Q19 links (one of every opposite pair; see CL_DX)
};

// one of every pair of opposite links, the one that points to the smaller cell number; the first three are the faces
#define CL_DX {-1, 0, 0, -1, 1, -1, 1, 0, 0}
#define CL_DY {0, -1, 0, -1, -1, 0, 0, -1, 1}
#define CL_DZ {0, 0, -1, 0, 0, -1, -1, -1, -1}

__device__ __forceinline__ unsigned cl_load(const unsigned *L, unsigned i) { return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above cell i; every turn takes a strictly smaller cell, so at most i turns (a value that is not smaller ends the walk)
__device__ __forceinline__ unsigned cl_find(const unsigned *L, unsigned i)
{
    for (;;) {
        const unsigned p = cl_load(L, i);
        if (p >= i) return i;
        i = p;
    }
}

// join the trees of a and b: the larger root is hung under the smaller one.  When the atomicMin finds that a was no root any more (old <
// a: somebody hung it first), whatever it has written is a smaller cell of the same cluster-to-be, and the turn is taken again from old:
// the larger of the two cells shrinks with every turn.
__device__ __forceinline__ void cl_union(unsigned *L, unsigned a, unsigned b)
{
    for (;;) {
        a = cl_find(L, a);
        b = cl_find(L, b);
        if (a == b) return;
        if (a < b) { const unsigned t = a; a = b; b = t; }
        const unsigned old = atomicMin(L + a, b);
        if (old >= a) return;
        a = old;
    }
}

template <typename Loader>
__global__ __launch_bounds__(CL_THREADS) void clusters_classify(const Loader load, ClGeom g, double cut, uint8_t *cls)
{
    const unsigned i = blockIdx.x * CL_THREADS + threadIdx.x;
    if (i >= g.n) return;
    const unsigned plane = i / g.plane_cells, k = i - plane * g.plane_cells;
    double phi = 0.;
    uint8_t c = 0;
    if (load(plane, k, phi) && integral_finite(phi)) c = phi > cut ? 1 : (phi <= -cut ? 2 : 0);
    cls[i] = c;
}

// grid (x segments, tiles along y, tiles along z), CL_TILE_THREADS threads; cells outside the lattice have class 0
__global__ __launch_bounds__(CL_TILE_THREADS) void clusters_tiles(ClGeom g, const uint8_t *cls, unsigned *lab)
{
    constexpr int DX[9] = CL_DX, DY[9] = CL_DY, DZ[9] = CL_DZ;
    __shared__ unsigned L[CL_TILE];
    __shared__ uint8_t C[CL_TILE];
    const unsigned x0 = blockIdx.x * CL_TX, y0 = blockIdx.y * CL_TY, z0 = blockIdx.z * CL_TZ;
    const unsigned row = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const unsigned x = x0 + lane, y = y0 + row;
    const bool inxy = x < g.nx && y < g.ny;
    for (unsigned dz = 0; dz < CL_TZ; ++dz) {
        const unsigned z = z0 + dz, l = (dz * CL_TY + row) * CL_TX + lane;
        unsigned c = 0;
        if (inxy && z < g.planes) c = cls[(size_t)z * g.plane_cells + y * g.nx + x];
        const unsigned left = __shfl_up(c, 1, 64);
        const bool begins = c && (lane == 0 || left != c);
        const unsigned long long starts = __ballot(begins);
        unsigned init = l;
        if (c) init = l - lane + (63u - (unsigned)__clzll((long long)(starts & (~0ull >> (63u - lane)))));      // the run's first cell
        C[l] = (uint8_t)c;
        L[l] = init;
    }
    __syncthreads();
    for (unsigned dz = 0; dz < CL_TZ; ++dz) {
        const unsigned l = (dz * CL_TY + row) * CL_TX + lane;
        const unsigned c = C[l];
        if (!c) continue;
        for (int d = 1; d < g.nlink; ++d) {
            const int xx = (int)lane + DX[d], yy = (int)row + DY[d], zz = (int)dz + DZ[d];
            if (xx < 0 || xx >= (int)CL_TX || yy < 0 || yy >= (int)CL_TY || zz < 0) continue;
            const unsigned m = ((unsigned)zz * CL_TY + (unsigned)yy) * CL_TX + (unsigned)xx;
            if (C[m] != c) continue;
            if (DX[d] == 0 && lane > 0 && C[l - 1] == c && C[m - 1] == c) continue;      // both cells go on a run to the left: that lane joins the two runs
            cl_union(L, l, m);
        }
    }
    __syncthreads();
    for (unsigned dz = 0; dz < CL_TZ; ++dz) {
        const unsigned z = z0 + dz, l = (dz * CL_TY + row) * CL_TX + lane;
        if (!(inxy && z < g.planes)) continue;
        unsigned out = CL_NONE;
        if (C[l]) {
            const unsigned r = cl_find(L, l);
            out = (z0 + r / (CL_TX * CL_TY)) * g.plane_cells + (y0 + (r / CL_TX) % CL_TY) * g.nx + x0 + r % CL_TX;
        }
        lab[(size_t)z * g.plane_cells + y * g.nx + x] = out;
    }
}

// one thread per cell: the links to smaller cells that the tile did not see -- they leave the tile, or wrap around x or y
__global__ __launch_bounds__(CL_THREADS) void clusters_merge(ClGeom g, const uint8_t *cls, unsigned *lab)
{
    constexpr int DX[9] = CL_DX, DY[9] = CL_DY, DZ[9] = CL_DZ;
    const unsigned i = blockIdx.x * CL_THREADS + threadIdx.x;
    if (i >= g.n) return;
    const unsigned c = cls[i];
    if (!c) return;
    const unsigned z = i / g.plane_cells, k = i - z * g.plane_cells, y = k / g.nx, x = k - y * g.nx;
    for (int d = 0; d < g.nlink; ++d) {
        if (DZ[d] < 0 && z == 0) continue;           // z does not wrap
        const unsigned zz = z - (DZ[d] < 0 ? 1u : 0u);
        int xx = (int)x + DX[d], yy = (int)y + DY[d];
        bool wrapped = false;
        if (xx < 0) { xx += (int)g.nx; wrapped = true; } else if (xx >= (int)g.nx) { xx -= (int)g.nx; wrapped = true; }
        if (yy < 0) { yy += (int)g.ny; wrapped = true; } else if (yy >= (int)g.ny) { yy -= (int)g.ny; wrapped = true; }
        if (!wrapped && (unsigned)xx / CL_TX == x / CL_TX && (unsigned)yy / CL_TY == y / CL_TY && zz / CL_TZ == z / CL_TZ) continue;
        const unsigned j = zz * g.plane_cells + (unsigned)yy * g.nx + (unsigned)xx;
        if (cls[j] == c) cl_union(lab, i, j);
    }
}

// one workgroup of CL_CHUNK threads per chunk: labels become roots; chunk_roots[chunk] = roots among the chunk's cells (a root is a
// root since the merge ended, whatever this launch has flattened so far)
__global__ __launch_bounds__(CL_CHUNK) void clusters_flatten(ClGeom g, const uint8_t *cls, unsigned *lab, unsigned *chunk_roots)
{
    __shared__ unsigned total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const unsigned i = blockIdx.x * CL_CHUNK + threadIdx.x;
    bool root = false;
    if (i < g.n && cls[i]) {
        const unsigned r = cl_find(lab, i);
        root = r == i;
        if (!root) __hip_atomic_store(lab + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const unsigned long long b = __ballot(root);
    if ((threadIdx.x & 63u) == 0 && b) atomicAdd(&total, (unsigned)__popcll(b));
    __syncthreads();
    if (threadIdx.x == 0) chunk_roots[blockIdx.x] = total;
}

// one workgroup of 1024 threads: counts[0 .. nchunk) become the sums of the chunks before, counts[nchunk] the number of clusters
__global__ __launch_bounds__(1024) void clusters_scan(unsigned *counts, unsigned nchunk)
{
    __shared__ unsigned s[1024];
    const unsigned t = threadIdx.x, per = (nchunk + 1023u) / 1024u;
    const unsigned lo = t * per < nchunk ? t * per : nchunk, hi = lo + per < nchunk ? lo + per : nchunk;
    unsigned sum = 0;
    for (unsigned k = lo; k < hi; ++k) sum += counts[k];
    s[t] = sum;
    __syncthreads();
    for (unsigned off = 1; off < 1024u; off <<= 1) {
        const unsigned v = t >= off ? s[t - off] : 0u;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    unsigned run = s[t] - sum;
    for (unsigned k = lo; k < hi; ++k) { const unsigned v = counts[k]; counts[k] = run; run += v; }
    if (t == 1023u) counts[nchunk] = s[t];
}

// rows: [3][n] -- labels (ascending), cells, class << 30 | zmax
__global__ __launch_bounds__(CL_CHUNK) void clusters_rows(ClGeom g, const uint8_t *cls, const unsigned *lab, const unsigned *chunk_first, unsigned *rows)
{
    __shared__ unsigned wsum[CL_CHUNK / 64];
    const unsigned i = blockIdx.x * CL_CHUNK + threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const bool root = i < g.n && cls[i] && lab[i] == i;
    const unsigned long long b = __ballot(root);
    if (lane == 0) wsum[wave] = (unsigned)__popcll(b);
    __syncthreads();
    if (!root) return;
    unsigned r = chunk_first[blockIdx.x] + (unsigned)__popcll(b & ((1ull << lane) - 1ull));
    for (unsigned w = 0; w < wave; ++w) r += wsum[w];
    rows[r] = i + g.base;
    rows[(size_t)g.n + r] = 0u;
    rows[2 * (size_t)g.n + r] = 0u;
}

__global__ __launch_bounds__(CL_THREADS) void clusters_sizes(ClGeom g, const uint8_t *cls, unsigned *lab, const unsigned *count_ptr, unsigned *rows)
{
    const unsigned i = blockIdx.x * CL_THREADS + threadIdx.x, lane = threadIdx.x & 63u;
    const unsigned c = i < g.n ? cls[i] : 0u;
    const unsigned l = c ? lab[i] : CL_NONE;
    const unsigned prev = __shfl_up(l, 1, 64);
    const bool begins = c && (lane == 0 || prev != l);
    const unsigned long long edges = __ballot(begins || !c);       // where a run of equal labels ends: at the next beginning or idle lane
    if (begins) {
        const unsigned long long above = lane == 63u ? 0ull : edges >> (lane + 1u);
        const unsigned len = above ? (unsigned)__ffsll((long long)above) : 64u - lane;
        const unsigned key = l + g.base, count = *count_ptr;
        unsigned lo = 0, hi = count;               // the row whose label is key: the labels ascend
        for (int turn = 0; turn < 32 && lo + 1u < hi; ++turn) {
            const unsigned mid = lo + (hi - lo) / 2u;
            if (rows[mid] <= key) lo = mid; else hi = mid;
        }
        if (lo < count && rows[lo] == key) {
            atomicAdd(rows + (size_t)g.n + lo, len);
            const unsigned v = (c << 30) | (g.z0 + (i + len - 1u) / g.plane_cells);       // the run's last cell lies in its highest plane
            unsigned *zc = rows + 2 * (size_t)g.n + lo;
            if (cl_load(zc, 0) < v) atomicMax(zc, v);
        }
    }
    if (c) lab[i] = l + g.base;
}

// ---- host side
struct ClState {
    uint8_t *cls = nullptr;      // [n]
    unsigned *lab = nullptr;     // [n]
    unsigned *rows = nullptr;    // [3][n]
    unsigned *chunks = nullptr;  // [nchunk + 1]
    bool valid = false;          // labels and rows are those of the state after `at_step` steps
    int64_t at_step = -1, count = 0;
    ClGeom g{};
};

inline unsigned cl_chunks(unsigned n) { return (n + CL_CHUNK - 1u) / CL_CHUNK; }

// the seven launches on `stream`, then the number of clusters to the host: one synchronisation, 4 bytes
template <typename Loader>
hipError_t clusters_run(const Loader &load, ClState &s, double cut, hipStream_t stream)
{
    const ClGeom &g = s.g;
    const unsigned nchunk = cl_chunks(g.n), flat = (g.n + CL_THREADS - 1u) / CL_THREADS;
    clusters_classify<Loader><<<dim3(flat), dim3(CL_THREADS), 0, stream>>>(load, g, cut, s.cls);
    clusters_tiles<<<dim3((g.nx + CL_TX - 1u) / CL_TX, (g.ny + CL_TY - 1u) / CL_TY, (g.planes + CL_TZ - 1u) / CL_TZ), dim3(CL_TILE_THREADS), 0, stream>>>(g, s.cls, s.lab);
    clusters_merge<<<dim3(flat), dim3(CL_THREADS), 0, stream>>>(g, s.cls, s.lab);
    clusters_flatten<<<dim3(nchunk), dim3(CL_CHUNK), 0, stream>>>(g, s.cls, s.lab, s.chunks);
    clusters_scan<<<dim3(1), dim3(1024), 0, stream>>>(s.chunks, nchunk);
    clusters_rows<<<dim3(nchunk), dim3(CL_CHUNK), 0, stream>>>(g, s.cls, s.lab, s.chunks, s.rows);
    clusters_sizes<<<dim3(flat), dim3(CL_THREADS), 0, stream>>>(g, s.cls, s.lab, s.chunks + nchunk, s.rows);
    hipError_t e = hipGetLastError();
    unsigned count = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&count, s.chunks + nchunk, sizeof count, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    s.count = (int64_t)count;
    return e;
}

// The clusters of a context's state after `steps` steps, labelled and counted with g and cut: the body of the lbmpm_*_clusters entry
// points behind their own checks.  The four device arrays come from `mem` with the first call (zero_on: as DeviceBlocks::alloc).
template <typename Loader>
int clusters_label(const Loader &load, ClState &s, const ClGeom &g, double cut, int64_t steps, lbmpm::DeviceBlocks &mem, hipStream_t zero_on, hipStream_t stream,
                   int64_t *count)
{
    s.valid = false;
    if (!s.chunks) {
        int rc = mem.alloc(&s.cls, g.n, zero_on);
        if (!rc) rc = mem.alloc(&s.lab, g.n, zero_on);
        if (!rc) rc = mem.alloc(&s.rows, 3 * (size_t)g.n, zero_on);
        if (!rc) rc = mem.alloc(&s.chunks, cl_chunks(g.n) + 1u, zero_on);
        if (rc) return rc;
    }
    s.g = g;
    LBMPM_HIP_TRY(clusters_run(load, s, cut, stream));
    s.valid = true; s.at_step = steps;
    *count = s.count;
    return LBMPM_OK;
}

// LBMPM_ERR_STATE unless the labels are those of the state after `steps` steps; then the context's device is the current one
inline int clusters_current(const char *who, const ClState &s, int64_t steps, int device)
{
    if (!(s.valid && s.at_step == steps)) {
        set_error("%s: no clusters of the current state (call the _clusters function first, and again after a step or a change of state)", who);
        return LBMPM_ERR_STATE;
    }
    LBMPM_HIP_TRY(hipSetDevice(device));
    return LBMPM_OK;
}

// The bodies of the lbmpm_*_clusters_table / _labels / _faces entry points (`who`) behind their null checks.
// out: [count][LBMPM_CLUSTER_COLS]
inline int clusters_table(const char *who, const ClState &s, int64_t steps, int device, hipStream_t stream, int64_t *out)
{
    static_assert(LBMPM_CLUSTER_COLS == 5 && LBMPM_CL_LABEL == 0 && LBMPM_CL_ZMAX == 4, "the columns of rk3d_clusters.h");
    { const int rc = clusters_current(who, s, steps, device); if (rc) return rc; }
    const size_t m = (size_t)s.count;
    if (!m) return LBMPM_OK;
    std::vector<unsigned> h(3 * m);
    for (int col = 0; col < 3; ++col)
        LBMPM_HIP_TRY(hipMemcpyAsync(h.data() + col * m, s.rows + (size_t)col * s.g.n, m * sizeof(unsigned), hipMemcpyDeviceToHost, stream));
    LBMPM_HIP_TRY(hipStreamSynchronize(stream));
    for (size_t r = 0; r < m; ++r) {
        int64_t *row = out + r * LBMPM_CLUSTER_COLS;
        row[LBMPM_CL_LABEL] = h[r];
        row[LBMPM_CL_CLASS] = h[2 * m + r] >> 30;
        row[LBMPM_CL_CELLS] = h[m + r];
        row[LBMPM_CL_ZMIN] = h[r] / s.g.plane_cells;
        row[LBMPM_CL_ZMAX] = h[2 * m + r] & 0x3FFFFFFFu;
    }
    return LBMPM_OK;
}

inline int clusters_labels(const char *who, const ClState &s, int64_t steps, int device, hipStream_t stream, uint32_t *out)
{
    { const int rc = clusters_current(who, s, steps, device); if (rc) return rc; }
    LBMPM_HIP_TRY(hipMemcpyAsync(out, s.lab, (size_t)s.g.n * sizeof(unsigned), hipMemcpyDeviceToHost, stream));
    LBMPM_HIP_TRY(hipStreamSynchronize(stream));
    return LBMPM_OK;
}

// [2][ny][nx]: the lowest and the highest own plane
inline int clusters_faces(const char *who, const ClState &s, int64_t steps, int device, hipStream_t stream, uint32_t *labels, uint8_t *classes)
{
    { const int rc = clusters_current(who, s, steps, device); if (rc) return rc; }
    const size_t pc = s.g.plane_cells, top = (size_t)(s.g.planes - 1u) * pc;
    LBMPM_HIP_TRY(hipMemcpyAsync(labels, s.lab, pc * sizeof(unsigned), hipMemcpyDeviceToHost, stream));
    LBMPM_HIP_TRY(hipMemcpyAsync(labels + pc, s.lab + top, pc * sizeof(unsigned), hipMemcpyDeviceToHost, stream));
    LBMPM_HIP_TRY(hipMemcpyAsync(classes, s.cls, pc, hipMemcpyDeviceToHost, stream));
    LBMPM_HIP_TRY(hipMemcpyAsync(classes + pc, s.cls + top, pc, hipMemcpyDeviceToHost, stream));
    LBMPM_HIP_TRY(hipStreamSynchronize(stream));
    return LBMPM_OK;
}

// the configuration of a call (cfg may be null: phi_cut 0, faces) into cut and g.nlink; an LBMPM_* status
inline int clusters_configure(const char *who, const lbmpm_clusters_config *cfg, unsigned long long lattice_cells, double *cut, ClGeom *g)
{
    const double pc = cfg ? cfg->phi_cut : 0.;
    const int conn = cfg ? (int)cfg->connectivity : 6;
    if (!(pc >= 0.)) { set_error("%s: phi_cut %g (it is >= 0)", who, pc); return LBMPM_ERR_INVALID; }
    if (conn != 6 && conn != 18) { set_error("%s: connectivity %d (6: faces, 18: the D3Q19 links)", who, conn); return LBMPM_ERR_UNSUPPORTED; }
    if (lattice_cells >= 0xFFFFFFFFull) { set_error("%s: labels are 32-bit cell numbers, the lattice has %llu cells", who, lattice_cells); return LBMPM_ERR_UNSUPPORTED; }
    *cut = pc;
    g->nlink = conn == 6 ? 3 : 9;
    return LBMPM_OK;
}
