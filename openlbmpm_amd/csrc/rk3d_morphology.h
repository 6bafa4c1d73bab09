// Phase morphology of the 3-D solvers (lbmpm_rk3d_morphology* / lbmpm_rk3dcsf_morphology*; the definition is in include/lbmpm.h): per own
// plane the cells of each class, the density sums of both phases, the pairs along every axis by their classes, and the 2 x 2 squares and
// 2 x 2 x 2 cubes of one phase -- interfacial and wetted areas, Euler characteristics and a phase-averaged pressure difference follow
// from them on the host.  Included by rk3d.hip and rk3d_csf.hip inside their unnamed namespaces, after rk3d_integrals.h, and templated
// over the flow's loader of that file (IntCell: rho_R, rho_B, phi; the velocity it also computes is dead code here).  Three launches:
//   1 classify   one byte per own cell (LBMPM_MORPH_S / _R / _B / _N) from the loader, into [planes + 1][ny][nx] bytes.  The extra plane
//                is the caller's `above` (the lowest plane of the slab over this one), or MORPH_NOTHING throughout: a fifth value that is
//                in no counted pair, square or cube, so that the highest plane of the lattice anchors nothing that reaches upwards.
//   2, 3         integral_stage1 / _stage2 of rk3d_integrals.h over MorphCols.  A cell -- solid ones too: a solid cell anchors the RS and
//                BS pairs towards +x, +y and +z -- brings the eight class bytes of the cube it anchors (x and y wrapped; read from cache,
//                every byte up to eight times) and, where it is R or B itself, rho_R + rho_B through the flow's loader once more.
// Every count is a sum of ones in doubles, exact in any order; the two density sums are added in the reducer's fixed order, which (nx, ny)
// and the plane's classes fix alone -- the table is the same bit for bit however the lattice is cut.  No atomics.
#pragma once

constexpr unsigned MORPH_NOTHING = 4;            // the plane over the lattice's last one
constexpr unsigned MORPH_THREADS = 256;

struct MorphCell {
    unsigned cls;                // eight class bytes, own cell lowest: bit 0 of the byte number is +x, bit 1 +y, bit 2 +z
    unsigned cls_hi;
    double rho;                  // rho_R + rho_B of an R or B anchor, else 0
};

struct MorphCols {
    using Cell = MorphCell;
    static constexpr int COLS = LBMPM_MORPH_COLS;
    static_assert(COLS == 28 && LBMPM_MO_CELLS_R == 0 && LBMPM_MO_RHO_R == 3 && LBMPM_MO_RR_X == 5 && LBMPM_MO_RR_Y == 10 && LBMPM_MO_RR_Z == 15 &&
                  LBMPM_MO_BS_Z == 19 && LBMPM_MO_SQ_R_XY == 20 && LBMPM_MO_SQ_B_XY == 23 && LBMPM_MO_CUBE_R == 26 && LBMPM_MO_CUBE_B == 27,
                  "the columns of rk3d_morphology.h");
    static __device__ __forceinline__ double init(int) { return 0.; }
    static __device__ __forceinline__ double one_if(bool b) { return b ? 1. : 0.; }
    // the pair of an anchor with its neighbour along one axis; m has the bit of either class (S 1, R 2, B 4, N 8, nothing 16).  Every
    // index into a[] is a constant: the accumulators stay in registers.
    template <int FIRST>
    static __device__ __forceinline__ void pair(double a[COLS], unsigned m)
    {
        a[FIRST + 0] += one_if(m == 2u);         // RR
        a[FIRST + 1] += one_if(m == 4u);         // BB
        a[FIRST + 2] += one_if(m == 6u);         // RB
        a[FIRST + 3] += one_if(m == 3u);         // RS
        a[FIRST + 4] += one_if(m == 5u);         // BS
    }
    static __device__ __forceinline__ void take(double a[COLS], const MorphCell &c)
    {
        unsigned b[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) { b[i] = 1u << ((c.cls >> (8 * i)) & 0xFFu); b[4 + i] = 1u << ((c.cls_hi >> (8 * i)) & 0xFFu); }
        a[LBMPM_MO_CELLS_R] += one_if(b[0] == 2u);
        a[LBMPM_MO_CELLS_B] += one_if(b[0] == 4u);
        a[LBMPM_MO_CELLS_N] += one_if(b[0] == 8u);
        if (b[0] == 2u) a[LBMPM_MO_RHO_R] += c.rho;
        if (b[0] == 4u) a[LBMPM_MO_RHO_B] += c.rho;
        pair<LBMPM_MO_RR_X>(a, b[0] | b[1]);
        pair<LBMPM_MO_RR_Y>(a, b[0] | b[2]);
        pair<LBMPM_MO_RR_Z>(a, b[0] | b[4]);
        const unsigned xy = b[0] & b[1] & b[2] & b[3], xz = b[0] & b[1] & b[4] & b[5], yz = b[0] & b[2] & b[4] & b[6];
        const unsigned cube = xy & b[4] & b[5] & b[6] & b[7];
        a[LBMPM_MO_SQ_R_XY] += one_if(xy == 2u);
        a[LBMPM_MO_SQ_R_XZ] += one_if(xz == 2u);
        a[LBMPM_MO_SQ_R_YZ] += one_if(yz == 2u);
        a[LBMPM_MO_SQ_B_XY] += one_if(xy == 4u);
        a[LBMPM_MO_SQ_B_XZ] += one_if(xz == 4u);
        a[LBMPM_MO_SQ_B_YZ] += one_if(yz == 4u);
        a[LBMPM_MO_CUBE_R] += one_if(cube == 2u);
        a[LBMPM_MO_CUBE_B] += one_if(cube == 4u);
    }
    static __device__ __forceinline__ double join(int, double a, double b) { return a + b; }
    static __device__ __forceinline__ double finish(int, double v) { return v; }
};

// the class of the cell k of the own plane `plane`
template <typename Flow>
__device__ __forceinline__ unsigned morph_class(const Flow &flow, unsigned plane, unsigned k, double cut)
{
    IntCell c;
    if (!flow(0u, plane, k, c)) return LBMPM_MORPH_S;
    if (!(integral_finite(c.phi) && integral_finite(c.rR) && integral_finite(c.rB))) return LBMPM_MORPH_N;
    return c.phi > cut ? LBMPM_MORPH_R : (c.phi <= -cut ? LBMPM_MORPH_B : LBMPM_MORPH_N);
}

// one thread per cell of the first n = planes * plane_cells cells (the face: planes = 1)
template <typename Flow>
__global__ __launch_bounds__(MORPH_THREADS) void morphology_classify(const Flow flow, unsigned n, unsigned plane_cells, double cut, uint8_t *cls)
{
    const unsigned i = blockIdx.x * MORPH_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned plane = i / plane_cells;
    cls[i] = (uint8_t)morph_class(flow, plane, i - plane * plane_cells, cut);
}

// the reducer's loader: every cell of a plane is an anchor.  cls: [planes + 1][ny][nx]
template <typename Flow>
struct MorphLoader {
    Flow flow;
    const uint8_t *cls;
    unsigned nx, ny;
    __device__ __forceinline__ bool operator()(unsigned, unsigned plane, unsigned k, MorphCell &c) const
    {
        const unsigned y = k / nx, x = k - y * nx;
        const unsigned xp = x + 1u < nx ? x + 1u : 0u, yp = y + 1u < ny ? y + 1u : 0u;
        const unsigned pc = nx * ny;
        const uint8_t *lo = cls + (size_t)plane * pc, *hi = lo + pc;
        const unsigned i00 = y * nx + x, i10 = y * nx + xp, i01 = yp * nx + x, i11 = yp * nx + xp;
        const unsigned own = lo[i00];
        c.cls = own | (unsigned)lo[i10] << 8 | (unsigned)lo[i01] << 16 | (unsigned)lo[i11] << 24;
        c.cls_hi = (unsigned)hi[i00] | (unsigned)hi[i10] << 8 | (unsigned)hi[i01] << 16 | (unsigned)hi[i11] << 24;
        c.rho = 0.;
        if (own == LBMPM_MORPH_R || own == LBMPM_MORPH_B) {
            IntCell f;
            if (flow(0u, plane, k, f)) c.rho = f.rR + f.rB;
        }
        return true;
    }
};

template <typename Flow>
__global__ __launch_bounds__(INTEGRAL_THREADS) void morphology_partial(const MorphLoader<Flow> load, unsigned plane_cells, double *partial)
{
    integral_stage1<MorphCols>(load, plane_cells, partial);
}

__global__ __launch_bounds__(64) void morphology_final(const double *partial, unsigned nchunk, double *out) { integral_stage2<MorphCols>(partial, nchunk, out); }

// the configuration of a call (cfg may be null: phi_cut 0); array_cells: those of the class array.  An LBMPM_* status
inline int morphology_configure(const char *who, const lbmpm_morphology_config *cfg, unsigned long long array_cells, double *cut)
{
    const double pc = cfg ? cfg->phi_cut : 0.;
    if (!(pc >= 0.) || pc > 1.7976931348623157e308) { set_error("%s: phi_cut %g (it is finite and >= 0)", who, pc); return LBMPM_ERR_INVALID; }
    if (array_cells >= 0xFFFFFFFFull) { set_error("%s: cells are numbered in 32 bits, the slab has %llu with the plane above", who, array_cells); return LBMPM_ERR_UNSUPPORTED; }
    *cut = pc;
    return LBMPM_OK;
}

// the class array of a context, [planes + 1][ny][nx] bytes from `mem` with the first call (zero_on: as DeviceBlocks::alloc)
inline int morphology_classes(lbmpm::DeviceBlocks &mem, uint8_t **cls, unsigned planes, unsigned plane_cells, hipStream_t zero_on)
{
    return *cls ? LBMPM_OK : mem.alloc(cls, ((size_t)planes + 1u) * plane_cells, zero_on);
}

// The body of the lbmpm_*_morphology_face entry points behind their own checks: the classes of the lowest own plane, classified into the
// first plane of cls and copied to the host.  One synchronisation, plane_cells bytes.
template <typename Flow>
int morphology_face(const Flow &flow, uint8_t *cls, unsigned plane_cells, double cut, uint8_t *host_out, hipStream_t stream)
{
    morphology_classify<Flow><<<dim3((plane_cells + MORPH_THREADS - 1u) / MORPH_THREADS), dim3(MORPH_THREADS), 0, stream>>>(flow, plane_cells, plane_cells, cut, cls);
    LBMPM_HIP_TRY(hipGetLastError());
    LBMPM_HIP_TRY(hipMemcpyAsync(host_out, cls, plane_cells, hipMemcpyDeviceToHost, stream));
    LBMPM_HIP_TRY(hipStreamSynchronize(stream));
    return LBMPM_OK;
}

// The body of the lbmpm_*_morphology entry points (`who`) behind their own checks.  above: host [ny][nx] or null.  The chunk partials and
// the table live for the length of the call ([planes][chunks + 1][28] doubles, not counted in device_bytes); host_out: [planes][28].
template <typename Flow>
int morphology_run(const char *who, const Flow &flow, uint8_t *cls, unsigned planes, unsigned nx, unsigned ny, double cut, const uint8_t *above,
                   double *host_out, hipStream_t stream)
{
    const unsigned plane_cells = nx * ny, n = planes * plane_cells, nchunk = integral_chunks(plane_cells);
    if (above)
        for (unsigned k = 0; k < plane_cells; ++k)
            if (above[k] > 3) { set_error("%s: above[%u] = %u (a class is 0 .. 3)", who, k, (unsigned)above[k]); return LBMPM_ERR_INVALID; }
    lbmpm::DeviceTemp<double> buf;
    if (buf.alloc(integral_buffer_doubles<MorphCols>(planes, plane_cells)) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: hipMalloc(%zu bytes) failed", who, integral_buffer_doubles<MorphCols>(planes, plane_cells) * sizeof(double));
        return LBMPM_ERR_NOMEM;
    }
    double *table = integral_table<MorphCols>(buf.get(), planes, plane_cells);
    if (above) LBMPM_HIP_TRY(hipMemcpyAsync(cls + n, above, plane_cells, hipMemcpyHostToDevice, stream));
    else LBMPM_HIP_TRY(hipMemsetAsync(cls + n, (int)MORPH_NOTHING, plane_cells, stream));
    morphology_classify<Flow><<<dim3((n + MORPH_THREADS - 1u) / MORPH_THREADS), dim3(MORPH_THREADS), 0, stream>>>(flow, n, plane_cells, cut, cls);
    LBMPM_HIP_TRY(hipGetLastError());
    const MorphLoader<Flow> load{flow, cls, nx, ny};
    morphology_partial<Flow><<<dim3(nchunk, planes), dim3(INTEGRAL_THREADS), 0, stream>>>(load, plane_cells, buf.get());
    morphology_final<<<dim3(planes), dim3(64), 0, stream>>>(buf.get(), nchunk, table);
    LBMPM_HIP_TRY(integrals_download<MorphCols>(table, planes, 1, host_out, stream));      // synchronises: buf may go
    return LBMPM_OK;
}
