// Plane integrals of the 3-D solvers (lbmpm_rk3d_integrals / lbmpm_rk3dcsf_integrals / lbmpm_rk3dcsf_tracer_integrals, include/lbmpm.h):
// per owned plane z a row of sums, counts and extrema that a run is read through, reduced on the device from the recorded state.
// Included by rk3d.hip and rk3d_csf.hip inside their unnamed namespaces.  The reduction is written once, over two template parameters:
//   Cols    the columns of a table: the cell type `Cell`, the count `COLS`, init(col) (what an accumulator starts from), take(a, cell)
//           (one cell into a thread's accumulators), join(col, a, b) (sum, max or min) and finish(col, v) (applied once, to the plane's
//           value).  FlowCols below is the flow's twelve (LBMPM_INT_*) and the only place that knows their order; the tracers' nine
//           (LBMPM_TRINT_*) are TracerCols of rk3d_tracer_integrals.h.
//   Loader  the cells of a context, see integrals_partial.  The flow's:
//   * perturbation model (rk3d.hip): the diagnostic arrays of the last lbmpm_rk3d_phase_field(ctx, 1) and the phase field, read as
//     lbmpm_rk3d_get_field reads them.  Fusing the reduction into the 23-value pull of rk3dq.h is left out on purpose: that model
//     goes through phase_field(ctx, 1) as before.
//   * CSF model (rk3d_csf.hip): cell_state<FIRST, true> and the arithmetic of csf3d_observe<., true>, reduced in registers -- no
//     staging array, no population array.
// A launch reduces `sets` tables at once (grid z; the flow: one, the tracers: one per tracer).  The stages are __device__ bodies; every
// table wraps them in a pair of kernels of its own.
//
// The numbers must not depend on how the lattice is cut into slabs, so every addition happens in an order that (nx, ny) and the
// plane's mask fix alone:
//   stage 1  one workgroup per (plane, chunk, set); a chunk is a run of INTEGRAL_CHUNK in-plane cell numbers y * nx + x (the last one of
//            a plane ragged; solid cells idle).  Thread t takes the cells begin + t, begin + t + 256, ... in that order; the wave joins
//            its 64 lanes in a __shfl_down tree, the four waves are joined in wave order through LDS; COLS plain stores per workgroup.
//   stage 2  one wave per (plane, set): lane c joins column c of the plane's chunks in chunk order.
// No floating-point atomics: their order is not fixed.  (A chunking by a fluid-cell number that counts from the slab's first plane,
// ghost planes included, would change with the cut.)
#pragma once

constexpr unsigned INTEGRAL_CHUNK = 1024;        // in-plane cells per workgroup of stage 1
constexpr unsigned INTEGRAL_THREADS = 256;
static_assert(INTEGRAL_CHUNK % INTEGRAL_THREADS == 0, "every thread of a full chunk walks the same number of cells");

struct IntCell { double rR, rB, ux, uy, uz, phi; };

__host__ __device__ __forceinline__ unsigned integral_chunks(unsigned plane_cells) { return (plane_cells + INTEGRAL_CHUNK - 1u) / INTEGRAL_CHUNK; }

__device__ __forceinline__ bool integral_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }      // false for NaN and +-Inf

// the flow's table
struct FlowCols {
    using Cell = IntCell;
    static constexpr int COLS = LBMPM_INTEGRAL_COLS;
    static_assert(COLS == 12 && LBMPM_INT_NONFINITE == 11 && LBMPM_INT_UMAX2 == 10, "the columns of rk3d_integrals.h");
    static __device__ __forceinline__ double init(int) { return 0.; }
    // one cell into a thread's twelve accumulators (one rounded product per cell and column, then the sum)
    static __device__ __forceinline__ void take(double a[COLS], const IntCell &c)
    {
        a[LBMPM_INT_CELLS] += 1.;
        if (!(integral_finite(c.rR) && integral_finite(c.rB) && integral_finite(c.ux) && integral_finite(c.uy) && integral_finite(c.uz) && integral_finite(c.phi))) {
            a[LBMPM_INT_NONFINITE] += 1.;            // a bad cell counts here and in `cells`, and contributes to nothing else
            return;
        }
        a[LBMPM_INT_MASS_R] += c.rR;
        a[LBMPM_INT_MASS_B] += c.rB;
        a[LBMPM_INT_FLUX_R] += c.rR * c.uz;
        a[LBMPM_INT_FLUX_B] += c.rB * c.uz;
        if (c.phi > 0.) { a[LBMPM_INT_CELLS_R] += 1.; a[LBMPM_INT_UZ_R] += c.uz; }
        else a[LBMPM_INT_UZ_B] += c.uz;
        const double rho = c.rR + c.rB;
        a[LBMPM_INT_MOM_X] += rho * c.ux;
        a[LBMPM_INT_MOM_Y] += rho * c.uy;
        const double u2 = c.ux * c.ux + c.uy * c.uy + c.uz * c.uz;
        a[LBMPM_INT_UMAX2] = u2 > a[LBMPM_INT_UMAX2] ? u2 : a[LBMPM_INT_UMAX2];
    }
    static __device__ __forceinline__ double join(int col, double a, double b) { return col == LBMPM_INT_UMAX2 ? (b > a ? b : a) : a + b; }
    static __device__ __forceinline__ double finish(int, double v) { return v; }
};

// Loader: bool operator()(unsigned set, unsigned plane, unsigned k, Cols::Cell &c) const -- the cell k = y * nx + x of the context's own
// plane `plane` (0: its first own plane) for the table `set`; false for a solid cell.
// Stage 1, the body of a kernel of INTEGRAL_THREADS threads on a grid (chunks, planes, sets); partial: [sets][planes][chunks][COLS].  The
// kernels themselves are thin __global__ wrappers, one pair per table (here the flow's; the tracers': rk3d_tracer_integrals.h), so that
// every table's launches carry a name of their own in a trace.
template <typename Cols, typename Loader>
__device__ __forceinline__ void integral_stage1(const Loader &load, unsigned plane_cells, double *partial)
{
    constexpr int COLS = Cols::COLS;
    __shared__ double lds[INTEGRAL_THREADS / 64][COLS];
    const unsigned chunk = blockIdx.x, plane = blockIdx.y, set = blockIdx.z;
    const unsigned begin = chunk * INTEGRAL_CHUNK;
    const unsigned end = begin + INTEGRAL_CHUNK < plane_cells ? begin + INTEGRAL_CHUNK : plane_cells;
    double a[COLS];
#pragma unroll
    for (int i = 0; i < COLS; ++i) a[i] = Cols::init(i);
    for (unsigned k = begin + threadIdx.x; k < end; k += INTEGRAL_THREADS) {
        typename Cols::Cell c;
        if (load(set, plane, k, c)) Cols::take(a, c);
    }
    // the wave: lane l takes lane l + off for off = 32, 16 .. 1 (every lane takes part; lane 0 ends with the sum in a fixed order)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int i = 0; i < COLS; ++i) a[i] = Cols::join(i, a[i], __shfl_down(a[i], off, 64));
    }
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < COLS; ++i) lds[wave][i] = a[i];
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)COLS) {
        const int i = (int)threadIdx.x;
        double r = lds[0][i];
        for (unsigned w = 1; w < INTEGRAL_THREADS / 64; ++w) r = Cols::join(i, r, lds[w][i]);
        partial[(((size_t)set * gridDim.y + plane) * gridDim.x + chunk) * COLS + i] = r;
    }
}

// Stage 2, the body of a kernel of 64 threads on a grid (planes, sets); out: [planes][sets][COLS]
template <typename Cols>
__device__ __forceinline__ void integral_stage2(const double *partial, unsigned nchunk, double *out)
{
    constexpr int COLS = Cols::COLS;
    const unsigned plane = blockIdx.x, set = blockIdx.y;
    if (threadIdx.x >= (unsigned)COLS) return;
    const int i = (int)threadIdx.x;
    const double *src = partial + ((size_t)set * gridDim.x + plane) * nchunk * COLS + i;
    double r = src[0];
#pragma unroll 4
    for (unsigned k = 1; k < nchunk; ++k) r = Cols::join(i, r, src[(size_t)k * COLS]);
    out[((size_t)plane * gridDim.y + set) * COLS + i] = Cols::finish(i, r);
}

// doubles of the device buffer of a context with `planes` own planes: [sets][planes][nchunk][COLS] partials, then [planes][sets][COLS]
template <typename Cols>
inline size_t integral_buffer_doubles(unsigned planes, unsigned plane_cells, unsigned sets = 1)
{
    return (size_t)sets * planes * (integral_chunks(plane_cells) + 1u) * Cols::COLS;
}
template <typename Cols>
inline double *integral_table(double *buf, unsigned planes, unsigned plane_cells, unsigned sets = 1)
{
    return buf + (size_t)sets * planes * integral_chunks(plane_cells) * Cols::COLS;
}

// the device buffer of a context, from `mem` with the first call (zero_on: as DeviceBlocks::alloc)
template <typename Cols>
inline int integral_buffer(lbmpm::DeviceBlocks &mem, double **buf, unsigned planes, unsigned plane_cells, unsigned sets, hipStream_t zero_on)
{
    return *buf ? LBMPM_OK : mem.alloc(buf, integral_buffer_doubles<Cols>(planes, plane_cells, sets), zero_on);
}

// after both launches on `stream`: the table to the host -- one synchronisation, planes * sets * COLS * 8 bytes
template <typename Cols>
hipError_t integrals_download(const double *table, unsigned planes, unsigned sets, double *host_out, hipStream_t stream)
{
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host_out, table, (size_t)planes * sets * Cols::COLS * sizeof(double), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return e;
}

// ---- the flow's table
template <typename Loader>
__global__ __launch_bounds__(INTEGRAL_THREADS) void integrals_partial(const Loader load, unsigned plane_cells, double *partial)
{
    integral_stage1<FlowCols>(load, plane_cells, partial);
}

__global__ __launch_bounds__(64) void integrals_final(const double *partial, unsigned nchunk, double *out) { integral_stage2<FlowCols>(partial, nchunk, out); }

// both launches on `stream`, then the table to the host: one synchronisation, planes * 96 bytes
template <typename Loader>
hipError_t integrals_run(const Loader &load, unsigned planes, unsigned plane_cells, double *buf, double *host_out, hipStream_t stream)
{
    const unsigned nchunk = integral_chunks(plane_cells);
    double *table = integral_table<FlowCols>(buf, planes, plane_cells);
    integrals_partial<Loader><<<dim3(nchunk, planes), dim3(INTEGRAL_THREADS), 0, stream>>>(load, plane_cells, buf);
    integrals_final<<<dim3(planes), dim3(64), 0, stream>>>(buf, nchunk, table);
    return integrals_download<FlowCols>(table, planes, 1, host_out, stream);
}
