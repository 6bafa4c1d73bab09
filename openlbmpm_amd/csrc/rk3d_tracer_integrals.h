// Plane integrals of the D3Q7 tracers (lbmpm_rk3dcsf_tracer_integrals, include/lbmpm.h): per own plane and tracer the LBMPM_TRINT_COLS
// numbers a transport run is read through -- mass balances, breakthrough curves, the spreading of a plume along the flow axis -- over the
// populations lbmpm_rk3dcsf_tracer_get_pdf would hand out.  The columns and the cell loader of the reduction in rk3d_integrals.h (same
// stages, same fixed order: the table is the same bit for bit however the lattice is cut); one table per tracer in one pair of
// launches (grid z).  Included by rk3d_csf.hip after rk3d_tracer.h and rk3d_integrals.h.  This header is the only place that knows the
// order of the columns (LBMPM_TRINT_*).
// Per fluid cell and tracer 7 doubles are read, and the six source numbers (through the caches again for every tracer after the first).
#pragma once

struct TrCell { double g[TQ]; };

struct TracerCols {
    using Cell = TrCell;
    static constexpr int COLS = LBMPM_TRINT_COLS;
    static_assert(COLS == 9 && LBMPM_TRINT_CMIN == 6 && LBMPM_TRINT_CMAX == 7 && LBMPM_TRINT_NONFINITE == 8, "the columns of rk3d_tracer_integrals.h");
    // the extrema start from their identities, not from 0: a lane or a chunk without cells must leave a plane's minimum and maximum alone
    static __device__ __forceinline__ double init(int col) { return col == LBMPM_TRINT_CMIN ? HUGE_VAL : col == LBMPM_TRINT_CMAX ? -HUGE_VAL : 0.; }
    static __device__ __forceinline__ void take(double a[COLS], const TrCell &c)
    {
        a[LBMPM_TRINT_CELLS] += 1.;
        const double C = tr_sum(c.g);
        bool fin = integral_finite(C);
#pragma unroll
        for (int i = 0; i < TQ; ++i) fin = fin && integral_finite(c.g[i]);
        if (!fin) {
            a[LBMPM_TRINT_NONFINITE] += 1.;          // a bad cell counts here and in `cells`, and contributes to nothing else
            return;
        }
        a[LBMPM_TRINT_MASS] += C;
        a[LBMPM_TRINT_FLUX_X] += c.g[1] - c.g[2];
        a[LBMPM_TRINT_FLUX_Y] += c.g[3] - c.g[4];
        a[LBMPM_TRINT_FLUX_Z] += c.g[5] - c.g[6];
        a[LBMPM_TRINT_SUM_C2] += C * C;
        a[LBMPM_TRINT_CMIN] = C < a[LBMPM_TRINT_CMIN] ? C : a[LBMPM_TRINT_CMIN];
        a[LBMPM_TRINT_CMAX] = C > a[LBMPM_TRINT_CMAX] ? C : a[LBMPM_TRINT_CMAX];
    }
    static __device__ __forceinline__ double join(int col, double a, double b)
    {
        return col == LBMPM_TRINT_CMIN ? (b < a ? b : a) : col == LBMPM_TRINT_CMAX ? (b > a ? b : a) : a + b;
    }
    // a plane without a finite fluid cell still holds the identities (no finite C is infinite): it reports 0, and the table is finite
    static __device__ __forceinline__ double finish(int col, double v)
    {
        return (col == LBMPM_TRINT_CMIN || col == LBMPM_TRINT_CMAX) && !integral_finite(v) ? 0. : v;
    }
};

// the populations of tracer `set` as tr3d_observe<FIRST> hands them out (streamed, the inlet plane of the undivided lattice applied; on a
// slab the pulls out of the ghost planes; WALL: the wall reaction's bounce-back); own planes only (plane 0 is lattice plane p.glo)
template <bool FIRST, bool WALL>
struct TrIntLoader {
    CsfDev p;
    TrDev t;
    __device__ __forceinline__ bool operator()(unsigned set, unsigned plane, unsigned k, TrCell &c) const
    {
        const unsigned z = plane + (unsigned)p.glo;
        const unsigned n = z * ((unsigned)p.nx * (unsigned)p.ny) + k;
        if (!(p.meta[n] & 1u)) return false;
        const unsigned j = p.cidx[n];
        unsigned s[TQ];
        tr_sources<FIRST>(p, t, j, s);
        tr_pull<FIRST, WALL>(p, t, (int)set, j, s, (int)z + p.zoff == p.nzg - 1, c.g, WALL ? tr_wall_word(t, j) : 0u);
        return true;
    }
};

template <typename Loader>
__global__ __launch_bounds__(INTEGRAL_THREADS) void trint_partial(const Loader load, unsigned plane_cells, double *partial)
{
    integral_stage1<TracerCols>(load, plane_cells, partial);
}

__global__ __launch_bounds__(64) void trint_final(const double *partial, unsigned nchunk, double *out) { integral_stage2<TracerCols>(partial, nchunk, out); }

// both launches on `stream` for all nT tracers, then the table [planes][nT][9] to the host: one synchronisation, planes * nT * 72 bytes
template <typename Loader>
hipError_t tracer_integrals_run(const Loader &load, unsigned planes, unsigned plane_cells, unsigned nT, double *buf, double *host_out, hipStream_t stream)
{
    const unsigned nchunk = integral_chunks(plane_cells);
    double *table = integral_table<TracerCols>(buf, planes, plane_cells, nT);
    trint_partial<Loader><<<dim3(nchunk, planes, nT), dim3(INTEGRAL_THREADS), 0, stream>>>(load, plane_cells, buf);
    trint_final<<<dim3(planes, nT), dim3(64), 0, stream>>>(buf, nchunk, table);
    return integrals_download<TracerCols>(table, planes, nT, host_out, stream);
}
