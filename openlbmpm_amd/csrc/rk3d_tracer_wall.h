// Uptake of the tracers at solid walls (lbmpm_rk3dcsf_tracer_wall_integrals, include/lbmpm.h): per own plane and tracer the
// LBMPM_TRWALL_COLS numbers the wall reaction of rk3d_tracer.h is read through -- how many wall links a plane has, what the walls took
// out of the tracer in the last completed sub-step and the concentration they saw.  The columns and the cell loader of the reduction in
// rk3d_integrals.h (same stages, same fixed order: the table is the same bit for bit however the lattice is cut); one table per tracer
// in one pair of launches (grid z).  Included by rk3d_csf.hip after rk3d_tracer_integrals.h.  This header is the only place that knows
// the order of the columns (LBMPM_TRWALL_*).
// A wall link is a fluid cell x and a direction i in 1 .. 6 whose source cell x - e_i is solid.  Over it the pull takes
// g_in = r g_out with g_out = g*_OPP[i](x), the stored population that left for the wall: the link's uptake is g_out - g_in, its wall
// concentration 3 (g_out + g_in).  Nothing is accumulated by the step: the stored populations and the table of source cells are all
// this reads (per fluid cell six source numbers, the class word, and one double per wall link).
#pragma once

struct TrWallCell { double links, uptake, wallc; bool bad; };

struct TracerWallCols {
    using Cell = TrWallCell;
    static constexpr int COLS = LBMPM_TRWALL_COLS;
    static_assert(COLS == 4 && LBMPM_TRWALL_LINKS == 0 && LBMPM_TRWALL_UPTAKE == 1 && LBMPM_TRWALL_C == 2 && LBMPM_TRWALL_NONFINITE == 3, "the columns of rk3d_tracer_wall.h");
    static __device__ __forceinline__ double init(int) { return 0.; }
    static __device__ __forceinline__ void take(double a[COLS], const TrWallCell &c)
    {
        a[LBMPM_TRWALL_LINKS] += c.links;
        if (c.bad) {
            a[LBMPM_TRWALL_NONFINITE] += 1.;         // a bad cell counts here and in the links, and contributes to nothing else
            return;
        }
        a[LBMPM_TRWALL_UPTAKE] += c.uptake;
        a[LBMPM_TRWALL_C] += c.wallc;
    }
    static __device__ __forceinline__ double join(int, double a, double b) { return a + b; }
    static __device__ __forceinline__ double finish(int, double v) { return v; }
};

// the wall links of tracer `set` at the cell as tr_pull<FIRST, true> takes them (a context without a wall reaction: r = 1, an uptake of
// exactly 0); FIRST: the populations stand where they were given, no wall event has happened -- links only.  Own planes only
template <bool FIRST>
struct TrWallLoader {
    CsfDev p;
    TrDev t;
    __device__ __forceinline__ bool operator()(unsigned set, unsigned plane, unsigned k, TrWallCell &c) const
    {
        constexpr int OPP[Q] = CSF_OPP;
        const unsigned z = plane + (unsigned)p.glo;
        const unsigned n = z * ((unsigned)p.nx * (unsigned)p.ny) + k;
        if (!(p.meta[n] & 1u)) return false;
        const unsigned j = p.cidx[n];
        const uint32_t word = tr_wall_word(t, j);
        const double *gt = t.gin + (size_t)set * TQ * p.FS;
        c.links = 0.; c.uptake = 0.; c.wallc = 0.; c.bad = false;
#pragma unroll
        for (int i = 1; i < TQ; ++i) {
            if (t.src[(size_t)(i - 1) * p.FS + j] != SRC_WALL) continue;
            c.links += 1.;
            if (FIRST) continue;
            const double gout = gt[(size_t)OPP[i] * p.FS + j];
            const double gin = tr_wall_r(t, (int)set, word, i) * gout;
            c.bad = c.bad || !integral_finite(gout);
            c.uptake += gout - gin;
            c.wallc += 3. * (gout + gin);
        }
        return true;
    }
};

template <typename Loader>
__global__ __launch_bounds__(INTEGRAL_THREADS) void trwall_partial(const Loader load, unsigned plane_cells, double *partial)
{
    integral_stage1<TracerWallCols>(load, plane_cells, partial);
}

__global__ __launch_bounds__(64) void trwall_final(const double *partial, unsigned nchunk, double *out) { integral_stage2<TracerWallCols>(partial, nchunk, out); }

// both launches on `stream` for all nT tracers, then the table [planes][nT][4] to the host: one synchronisation, planes * nT * 32 bytes
template <typename Loader>
hipError_t tracer_wall_integrals_run(const Loader &load, unsigned planes, unsigned plane_cells, unsigned nT, double *buf, double *host_out, hipStream_t stream)
{
    const unsigned nchunk = integral_chunks(plane_cells);
    double *table = integral_table<TracerWallCols>(buf, planes, plane_cells, nT);
    trwall_partial<Loader><<<dim3(nchunk, planes, nT), dim3(INTEGRAL_THREADS), 0, stream>>>(load, plane_cells, buf);
    trwall_final<<<dim3(planes, nT), dim3(64), 0, stream>>>(buf, nchunk, table);
    return integrals_download<TracerWallCols>(table, planes, nT, host_out, stream);
}
