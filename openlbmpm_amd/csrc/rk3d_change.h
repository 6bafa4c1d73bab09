// Steady-state monitor of the 3-D solvers (lbmpm_rk3d_change* / lbmpm_rk3dcsf_change*; the definition is in include/lbmpm.h): how far the
// recorded state has moved since a snapshot of it -- per own plane the squared change of the velocity by phase, of the phase field, the
// cells that changed colour, the two largest changes.  Included by rk3d.hip and rk3d_csf.hip inside their unnamed namespaces, after
// rk3d_integrals.h, and templated over the flow's loader of that file.
//   snapshot   ux, uy, uz, phi of every own cell as the loader yields them: four arrays [planes][ny][nx] one after the other (32 bytes per
//              own lattice cell, the same in both models, coalesced along k = y * nx + x), from the context's DeviceBlocks with the first
//              mark.  Solid cells are never written and never read.
//   one pass   integral_stage1 / _stage2 of rk3d_integrals.h over ChangeCols with ChangeLoader<Flow, HAVE_OLD, REMARK>: the cell through
//              the flow's loader, the old four values (HAVE_OLD), the current four over them (REMARK; also where they are not finite).
//              One thread per cell and pass: the read and the write of a cell are the same thread's, in that order.  The first mark is
//              <false, true>: it reads nothing of the snapshot, and its table is not looked at.
// The sums are taken in the reducer's fixed order, and a snapshot belongs to the cell: the table is the same bit for bit however the
// lattice is cut, slabs exchange nothing.  No atomics.
#pragma once

struct ChangeCell {
    double ux, uy, uz, phi;          // now
    double ux0, uy0, uz0, phi0;      // the snapshot
    bool bad;                        // one of rho_R, rho_B, u, phi (now) is not finite
};

struct ChangeCols {
    using Cell = ChangeCell;
    static constexpr int COLS = LBMPM_CHANGE_COLS;
    static_assert(COLS == 11 && LBMPM_CH_CELLS == 0 && LBMPM_CH_FLIPPED == 2 && LBMPM_CH_U2_R == 3 && LBMPM_CH_DU2_R == 5 && LBMPM_CH_DPHI2 == 7 &&
                  LBMPM_CH_DUMAX2 == 8 && LBMPM_CH_DPHIMAX == 9 && LBMPM_CH_NONFINITE == 10, "the columns of rk3d_change.h");
    static __device__ __forceinline__ double init(int) { return 0.; }
    // one cell into a thread's eleven accumulators (every term left to right, one rounding per operation)
    static __device__ __forceinline__ void take(double a[COLS], const ChangeCell &c)
    {
        a[LBMPM_CH_CELLS] += 1.;
        if (c.bad || !(integral_finite(c.ux0) && integral_finite(c.uy0) && integral_finite(c.uz0) && integral_finite(c.phi0))) {
            a[LBMPM_CH_NONFINITE] += 1.;             // a bad cell counts here and in `cells`, and contributes to nothing else
            return;
        }
        const bool red = c.phi > 0.;
        if (red) a[LBMPM_CH_CELLS_R] += 1.;
        if (red != (c.phi0 > 0.)) a[LBMPM_CH_FLIPPED] += 1.;
        const double u2 = c.ux * c.ux + c.uy * c.uy + c.uz * c.uz;
        const double dx = c.ux - c.ux0, dy = c.uy - c.uy0, dz = c.uz - c.uz0;
        const double du2 = dx * dx + dy * dy + dz * dz;
        if (red) { a[LBMPM_CH_U2_R] += u2; a[LBMPM_CH_DU2_R] += du2; }
        else { a[LBMPM_CH_U2_B] += u2; a[LBMPM_CH_DU2_B] += du2; }
        const double d = c.phi - c.phi0;
        a[LBMPM_CH_DPHI2] += d * d;
        a[LBMPM_CH_DUMAX2] = du2 > a[LBMPM_CH_DUMAX2] ? du2 : a[LBMPM_CH_DUMAX2];
        const double ad = fabs(d);
        a[LBMPM_CH_DPHIMAX] = ad > a[LBMPM_CH_DPHIMAX] ? ad : a[LBMPM_CH_DPHIMAX];
    }
    static __device__ __forceinline__ double join(int col, double a, double b)
    {
        return col == LBMPM_CH_DUMAX2 || col == LBMPM_CH_DPHIMAX ? (b > a ? b : a) : a + b;
    }
    static __device__ __forceinline__ double finish(int, double v) { return v; }
};

// the reducer's loader.  snap: [4][cells] with cells = planes * plane_cells
template <typename Flow, bool HAVE_OLD, bool REMARK>
struct ChangeLoader {
    Flow flow;
    double *snap;
    size_t cells;
    unsigned plane_cells;
    __device__ __forceinline__ bool operator()(unsigned, unsigned plane, unsigned k, ChangeCell &c) const
    {
        IntCell f;
        if (!flow(0u, plane, k, f)) return false;
        c.ux = f.ux; c.uy = f.uy; c.uz = f.uz; c.phi = f.phi;
        c.bad = !(integral_finite(f.rR) && integral_finite(f.rB) && integral_finite(f.ux) && integral_finite(f.uy) && integral_finite(f.uz) && integral_finite(f.phi));
        const size_t i = (size_t)plane * plane_cells + k;
        if (HAVE_OLD) { c.ux0 = snap[i]; c.uy0 = snap[cells + i]; c.uz0 = snap[2 * cells + i]; c.phi0 = snap[3 * cells + i]; }
        else { c.ux0 = f.ux; c.uy0 = f.uy; c.uz0 = f.uz; c.phi0 = f.phi; }
        if (REMARK) { snap[i] = f.ux; snap[cells + i] = f.uy; snap[2 * cells + i] = f.uz; snap[3 * cells + i] = f.phi; }
        return true;
    }
};

template <typename Flow, bool HAVE_OLD, bool REMARK>
__global__ __launch_bounds__(INTEGRAL_THREADS) void change_partial(const ChangeLoader<Flow, HAVE_OLD, REMARK> load, unsigned plane_cells, double *partial)
{
    integral_stage1<ChangeCols>(load, plane_cells, partial);
}

__global__ __launch_bounds__(64) void change_final(const double *partial, unsigned nchunk, double *out) { integral_stage2<ChangeCols>(partial, nchunk, out); }

// what a context keeps for the monitor; nothing is allocated before the first mark
struct ChState {
    double *snap = nullptr;          // [4][planes][ny][nx]
    double *buf = nullptr;           // chunk partials + the table (integral_buffer<ChangeCols>)
    bool valid = false;              // a snapshot of the state the context still steps from (set_* void it)
    int64_t at_step = 0;             // the context's step counter at the mark
};

// The body of the lbmpm_*_change_mark entry points behind their own checks: the snapshot of the recorded state, enqueued on `stream`
template <typename Flow>
int change_mark(const Flow &flow, ChState &s, int64_t step, unsigned planes, unsigned plane_cells, lbmpm::DeviceBlocks &mem, hipStream_t stream)
{
    const size_t cells = (size_t)planes * plane_cells;
    if (!s.snap) { const int rc = mem.alloc(&s.snap, 4 * cells, nullptr); if (rc) return rc; }
    { const int rc = integral_buffer<ChangeCols>(mem, &s.buf, planes, plane_cells, 1, nullptr); if (rc) return rc; }
    s.valid = false;
    const ChangeLoader<Flow, false, true> load{flow, s.snap, cells, plane_cells};
    change_partial<Flow, false, true><<<dim3(integral_chunks(plane_cells), planes), dim3(INTEGRAL_THREADS), 0, stream>>>(load, plane_cells, s.buf);
    LBMPM_HIP_TRY(hipGetLastError());
    s.valid = true;
    s.at_step = step;
    return LBMPM_OK;
}

// The body of the lbmpm_*_change entry points (`who`) behind their own checks: the table against the snapshot, the snapshot replaced in the
// same pass with remark.  One synchronisation, planes * 88 bytes; host_out: [planes][11]
template <typename Flow>
int change_run(const char *who, const Flow &flow, ChState &s, int remark, int64_t step, int64_t *steps_between, unsigned planes, unsigned plane_cells,
               double *host_out, hipStream_t stream)
{
    if (!s.valid || !s.snap) {
        set_error("%s: no snapshot to compare with (call the model's change_mark first; set_density / set_macro / set_pdf / set_state void it)", who);
        return LBMPM_ERR_STATE;
    }
    const size_t cells = (size_t)planes * plane_cells;
    const unsigned nchunk = integral_chunks(plane_cells);
    double *table = integral_table<ChangeCols>(s.buf, planes, plane_cells);
    if (remark) {
        const ChangeLoader<Flow, true, true> load{flow, s.snap, cells, plane_cells};
        change_partial<Flow, true, true><<<dim3(nchunk, planes), dim3(INTEGRAL_THREADS), 0, stream>>>(load, plane_cells, s.buf);
    } else {
        const ChangeLoader<Flow, true, false> load{flow, s.snap, cells, plane_cells};
        change_partial<Flow, true, false><<<dim3(nchunk, planes), dim3(INTEGRAL_THREADS), 0, stream>>>(load, plane_cells, s.buf);
    }
    change_final<<<dim3(planes), dim3(64), 0, stream>>>(s.buf, nchunk, table);
    const hipError_t e = integrals_download<ChangeCols>(table, planes, 1, host_out, stream);
    if (e != hipSuccess) { s.valid = false; LBMPM_HIP_TRY(e); }       // (a pass that may have half replaced the snapshot)
    if (steps_between) *steps_between = step - s.at_step;
    if (remark) s.at_step = step;
    return LBMPM_OK;
}
