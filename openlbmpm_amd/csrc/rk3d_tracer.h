// rk3d_tracer.h -- D3Q7 tracer transport coupled to the D3Q19 CSF colour-gradient flow (included by rk3d_csf.hip inside its unnamed
// namespace: the kernels use its CsfDev, its block order and its cell numbering).
//
// The reference couples tracers to its 2-D CSF loop only (RKCG2D/Transport2DRK.py:1341-1418, kernels of AccelerateTransport2DRK.py = "T:",
// restated in oracle/tr_oracle.c::tr_substep); this is that sub-step carried to three dimensions statement by statement:
//   lattice        rest, +x, -x, +y, -y, +z, -z (the flow's directions 0 .. 6), weights 0, 1/6 x 6: c_s^2 = 1/3.  On a lattice uniform in y
//                  it projects onto the reference's D2Q5 (1/3, 1/6 x 4) with g0 + g(+y) + g(-y) as the rest population
//   indicator      T:957-970   rhoR > criteria_rho
//   collision      T:535-590   g += -M^-1 S^-1 (M g - M g_eq), g_eq = C w_i (1 + 3 e_i.u).  Moments C, j_x, j_y, j_z, 6 g0 - sum(others),
//                  xx - zz, xx + zz - 2 yy (rows mutually orthogonal); rates 1 except the flux block S = 1/2 I + 3 D.  With rate 1 every
//                  moment but the flux lands on its equilibrium, so  g_i <- g_eq,i + 1/2 e_i . (I - S^-1)(j - j_eq):  nine numbers per tracer
//   interface      T:976-1013  g_i += beta ind w_i C cos(e_i, -G / |G|), the reference's 1e-8 switches
//   reaction       T:95-111    A + B -> C between tracers 0, 1, 2, source k C_0 C_1 spread with J0', (1 - J0') / 6 x 6
//   free outlet    T:461-478   plane 0 <- plane 1, all seven populations (after the collision)
//   streaming      T:139-194   half-way bounce-back on solids; as a PULL of the post-collision populations, like the flow's
//   inlet          T:682-698   Inamuro on plane nz-1: the population moving down is C_in - sum(others)
//   concentration  T:78-90
//   wall reaction  (not in the reference; lbmpm_rk3dcsf_tracer_set_wall_reaction, include/lbmpm.h) the linear surface reaction
//                  D dC/dn = k C_wall as a reactive bounce-back: the population that comes back off a solid is r times the one that
//                  left, r = (1 - 3 k) / (1 + 3 k) per tracer and mineral class of that solid.  Kernels with WALL = false are the ones
//                  a context without a wall reaction launches
// Stored: the post-collision populations, SoA [tracer][7][FS] over fluid cells like the flow's planes, two buffers.  tr3d_step pulls
// (streaming + inlet + concentration: the end of sub-step k - 1) and collides with rhoR, u, G of flow step k (the start of sub-step k).
// Slabs (a context with ghost planes, SLAB): the outlet and the inlet are planes of the UNDIVIDED lattice (z + zoff), the ghost planes'
// cells are received, not computed.  Of all a cell pulls, one population per tracer comes from beyond a z-face: direction 5 (+z) out of
// the first ghost plane below, 6 (-z) out of the one above (tr3d_setup_src / csf3d_setup_src number the ghost cell, SRC_WALL where it is
// solid: half-way bounce-back across a cut).  Those runs travel inside LBMPM_CSF_MSG_PDF (face_runs in rk3d_csf.hip).
// rhoR and u of the step are what csf3d_collide / csf3d_collide_deep<TR = true> leave in `flow` [4][FS]; G is the flow's own array
// (zeros in the deep blocks).  14 doubles per tracer + 7 (rhoR, u, G) + 6 source numbers read, + the 4 doubles the collision wrote.

struct TrDev {
    int nT, inlet, outlet, reaction;
    const double *gin;
    double *gout;
    const double *flow;          // [4][FS] rhoR, vx, vy, vz of this flow step, per fluid cell
    const uint32_t *src;         // [6][FS] the fluid cell x - e_i, SRC_WALL off a solid (the first six planes of CsfDev::src)
    double crit, rate;
    double B[4][9];              // I - S^-1 of every tracer, row-major over (x, y, z)
    double beta[4], cin[4], j0[4];
    // wall reaction: read by the WALL instances and by the uptake reduction (rk3d_tracer_wall.h) only
    double r[4][8];              // [tracer][mineral class] (1 - 3 k) / (1 + 3 k); ones without a wall reaction
    const uint32_t *wcls;        // [FS] nibble i - 1: the class of the solid at x - e_i (0 off a solid); null: every solid is class 0
};

constexpr int TQ = 7;
constexpr double TW = 1. / 6.;

// the populations of one tracer at fluid cell js as a completed sub-step leaves them: streamed (FIRST: taken where they stand), inlet plane
// the class word of fluid cell js (WALL only; one load per cell, shared by its tracers)
__device__ __forceinline__ uint32_t tr_wall_word(const TrDev &t, unsigned js) { return t.wcls ? t.wcls[js] : 0u; }
__device__ __forceinline__ double tr_wall_r(const TrDev &t, int tr, uint32_t word, int i) { return t.r[tr][(word >> (4 * (i - 1))) & 7u]; }

template <bool FIRST, bool WALL = false>
__device__ __forceinline__ void tr_pull(const CsfDev &p, const TrDev &t, int tr, unsigned js, const unsigned s[TQ], bool top, double g[TQ], uint32_t word = 0u)
{
    constexpr int OPP[Q] = CSF_OPP;
    const double *gt = t.gin + (size_t)tr * TQ * p.FS;
    g[0] = gt[js];
#pragma unroll
    for (int i = 1; i < TQ; ++i) {
        size_t off = (size_t)i * p.FS + js;
        if (!FIRST) off = s[i] != SRC_WALL ? (size_t)i * p.FS + s[i] : (size_t)OPP[i] * p.FS + js;
        g[i] = gt[off];
        if (!FIRST && WALL && s[i] == SRC_WALL) g[i] = tr_wall_r(t, tr, word, i) * g[i];      // (k = 0: r = 1.0, the product is exact)
    }
    if (!FIRST && top && t.inlet) {              // T:682-698
        const double sum = g[0] + g[1] + g[2] + g[3] + g[4] + g[5];
        const double u = (t.cin[tr] - sum) / TW;
        g[6] = TW * u;
    }
}
__device__ __forceinline__ double tr_sum(const double g[TQ])
{
    double c = 0.;
#pragma unroll
    for (int i = 0; i < TQ; ++i) c += g[i];
    return c;
}
template <bool FIRST>
__device__ __forceinline__ void tr_sources(const CsfDev &p, const TrDev &t, unsigned js, unsigned s[TQ])
{
    s[0] = js;
#pragma unroll
    for (int i = 1; i < TQ; ++i) s[i] = FIRST ? js : t.src[(size_t)(i - 1) * p.FS + js];
}

template <bool FIRST, int NT, bool SLAB, bool WALL>
__global__ __launch_bounds__(256) void tr3d_step(CsfDev p, TrDev t)
{
    constexpr int CX[Q] = CSF_CX, CY[Q] = CSF_CY, CZ[Q] = CSF_CZ;
    const unsigned j = block_of() * 256u + threadIdx.x;
    if (j >= p.NF) return;
    const unsigned n = p.cells[j], pl = (unsigned)p.nx * (unsigned)p.ny;
    const unsigned z = n / pl;
    if (SLAB && ((int)z < p.glo || (int)z >= p.nz - p.ghi)) return;   // (an image of the neighbour's cell: its populations arrive with the face message)
    const int zg = SLAB ? (int)z + p.zoff : (int)z, nzg = SLAB ? p.nzg : p.nz;        // the plane of the undivided lattice
    unsigned js = j, ns = n;
    if (t.outlet && zg == 0) { ns = n + pl; js = p.cidx[ns]; }       // T:461-478: plane 0 holds what plane 1's cell computes (same mask)
    const bool top = zg == nzg - 1;
    unsigned s[TQ];
    tr_sources<FIRST>(p, t, js, s);
    double g[NT][TQ], C[NT];
    const uint32_t word = WALL ? tr_wall_word(t, js) : 0u;
#pragma unroll
    for (int tr = 0; tr < NT; ++tr) { tr_pull<FIRST, WALL>(p, t, tr, js, s, top, g[tr], word); C[tr] = tr_sum(g[tr]); }
    const double rhoR = t.flow[js], vx = t.flow[p.FS + js], vy = t.flow[2 * p.FS + js], vz = t.flow[3 * p.FS + js];
    const double gx = p.G[ns], gy = p.G[p.NS + ns], gz = p.G[2 * p.NS + ns];
    const double ind = rhoR > t.crit ? -(1. - 1.) : -(1. - 0.);
    const double gn = sqrt(gx * gx + gy * gy + gz * gz);
    double ux = 0., uy = 0., uz = 0., un = 0.;
    if (gn > 1.0e-8) { ux = -gx / gn; uy = -gy / gn; uz = -gz / gn; un = sqrt(ux * ux + uy * uy + uz * uz); }
    double react = 0.;
    if (NT == 3 && t.reaction) react = t.rate * C[0] * C[1];
#pragma unroll
    for (int tr = 0; tr < NT; ++tr) {
        double eq[TQ];
        eq[0] = 0.;
#pragma unroll
        for (int i = 1; i < TQ; ++i) eq[i] = C[tr] * TW * (1. + 3. * edotv(CX[i], CY[i], CZ[i], vx, vy, vz));
        const double jx = (g[tr][1] - g[tr][2]) - (eq[1] - eq[2]), jy = (g[tr][3] - g[tr][4]) - (eq[3] - eq[4]), jz = (g[tr][5] - g[tr][6]) - (eq[5] - eq[6]);
        const double *B = t.B[tr];
        const double hx = 0.5 * (B[0] * jx + B[1] * jy + B[2] * jz), hy = 0.5 * (B[3] * jx + B[4] * jy + B[5] * jz), hz = 0.5 * (B[6] * jx + B[7] * jy + B[8] * jz);
        double o[TQ];
        o[0] = 0.;
#pragma unroll
        for (int i = 1; i < TQ; ++i) o[i] = eq[i] + edotv(CX[i], CY[i], CZ[i], hx, hy, hz);
#pragma unroll
        for (int i = 1; i < TQ; ++i) {           // T:976-1013 (|e_i| = 1)
            double c = 0.;
            if (un > 1.0e-8) c = edotv(CX[i], CY[i], CZ[i], ux, uy, uz) / un;
            o[i] = o[i] + t.beta[tr] * ind * (TW * C[tr]) * c;
        }
        if (NT == 3 && t.reaction) {             // T:95-111
            const double S = tr == 2 ? react : -react, jm = (1. - t.j0[tr]) / 6.;
            o[0] = o[0] + t.j0[tr] * S;
#pragma unroll
            for (int i = 1; i < TQ; ++i) o[i] = o[i] + jm * S;
        }
        double *out = t.gout + (size_t)tr * TQ * p.FS + j;
#pragma unroll
        for (int i = 0; i < TQ; ++i) __builtin_nontemporal_store(o[i], out + (size_t)i * p.FS);
    }
}

// what the reference's arrays hold after the last completed sub-step (the pull, the inlet plane, the sum), dense: out_g [N][7] (may be
// null), out_c [N]; zeros off the fluid
template <bool FIRST, bool WALL>
__global__ __launch_bounds__(256) void tr3d_observe(CsfDev p, TrDev t, int tr, double *out_g, double *out_c)
{
    const unsigned n = blockIdx.x * 256u + threadIdx.x;
    if (n >= p.N) return;
    double g[TQ] = {0., 0., 0., 0., 0., 0., 0.};
    double c = 0.;
    if (p.meta[n] & 1u) {
        const unsigned j = p.cidx[n], pl = (unsigned)p.nx * (unsigned)p.ny;
        unsigned s[TQ];
        tr_sources<FIRST>(p, t, j, s);
        tr_pull<FIRST, WALL>(p, t, tr, j, s, (int)(n / pl) + p.zoff == p.nzg - 1, g, WALL ? tr_wall_word(t, j) : 0u);      // (the inlet plane of the undivided lattice)
        c = tr_sum(g);
    }
    if (out_g) {
#pragma unroll
        for (int i = 0; i < TQ; ++i) out_g[(size_t)n * TQ + i] = g[i];
    }
    out_c[n] = c;
}

// populations of one tracer from a dense concentration [N] (g_i = C w_i, Transport2DRK.py:399-470) or dense populations [N][7]
__global__ __launch_bounds__(256) void tr3d_import(CsfDev p, double *g, const double *conc, const double *pdf)
{
    const unsigned n = blockIdx.x * 256u + threadIdx.x;
    if (n >= p.N) return;
    if (!(p.meta[n] & 1u)) return;
    const unsigned j = p.cidx[n];
#pragma unroll
    for (int i = 0; i < TQ; ++i) g[(size_t)i * p.FS + j] = conc ? (i == 0 ? 0. : conc[n] * TW) : pdf[(size_t)n * TQ + i];
}

// the table of source cells of the six axis directions (a context without the bulk skip has no CsfDev::src)
__global__ __launch_bounds__(256) void tr3d_setup_src(CsfDev p, uint32_t *src)
{
    constexpr int CX[Q] = CSF_CX, CY[Q] = CSF_CY, CZ[Q] = CSF_CZ, OPP[Q] = CSF_OPP;
    const unsigned j = blockIdx.x * 256u + threadIdx.x;
    if (j >= p.NF) return;
    const unsigned n = p.cells[j];
    int x, y, z;
    cell_of(p, n, x, y, z);
    const Nb nb = make_nb(p, x, y, z);
    const uint32_t m = p.meta[n];
#pragma unroll
    for (int i = 1; i < TQ; ++i)
        src[(size_t)(i - 1) * p.FS + j] = ((m >> OPP[i]) & 1u) ? p.cidx[at(nb, -CX[i], -CY[i], -CZ[i])] : SRC_WALL;
}

// the class words of the wall reaction (TrDev::wcls) from a class byte per lattice cell: nibble i - 1 is the class of the solid the
// direction i would be pulled from, 0 where that neighbour is fluid
__global__ __launch_bounds__(256) void tr3d_setup_wall(CsfDev p, const uint8_t *cls, uint32_t *wcls)
{
    constexpr int CX[Q] = CSF_CX, CY[Q] = CSF_CY, CZ[Q] = CSF_CZ, OPP[Q] = CSF_OPP;
    const unsigned j = blockIdx.x * 256u + threadIdx.x;
    if (j >= p.NF) return;
    const unsigned n = p.cells[j];
    int x, y, z;
    cell_of(p, n, x, y, z);
    const Nb nb = make_nb(p, x, y, z);
    const uint32_t m = p.meta[n];
    uint32_t w = 0u;
#pragma unroll
    for (int i = 1; i < TQ; ++i)
        if (!((m >> OPP[i]) & 1u)) w |= (uint32_t)(cls[at(nb, -CX[i], -CY[i], -CZ[i])] & 7u) << (4 * (i - 1));
    wcls[j] = w;
}
