"""Reference for the 3-D CSF solver's body force (lbmpm_rk3dcsf_set_body_force), built AROUND the unchanged oracle
(oracle/rk3d_csf_oracle.c): TEST INFRASTRUCTURE ONLY.

The model (include/lbmpm.h): per colour an acceleration g_R, g_B; in every fluid cell F_b = rho_R g_R + rho_B g_B with the densities the
cell has after the step's boundary-plane rules; u = ((sum e f_tot + F_csf / 2) + F_b / 2) / rho; the Guo source takes F_csf + F_b.

The oracle exports the two halves of a step.  Collision, recolouring (f_c = rho_c / rho t + ...) and streaming are linear in the Guo
source, so one body-force step is, exact to rounding:
  1. step_a                                   boundary planes, densities, u with half the CSF force, phi, gradient
  2. u += F_b / (2 rho) at the fluid cells
  3. step_b                                   CSF force, collision and CSF source with that u, recolouring, streaming
  4. f_c += streamed (rho_c / rho) S(u, F_b)  SRT: S_i = w_i (3 e.F + 9 (e.u)(e.F) - 3 u.F)(1 - 1 / 2 tau) with the oracle's tau(phi);
                                              MRT: M^-1 (I - S / 2) M applied to the same bracket; streamed as the oracle streams:
                                              pulled from x - e_i, the cell's own opposite population off a solid
  5. f_tot, rho_R, rho_B rebuilt (in sum19's order)
With g = 0 the steps 2 and 4 add zeros and 5 rebuilds what step_b left: the recipe is then oracle.run (tests/test_body_force_cpu.py).
"""
import ctypes as C

import numpy as np

from oracle.rk3dcsf import RK3DCSFOracle

CX = np.array([0, 1, -1, 0, 0, 0, 0, 1, -1, 1, -1, 1, -1, 1, -1, 0, 0, 0, 0])
CY = np.array([0, 0, 0, 1, -1, 0, 0, 1, -1, -1, 1, 0, 0, 0, 0, 1, -1, 1, -1])
CZ = np.array([0, 0, 0, 0, 0, 1, -1, 0, 0, 0, 0, 1, -1, -1, 1, 1, -1, -1, 1])
OPP = np.array([0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15, 18, 17])
W = np.array([1. / 3.] + [1. / 18.] * 6 + [1. / 36.] * 12)
CRISP = 2.0 ** -51               # the library's "one colour alone" rule (tests/test_rk3d_csf_gpu.py)

# two sets of six pairwise distinct non-zero accelerations, g_R != g_B; lattice units: with rho ~ 1 a step adds g to u, so ten steps stay
# far inside |u| < 0.1 and far above the comparison's 1e-10
G_SETS = {"G1": ((1.0e-5, -2.0e-5, 3.0e-5), (-2.5e-5, 1.5e-5, -6.0e-5)),
          "G2": ((-4.0e-5, 0.5e-5, -1.2e-5), (0.8e-5, 3.5e-5, 2.2e-5))}


def sum19(f):
    """sum over the last axis in the oracle's (and the kernels') order"""
    r = np.zeros(f.shape[:-1])
    for i in range(19):
        r = r + f[..., i]
    return r


class BodyForceRef:
    """RK3DCSFOracle stepped by the recipe above.  field() as the oracle's; `crisp` as tests/test_rk3d_csf_gpu.py passes it"""

    def __init__(self, dom, rhoR0, rhoB0, params=None, g_r=(0., 0., 0.), g_b=(0., 0., 0.), crisp=CRISP, velocity=None):
        self.o = RK3DCSFOracle(dom, rhoR0, rhoB0, dict(params or {}, crisp=crisp), velocity=velocity)
        self.dom = self.o.dom
        self.fl = self.dom == 1
        self.shape = self.o.shape
        self.set_body_force(g_r, g_b)
        self.steps = 0
        self._views = {}
        M = np.zeros((19, 19))
        self.o._L.rk3dcsf_mrt_basis_public(M.ctypes.data_as(C.POINTER(C.c_double)))
        self.M, self.nrm = M, (M * M).sum(axis=1)
        # the cell a population is pulled from is fluid (else: the cell's own opposite population)
        self.from_fluid = np.stack([np.roll(self.dom, (CZ[i], CY[i], CX[i]), axis=(0, 1, 2)) == 1 for i in range(19)], axis=-1)
        self.from_fluid[..., 0] = True

    def set_body_force(self, g_r, g_b):
        self.g_r, self.g_b = np.asarray(g_r, dtype=np.float64), np.asarray(g_b, dtype=np.float64)

    W_ = property(lambda self: self.o.W)

    def field(self, name):
        return self.o.field(name)

    def _view(self, name):
        """the oracle's array behind `name` as it stands now (the populations swap buffers inside the C struct), writable"""
        ptr = getattr(self.o._s, name)
        key = C.addressof(ptr.contents)          # (np.ctypeslib.as_array builds a ctypes type per call: kept per buffer)
        if key not in self._views:
            n = int(np.prod(self.shape))
            q = 19 if name in ("fR", "fB", "fT") else 1
            self._views[key] = np.ctypeslib.as_array(ptr, shape=(n * q,)).reshape(self.shape + ((19,) if q == 19 else ()))
        return self._views[key]

    def _tau(self, phi, rR, rB):
        """tau(phi) of oracle/rk3d_csf_oracle.c (A:1815-1827)"""
        p = self.o.p
        tR, tB, delta = p["tauR"], p["tauB"], p["delta"]
        with np.errstate(divide="ignore", invalid="ignore"):
            if int(p["tautype"]) == 1:
                mid = 0.5 + 1. / ((1. + phi) / (2. * (tR - 0.5)) + (1. - phi) / (2. * (tB - 0.5)))
            else:
                ratioR, ratioB = rR / (rR + rB), rB / (rR + rB)
                mid = 3. * (1. / (ratioR * (3. / (tR - 0.5)) + ratioB * (3. / (tB - 0.5)))) + 0.5
        return np.where(phi > delta, tR, np.where(phi < -delta, tB, mid))

    def body_force_density(self):
        """F_b [3][nz][ny][nx] from the oracle's densities as they stand (after step_a: those of the step)"""
        rR, rB = self._view("rhoR"), self._view("rhoB")
        return [np.where(self.fl, rR * self.g_r[a] + rB * self.g_b[a], 0.0) for a in range(3)]

    def step_a(self):
        """the first half with the body force's share of u: what the solver records (rec_*)"""
        self.o.step_a()
        Fb = self.body_force_density()
        rho = self._view("rhoB") + self._view("rhoR")
        for a, c in enumerate(("vx", "vy", "vz")):
            v = self._view(c)
            v[self.fl] = v[self.fl] + 0.5 * Fb[a][self.fl] / rho[self.fl]
        return Fb

    def step(self, hook=None):
        """hook: called once, between the two halves -- after step_a() has put the force's half into u, before rk3dcsf_step_b: the
        moment the solver's tracer sub-step reads rho_R, u and G (tests/tr3d_ref.py).  It reads; the recipe's bits do not depend on it"""
        fl = self.fl
        Fb = self.step_a()
        if hook is not None:
            hook()
        rR, rB = self._view("rhoR").copy(), self._view("rhoB").copy()
        u = [self._view(c).copy() for c in ("vx", "vy", "vz")]
        phi = self._view("phi").copy()
        self.o._L.rk3dcsf_step_b(C.byref(self.o._s))
        # the Guo bracket of F_b
        uf = u[0] * Fb[0] + u[1] * Fb[1] + u[2] * Fb[2]
        S = np.zeros(self.shape + (19,))
        for i in range(19):
            ef = CX[i] * Fb[0] + CY[i] * Fb[1] + CZ[i] * Fb[2]
            eu = CX[i] * u[0] + CY[i] * u[1] + CZ[i] * u[2]
            S[..., i] = W[i] * (3. * ef + 9. * eu * ef - 3. * uf)
        with np.errstate(divide="ignore", invalid="ignore"):
            tau = np.where(fl, self._tau(phi, rR, rB), 1.0)
        if self.o.p["relax"] == "MRT":
            r = self.o.p["rates"]
            it = 1. / tau
            one = np.ones_like(tau)
            rates = np.stack([r[5] * one, r[0] * one, r[1] * one, r[5] * one, r[2] * one, r[5] * one, r[2] * one, r[5] * one, r[2] * one, it, r[3] * one,
                              it, r[3] * one, it, it, it, r[4] * one, r[4] * one, r[4] * one], axis=-1)
            m = (S @ self.M.T) * (1. - 0.5 * rates) / self.nrm
            S = m @ self.M
        else:
            S = S * (1. - 1. / (2. * tau))[..., None]
        tot = rR + rB
        with np.errstate(divide="ignore", invalid="ignore"):
            shareR, shareB = np.where(fl, rR / tot, 0.0), np.where(fl, rB / tot, 0.0)
        crisp = self.o.p["crisp"]
        if crisp > 0.:           # the oracle's crisp rule: an absent colour hands on zeros, the other one takes f_tot
            noB = np.abs(rB) <= crisp * tot
            noR = ~noB & (np.abs(rR) <= crisp * tot)
            shareR = np.where(noB, 1.0, np.where(noR, 0.0, shareR)); shareB = np.where(noR, 1.0, np.where(noB, 0.0, shareB))
        for name, share in (("fR", shareR), ("fB", shareB)):
            inc = share[..., None] * S * fl[..., None]
            pulled = np.stack([np.roll(inc[..., i], (CZ[i], CY[i], CX[i]), axis=(0, 1, 2)) for i in range(19)], axis=-1)
            streamed = np.where(self.from_fluid, pulled, inc[..., OPP])
            f = self._view(name)
            f[fl] = f[fl] + streamed[fl]
        fR, fB = self._view("fR"), self._view("fB")
        self._view("fT")[fl] = (fR + fB)[fl]
        self._view("rhoR")[fl] = sum19(fR)[fl]
        self._view("rhoB")[fl] = sum19(fB)[fl]
        self.steps += 1
        return self

    def run(self, n, hook=None):
        for _ in range(int(n)):
            self.step(hook)
        return self


# ------------------------------------------------------------------------------------------------ two physics cases
# an 18 x 4 x 12 lattice with walls at x = 0 and x = 17 (half-way bounce-back: the gap is 16 cells wide, its walls at x = 1/2 and 16 1/2)
PHYS_SHAPE = (12, 4, 18)
HYDROSTATIC_STEPS, HYDROSTATIC_DROP_BOUND = 6000, 0.005
POISEUILLE_STEPS, POISEUILLE_BOUND = 8000, 0.02


def _gap():
    dom = np.ones(PHYS_SHAPE, dtype=np.uint8)
    dom[:, :, 0] = dom[:, :, -1] = 0
    return dom, np.mgrid[0:PHYS_SHAPE[0], 0:PHYS_SHAPE[1], 0:PHYS_SHAPE[2]][2]


def hydrostatic_case(layers, relax):
    """a column at rest under g along x between the walls: Neumann inlet with zero velocity, convective outlet.  layers = 1: red alone,
    g_x = 1e-4; 2: red below x = 9, blue from there on, g_Rx = 1e-4, g_Bx = 3e-5, and no surface tension: the interface is flat and parallel
    to the walls, so its tension has no part in the balance (with the default sigma = 0.1 the discrete curvature of the diffuse interface
    shifts the drop by 1.2 - 1.5 %: a property of the CSF force, not of the body force).  (dom, rhoR, rhoB, params, (g_R, g_B))"""
    dom, xx = _gap()
    fl = dom == 1
    par = dict(relax=relax, inlet="Neumann", outlet="Convective", velocityZR=0.0, velocityZB=0.0)
    if layers == 1:
        return dom, np.where(fl, 1.0, 0.0), np.zeros(dom.shape), par, ((1.0e-4, 0.0, 0.0), (0.0, 0.0, 0.0))
    return dom, np.where(fl & (xx < 9), 1.0, 0.0), np.where(fl & (xx >= 9), 1.0, 0.0), dict(par, sigma=0.0), ((1.0e-4, 0.0, 0.0), (3.0e-5, 0.0, 0.0))


def hydrostatic_errors(rho, Fbx, umax):
    """p = rho / 3 balances the force: rho(x + 1) - rho(x) = 3 (F_b(x) + F_b(x + 1)) / 2 between neighbouring cells, and summed over the
    gap rho(16) - rho(1) = 3 (sum_x F_b - (F_b(1) + F_b(16)) / 2).  Taken along x on the middle plane: the open planes let a weak
    circulation through (|u| up to g / 2), which is strongest there -- 0.34 % on that plane, 1e-5 two planes from the outlet.
    (relative error of the drop, the worst one per pair of neighbouring cells, umax)"""
    a, F = rho[rho.shape[0] // 2, 1], Fbx[rho.shape[0] // 2, 1]
    drop = (a[16] - a[1]) / (3. * (F[1:17].sum() - 0.5 * (F[1] + F[16]))) - 1.
    cell = np.diff(a[1:17]) / (1.5 * (F[1:16] + F[2:17])) - 1.
    return abs(float(drop)), float(np.max(np.abs(cell))), umax


def poiseuille_case(relax):
    """force-driven plane Poiseuille flow along z: Dirichlet inlet and outlet at the same densities rho_R = 1, rho_B = 5e-8, g_z = -1e-6 on
    both colours, tau = 1"""
    dom, _ = _gap()
    fl = dom == 1
    par = dict(relax=relax, inlet="Dirichlet", outlet="Dirichlet", densityRH=1.0, densityBH=5.0e-8, densityRL=1.0, densityBL=5.0e-8, tauR=1.0, tauB=1.0,
               velocityZR=0.0, velocityZB=0.0)
    g = (0.0, 0.0, -1.0e-6)
    return dom, np.where(fl, 1.0, 0.0), np.where(fl, 5.0e-8, 0.0), par, (g, g)


def poiseuille_errors(vz):
    """u_z(x) = g / (2 nu) (x - 1/2)(nx - 3/2 - x), nu = (tau - 1/2) / 3 = 1/6, on the middle plane: (worst relative deviation over the
    gap -- at the wall cells --, the one at the two centre cells)"""
    nz, ny, nx = vz.shape
    x = np.arange(1, nx - 1, dtype=np.float64)
    want = -1.0e-6 / (2. * (1. / 6.)) * (x - 0.5) * (nx - 1.5 - x)
    dev = np.abs(vz[nz // 2, 1, 1:nx - 1] / want - 1.)
    return float(dev.max()), float(dev[nx // 2 - 2:nx // 2].max())
