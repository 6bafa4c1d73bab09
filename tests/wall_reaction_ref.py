"""CPU restatement (NumPy) of the tracers' first-order reaction at solid walls: tests/tr3d_ref.Tracer3DRef with the bounce-back line of
its sub-step changed -- a population that meets a solid comes back times r = (1 - 3 k) / (1 + 3 k), k the surface rate of that tracer
at that solid voxel's mineral class -- and the step's uptake kept.  TEST INFRASTRUCTURE ONLY: the product never imports it.

The reference code has no wall reaction; this is held to Tracer3DRef (rates 0: bit-equal) and to the analytic slit eigenmode
(tests/test_wall_reaction_cpu.py)."""
import math

import numpy as np

from tr3d_ref import E, OPP, W7, Coupled3DRef, Tracer3DRef, _shift


def reflection(k):
    """r of one rate, by the library's expression in double; inf -> -1.0"""
    k = float(k)
    if not k >= 0.0:
        raise ValueError("a wall reaction rate is >= 0 (inf allowed), not %r" % k)
    return -1.0 if math.isinf(k) else (1. - 3. * k) / (1. + 3. * k)


class WallReactionRef(Tracer3DRef):
    """rates: [classes][nT] (or [nT], or a number); minerals: [nz][ny][nx] class of every solid cell (None: all class 0).
    After a sub-step: uptake, wall_c [nT][nz] and links [nz], the sums per plane over the plane's wall links of g_out - g_in,
    3 (g_out + g_in) and 1."""

    def __init__(self, dom, conc0, tracer=None, pdf0=None, rates=0.0, minerals=None):
        super().__init__(dom, conc0, tracer, pdf0=pdf0)
        self.minerals = np.zeros(self.dom.shape, dtype=np.int64) if minerals is None else np.asarray(minerals).astype(np.int64)
        self.set_rates(rates)
        nz = self.dom.shape[0]
        self.links = np.array([sum(int((self.dom & ~self.to_fluid[j])[z].sum()) for j in range(1, 7)) for z in range(nz)], dtype=np.float64)
        self.uptake = np.zeros((self.nT, nz))
        self.wall_c = np.zeros((self.nT, nz))

    def set_rates(self, rates):
        a = np.asarray(rates, dtype=np.float64)
        a = np.full((1, self.nT), float(a)) if a.ndim == 0 else a.reshape(-1, self.nT)
        self.rates = a
        rtab = np.array([[reflection(a[m, k]) for m in range(a.shape[0])] for k in range(self.nT)])       # [nT][classes]
        if int(self.minerals[~self.dom].max(initial=0)) >= a.shape[0]:
            raise ValueError("a solid cell of class %d, %d classes given" % (int(self.minerals[~self.dom].max()), a.shape[0]))
        cls = np.where(self.dom, 0, self.minerals)
        # r_link[k][j] at cell n: r of the solid at n + e_j (1 where that neighbour is fluid: never read)
        self.r_link = [[rtab[k][_shift(cls, -E[j])] for j in range(7)] for k in range(self.nT)]
        return self

    def substep(self, rhoR, vx, vy, vz, Gx, Gy, Gz):
        t, dom, g, C_ = self.t, self.dom, self.g, self.C
        ind = np.where(rhoR > t["crit"], -(1. - 1.), -(1. - 0.))
        v = (vx, vy, vz)
        for k in range(self.nT):
            eq = np.array([C_[k] * W7[j] * (1. + 3. * (E[j, 0] * v[0] + E[j, 1] * v[1] + E[j, 2] * v[2])) for j in range(7)])
            diff = np.einsum("jk,k...->j...", self.M, g[k]) - np.einsum("jk,k...->j...", self.M, eq)
            g[k] = g[k] + np.einsum("jk,k...->j...", self.A[k], diff)
        gn = np.sqrt(Gx * Gx + Gy * Gy + Gz * Gz)
        on = gn > 1.0e-8
        safe = np.where(on, gn, 1.)
        ux, uy, uz = np.where(on, -Gx / safe, 0.), np.where(on, -Gy / safe, 0.), np.where(on, -Gz / safe, 0.)
        un = np.where(on, np.sqrt(ux * ux + uy * uy + uz * uz), 0.)
        uns = np.where(un > 1.0e-8, un, 1.)
        for k in range(self.nT):
            for j in range(1, 7):
                c = np.where(un > 1.0e-8, (E[j, 0] * ux + E[j, 1] * uy + E[j, 2] * uz) / (1. * uns), 0.)
                g[k, j] = g[k, j] + self.beta[k] * ind * (W7[j] * C_[k]) * c
        if t["reaction_rate"]:
            r = t["reaction_rate"] * C_[0] * C_[1]
            for k, S in enumerate((-r, -r, r)):
                for j in range(7):
                    g[k, j] = g[k, j] + self.J[k, j] * S
        g *= dom
        if t["free_outlet"]:
            g[:, :, 0] = np.where(dom[0], g[:, :, 1], 0.)
        new = np.zeros_like(g)
        new[:, 0] = g[:, 0]
        self.uptake = np.zeros_like(self.uptake)
        self.wall_c = np.zeros_like(self.wall_c)
        for j in range(1, 7):
            new[:, j] += _shift(np.where(self.to_fluid[j], g[:, j], 0.), E[j])
            for k in range(self.nT):                                                   # the line that differs from Tracer3DRef
                out = np.where(dom & ~self.to_fluid[j], g[k, j], 0.)
                back = self.r_link[k][j] * out
                new[k, OPP[j]] += back
                self.uptake[k] += (out - back).sum(axis=(1, 2))
                self.wall_c[k] += (3. * (out + back)).sum(axis=(1, 2))
        g = new
        if t["dirichlet_inlet"]:
            top = g[:, :, -1]
            s = top[:, 0] + top[:, 1] + top[:, 2] + top[:, 3] + top[:, 4] + top[:, 5]
            for k in range(self.nT):
                u = (self.cb[k] - s[k]) / W7[6]
                top[k, 6] = np.where(dom[-1], W7[6] * u, 0.)
        self.g = g
        self.C = self._conc()
        return self

    def table(self):
        """[nz][nT][4] in the columns of integrals.TracerWallIntegrals (no non-finite cells here)"""
        nz = self.dom.shape[0]
        t = np.zeros((nz, self.nT, 4))
        t[:, :, 0] = self.links[:, None]
        t[:, :, 1] = self.uptake.T
        t[:, :, 2] = self.wall_c.T
        return t

    def mass(self):
        return self.C.reshape(self.nT, -1).sum(axis=1)


def coupled(dom, conc0, tracer, flow, rates, minerals=None, **kw):
    """tr3d_ref.Coupled3DRef whose tracer sub-step is WallReactionRef's"""
    c = Coupled3DRef(dom, conc0=conc0, tracer=tracer, flow=flow, **kw)
    c.tr = WallReactionRef(dom, conc0, tracer, rates=rates, minerals=minerals)
    return c


# ---- the slit: H fluid cells along x between two reactive plates, fluid at rest, the first even eigenmode
def slit_lambda(k, D, H):
    """the first root of lambda tan(lambda H / 2) = k / D in (0, pi / H]"""
    if math.isinf(k):
        return math.pi / H
    lo, hi = 0.0, math.pi / H
    f = lambda x: x * math.tan(x * H / 2.) - k / D
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if f(mid) > 0. or mid * H / 2. >= math.pi / 2.:
            hi = mid
        else:
            lo = mid
    return 0.5 * (lo + hi)


def slit_case(k, D, H=16, nz=4, ny=3):
    """dom [nz][ny][H + 2] with plates at x = 0 and x = H + 1 (the walls sit half-way: x = 1/2 and H + 1/2), the eigenmode's
    concentration, the tracer dict and lambda"""
    dom = np.ones((nz, ny, H + 2), dtype=np.uint8)
    dom[:, :, 0] = 0; dom[:, :, -1] = 0
    lam = slit_lambda(k, D, H)
    x = np.arange(H + 2) - (H + 1) / 2.
    prof = np.cos(lam * x)
    conc = np.broadcast_to(prof, dom.shape) * dom
    tracer = dict(diffX=(D,), beta=(0.,), inlet_conc=(0.,), free_outlet=False, dirichlet_inlet=False)
    return dom, np.ascontiguousarray(conc), tracer, lam, prof[1:-1]


def slit_deviations(mass200, mass400, profile400, D, lam, mode):
    """(relative deviation of the decay rate between steps 200 and 400 from D lambda^2, largest deviation of the profile from the
    eigenmode, both normalised to their largest value)"""
    rate = math.log(mass200 / mass400) / 200.
    return abs(rate / (D * lam * lam) - 1.), float(np.max(np.abs(profile400 / profile400.max() - mode / mode.max())))
