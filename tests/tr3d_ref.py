"""CPU restatement (NumPy) of the D3Q7 tracer sub-step coupled to the D3Q19 CSF flow: the reference's sub-step
(Transport2DRK.py:1341-1418 = oracle/tr_oracle.c::tr_substep) carried to three dimensions statement by statement, with the dense 7 x 7
matrices the reference builds on the host (Transport2DRK.py:313-347).  TEST INFRASTRUCTURE ONLY: the product never imports it.

Pinned by reduction (tests/test_tr3d_ref.py): on a lattice uniform in y it equals oracle/tr_oracle.c, which is pinned to captures of
the real driver.  Arrays are dense [nz][ny][nx]; populations [nT][7][nz][ny][nx] in the order rest, +x, -x, +y, -y, +z, -z."""
import ctypes as C

import numpy as np

E = np.array([(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)])     # (ex, ey, ez)
OPP = (0, 2, 1, 4, 3, 6, 5)
W7 = np.array([0.] + [1. / 6.] * 6)
F64P = C.POINTER(C.c_double)

DEFAULT_TRACER3D = dict(diffX=(1. / 6.,), diffY=None, diffZ=None, dXY=0., dYX=0., dXZ=0., dZX=0., dYZ=0., dZY=0., beta=(1.0,), crit=0.5,
                        inlet_conc=(1.0,), free_outlet=True, dirichlet_inlet=True, reaction_rate=0.0, diffJ=None)


def tracer_matrices3d(t):
    """M (rows C, jx, jy, jz, 6 g0 - sum, xx - zz, xx + zz - 2 yy) and A[i] = -M^-1 S^-1, S = 1 except the flux block 1/2 I + 3 D"""
    ex, ey, ez = E[:, 0].astype(float), E[:, 1].astype(float), E[:, 2].astype(float)
    M = np.array([np.ones(7), ex, ey, ez, np.array([6.] + [-1.] * 6), ex * ex - ez * ez, ex * ex + ez * ez - 2. * ey * ey])
    Minv = np.linalg.inv(M)
    nT = len(t["diffX"])
    dy = t["diffY"] or t["diffX"]
    dz = t["diffZ"] or t["diffX"]
    A = np.zeros((nT, 7, 7))
    for i in range(nT):
        D = np.array([[t["diffX"][i], t["dXY"], t["dXZ"]], [t["dYX"], dy[i], t["dYZ"]], [t["dZX"], t["dZY"], dz[i]]])
        S = np.eye(7)
        S[1:4, 1:4] = 0.5 * np.eye(3) + 3. * D
        A[i] = -Minv @ np.linalg.inv(S)
    return M, A


def _shift(a, e):
    """a[n - e] at n: what arrives from the cell behind (periodic, like the reference's neighbour tables)"""
    return np.roll(a, (int(e[2]), int(e[1]), int(e[0])), axis=(-3, -2, -1))


class Tracer3DRef:
    def __init__(self, dom, conc0, tracer=None, pdf0=None, seam_wall=False):
        """seam_wall = True: nothing is pulled across the seam between plane nz-1 and plane 0; the populations that would cross it bounce
        back there (a negative control: a tracer step that forgot to wrap z)"""
        t = dict(DEFAULT_TRACER3D); t.update(tracer or {})
        self.t = t
        self.dom = np.asarray(dom) == 1
        self.nT = len(t["diffX"])
        self.M, self.A = tracer_matrices3d(t)
        self.beta = np.asarray(t["beta"], dtype=np.float64); self.cb = np.asarray(t["inlet_conc"], dtype=np.float64)
        if t["reaction_rate"] and self.nT != 3:
            raise ValueError("the reaction couples exactly three tracers")
        dj = t["diffJ"] or (0.,) * self.nT          # J0' on this lattice
        self.J = np.array([[dj[i]] + [(1. - dj[i]) / 6.] * 6 for i in range(self.nT)])
        if pdf0 is not None:
            self.g = np.array(pdf0, dtype=np.float64)
        else:
            c = np.asarray(conc0, dtype=np.float64).reshape((self.nT,) + self.dom.shape)
            self.g = c[:, None] * W7[None, :, None, None, None]
        self.g = self.g * self.dom
        self.C = self._conc()
        # where the neighbour in direction i is fluid
        self.to_fluid = [self.dom & _shift(self.dom, -E[i]) for i in range(7)]
        if seam_wall:
            self.to_fluid[5][-1] = False; self.to_fluid[6][0] = False

    def _conc(self):
        c = np.zeros((self.nT,) + self.dom.shape)
        for j in range(7):                         # T:78-90, in order
            c = c + self.g[:, j]
        return c

    def substep(self, rhoR, vx, vy, vz, Gx, Gy, Gz):
        t, dom, g, C_ = self.t, self.dom, self.g, self.C
        ind = np.where(rhoR > t["crit"], -(1. - 1.), -(1. - 0.))                      # T:957-970
        v = (vx, vy, vz)
        for k in range(self.nT):                                                       # T:535-590
            eq = np.array([C_[k] * W7[j] * (1. + 3. * (E[j, 0] * v[0] + E[j, 1] * v[1] + E[j, 2] * v[2])) for j in range(7)])
            diff = np.einsum("jk,k...->j...", self.M, g[k]) - np.einsum("jk,k...->j...", self.M, eq)
            g[k] = g[k] + np.einsum("jk,k...->j...", self.A[k], diff)
        gn = np.sqrt(Gx * Gx + Gy * Gy + Gz * Gz)                                      # T:976-1013
        on = gn > 1.0e-8
        safe = np.where(on, gn, 1.)
        ux, uy, uz = np.where(on, -Gx / safe, 0.), np.where(on, -Gy / safe, 0.), np.where(on, -Gz / safe, 0.)
        un = np.where(on, np.sqrt(ux * ux + uy * uy + uz * uz), 0.)
        uns = np.where(un > 1.0e-8, un, 1.)
        for k in range(self.nT):
            for j in range(1, 7):
                c = np.where(un > 1.0e-8, (E[j, 0] * ux + E[j, 1] * uy + E[j, 2] * uz) / (1. * uns), 0.)
                g[k, j] = g[k, j] + self.beta[k] * ind * (W7[j] * C_[k]) * c
        if t["reaction_rate"]:                                                         # T:95-111
            r = t["reaction_rate"] * C_[0] * C_[1]
            for k, S in enumerate((-r, -r, r)):
                for j in range(7):
                    g[k, j] = g[k, j] + self.J[k, j] * S
        g *= dom
        if t["free_outlet"]:                                                           # T:461-478
            g[:, :, 0] = np.where(dom[0], g[:, :, 1], 0.)
        new = np.zeros_like(g)                                                         # T:139-194
        new[:, 0] = g[:, 0]
        for j in range(1, 7):
            new[:, j] += _shift(np.where(self.to_fluid[j], g[:, j], 0.), E[j])
            new[:, OPP[j]] += np.where(dom & ~self.to_fluid[j], g[:, j], 0.)
        g = new
        if t["dirichlet_inlet"]:                                                       # T:682-698
            top = g[:, :, -1]
            s = top[:, 0] + top[:, 1] + top[:, 2] + top[:, 3] + top[:, 4] + top[:, 5]
            for k in range(self.nT):
                u = (self.cb[k] - s[k]) / W7[6]
                top[k, 6] = np.where(dom[-1], W7[6] * u, 0.)
        self.g = g
        self.C = self._conc()
        return self


class Coupled3DRef:
    """A flow reference with the restated tracer sub-step spliced between the two halves of its step (after the wetting-corrected colour
    gradient, before the CSF force); after_b = True: spliced after the second half instead (the negative control).
    The flow is oracle/rk3d_csf_oracle.c's (rhoR0, rhoB0, flow_params), or `flow`: a tests/body_force_ref.BodyForceRef or a
    tests/periodic_ref.PeriodicRef made by the caller -- anything with dom, field(name) in the solver's axes and step(hook), which calls
    the hook between its halves with the body force's half in u.  The sub-step runs in the solver's axes either way.
    alter: f(fields, self) -> fields, applied to [rhoR, vx, vy, vz, Gx, Gy, Gz] before the sub-step reads them (negative controls)"""

    def __init__(self, dom, rhoR0=None, rhoB0=None, conc0=None, flow_params=None, tracer=None, flow=None, alter=None, seam_wall=False):
        if flow is None:
            from oracle.rk3dcsf import RK3DCSFOracle
            flow = RK3DCSFOracle(dom, rhoR0, rhoB0, flow_params)
        self.flow = flow
        self.tr = Tracer3DRef(dom, conc0, tracer, seam_wall=seam_wall)
        self.alter = alter
        self.steps = 0

    def _fields(self):
        f = [self.flow.field(n) for n in ("rhoR", "vx", "vy", "vz", "Gx", "Gy", "Gz")]
        return self.alter(f, self) if self.alter else f

    def _substep(self):
        self.tr.substep(*self._fields())

    def run(self, n, after_b=False):
        f = self.flow
        for _ in range(int(n)):
            if hasattr(f, "step"):
                f.step(None if after_b else self._substep)
            else:
                f._L.rk3dcsf_step_a(C.byref(f._s))
                if not after_b:
                    self._substep()
                f._L.rk3dcsf_step_b(C.byref(f._s))
            if after_b:
                self._substep()
            self.steps += 1
        return self

    @property
    def C(self):
        return self.tr.C

    @property
    def g(self):
        return self.tr.g


def project_g(g3):
    """[7][nz][ny][nx] -> the D2Q5 populations [nz][nx][5] of the plane y = 0 (rest = g0 + g(+y) + g(-y); E, W = +-x; N, S = +-z)"""
    return np.stack([g3[0][:, 0] + g3[3][:, 0] + g3[4][:, 0], g3[1][:, 0], g3[2][:, 0], g3[5][:, 0], g3[6][:, 0]], axis=-1)
