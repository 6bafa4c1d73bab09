"""The 2-D CSF step under a per-colour body force, and on a lattice periodic in y, stated around the unchanged oracle.

oracle/liblbmpm_oracle.so exports every stage of the 2-D loop and oracle.rk.RKOracle keeps its arrays as numpy members, so one forced step
is the stages of rk_csf_step called one by one with two insertions (ForcedOracle.step):

    rk_csf_step_a (tracers: rk_csf_step_a_transport)     boundary rows ... wetting-corrected colour gradient; u with the lagged CSF force
    vx, vy += F_b / (2 rho)                              F_b = rho_R g_R + rho_B g_B, the densities the rows' rules left
    tr_substep                                           tracers only, where oracle.tr.CoupledOracle.run calls it
    rk_force                                             the CSF force of this step (stays the CSF force alone)
    rk_collide_srt | rk_collide_mrt
    rk_force_srt | rk_force_mrt                          with Fx + F_bx, Fy + F_by in place of Fx, Fy
    rk_recolor, rk_stream1 x 2, rk_stream2 x 2, rk_total_pdf, rk_macro_density

With g = 0 this is RKOracle.run / CoupledOracle.run bit for bit (tests/test_rk2d_force_cpu.py).

Periodic y has an exact reference as well: the same recipe on the TRANSPOSED lattice with outlet 'Convective', when the solver's lattice
carries >= 4 solid columns at both ends of x.  The transposed rows 0 .. 3, ny-2, ny-1 then hold no fluid, the oracle's row rules touch
nothing, and its x wrap is the solver's y wrap.  Directions go through the x <-> y exchange EXCH, g and the vector fields swap components,
the tracers' diffX <-> diffY and dXY <-> dYX.  ('Dirichlet' would not do: the ghost-outlet rule picks its nodes by compact index.)
"""
import ctypes as C

import numpy as np

from oracle.rk import RKOracle, F64P, I64P
from oracle.tr import CoupledOracle

EXCH = [0, 2, 1, 4, 3, 5, 8, 7, 6]           # D2Q9 direction i of the solver's lattice = direction EXCH[i] of the transposed one
FLOW_FIELDS = ("fR", "fB", "rhoR", "rhoB", "phi", "vx", "vy", "Gx", "Gy", "Fx", "Fy", "K")
# two acceleration sets (lattice units): every component non-zero, no two equal, the colours' differ
G_SETS = (((1.0e-5, -2.0e-5), (-2.5e-5, 1.5e-5)), ((-3.0e-5, 1.2e-5), (0.8e-5, 2.2e-5)))
_FLOW_KEYS = ("sigma", "theta", "wetting", "beta", "delta", "tauR", "tauB", "tautype", "relax", "inlet", "outlet", "vyR", "vyB", "rhoBH", "rhoRH",
              "rhoBL", "rhoRL")


def _d(a):
    return a.ctypes.data_as(F64P)


def _i(a):
    return a.ctypes.data_as(I64P)


class ForcedOracle:
    """RKOracle (conc=None) or CoupledOracle stepped stage by stage with the body force (gR, gB) = ((gx, gy), (gx, gy)).
    half_in_u=False leaves F_b / 2 out of u -- the mistake the sensitivity test must see."""

    def __init__(self, dom, params, rR, rB, gR=(0., 0.), gB=(0., 0.), conc=None, tracer=None, half_in_u=True):
        flow = {k: v for k, v in (params or {}).items() if k in _FLOW_KEYS}
        if conc is None:
            self.co, self.flow = None, RKOracle(dom, flow, rR, rB)
        else:
            self.co = CoupledOracle(dom, flow, rR, rB, conc, tracer)
            self.flow = self.co.flow
        self.gR, self.gB, self.half_in_u = tuple(map(float, gR)), tuple(map(float, gB)), half_in_u
        self.forced = True

    def set_body_force(self, gR=None, gB=None):
        self.forced = gR is not None
        self.gR, self.gB = (tuple(map(float, gR)), tuple(map(float, gB))) if self.forced else ((0., 0.), (0., 0.))

    def step(self):
        f = self.flow
        L, s, N = f._L, f._s, C.c_int64(f.N)
        (L.rk_csf_step_a_transport if self.co else L.rk_csf_step_a)(C.byref(s))
        Fbx = f.rhoR * self.gR[0] + f.rhoB * self.gB[0]
        Fby = f.rhoR * self.gR[1] + f.rhoB * self.gB[1]
        if self.half_in_u:
            rho = f.rhoB + f.rhoR
            f.vx += Fbx / (2. * rho)           # (in place: the oracle holds pointers to these arrays)
            f.vy += Fby / (2. * rho)
        # what the result file records at the start of a step (rec_* of RK2DSolver.get): after n steps it is the `rec` of step n + 1
        self.rec = dict(fR=f.fR.copy(), fB=f.fB.copy(), rhoR=f.rhoR.copy(), rhoB=f.rhoB.copy(), vx=f.vx.copy(), vy=f.vy.copy())
        if self.co:
            L.tr_substep(C.byref(self.co._s), _d(f.rhoR), _d(f.vx), _d(f.vy), _d(f.Gx), _d(f.Gy))
        L.rk_force(N, C.c_int(s.wettingType), C.c_double(s.sigma), _i(f.nbr), _d(f.Gx), _d(f.Gy), _d(f.Fx), _d(f.Fy), _d(f.K))
        Fx, Fy = np.ascontiguousarray(f.Fx + Fbx), np.ascontiguousarray(f.Fy + Fby)
        tau = (C.c_int(s.tauType), C.c_double(s.tauR), C.c_double(s.tauB), C.c_double(s.delta))
        if not s.mrt:
            L.rk_collide_srt(N, *tau, _d(f.vx), _d(f.vy), _d(f.rhoR), _d(f.rhoB), _d(f.phi), _d(f.fT))
            L.rk_force_srt(N, *tau, _d(f.vx), _d(f.vy), _d(Fx), _d(Fy), _d(f.phi), _d(f.fT), _d(f.rhoR), _d(f.rhoB))
        else:
            L.rk_collide_mrt(N, *tau, _d(f.vx), _d(f.vy), _d(f.rhoR), _d(f.rhoB), _d(f.phi), _d(f.fT), _d(f.M), _d(f.Minv), _d(f.S))
            L.rk_force_mrt(N, *tau, _d(f.vx), _d(f.vy), _d(Fx), _d(Fy), _d(f.phi), _d(f.fT), _d(f.M), _d(f.Minv), _d(f.S), _d(f.rhoR), _d(f.rhoB))
        L.rk_recolor(N, C.c_double(s.beta), _d(f.rhoR), _d(f.rhoB), _d(f.Gx), _d(f.Gy), _d(f.fR), _d(f.fB), _d(f.fT))
        L.rk_stream1(N, _i(f.nbr), _d(f.fR), _d(f.fRn))
        L.rk_stream1(N, _i(f.nbr), _d(f.fB), _d(f.fBn))
        L.rk_stream2(N, _d(f.fRn), _d(f.fR))
        L.rk_stream2(N, _d(f.fBn), _d(f.fB))
        L.rk_total_pdf(N, _d(f.fR), _d(f.fB), _d(f.fT))
        L.rk_macro_density(N, _d(f.fR), _d(f.fB), _d(f.rhoR), _d(f.rhoB))

    def run(self, n):
        for _ in range(int(n)):
            self.step()
        return self

    def fields(self):
        """compact copies of the compared fields (+ K_live, + C0 .. with tracers), as tests/param_points.oracle_run returns them"""
        f = {k: getattr(self.flow, k).copy() for k in FLOW_FIELDS}
        f["K_live"] = np.hypot(f["Gx"], f["Gy"]) > 1e-6
        if self.co:
            f.update({"C%d" % k: self.co.C[k].copy() for k in range(self.co.nT)})
        return f


def forced_run(dom, params, rR, rB, gR, gB, checkpoints, conc=None, tracer=None, **kw):
    """{step: fields} of the forced recipe between open rows"""
    o = ForcedOracle(dom, params, rR, rB, gR, gB, conc, tracer, **kw)
    out, done = {}, 0
    for n in checkpoints:
        o.run(n - done); done = n
        out[n] = o.fields()
    return out


# ------------------------------------------------------------------------------------------------ periodic y by transposition
def exchange_tracer(tracer):
    """the tracer keywords on the transposed lattice: diffX <-> diffY, dXY <-> dYX, both ends off"""
    if tracer is None:
        return None
    t = dict(tracer)
    t["diffX"], t["diffY"] = tracer["diffY"], tracer["diffX"]
    t["dXY"], t["dYX"] = tracer["dYX"], tracer["dXY"]
    t["dirichlet_inlet"], t["free_outlet"] = False, False
    return t


def walls_suffice(dom, n=4):
    return not np.any(np.asarray(dom)[:, :n] == 1) and not np.any(np.asarray(dom)[:, -n:] == 1)


class RingOracle:
    """the forced recipe for the solver's lattice `dom` periodic in y: run on dom.T with the convective outlet (module docstring)"""

    def __init__(self, dom, params, rR, rB, gR=(0., 0.), gB=(0., 0.), conc=None, tracer=None, **kw):
        dom = np.asarray(dom)
        assert walls_suffice(dom), "the transposed reference needs >= 4 solid columns at both ends of x"
        p = {k: v for k, v in (params or {}).items() if k in _FLOW_KEYS}
        p.update(inlet="Neumann", outlet="Convective")
        T = lambda a: np.ascontiguousarray(np.asarray(a).T)
        concT = None if conc is None else np.ascontiguousarray(np.asarray(conc).transpose(0, 2, 1))
        self.shape = dom.shape
        self.sel = dom.reshape(-1) == 1
        self.o = ForcedOracle(T(dom), p, T(rR), T(rB), (gR[1], gR[0]), (gB[1], gB[0]), concT, exchange_tracer(tracer), **kw)

    def run(self, n):
        self.o.run(n)
        return self

    def _back(self, a):
        """a compact field of the transposed oracle as a compact field of the solver's lattice"""
        fl = self.o.flow
        d = np.zeros((fl.ny * fl.nx,) + a.shape[1:])
        d[fl.fluidNodes] = a
        d = d.reshape((fl.ny, fl.nx) + a.shape[1:]).swapaxes(0, 1)
        return np.ascontiguousarray(d).reshape((-1,) + a.shape[1:])[self.sel]

    def rec(self):
        """the record of the step taken last (ForcedOracle.rec), on the solver's lattice"""
        t = self.o.rec
        f = {k: self._back(t[k]) for k in ("rhoR", "rhoB")}
        f["fR"], f["fB"] = self._back(t["fR"])[:, EXCH], self._back(t["fB"])[:, EXCH]
        f["vx"], f["vy"] = self._back(t["vy"]), self._back(t["vx"])
        return f

    def fields(self):
        t = self.o.fields()
        f = {k: self._back(t[k]) for k in ("rhoR", "rhoB", "phi", "K")}
        f["fR"], f["fB"] = self._back(t["fR"])[:, EXCH], self._back(t["fB"])[:, EXCH]
        for a, b in (("vx", "vy"), ("Gx", "Gy"), ("Fx", "Fy")):
            f[a], f[b] = self._back(t[b]), self._back(t[a])
        f["K_live"] = np.hypot(f["Gx"], f["Gy"]) > 1e-6
        f.update({k: self._back(v) for k, v in t.items() if k[0] == "C"})
        return f


def ring_run(dom, params, rR, rB, gR, gB, checkpoints, conc=None, tracer=None, **kw):
    o = RingOracle(dom, params, rR, rB, gR, gB, conc, tracer, **kw)
    out, done = {}, 0
    for n in checkpoints:
        o.run(n - done); done = n
        out[n] = o.fields()
    return out


# ------------------------------------------------------------------------------------------------ lattices of the ring tests
_cache = {}


def ring_lattice(ny, nx=70, wall=4):
    """(dom, rR, rB): a sealed lattice nx wide -- `wall` solid columns at both ends of x -- with discs of radius >= 3, one of them across
    the seam y = 0 / ny-1, and a slanted, rippled interface that crosses the seam twice (red in a band around the lattice's middle,
    2 % of the other colour everywhere)"""
    if (ny, nx, wall) not in _cache:
        dom = np.ones((ny, nx), dtype=np.uint8)
        dom[:, :wall] = 0; dom[:, -wall:] = 0
        yy, xx = np.mgrid[0:ny, 0:nx]
        discs = [(0.0, 0.30 * nx, 3.6), (0.55 * ny, 0.62 * nx, 3.3), (0.30 * ny, 0.80 * nx, 3.0)]
        for cy, cx, r in discs:
            dy = np.minimum(np.abs(yy - cy), ny - np.abs(yy - cy))        # (periodic distance in y: the first disc lies across the seam)
            dom[dy * dy + (xx - cx) * (xx - cx) <= r * r] = 0
        ripple = 1.0 + 1.0e-3 * np.sin(0.37 * xx + 0.11 * yy)
        fluid = dom == 1
        s = yy + 0.12 * xx
        red = (s > 0.22 * ny + 3) & (s < 0.70 * ny + 4)
        # a little of the other colour in every node, varying: the phase field of a pure node is +-1 whatever its density, a colour
        # gradient built from +-1 alone meets the wetting rules' ties exactly (both candidates equally far), and the branch then hangs on
        # the order of a sum -- the GPU's, the oracle's and the transposed oracle's differ
        other = 0.02 * (1.0 + 0.5 * np.sin(0.23 * xx - 0.41 * yy))
        _cache[(ny, nx, wall)] = (dom, np.where(fluid, np.where(red, ripple, other), 0.0), np.where(fluid, np.where(red, other, ripple), 0.0))
    return _cache[(ny, nx, wall)]


def two_layer_profile(H, rho, nuR, nuB, gR, gB, h):
    """u_y(x) of two layers between walls at x = 0 and x = H (half-way: the fluid nodes sit at x = 1/2 ... H - 1/2): layer R of kinematic
    viscosity nuR and acceleration gR on 0 < x < h, layer B on h < x < H, equal density rho; u and the shear stress rho nu u' continuous
    at h, no slip at both walls.  Returns a function of x."""
    # u_R = -gR x^2 / (2 nuR) + a x ; u_B = -gB (H - x)^2 / (2 nuB) + b (H - x) ; stress: nuR u_R'(h) = nuB u_B'(h)
    hb = H - h
    A = np.array([[h, -hb], [nuR, nuB]])
    r = np.array([gR * h * h / (2. * nuR) - gB * hb * hb / (2. * nuB), gR * h + gB * hb])
    a, b = np.linalg.solve(A, r)
    return lambda x: np.where(x < h, -gR * x * x / (2. * nuR) + a * x, -gB * (H - x) ** 2 / (2. * nuB) + b * (H - x))


# The two-layer force-driven flow on a ring: a gap of 32 nodes between walls 4 thick (the transposed reference wants four), lattice
# 40 x 8 periodic in y, red on the 16 nodes next to the lower wall, blue on the other 16, each colour with a relaxation time and an
# acceleration along y of its own; theta = 90 keeps the interface flat.  rec_vy across the gap against two_layer_profile (half-way
# walls at s = 0 and s = 32, s = x - 7/2), as the worst deviation in shares of the analytic peak.  The CPU reference (RingOracle, its
# record view, the same 16 000 steps) shows 1.278 % for MRT and 1.319 % for SRT (1.26 % / 1.30 % after 8000 steps: the profile has
# settled; the deviation sits at the interface, where the relaxation time changes over the interface's width and the profile's kink is
# smeared).  tests/test_rk2d_force_cpu.py re-measures the SRT figure.  The GPU bound is 1.5 times the larger, for a state one step off.
TWO_LAYER = dict(gap=32, wall=4, ny=8, steps=16000, gR=(0., 1.0e-6), gB=(0., 2.0e-6),
                 params=dict(tauR=1.0, tauB=0.7, sigma=0.05, theta=90.0, ring=True))        # (ring: the GPU test's periodic_y=True)
TWO_LAYER_REFERENCE = dict(MRT=1.278e-2, SRT=1.319e-2)
TWO_LAYER_BOUND = 1.5 * 1.319e-2


def two_layer_lattice():
    t = TWO_LAYER
    nx = t["gap"] + 2 * t["wall"]
    dom = np.ones((t["ny"], nx), dtype=np.uint8)
    dom[:, :t["wall"]] = 0; dom[:, -t["wall"]:] = 0
    x = np.mgrid[0:t["ny"], 0:nx][1]
    fl = dom == 1
    red = x < t["wall"] + t["gap"] // 2
    return dom, np.where(fl & red, 1.0, 0.0), np.where(fl & ~red, 1.0, 0.0)


def two_layer_error(vy_row):
    """vy_row: u_y of the 32 nodes across the gap; its worst deviation from the analytic profile in shares of the analytic peak"""
    t = TWO_LAYER
    nuR, nuB = (t["params"]["tauR"] - 0.5) / 3., (t["params"]["tauB"] - 0.5) / 3.
    u = two_layer_profile(float(t["gap"]), 1.0, nuR, nuB, t["gR"][1], t["gB"][1], t["gap"] / 2.)
    peak = float(np.max(u(np.linspace(0., t["gap"], 6401))))
    return float(np.max(np.abs(np.asarray(vy_row) - u(np.arange(t["gap"]) + 0.5))) / peak)
