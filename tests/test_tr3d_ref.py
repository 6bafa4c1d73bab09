"""The restated 3-D tracer sub-step (tests/tr3d_ref.py) against the pinned 2-D oracle, on lattices uniform in y.

A D3Q7 tracer with rest weight 0 and six weights 1/6 projects onto the reference's D2Q5 scheme (1/3, 1/6 x 4) when nothing depends on y:
the D2Q5 rest population is g0 + g(+y) + g(-y), and since every second-order moment relaxes at rate 1 the projected collision closes
for the MRT operator with distinct flux rates.  Both sides are spliced the same way -- 2-D: rk_csf_step_a -> tr_substep -> rk_csf_step_b
(oracle/rk_oracle.c, oracle/tr_oracle.c, the latter pinned to captures of the real driver); 3-D: rk3dcsf_step_a -> restatement ->
rk3dcsf_step_b -- on the set-up of the capture rk_csf_srt_capillary (SRT: the only branch whose 3-D flow reduces)."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import GOLDEN, load_params, rel_err
from tr3d_ref import Coupled3DRef, project_g

F64P = C.POINTER(C.c_double)
STEPS = 60
# Field-relative, every step, concentration and projected populations.  Measured worst over the four cases and 60 steps: 1.6e-11 (1.1e-11 .. 1.6e-11 per case:
# the flow's own reduction error, fed back through the interface term, dominates; the tracer arithmetic alone agrees to 7e-16).  The bound
# is one decade above, below the project's reduction tolerance of 1e-9.  The misplaced sub-step of the negative control: 0.4.
TOL = 2e-10

CASES = {
    "one tracer": (dict(diffX=(1. / 6.,), diffY=(1. / 6.,), dXY=0., dYX=0., beta=(1.0,), free_outlet=False, dirichlet_inlet=False), {}),
    "three tracers with the reaction": (dict(diffX=(1. / 6., 0.1, 0.2), diffY=(1. / 6., 0.1, 0.2), dXY=0., dYX=0., beta=(1.0, 0.5, 0.0), inlet_conc=(1., 0.5, 0.),
                                             free_outlet=False, dirichlet_inlet=False, reaction_rate=0.02, diffJ=(1. / 3., 0.5, 0.4)), {}),
    "anisotropic D with off-diagonals": (dict(diffX=(0.25,), diffY=(0.08,), dXY=0.03, dYX=-0.02, beta=(0.7,), free_outlet=False, dirichlet_inlet=False), dict(diffY=(0.12,))),
    "free outlet and Dirichlet inlet": (dict(diffX=(1. / 6.,), diffY=(0.1,), dXY=0., dYX=0., beta=(1.0,), inlet_conc=(0.8,), free_outlet=True, dirichlet_inlet=True), {}),
}


def extrude(a2, ny):
    return np.ascontiguousarray(np.repeat(np.asarray(a2)[:, None, :], ny, axis=1))


def setup(name, ny=3):
    from oracle.rk import initial_densities
    from oracle.tr import CoupledOracle
    d = np.load(os.path.join(GOLDEN, "rk_csf_srt_capillary.npz"))
    p = load_params(d)
    assert p["relax"] == "SRT"
    dom2 = d["isDomain"]
    rR2, rB2 = initial_densities(dom2, False, p["nbuf"])
    flow2 = {k: p[k] for k in ("sigma", "theta", "wetting", "beta", "delta", "tauR", "tauB", "tautype", "relax", "inlet", "outlet", "vyR", "vyB",
                                "rhoBH", "rhoRH", "rhoBL", "rhoRL")}
    flow2["theta"] = float(flow2["theta"])
    flow3 = dict(sigma=p["sigma"], theta=float(p["theta"]), wetting=p["wetting"], beta=p["beta"], delta=p["delta"], tauR=p["tauR"], tauB=p["tauB"],
                 tautype=p["tautype"], relax=p["relax"], inlet=p["inlet"], outlet=p["outlet"], velocityZR=p["vyR"], velocityZB=p["vyB"],
                 densityBH=p["rhoBH"], densityRH=p["rhoRH"], densityBL=p["rhoBL"], densityRL=p["rhoRL"])
    t2, over3 = CASES[name]
    nT = len(t2["diffX"])
    nz, nx = dom2.shape
    zz, xx = np.mgrid[0:nz, 0:nx]
    conc2 = np.array([(0.5 + 0.3 * np.sin(2 * np.pi * (xx + 3 * k) / nx) * np.cos(2 * np.pi * (zz + 5 * k) / nz)) * (dom2 == 1) for k in range(nT)])
    # the same case on the D3Q7 lattice: the 2-D y axis is z; D_yy is free on a y-uniform lattice; J0' = (3 J0 - 1) / 2
    t3 = dict(diffX=t2["diffX"], diffZ=t2["diffY"], diffY=over3.get("diffY", t2["diffY"]), dXZ=t2["dXY"], dZX=t2["dYX"], beta=t2["beta"],
              inlet_conc=t2.get("inlet_conc", (1.0,) * nT), free_outlet=t2["free_outlet"], dirichlet_inlet=t2["dirichlet_inlet"],
              reaction_rate=t2.get("reaction_rate", 0.0), diffJ=tuple((3. * j - 1.) / 2. for j in t2["diffJ"]) if t2.get("diffJ") else None)
    o2 = CoupledOracle(dom2, flow2, rR2, rB2, conc2, dict(t2, crit=0.5))
    o3 = Coupled3DRef(extrude(dom2, ny), extrude(rR2, ny), extrude(rB2, ny), np.array([extrude(c, ny) for c in conc2]), flow3, dict(t3, crit=0.5))
    return dom2, o2, o3


def step2(o2):
    """2-D: first half of the CSF flow step, the tracer sub-step, the second half"""
    from oracle import lib
    L, f = lib(), o2.flow
    P = lambda a: a.ctypes.data_as(F64P)
    L.rk_csf_step_a(C.byref(f._s))
    L.tr_substep(C.byref(o2._s), P(f.rhoR), P(f.vx), P(f.vy), P(f.Gx), P(f.Gy))
    L.rk_csf_step_b(C.byref(f._s))


def dense2(o2, a):
    out = np.zeros((o2.flow.ny * o2.flow.nx,) + a.shape[1:])
    out[o2.flow.fluidNodes] = a
    return out.reshape((o2.flow.ny, o2.flow.nx) + a.shape[1:])


def worst_difference(dom2, o2, o3, steps, after_b=False):
    worst, fl = 0.0, dom2 == 1
    for _ in range(steps):
        step2(o2)
        o3.run(1, after_b=after_b)
        for k in range(o3.tr.nT):
            c3, g3 = o3.C[k], o3.g[k]
            assert np.max(np.abs(c3 - c3[:, :1, :])) <= 1e-13 * np.max(np.abs(c3)), "the concentration is not uniform along y"
            worst = max(worst, rel_err(c3[:, 0, :][fl], dense2(o2, o2.C[k])[fl]), rel_err(project_g(g3)[fl], dense2(o2, o2.g[k])[fl]))
    return worst


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_3d_substep_reduces_to_the_pinned_2d_oracle(name):
    dom2, o2, o3 = setup(name)
    w = worst_difference(dom2, o2, o3, STEPS)
    print("%s: worst field-relative difference over %d steps %.3e" % (name, STEPS, w))
    assert w < TOL, (name, w)


def test_a_misplaced_substep_is_seen():
    """negative control (as tests/test_tr_coupled.py has): the sub-step spliced AFTER the flow step's second half misses the bound by
    orders of magnitude"""
    dom2, o2, o3 = setup("one tracer")
    w = worst_difference(dom2, o2, o3, 20, after_b=True)
    print("misplaced sub-step: %.3e" % w)
    assert w > 1e4 * TOL, w
