"""The cases the wall reaction of the 3-D tracers is held to a reference on, shared by tests/test_wall_reaction_cpu.py (conditioning,
sensitivity) and tests/test_rk3d_tracer_wall_gpu.py (parity): lattices, flows, tracers, rates, the mineral map, the references.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

import body_force_ref as R
import periodic_ref as PR
from wall_reaction_ref import coupled

INF = float("inf")
STEPS = (1, 10)
# [class][tracer]: distinct per class and per tracer, one of them the instantaneous reaction
RATES = np.array([[0.02, INF], [0.2, 0.01], [1.0, 0.5]])
CLASSES = 3


def minerals_of(dom, seed=5):
    """three classes scattered cell by cell over the whole lattice (read at the solid cells): fluid cells next to a wall piece touch
    two classes and more"""
    return np.random.default_rng(seed).integers(0, CLASSES, size=np.shape(dom)).astype(np.uint8)


def touches_two_classes(dom, minerals):
    """fluid cells whose six axis neighbours hold solids of at least two classes"""
    from tr3d_ref import E, _shift
    fl = np.asarray(dom) == 1
    seen = [np.zeros(fl.shape, dtype=bool) for _ in range(CLASSES)]
    for j in range(1, 7):
        solid, cls = _shift(~fl, -E[j]), _shift(minerals, -E[j])
        for m in range(CLASSES):
            seen[m] |= fl & solid & (cls == m)
    return int((sum(s.astype(int) for s in seen) >= 2).sum())


def open_case():
    """between open planes: 18 x 11 x 16 (blob3's mask at that size), MRT, velocity inlet, two tracers at tracer_case with the Dirichlet
    inlet and the free outlet"""
    from test_oracle_rk3d_csf import blob3
    from test_rk3d_tracer_gpu import CRISP, concentrations, tracer_case
    dom, rR, rB = blob3(nx=18, ny=11, nz=16)
    par = dict(theta=50.0, tauB=0.8, velocityZR=0.0, velocityZB=-1.0e-2, sigma=0.05, relax="MRT")
    kw, ref = tracer_case(2)
    return dict(name="open", dom=dom, rR=rR, rB=rB, par=par, opar=dict(par, crisp=CRISP), kw=kw, ref=ref, nT=2, c0=concentrations(dom, 2), g=None,
                minerals=minerals_of(dom))


def periodic_case():
    """periodic z under the body force G1: periodic_ref.parity_lattice (10 x 6 x 14), MRT, two tracers at tracer point B"""
    from test_rk3d_tracer_features_gpu import periodic_concentrations
    from test_rk3d_tracer_gpu import tracer_point_b
    dom, rR, rB = PR.parity_lattice()
    kw, ref = tracer_point_b(2, dirichlet_inlet=False, free_outlet=False)
    return dict(name="periodic", dom=dom, rR=rR, rB=rB, par=PR.parity_params("MRT", 2), kw=kw, ref=ref, nT=2, c0=periodic_concentrations(dom)[:2],
                g=R.G_SETS["G1"], minerals=minerals_of(dom))


CASES = {"open": open_case, "periodic": periodic_case}


def reference(c, rates=RATES, minerals="case", rR=None, rB=None):
    """Coupled3DRef with the wall reaction's sub-step for the case c"""
    rR, rB = c["rR"] if rR is None else rR, c["rB"] if rB is None else rB
    m = c["minerals"] if isinstance(minerals, str) else minerals
    if c["g"] is None:
        from oracle.rk3dcsf import RK3DCSFOracle
        flow = RK3DCSFOracle(c["dom"], rR, rB, c["opar"])
    else:
        flow = PR.PeriodicRef(c["dom"], rR, rB, c["par"], *c["g"])
    return coupled(c["dom"], c["c0"], c["ref"], flow, rates, m)


def start(s, c, rates=RATES, minerals="case"):
    """the solver (or cluster) s at the start of the case c"""
    if c["g"] is not None:
        s.set_body_force(red=c["g"][0], blue=c["g"][1])
    s.set_macro(c["rR"], c["rB"])
    for k in range(c["nT"]):
        s.set_concentration(k, c["c0"][k])
    if rates is not None:
        s.set_wall_reaction(rates, c["minerals"] if isinstance(minerals, str) else minerals)
    return s
