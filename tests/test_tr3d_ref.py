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


# the flow's other open planes: overrides on the capture's parameters, on the 2-D and the 3-D side alike
OPEN_PLANES = {"convective outlet": dict(outlet="Convective"), "pressure inlet": dict(inlet="Dirichlet"),
               "convective outlet and pressure inlet": dict(outlet="Convective", inlet="Dirichlet")}
# (case, flow) of the reduction tests; the first four keep the capture's flow and the names they had
REDUCTIONS = [(n, None) for n in sorted(CASES)] + [(n, f) for n in ("anisotropic D with off-diagonals", "free outlet and Dirichlet inlet") for f in sorted(OPEN_PLANES)]
REDUCTION_IDS = [n if f is None else "%s-%s" % (n, f) for n, f in REDUCTIONS]


def setup(name, ny=3, flow=None):
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
    flow2.update(OPEN_PLANES[flow] if flow else {})
    flow3 = dict(sigma=p["sigma"], theta=float(p["theta"]), wetting=p["wetting"], beta=p["beta"], delta=p["delta"], tauR=p["tauR"], tauB=p["tauB"],
                 tautype=p["tautype"], relax=p["relax"], inlet=p["inlet"], outlet=p["outlet"], velocityZR=p["vyR"], velocityZB=p["vyB"],
                 densityBH=p["rhoBH"], densityRH=p["rhoRH"], densityBL=p["rhoBL"], densityRL=p["rhoRL"])
    flow3.update(OPEN_PLANES[flow] if flow else {})
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


@pytest.mark.parametrize("name,flow", REDUCTIONS, ids=REDUCTION_IDS)
def test_the_3d_substep_reduces_to_the_pinned_2d_oracle(name, flow):
    """flow = None: the capture's velocity inlet and pressure outlet.  Otherwise the flow's convective outlet (planes 0 .. 2 take plane 3's
    streamed state, the tracers' free outlet copies plane 1 onto plane 0 on top of it), its pressure inlet, or both"""
    dom2, o2, o3 = setup(name, flow=flow)
    assert flow is None or all(o3.flow.p[k] == v for k, v in OPEN_PLANES[flow].items())
    w = worst_difference(dom2, o2, o3, STEPS)
    print("%s, %s: worst field-relative difference over %d steps %.3e" % (name, flow or "the capture's flow", STEPS, w))
    assert w < TOL, (name, flow, w)


def test_a_misplaced_substep_is_seen():
    """negative control (as tests/test_tr_coupled.py has): the sub-step spliced AFTER the flow step's second half misses the bound by
    orders of magnitude"""
    dom2, o2, o3 = setup("one tracer")
    w = worst_difference(dom2, o2, o3, 20, after_b=True)
    print("misplaced sub-step: %.3e" % w)
    assert w > 1e4 * TOL, w


# ---- what the reduction cannot see: everything that involves y.  The sub-step has no preferred axis but for its open planes (z)

AXIS = {"x": -1, "y": -2, "z": -3}                  # of an array [nz][ny][nx]
POP = {"x": (1, 2), "y": (3, 4), "z": (5, 6)}      # (+, -) populations
FULL_TENSOR = dict(diffX=(1. / 6., 0.1, 0.2), diffY=(0.12, 0.1, 0.15), diffZ=(0.2, 0.08, 0.1), dXY=0.01, dYX=-0.02, dXZ=0.03, dZX=0.015, dYZ=-0.01,
                   dZY=0.02, beta=(1.0, 0.5, 0.8), crit=0.5, inlet_conc=(0.8, 0.4, 0.0), reaction_rate=0.03, diffJ=(0.0, 0.25, 0.1))


def exchanged(a, b):
    """the axis names under the exchange a <-> b"""
    return {c: (b if c == a else a if c == b else c) for c in "xyz"}


def exchange_tracer(t, a, b, pair_as_it_was=False):
    """the tracer parameters of the problem with the axes a and b exchanged: D' = P D P^T.  pair_as_it_was: the two off-diagonals of the
    exchanged pair keep their places (D read with the transposed convention) -- the negative control"""
    s = {k.upper(): v.upper() for k, v in exchanged(a, b).items()}
    out = dict(t)
    for p in "XYZ":
        out["diff" + s[p]] = t["diff" + p]
        for q in "XYZ":
            if p != q:
                out["d" + s[p] + s[q]] = t["d" + p + q]
    if pair_as_it_was:
        A, B = a.upper(), b.upper()
        out["d" + A + B], out["d" + B + A] = t["d" + A + B], t["d" + B + A]
    return out


def exchange_field(f, a, b):
    return np.ascontiguousarray(np.swapaxes(f, AXIS[a], AXIS[b]))


def exchange_vector(v, a, b):
    """{x, y, z: array} of the exchanged problem"""
    s = exchanged(a, b)
    return {s[c]: exchange_field(v[c], a, b) for c in "xyz"}


def exchange_populations(g, a, b):
    """[nT][7][nz][ny][nx] of the exchanged problem: arrays transposed, +a <-> +b, -a <-> -b"""
    out = exchange_field(g, a, b)
    idx = list(range(7))
    for sign in (0, 1):
        idx[POP[a][sign]], idx[POP[b][sign]] = POP[b][sign], POP[a][sign]
    return np.ascontiguousarray(out[:, idx])


def smooth(rng, shape, terms=6):
    """a few long waves with random amplitudes and phases, largest value 1: periodic like the lattice"""
    nz, ny, nx = shape
    zz, yy, xx = np.mgrid[0:nz, 0:ny, 0:nx]
    f = np.zeros(shape)
    for _ in range(terms):
        kx, ky, kz = rng.integers(-2, 3, 3)
        f += rng.standard_normal() * np.cos(2 * np.pi * (kx * xx / nx + ky * yy / ny + kz * zz / nz) + rng.uniform(0, 2 * np.pi))
    return f / np.max(np.abs(f))


def prescribed_problem(nx=18, ny=11, nz=13, seed=11):
    """a mask without any symmetry (a sphere, wall pieces; planes 0 = 1 and nz-1 = nz-2 as the open planes ask), rho_R on both sides of
    criteria_rho, u of order 0.05, G with exact zeros in part of the lattice (both sides of the 1e-8 switch), three concentrations"""
    rng = np.random.default_rng(seed)
    shape = (nz, ny, nx)
    zz, yy, xx = np.mgrid[0:nz, 0:ny, 0:nx]
    dom = np.ones(shape, dtype=np.uint8)
    dom[(zz - 6.3) ** 2 + (yy - 4.1) ** 2 + (xx - 7.2) ** 2 <= 7.5] = 0
    dom[3:9, 0, 2:15] = 0
    dom[4:10, 3:9, 0] = 0
    dom[2:4, 7:10, 11:16] = 0
    dom[0] = dom[1]; dom[-1] = dom[-2]
    rhoR = 0.5 + 0.4 * smooth(rng, shape)
    v = {c: 0.05 * smooth(rng, shape) for c in "xyz"}
    part = smooth(rng, shape) > -0.2
    G = {c: 0.1 * smooth(rng, shape) * part for c in "xyz"}
    c0 = np.array([(0.5 + 0.3 * np.sin(2 * np.pi * (xx + 2 * k) / nx) * np.cos(2 * np.pi * (yy + k) / ny) * np.cos(2 * np.pi * (zz + 3 * k) / nz)) * (dom == 1)
                   for k in range(3)])
    return dom, rhoR, v, G, c0


def run_prescribed(dom, rhoR, v, G, c0, tracer, steps):
    from tr3d_ref import Tracer3DRef
    r = Tracer3DRef(dom, c0, tracer)
    for _ in range(steps):
        r.substep(rhoR, v["x"], v["y"], v["z"], G["x"], G["y"], G["z"])
    return r


@pytest.mark.parametrize("a,b,open_planes", [("x", "y", True), ("y", "z", False), ("x", "z", False)], ids=["x-y, open planes", "y-z", "x-z"])
def test_exchanging_two_axes_exchanges_the_tracers(a, b, open_planes):
    """Tracer3DRef driven with prescribed fields, 3 tracers with the reaction, all six off-diagonals nonzero and distinct, 40 sub-steps,
    against the problem with two axes exchanged (arrays transposed, vector components, diffX / Y / Z and every dAB renamed): only the order
    of sums changes.  x <-> y ties dXY to dYX and the +-y pull, bounce-back and interface cosine to the +-x ones; y <-> z (no open planes: z
    is then periodic like x and y) ties them to dXZ / dZX, which the reduction to the 2-D oracle pins.
    Measured (18 x 11 x 13): 2.8e-16 .. 3.3e-16 for the three exchanges; the exchanged pair's off-diagonals left in place: 4.1e-2 (x <-> y),
    6.9e-2 (y <-> z), 1.9e-2 (x <-> z); the change of the field from its start: 2.6 .. 3.0 of its largest value."""
    dom, rhoR, v, G, c0 = prescribed_problem()
    assert np.array_equal(dom[0], dom[1]) and np.array_equal(dom[-1], dom[-2])
    gn = np.sqrt(G["x"] ** 2 + G["y"] ** 2 + G["z"] ** 2)[dom == 1]
    assert np.any(gn == 0.0) and np.any(gn > 1e-3) and np.any(rhoR[dom == 1] > 0.5) and np.any(rhoR[dom == 1] < 0.5)
    t = dict(FULL_TENSOR, free_outlet=open_planes, dirichlet_inlet=open_planes)
    assert len({t["d" + p + q] for p in "XYZ" for q in "XYZ" if p != q}) == 6
    steps = 40
    one = run_prescribed(dom, rhoR, v, G, c0, t, steps)
    x = lambda f: exchange_field(f, a, b)
    args = (x(dom), x(rhoR), exchange_vector(v, a, b), exchange_vector(G, a, b), x(c0))
    two = run_prescribed(*args, exchange_tracer(t, a, b), steps)
    ec, eg = rel_err(two.C, x(one.C)), rel_err(two.g, exchange_populations(one.g, a, b))
    bad = run_prescribed(*args, exchange_tracer(t, a, b, pair_as_it_was=True), steps)
    miss = rel_err(bad.C, x(one.C))
    moved = rel_err(one.C, c0)
    print("%s <-> %s: concentration %.3e populations %.3e; the pair's off-diagonals left in place %.3e; moved %.3e" % (a, b, ec, eg, miss, moved))
    assert ec < 1e-13 and eg < 1e-13, (a, b, ec, eg)
    assert miss > 1e-3, (a, b, miss)
    assert moved > 0.1, (a, b, moved)


# ---- the analytic law: a Gaussian under a full diffusion tensor

BLOB_D = np.array([[0.06, 0.03, -0.02], [-0.01, 0.09, 0.025], [0.015, -0.03, 0.12]])       # nonsymmetric; the largest entry of D + D^T is 0.24
BLOB_DRIFT = (0.01, -0.02, 0.015)


def blob_tracer(D=BLOB_D):
    return dict(diffX=(D[0, 0],), diffY=(D[1, 1],), diffZ=(D[2, 2],), dXY=D[0, 1], dYX=D[1, 0], dXZ=D[0, 2], dZX=D[2, 0], dYZ=D[1, 2], dZY=D[2, 1],
                beta=(0.0,), free_outlet=False, dirichlet_inlet=False)


def blob_moments(c):
    """(mass, centre (x, y, z), covariance [3][3] over (x, y, z)) of a concentration [nz][ny][nx]"""
    zz, yy, xx = np.mgrid[0:c.shape[0], 0:c.shape[1], 0:c.shape[2]].astype(np.float64)
    m = c.sum()
    mu = [(c * a).sum() / m for a in (xx, yy, zz)]
    d = [a - mu_a for a, mu_a in zip((xx, yy, zz), mu)]
    return m, np.array(mu), np.array([[(c * d[i] * d[j]).sum() / m for j in range(3)] for i in range(3)])


# |d cov_ij / dt - (D_ij + D_ji)| / 0.24 that this test measures, [run][i][j] over (x, y, z); the bounds are three times these
BLOB_MEASURED = {
    "at rest": np.array([[7.25e-7, 2.32e-5, 3.81e-5], [2.32e-5, 2.69e-5, 4.27e-5], [3.81e-5, 4.27e-5, 2.55e-4]]),
    "drifting": np.array([[7.50e-5, 4.70e-5, 1.98e-4], [4.70e-5, 7.04e-4, 9.88e-4], [1.98e-4, 9.88e-4, 1.001e-3]]),
}
BLOB_DRIFT_MEASURED = 3.23e-5          # |d centre / dt - u|, the largest component, of the drifting run (at rest: 2e-17)


@pytest.mark.parametrize("run", ["at rest", "drifting"])
def test_a_gaussian_blob_spreads_as_d_plus_d_transposed(run):
    """A Gaussian blob (sigma^2 = 9) on an all-fluid periodic 48^3 box, beta = 0, uniform rho_R and u, G = 0: d cov_ij / dt = D_ij + D_ji
    for all six entries of a nonsymmetric D, the centre moves with u, the mass stays.  The analytic law is the reference.  Slopes between
    sub-steps 40 and 100, once at rest and once with u = (0.01, -0.02, 0.015): part of the error is the scheme's O(u_i u_j) term.
    Measured, relative to the largest entry of D + D^T (0.24), entry by entry in BLOB_MEASURED: at rest 7.2e-7 (xx) .. 2.5e-4 (zz, the widest
    blob: what wraps round the box), drifting 4.7e-5 (xy) .. 1.0e-3 (zz); the centre's velocity within 3.2e-5 of u; the mass to 4e-15.
    Each bound is three times the measured error of its entry."""
    from tr3d_ref import Tracer3DRef
    n = 48
    shape = (n, n, n)
    dom = np.ones(shape, dtype=np.uint8)
    u = BLOB_DRIFT if run == "drifting" else (0., 0., 0.)
    zz, yy, xx = np.mgrid[0:n, 0:n, 0:n].astype(np.float64)
    c0 = np.exp(-((xx - 23.5) ** 2 + (yy - 23.5) ** 2 + (zz - 23.5) ** 2) / (2. * 9.))
    r = Tracer3DRef(dom, c0[None], blob_tracer())
    one, zero = np.ones(shape), np.zeros(shape)
    fields = (one, u[0] * one, u[1] * one, u[2] * one, zero, zero, zero)
    for _ in range(40):
        r.substep(*fields)
    m1, mu1, cov1 = blob_moments(r.C[0])
    for _ in range(60):
        r.substep(*fields)
    m2, mu2, cov2 = blob_moments(r.C[0])
    want = BLOB_D + BLOB_D.T
    err = np.abs((cov2 - cov1) / 60. - want) / np.max(want)
    drift = np.max(np.abs((mu2 - mu1) / 60. - np.array(u)))
    print("%s: |d cov / dt - (D + D^T)| / %.2f =\n%s\ndrift off u by %.3e, mass off by %.3e" % (run, np.max(want), np.array2string(err, precision=3), drift, abs(m2 - m1) / m1))
    assert abs(m2 - m1) < 1e-13 * m1
    assert np.all(err <= 3. * BLOB_MEASURED[run]), (run, err)
    assert drift <= 3. * BLOB_DRIFT_MEASURED, drift
    assert np.all(np.abs(want[np.triu_indices(3, 1)]) > 4e-3)          # no off-diagonal of D + D^T is idle


# ---- the conditioning of the samples the kernels are compared on

@pytest.mark.parametrize("lattice", ["obstacle", "odd nx", "5 x 1 x 16", "1 x 6 x 12", "70 x 3 x 9"])
def test_the_cases_of_the_gpu_comparison_are_well_conditioned(lattice):
    """tests/test_rk3d_tracer_gpu.py holds the kernels to this reference at 1e-10 after 200 steps.  A reference that does not follow
    ITSELF to that tolerance when its start differs in the last bit cannot be followed to it by anything else -- and it does not where the
    flow's wetting rule meets an interface parallel to a wall (LATTICE_FLOW there).  The bound is the comparison's own tolerance: the
    necessary condition, no more.  Measured, 3 tracers, concentrations and populations: obstacle 1.1e-13, odd nx 1.7e-11 (a transient of
    the first steps), the three odd sizes 5.4e-15 .. 5.8e-15; the 70 x 3 x 9 box WITH the wetting rule: 1e-3."""
    import test_rk3d_tracer_gpu as T
    dom, rR, rB = T.LATTICES[lattice]()
    par = dict(theta=50.0, tauB=0.8, velocityZR=0.0, velocityZB=-1.0e-2, sigma=0.05, relax="MRT", crisp=T.CRISP); par.update(T.LATTICE_FLOW.get(lattice, {}))
    _, ref = T.tracer_case(3)
    c0 = T.concentrations(dom, 3)
    rng = np.random.default_rng(0)
    last_bit = lambda a: a * (1. + 2.0 ** -52 * rng.integers(-1, 2, a.shape))
    one, two = Coupled3DRef(dom, rR, rB, c0, par, ref), Coupled3DRef(dom, last_bit(rR), last_bit(rB), c0, par, ref)
    worst = 0.0
    for _ in range(T.STEPS // 10):
        one.run(10); two.run(10)
        worst = max(worst, rel_err(two.C, one.C), rel_err(two.g, one.g))
    print("%s: the reference against itself from a start that differs in the last bit, worst over %d steps: %.3e" % (lattice, T.STEPS, worst))
    assert np.any(two.flow.field("fR") != one.flow.field("fR")) and worst < T.TOL, (lattice, worst)
