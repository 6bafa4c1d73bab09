"""Plane integrals of the D3Q7 tracers reduced on the device (lbmpm_rk3dcsf_tracer_integrals, csrc/rk3d_tracer_integrals.h over the
reduction of csrc/rk3d_integrals.h) against a numpy restatement from the fields the solver already hands out: get_concentration(k) and
get_tracer_pdf(k) over the fluid cells -- the same per-cell terms (the library is built with -ffp-contract=off, so g[1] - g[2], C C are the
same doubles), numpy's own order of summation.

Tolerance of a sum column, per plane and tracer: 2 (n - 1) 2^-53 sum|term| with n the plane's fluid cells, the bound
tests/test_integrals_gpu.py derives (two orders of summation of the same rounded terms).  Counts, the minimum, the maximum and the
non-finite count are equal exactly.  INTEGRAL_CHUNK is 1024: a plane of the 70 x 33 box has 2310 cells = two whole chunks and a ragged
third; its plane 5 has five fluid cells in chunks 0 and 1 only, so chunk 2 of that plane -- and most lanes of the other two -- are empty.
"""
import numpy as np
import pytest

from test_integrals_gpu import CSF_PAR, _box
from test_rk3d_csf_gpu import _slab_case
from test_rk3d_tracer_gpu import concentrations, porous_box, tracer_case

pytestmark = pytest.mark.gpu

CELLS, MASS, FLUX_X, FLUX_Y, FLUX_Z, SUM_C2, CMIN, CMAX, NONFINITE = range(9)
EXACT = (CELLS, CMIN, CMAX, NONFINITE)
SUMS = (MASS, FLUX_X, FLUX_Y, FLUX_Z, SUM_C2)
U = 2.0 ** -53


def solver(dom, par, **kw):
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    return RK3DCSFSolver(dom, par, **kw)


def restate(dom, c, g):
    """the nine columns of one tracer per plane from its concentration c [nz][ny][nx] and populations g [nz][ny][nx][7] over dom == 1;
    returns (table [nz][9], sum|term| per entry)"""
    nz = dom.shape[0]
    T, A = np.zeros((nz, 9)), np.zeros((nz, 9))
    for z in range(nz):
        fl = dom[z] == 1
        C, G = c[z][fl], g[z][fl]
        fin = np.isfinite(C) & np.all(np.isfinite(G), axis=1)
        T[z, CELLS], T[z, NONFINITE] = fl.sum(), (~fin).sum()
        C, G = C[fin], G[fin]
        terms = {MASS: C, FLUX_X: G[:, 1] - G[:, 2], FLUX_Y: G[:, 3] - G[:, 4], FLUX_Z: G[:, 5] - G[:, 6], SUM_C2: C * C}
        for col, t in terms.items():
            T[z, col], A[z, col] = t.sum(), np.abs(t).sum()
        T[z, CMIN], T[z, CMAX] = (C.min(), C.max()) if C.size else (0.0, 0.0)
    return T, A


def compare(planes, T, A, what):
    """planes, T, A: [nz][9] of one tracer"""
    assert planes.shape == T.shape, what
    for col in EXACT:
        assert np.array_equal(planes[:, col], T[:, col]), (what, col, planes[:, col], T[:, col])
    bound = 2.0 * np.maximum(T[:, CELLS] - T[:, NONFINITE] - 1.0, 0.0)[:, None] * U * A
    err = np.abs(planes - T)
    for col in SUMS:
        print("%s col %d: worst error %.3e, bound there %.3e" % (what, col, err[:, col].max(), bound[np.argmax(err[:, col]), col]))
        assert np.all(err[:, col] <= bound[:, col]), (what, col, err[:, col], bound[:, col])


def compare_with_fields(s, dom, nT, what):
    t = s.tracer_integrals()
    assert t.planes.shape == (dom.shape[0], nT, 9) and (t.nx, t.ny) == (dom.shape[2], dom.shape[1])
    for k in range(nT):
        T, A = restate(dom, s.get_concentration(k), s.get_tracer_pdf(k))
        compare(t.planes[:, k], T, A, "%s tracer %d" % (what, k))
    assert np.array_equal(t.planes, s.tracer_integrals().planes)           # the same call twice: the same bits
    return t


# ---------------------------------------------------------------------------------------------- 1. against the fields
@pytest.fixture(scope="module")
def box():
    return _box()


@pytest.mark.parametrize("nT,negated", [(1, None), (1, 0), (3, 1), (4, 3)])
def test_against_the_fields(box, nT, negated):
    """The concentrations of concentrations() are all >= 0.2, those of the negated tracer all <= -0.2: a chunk or a lane without cells
    that contributed a 0 -- or an identity, +-Inf -- would show in cmin of the one and in cmax of the other, on every plane and above all
    on plane 5 (five cells)."""
    dom, rR, rB = box
    kw, _ = tracer_case(nT)
    assert kw["dirichlet_inlet"] and kw["free_outlet"] and (kw["reaction_rate"] > 0) == (nT == 3)
    c0 = concentrations(dom, nT)
    if negated is not None:
        c0[negated] = -c0[negated]
    s = solver(dom, CSF_PAR)
    s.configure_tracers(**kw)
    s.set_macro(rR, rB)
    for k in range(nT):
        s.set_concentration(k, c0[k])
    t = compare_with_fields(s, dom, nT, "%d tracers, step 0" % nT)         # before the first step: the FIRST instance
    assert t.planes[5, 0, CELLS] == 5 and t.nonfinite == 0 and np.all(np.isfinite(t.planes))
    for k in range(nT):
        if k == negated:
            assert np.all(t.column("cmax", k) <= -0.2 + 1e-12) and t.cmax(k) <= -0.2 + 1e-12, (k, t.column("cmax", k))
        else:
            assert np.all(t.column("cmin", k) >= 0.2 - 1e-12) and t.cmin(k) >= 0.2 - 1e-12, (k, t.column("cmin", k))
    s.step(5)
    t = compare_with_fields(s, dom, nT, "%d tracers, step 5" % nT)
    assert t.nonfinite == 0 and np.all(np.isfinite(t.planes))
    assert not np.array_equal(t.column("flux_z", 0), np.zeros(dom.shape[0]))
    s.close()


# ---------------------------------------------------------------------------------------------- 2. cut-independence, bit for bit
def test_slabs_give_the_bits_of_the_undivided_lattice():
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster
    dom, rR, rB = _slab_case()
    kw, _ = tracer_case(3)
    assert kw["reaction_rate"] > 0
    c0 = concentrations(dom, 3)

    def start(s):
        s.set_macro(rR, rB)
        for k in range(3):
            s.set_concentration(k, c0[k])
        s.step(6)
    a = solver(dom, CSF_PAR, tracers=kw)
    start(a)
    ref = a.tracer_integrals().planes
    assert ref.shape == (44, 3, 9) and np.array_equal(ref, a.tracer_integrals().planes)
    a.close()
    for cut in (dict(nslabs=4), dict(cuts=[0, 9, 23, 44])):
        c = RK3DCSFCluster(dom, CSF_PAR, tracers=kw, **cut)
        start(c)
        got = c.tracer_integrals()
        assert got.planes.shape == ref.shape and np.array_equal(got.planes, ref), cut
        assert np.array_equal(got.planes, c.tracer_integrals().planes)
        c.close()


# ---------------------------------------------------------------------------------------------- 3. a bad cell
def test_a_bad_cell_is_counted_and_left_out():
    dom, rR, rB = _slab_case()
    kw, _ = tracer_case(3)
    c0 = concentrations(dom, 3)
    s = solver(dom, CSF_PAR)
    s.configure_tracers(**kw)
    s.set_macro(rR, rB)
    for k in range(3):
        s.set_concentration(k, c0[k])
    clean = s.tracer_integrals().planes
    c1, g1 = s.get_concentration(1), s.get_tracer_pdf(1)
    y, x = np.argwhere(dom[4] == 1)[37]
    bad = g1.copy()
    bad[4, y, x, 3] = np.nan
    s.set_tracer_pdf(1, bad)
    t = s.tracer_integrals()
    dirty = t.planes
    assert np.all(np.isfinite(dirty)) and t.nonfinite == 1
    for k in (0, 2):
        assert np.array_equal(dirty[:, k], clean[:, k]), k                  # the other tracers: the same bits
    others = [z for z in range(dom.shape[0]) if z != 4]
    assert np.array_equal(dirty[others, 1], clean[others, 1])               # no other plane is touched
    assert dirty[4, 1, NONFINITE] == 1 and dirty[4, 1, CELLS] == clean[4, 1, CELLS]
    # plane 4 of tracer 1: the clean state with that cell left out (cells and nonfinite aside)
    hole = dom.copy()
    hole[4, y, x] = 0
    T, A = restate(hole, c1, g1)
    for col in (CMIN, CMAX):
        assert dirty[4, 1, col] == T[4, col], col
    n = clean[4, 1, CELLS] - 1
    for col in SUMS:
        assert abs(dirty[4, 1, col] - T[4, col]) <= 2.0 * (n - 1) * U * A[4, col], (col, dirty[4, 1, col], T[4, col])
    s.close()


# ---------------------------------------------------------------------------------------------- 4. no staging
def test_the_reduction_allocates_no_per_cell_staging():
    dom, rR, rB = _slab_case()
    N = dom.size
    kw, _ = tracer_case(3)
    c0 = concentrations(dom, 3)
    s = solver(dom, CSF_PAR)
    s.configure_tracers(**kw)
    s.set_macro(rR, rB)
    for k in range(3):
        s.set_concentration(k, c0[k])
    before = s.device_bytes
    s.tracer_integrals()
    grown = s.device_bytes - before
    assert 0 < grown < 8 * N, (grown, 8 * N)            # less than one double per cell
    s.tracer_integrals()
    assert s.device_bytes - before == grown             # allocated once
    s.close()


# ---------------------------------------------------------------------------------------------- 5. conservation, read through the table
@pytest.mark.parametrize("reaction", [False, True])
def test_conservation_read_through_the_table(reaction):
    """the closed lattice of tests/test_rk3d_tracer_gpu.py::test_conservation (no tracer inlet, no outlet), 50 steps, its tolerance: the
    masses of the table are constant to rounding; under the reaction mass(0) - mass(1) and mass(0) + mass(2) are"""
    dom, rR, rB = porous_box()
    par = dict(relax="MRT", theta=50.0, tauB=0.8, velocityZR=0.0, velocityZB=-3.0e-3, sigma=0.05)
    kw, _ = tracer_case(3, reaction=reaction, dirichlet_inlet=False, free_outlet=False)
    c0 = concentrations(dom, 3)
    s = solver(dom, par)
    s.configure_tracers(**kw); s.set_macro(rR, rB)
    for k in range(3):
        s.set_concentration(k, c0[k])
    total = lambda: np.array([s.tracer_integrals().mass(k) for k in range(3)])
    t0 = total()
    assert np.all(np.abs(t0 - np.array([c0[k].sum() for k in range(3)])) < 1e-11 * np.abs(t0))
    s.step(50)
    t1 = total()
    print("conservation through the table (reaction %s): masses %s -> %s" % (reaction, t0, t1))
    if not reaction:
        assert np.all(np.abs(t1 - t0) < 1e-11 * np.abs(t0)), (t0, t1)
    else:
        assert abs((t1[0] - t1[1]) - (t0[0] - t0[1])) < 1e-11 * abs(t0[0]) and abs((t1[0] + t1[2]) - (t0[0] + t0[2])) < 1e-11 * abs(t0[0] + t0[2]), (t0, t1)
        assert t0[0] - t1[0] > 1e-4 * t0[0]          # the reaction did consume A
    s.close()


# ---------------------------------------------------------------------------------------------- 6. moments along z
def test_the_moments_along_z_equal_those_of_the_field():
    """The Gaussian blob of tests/test_rk3d_tracer_gpu.py::test_a_gaussian_blob_spreads_as_2_d_t: centre_z and variance_z of the table
    against the same moments of get_concentration(0) summed by numpy.  No physics tolerance: both routes evaluate the same sums
    S_w = sum_i w_i C_i over the N fluid cells (w = 1, z, (z - mu)^2) in floating point, in different orders and with the weight applied
    per cell (numpy) or per plane (the table).  Any such evaluation is within gamma sum_i |w_i C_i| of the exact sum, gamma =
    (N + 8) u / (1 - (N + 8) u), u = 2^-53 (N - 1 additions, the product, and a few more roundings for z - mu, its square and the
    quotient): the summation bound of test 1 with one more term per rounding.  Two routes therefore differ by at most
        |dS_w| <= 2 gamma A_w,   A_w = sum_i |w_i| |C_i|.
    Propagated: mu = S_z / S_1 gives |d mu| <= (2 gamma A_z + |mu| 2 gamma A_1) / |S_1| (first order; doubled below for the rest);
    var = S_(z-mu)^2 / S_1 with the routes' own mu: |(z - mu')^2 - (z - mu)^2| <= 2 nz |d mu| for 0 <= z, mu < nz, so
        |d var| <= (2 gamma A_(z-mu)^2 + |var| 2 gamma A_1) / |S_1| + 2 nz |d mu|   (doubled likewise)."""
    nx, ny, nz = 64, 64, 160
    dom = np.ones((nz, ny, nx), dtype=np.uint8)
    Uz = -0.01
    par = dict(relax="MRT", velocityZR=Uz, velocityZB=0.0, densityRL=1.0, densityBL=0.0, sigma=0.0)
    s = solver(dom, par)
    s.configure_tracers(num_tracers=1, diffusion_x=0.04, diffusion_y=0.08, diffusion_z=0.12, beta_interface=0.0)
    one = np.ones(dom.shape)
    s.set_macro(one, 0.0 * one, vz=Uz * one)
    zz, yy, xx = np.mgrid[0:nz, 0:ny, 0:nx].astype(np.float64)
    s.set_concentration(0, np.exp(-((xx - 31.5) ** 2 + (yy - 31.5) ** 2 + (zz - 90.0) ** 2) / (2. * 16.)))
    N = dom.size
    gamma = (N + 8) * U / (1. - (N + 8) * U)
    seen = []
    for steps in (0, 10):
        if steps:
            s.step(steps)
        c = s.get_concentration(0)
        m = c.sum()
        mu = (c * zz).sum() / m
        var = (c * (zz - mu) ** 2).sum() / m
        a = np.abs(c)
        A1, Az, A2 = a.sum(), (a * zz).sum(), (a * (zz - mu) ** 2).sum()
        dmu = 2. * (2. * gamma * Az + abs(mu) * 2. * gamma * A1) / abs(m)
        dvar = 2. * (2. * gamma * A2 + abs(var) * 2. * gamma * A1) / abs(m) + 2. * nz * dmu
        t = s.tracer_integrals()
        print("step %d: centre_z %.15g vs %.15g (bound %.3e), variance_z %.15g vs %.15g (bound %.3e)" % (steps, t.centre_z(0), mu, dmu, t.variance_z(0), var, dvar))
        assert abs(t.mass(0) - m) <= 2. * gamma * A1
        assert abs(t.centre_z(0) - mu) <= dmu, (steps, t.centre_z(0), mu, dmu)
        assert abs(t.variance_z(0) - var) <= dvar, (steps, t.variance_z(0), var, dvar)
        seen.append((t.centre_z(0), t.variance_z(0)))
    assert abs(seen[0][0] - 90.0) < 1e-6 and abs(seen[0][1] - 16.0) < 1e-3          # the blob as it was set
    assert seen[1][0] < seen[0][0] and seen[1][1] > seen[0][1]                      # it drifts towards -z and spreads
    s.close()


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals():
    from openlbmpm_amd._lib import ERR_STATE, LbmpmError
    dom, rR, rB = _slab_case()
    s = solver(dom, CSF_PAR)
    s.set_macro(rR, rB)
    with pytest.raises(LbmpmError) as e:
        s.tracer_integrals()                    # no tracers configured
    assert e.value.status == ERR_STATE and "tracer_configure" in str(e.value)
    s.configure_tracers(num_tracers=2)
    with pytest.raises(LbmpmError) as e:
        s.tracer_integrals()                    # configured, no concentration or populations set
    assert e.value.status == ERR_STATE and "set_concentration" in str(e.value)
    for k in range(2):
        s.set_concentration(k, concentrations(dom, 2)[k])
    assert s.tracer_integrals().planes.shape == (44, 2, 9)
    s.close()
