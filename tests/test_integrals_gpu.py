"""Plane integrals reduced on the device (lbmpm_rk3d_integrals / lbmpm_rk3dcsf_integrals, csrc/rk3d_integrals.h) against a numpy
restatement from the fields the solvers already hand out: the same masks, the same per-cell products (the library is built with
-ffp-contract=off, so the terms are the same doubles), numpy's own order of summation.

Tolerance of a sum column, per plane: 2 (n - 1) 2^-53 sum|term| with n the plane's fluid cells -- the worst-case distance between two
orders of summation of the same rounded terms (each order is within (n - 1) u sum|term| of the exact sum, u = 2^-53).  Counts and the
maximum are equal exactly.  INTEGRAL_CHUNK is 1024: a plane of the 70 x 33 box has 2310 cells = two whole chunks and a ragged third.
"""
import numpy as np
import pytest

from test_rk3d_csf_gpu import _slab_case

pytestmark = pytest.mark.gpu

FIELDS = ("rhoR", "rhoB", "vx", "vy", "vz", "phi")
EXACT = (0, 1, 10, 11)
CSF_PAR = dict(relax="MRT", theta=55.0, tauB=0.8, velocityZR=0.0, velocityZB=-3.0e-3, sigma=0.06)


def _box(nx=70, ny=33, nz=12, seed=17):
    """a porous box: open planes at either end (four at the bottom with one mask: the convective outlet copies plane 3 onto the planes
    below it), seeded blocks in between, row y = 7 all solid and plane 5 with five fluid cells; nx is no multiple of 64 (rows of two
    segments), 2310 cells per plane"""
    rng = np.random.default_rng(seed)
    dom = np.ones((nz, ny, nx), dtype=np.uint8)
    for _ in range(60):
        z, y, x = rng.integers(4, nz - 3), rng.integers(0, ny - 3), rng.integers(0, nx - 4)
        dom[z:z + 2, y:y + 3, x:x + 4] = 0
    dom[4:nz - 2, 7, :] = 0
    dom[5] = 0
    dom[5, 20, 30:33] = 1
    dom[5, 3, 68:70] = 1
    assert int((dom[5] == 1).sum()) == 5 and not (dom[6, 7] == 1).any()
    from openlbmpm_amd.geometry import initial_densities_rk3d
    rR, rB = initial_densities_rk3d(dom, 3)
    return dom, rR, rB


def restate(dom, f):
    """the twelve columns per plane from the fields f[name] [nz][ny][nx]; returns (table, sum|term| per entry)"""
    nz = dom.shape[0]
    T, A = np.zeros((nz, 12)), np.zeros((nz, 12))
    for z in range(nz):
        fl = dom[z] == 1
        v = [f[k][z][fl] for k in FIELDS]
        fin = np.ones(int(fl.sum()), dtype=bool)
        for a in v:
            fin &= np.isfinite(a)
        T[z, 0], T[z, 11] = fl.sum(), (~fin).sum()
        rR, rB, ux, uy, uz, phi = (a[fin] for a in v)
        red = phi > 0
        T[z, 1] = red.sum()
        rho = rR + rB
        terms = {2: rR, 3: rB, 4: rR * uz, 5: rB * uz, 6: uz[red], 7: uz[~red], 8: rho * ux, 9: rho * uy}
        for c, t in terms.items():
            T[z, c], A[z, c] = t.sum(), np.abs(t).sum()
        u2 = ux * ux + uy * uy + uz * uz
        T[z, 10] = u2.max() if u2.size else 0.0
    return T, A


def compare(planes, dom, f, what):
    T, A = restate(dom, f)
    assert planes.shape == T.shape, what
    for c in EXACT:
        assert np.array_equal(planes[:, c], T[:, c]), (what, c, planes[:, c], T[:, c])
    n = T[:, 0]
    bound = 2.0 * np.maximum(n - 1.0, 0.0)[:, None] * 2.0 ** -53 * A
    err = np.abs(planes - T)
    for c in range(2, 10):
        print("%s col %d: worst error %.3e, bound there %.3e" % (what, c, err[:, c].max(), bound[np.argmax(err[:, c]), c]))
        assert np.all(err[:, c] <= bound[:, c]), (what, c, err[:, c], bound[:, c])
    return T


@pytest.fixture(scope="module")
def box():
    return _box()


def _pert(dom, relax="SRT"):
    from openlbmpm_amd.rk3d import RK3DSlab
    return RK3DSlab(dom, 0, dom.shape[0], dict(relax=relax, tauB=0.8))      # velocity inlet, pressure outlet: the defaults


def _fields(s, prefix=""):
    return {k: s.get(prefix + k) for k in FIELDS}


# ---------------------------------------------------------------------------------------------- 1. perturbation model vs its fields
@pytest.mark.parametrize("relax", ["MRT", "SRT"])
def test_perturbation_model_against_its_fields(box, relax):
    dom, rR, rB = box
    s = _pert(dom, relax)
    s.set_density(rR, rB)
    for steps in (0, 7):
        if steps:
            s.step_single(steps)
        s.phase_field(diagnostics=True)
        g = s.integrals()
        assert g.nx == 70 and g.ny == 33 and g.planes.shape == (12, 12)
        T = compare(g.planes, dom, _fields(s), "rk3d %s step %d" % (relax, steps))
        assert T[5, 0] == 5 and T[:, 11].sum() == 0 and g.nonfinite == 0
        assert np.array_equal(g.planes, s.integrals().planes)              # the same call twice: the same bits
    assert g.total("umax2") > 0 and 0 < g.saturation_R < 1
    s.close()


# ---------------------------------------------------------------------------------------------- 2. CSF model vs the rec_* fields
@pytest.mark.parametrize("over", [{}, dict(outlet="Convective"), dict(inlet="Dirichlet", densityBH=1.0, densityRH=1e-8)],
                         ids=["default", "convective-outlet", "pressure-inlet"])
@pytest.mark.parametrize("mask", ["box", "slab_case"])
def test_csf_model_against_its_record_fields(box, mask, over):
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    dom, rR, rB = box if mask == "box" else _slab_case()
    s = RK3DCSFSolver(dom, dict(CSF_PAR, **over))
    s.set_macro(rR, rB)
    for steps in (0, 5):               # before the first step (the FIRST instance), after five
        if steps:
            s.step(steps)
        g = s.integrals()
        T = compare(g.planes, dom, _fields(s, "rec_"), "csf %s %s step %d" % (mask, sorted(over), steps))
        assert T[:, 11].sum() == 0
    assert g.total("umax2") > 0 and 0 < g.saturation_R < 1
    s.close()


# ---------------------------------------------------------------------------------------------- 3. cut-independence, bit for bit
def test_csf_slabs_give_the_bits_of_the_undivided_lattice():
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster, RK3DCSFSolver
    dom, rR, rB = _slab_case()
    a = RK3DCSFSolver(dom, CSF_PAR)
    a.set_macro(rR, rB); a.step(6)
    ref = a.integrals().planes
    assert np.array_equal(ref, a.integrals().planes)
    a.close()
    for kw in (dict(nslabs=4), dict(cuts=[0, 9, 23, 44])):
        c = RK3DCSFCluster(dom, CSF_PAR, **kw)
        c.set_macro(rR, rB); c.step(6)
        got = c.integrals()
        assert got.planes.shape == ref.shape and np.array_equal(got.planes, ref), kw
        assert np.array_equal(got.planes, c.integrals().planes)
        c.close()


def test_perturbation_slabs_give_the_bits_of_the_undivided_lattice(box):
    from openlbmpm_amd.rk3d import RK3DCluster
    dom, rR, rB = box
    s = _pert(dom, "MRT")
    s.set_density(rR, rB); s.step_single(6); s.phase_field(diagnostics=True)
    ref = s.integrals().planes
    s.close()
    for k in (2, 3):
        c = RK3DCluster(dom, k, dict(relax="MRT", tauB=0.8))
        c.set_density(rR, rB); c.step(6)
        got = c.integrals()                      # (stale after the steps: observes first)
        assert np.array_equal(got.planes, ref), k
        assert np.array_equal(got.planes, c.integrals().planes)
        c.close()


# ---------------------------------------------------------------------------------------------- 4. no staging
def test_the_csf_reduction_allocates_no_per_cell_staging():
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    dom, rR, rB = _slab_case()
    N = dom.size
    s = RK3DCSFSolver(dom, CSF_PAR)
    s.set_macro(rR, rB)
    before = s.device_bytes
    s.integrals()
    grown = s.device_bytes - before
    assert 0 < grown < 8 * N, (grown, 8 * N)            # less than one double per cell
    s.integrals()
    assert s.device_bytes - before == grown             # allocated once
    s.close()
    s = RK3DCSFSolver(dom, CSF_PAR)
    s.set_macro(rR, rB)
    before = s.device_bytes
    s.get("rec_rhoR")
    assert s.device_bytes - before == 48 * N            # the route that exists beside it: six doubles per cell
    s.close()


# ---------------------------------------------------------------------------------------------- 5. bad cells
def _with_one_nan(dom, rR):
    """rho_R = NaN in one fluid cell of plane 4"""
    y, x = np.argwhere(dom[4] == 1)[37]
    bad = rR.copy()
    bad[4, y, x] = np.nan
    hole = dom.copy()
    hole[4, y, x] = 0
    return bad, hole


def _check_one_bad_cell(clean, dirty, hole, fields, what):
    """clean / dirty: the device tables of the clean state and of the state with the NaN; fields: the clean state's; hole: the mask without
    that cell"""
    want11 = np.zeros(clean.shape[0]); want11[4] = 1
    assert np.array_equal(dirty[:, 11], want11), what
    assert np.array_equal(dirty[:, 0], clean[:, 0]), what
    assert np.all(np.isfinite(dirty)), what
    others = [z for z in range(clean.shape[0]) if z != 4]
    assert np.array_equal(dirty[others], clean[others]), what          # no other plane is touched
    # plane 4: the clean state with that cell left out (columns 0 and 11 aside)
    T, A = restate(hole, fields)
    n = clean[4, 0]
    for c in (1, 10):
        assert dirty[4, c] == T[4, c], (what, c)
    for c in range(2, 10):
        assert abs(dirty[4, c] - T[4, c]) <= 2.0 * (n - 1) * 2.0 ** -53 * A[4, c], (what, c, dirty[4, c], T[4, c])


def test_a_bad_cell_is_counted_and_left_out_csf():
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    dom, rR, rB = _slab_case()
    bad, hole = _with_one_nan(dom, rR)
    s = RK3DCSFSolver(dom, CSF_PAR)
    s.set_macro(rR, rB)
    clean, fields = s.integrals().planes, _fields(s, "rec_")
    s.set_macro(bad, rB)
    g = s.integrals()
    _check_one_bad_cell(clean, g.planes, hole, fields, "csf")
    assert g.nonfinite == 1 and np.isfinite(g.saturation_R)
    s.close()


def test_a_bad_cell_is_counted_and_left_out_perturbation(box):
    dom, rR, rB = box
    bad, hole = _with_one_nan(dom, rR)
    s = _pert(dom)
    s.set_density(rR, rB); s.phase_field(diagnostics=True)
    clean, fields = s.integrals().planes, _fields(s)
    s.set_density(bad, rB); s.phase_field(diagnostics=True)
    g = s.integrals()
    _check_one_bad_cell(clean, g.planes, hole, fields, "rk3d")
    assert g.nonfinite == 1
    s.close()


# ---------------------------------------------------------------------------------------------- 6. stale state
def test_stale_diagnostics_are_refused(box):
    from openlbmpm_amd._lib import ERR_STATE, LbmpmError
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    dom, rR, rB = box
    s = _pert(dom)
    s.set_density(rR, rB)
    s.phase_field(diagnostics=True)
    s.integrals()
    s.step_single(1)
    with pytest.raises(LbmpmError) as e:
        s.integrals()
    assert e.value.status == ERR_STATE and "stale" in str(e.value)
    s.phase_field(diagnostics=True)
    s.integrals()
    s.close()
    c = RK3DCSFSolver(dom, CSF_PAR)
    with pytest.raises(LbmpmError) as e:
        c.integrals()                       # before set_macro / set_pdf
    assert e.value.status == ERR_STATE
    c.close()
