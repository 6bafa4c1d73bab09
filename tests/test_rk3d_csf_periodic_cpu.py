"""Periodic z of the 3-D CSF solver without a GPU: the reference's own conditions (tests/periodic_ref.py), the ini readers, the drivers'
mask and result file, and what the Python classes hand to the library."""
import numpy as np
import pytest

import body_force_ref as R
import periodic_ref as PR
from helpers import rel_err
from test_param_points_cpu import _Capture

G1 = R.G_SETS["G1"]
# The GPU tests hold the solver to 1e-10 of this reference; the reference's own error -- what is left of the model's symmetry after
# rounding -- has to stay a decade below that to be worth the name.
SELF_TOL = 1.0e-11


# ------------------------------------------------------------------------------------------------ the reference
def _fields(ref):
    return {f: ref.field(f) for f in ("rhoR", "rhoB", "phi", "K", "vx", "vy", "vz", "Fx", "Fy", "Fz", "fR", "fB")}


@pytest.mark.parametrize("relax,tautype", [("SRT", 1), ("SRT", 2), ("MRT", 1), ("MRT", 2)])
def test_the_transposed_oracle_is_a_periodic_reference(relax, tautype):
    """On the parity lattice: (a) the seal holds -- the oracle's four open planes are solid, every value stays finite and the colours'
    masses are conserved to 1e-12, which an open plane that acted would break; (b) the model is symmetric under a permutation of the
    axes -- the same lattice with its two periodic axes (y and z) exchanged gives the exchanged fields; together: the unchanged oracle
    computes the z-periodic model"""
    dom, rR, rB = PR.parity_lattice()
    par = PR.parity_params(relax, tautype)
    a = PR.PeriodicRef(dom, rR, rB, par, *G1)
    assert PR.sealed(dom) and not np.any(a.ref.dom[:2] == 1) and not np.any(a.ref.dom[-2:] == 1)
    yz = lambda f: np.ascontiguousarray(np.swapaxes(f, 0, 1))
    g = lambda v: (v[0], v[2], v[1])
    b = PR.PeriodicRef(yz(dom), yz(rR), yz(rB), par, g(G1[0]), g(G1[1]))
    m0 = (float(rR.sum()), float(rB.sum()))
    # direction i of the y-z exchanged lattice
    YZ = [[j for j in range(19) if (R.CX[j], R.CY[j], R.CZ[j]) == (R.CX[i], R.CZ[i], R.CY[i])][0] for i in range(19)]
    names = dict(vy="vz", vz="vy", Fy="Fz", Fz="Fy")
    done = 0
    for k in (1, 9, 40):
        a.run(k - done); b.run(k - done)
        done = k
        fa, fb = _fields(a), _fields(b)
        fl = a.fl
        umax = max(float(np.max(np.abs(fa[c][fl]))) for c in ("vx", "vy", "vz"))
        fmax = max(float(np.max(np.abs(fa[c][fl]))) for c in ("Fx", "Fy", "Fz"))
        for f, x in fa.items():
            assert np.all(np.isfinite(x)), (k, f)
            y = yz(fb[names.get(f, f)])
            if y.ndim == 4:
                y = y[..., YZ]
            e = rel_err(x[fl], y[fl], scale=umax if f[0] == "v" else (fmax if f[0] == "F" else None))
            assert e < SELF_TOL, "step %d: %s differs by %.3e from the run with y and z exchanged" % (k, f, e)
        assert abs(float(fa["rhoR"].sum()) / m0[0] - 1.) < 1e-12 and abs(float(fa["rhoB"].sum()) / m0[1] - 1.) < 1e-12, k
    assert np.max(np.abs(fa["K"])) > 1e-3 and np.max(np.abs(fa["vz"])) > 1e-5       # an interface with curvature, a flow along z


def test_the_reference_refuses_a_lattice_that_is_not_sealed():
    dom, rR, rB = PR.parity_lattice()
    dom[3, 3, 1] = 1
    with pytest.raises(ValueError):
        PR.PeriodicRef(dom, rR, rB, PR.parity_params("MRT", 2))


def test_the_free_lattice_keeps_its_blocks_under_the_rolls():
    """what tests/periodic_ref.py says about the 16^3 lattice: a roll by k <= 8 renumbers the fluid cells by k * 256 round the ring"""
    dom, _, _ = PR.free_lattice()
    cells = np.flatnonzero(dom.reshape(-1) == 1)
    assert cells.size == 15 * 256
    number = -np.ones(dom.size, dtype=np.int64)
    number[cells] = np.arange(cells.size)
    for k in PR.ROLLS:
        rolled = np.roll(dom, k, axis=0)
        rc = np.flatnonzero(rolled.reshape(-1) == 1)
        assert np.array_equal(np.roll(number.reshape(dom.shape), k, axis=0).reshape(-1)[rc], (np.arange(rc.size) - k * 256) % cells.size)


def test_the_analytic_two_layer_profile():
    """no slip at both walls, continuous velocity and stress at the interface, nu u'' = -g in either layer"""
    g, n1, n2 = PR.TWO_LAYER["g_z"], (1.0 - 0.5) / 3., (0.7 - 0.5) / 3.
    u = PR.two_layer_profile
    e = 1e-4
    assert abs(u(0.)) < 1e-18 and abs(u(32.)) < 1e-18 and abs(u(16. - 1e-9) - u(16. + 1e-9)) < 1e-12
    assert abs(n1 * (u(16. - e) - u(16. - 2 * e)) / e - n2 * (u(16. + 2 * e) - u(16. + e)) / e) < 1e-4 * g * 16.
    for s, n in ((7.3, n1), (25.1, n2)):
        assert abs(n * (u(s + e) - 2. * u(s) + u(s - e)) / (e * e) + g) < 1e-3 * g
    assert PR.two_layer_errors(u(np.arange(32) + 0.5))[2] == 0.0


# ------------------------------------------------------------------------------------------------ the ring box
def ring_classes(name, dom=None):
    """the class field (0 solid, 1 R, 2 B) of a prescribed sharp pattern on the ring box"""
    dom = PR.ring_box() if dom is None else dom
    rR, rB = PR.ring_densities(name, dom)
    return np.where(dom == 1, np.where(rR > rB, 1, 2), 0).astype(np.uint8)


def seam_rows(table, nz=12):
    """the R rows of a cluster table that touch the first plane and not the last, and the other way round"""
    red = table[table[:, 1] == 1]
    return red[(red[:, 3] == 0) & (red[:, 4] < nz - 1)], red[(red[:, 3] > 0) & (red[:, 4] == nz - 1)]


UPWARDS = ("RR_z", "BB_z", "RB_z", "RS_z", "BS_z", "sq_R_xz", "sq_R_yz", "sq_B_xz", "sq_B_yz", "cube_R", "cube_B")


def test_the_ring_box_is_made_for_a_ring():
    dom = PR.ring_box()
    fl = dom == 1
    assert dom.shape == (12, 33, 70) and dom.dtype == np.uint8
    for a, b in ((0, 11), (0, 1), (11, 10), (1, 10)):
        assert not np.array_equal(dom[a], dom[b]), (a, b)
    assert not fl[[11, 0], 24:28, 8:14].any() and fl[[10, 1], 24:28, 8:14].all()          # a grain across the seam, and only there
    assert int((fl[0] & ~fl[11]).sum()) >= 18 and int((fl[11] & ~fl[0]).sum()) >= 18       # fluid of either plane faces solid across the seam
    assert int(fl[5].sum()) == 5 and not fl[3:9, 7].any()
    assert all(int(fl[z].sum()) > 1500 for z in range(12) if z != 5)
    red = PR.ring_red_cells()
    assert fl[red].all()                                                                   # the ganglion lies in fluid
    for half in (red[9:12], red[0:3]):
        assert all(int(p.sum()) == 60 for p in half)                                       # three planes thick on either side
    assert 0 < int((red[11] & red[0]).sum()) < 60 and not red[3:9].any()                   # the footprints differ and overlap
    c = PR.ring_concentration(dom)
    assert np.all(c[fl] > 0.04) and not np.array_equal(c[0], c[11])


@pytest.mark.parametrize("conn", [6, 18])
def test_the_seam_ganglion_counts_as_two(conn):
    """z does not wrap in the labeller: the ganglion is one red row that starts at plane 0 and one that ends at plane 11, and the same
    classes rolled by six planes -- the seam in the middle -- have fewer clusters.  An implementation that wrapped z would hand out
    another table"""
    from test_clusters_cpu import cpu_label
    cls = ring_classes(PR.SEAM)
    _, tab = cpu_label(cls, conn)
    _, rolled = cpu_label(np.roll(cls, 6, axis=0), conn)
    assert tab.shape[0] > rolled.shape[0], (tab.shape, rolled.shape)
    low, high = seam_rows(tab)
    assert low.shape[0] == 1 and high.shape[0] == 1 and int((tab[:, 1] == 1).sum()) == 2, tab
    assert tuple(low[0, 2:]) == (180, 0, 2) and tuple(high[0, 2:]) == (180, 9, 11)
    red = rolled[rolled[:, 1] == 1]
    assert red.shape[0] == 1 and tuple(red[0, 2:]) == (360, 3, 8)                          # joined, were the seam no end
    # the Python join of slab tables takes the stack as a chain: the cuts of the GPU tests give the undivided table
    from test_clusters_cpu import by_slabs
    for cuts in ([0, 6, 12], [0, 4, 8, 12]):
        assert np.array_equal(by_slabs(cls, conn, cuts)[1], tab), cuts


def test_the_seam_shows_in_the_plane_above_and_in_the_end_rows():
    """for every prescribed pattern: morphology's row 11 with plane 0 as the plane above differs from the row with nothing above in
    columns that reach upwards (a wrapping count would show); the integrals' rows 0 and 1, 10 and 11, and the change table's rows 0 and
    3 differ by more than the comparison's bound (a leftover redirect of an open plane to its neighbour would show)"""
    import change_ref
    from test_clusters_gpu import SHARP
    from test_integrals_gpu import restate
    from test_morphology_cpu import C, cpu_morphology
    dom = PR.ring_box()
    up = [C[n] for n in UPWARDS]
    flat = [c for c in range(28) if c not in up]
    for name in SHARP + (PR.SEAM,):
        rR, rB = PR.ring_densities(name, dom)
        cls = ring_classes(name, dom)
        alone, joined = cpu_morphology(cls, rR + rB), cpu_morphology(cls, rR + rB, above=cls[0])
        assert np.array_equal(alone[:11], joined[:11]) and np.array_equal(alone[11, flat], joined[11, flat])
        assert not np.array_equal(alone[11, up], joined[11, up]), name
        zero = np.zeros(dom.shape)
        now = dict(rhoR=rR, rhoB=rB, vx=zero, vy=zero, vz=zero, phi=np.where(dom == 1, (rR - rB) / np.maximum(rR + rB, 1e-300), 0.0))
        T, A = restate(dom, now)
        for a, b in ((0, 1), (10, 11)):
            assert rows_differ(T, A, a, b, (2, 3)), (name, a, b)
        T, A = change_ref.restate(dom, now, dict(now, phi=-now["phi"]))
        assert rows_differ(T, A, 0, 3, (7,)), name


def rows_differ(T, A, a, b, cols):
    """the columns among `cols` in which the rows a and b of a restated table lie further apart than the two rows' summation bounds
    (2 (n - 1) 2^-53 sum|term| each: tests/test_integrals_gpu.py) together"""
    bound = lambda r: 2.0 * max(T[r, 0] - 1.0, 0.0) * 2.0 ** -53 * A[r]
    return [c for c in cols if abs(T[a, c] - T[b, c]) > bound(a)[c] + bound(b)[c]]


# ------------------------------------------------------------------------------------------------ the Python classes
@pytest.fixture
def seen(monkeypatch):
    from openlbmpm_amd import _lib
    cap = _Capture()
    monkeypatch.setattr(_lib, "lib", lambda: cap)
    return cap.seen


def test_periodic_goes_to_the_two_type_fields_and_nowhere_else(seen):
    from openlbmpm_amd import rk3dcsf
    dom = np.ones((8, 8, 8), np.uint8)
    s = rk3dcsf.RK3DCSFSolver(dom)
    plain = dict(seen)
    assert s.periodic_z is False and plain["inlet_type"] == 0 and plain["outlet_type"] == 0
    s = rk3dcsf.RK3DCSFSolver(dom, dict(inlet="Periodic", outlet="Periodic"))
    assert s.periodic_z is True and seen["inlet_type"] == 2 and seen["outlet_type"] == 2
    assert {k for k in seen if seen[k] != plain[k]} == {"inlet_type", "outlet_type"}
    for one in (dict(inlet="Periodic"), dict(outlet="Periodic"), dict(inlet="Periodic", outlet="Convective"), dict(inlet="Dirichlet", outlet="Periodic")):
        seen.clear()
        for make in (lambda: rk3dcsf.RK3DCSFSolver(dom, one), lambda: rk3dcsf.RK3DCSFCluster(np.ones((16, 8, 8), np.uint8), one, nslabs=2)):
            with pytest.raises(ValueError, match="Periodic"):
                make()
        assert not seen         # refused before anything reaches the library
    c = rk3dcsf.RK3DCSFCluster(np.ones((12, 6, 6), np.uint8), dict(inlet="Periodic", outlet="Periodic"), nslabs=3)
    assert c.periodic_z is True and all(s.periodic_z for s in c.slabs) and seen["inlet_type"] == 2 and seen["ghost_lo"] == 2 and seen["global_nz"] == 12
    assert rk3dcsf.RK3DCSFCluster(np.ones((16, 6, 6), np.uint8), nslabs=2).periodic_z is False
    assert rk3dcsf._periodic_params(None) is False and rk3dcsf._periodic_params(dict(inlet="Periodic", outlet="Periodic")) is True


def test_the_other_solvers_do_not_know_the_word(seen):
    from openlbmpm_amd import rk2d, rk3d
    for make in (lambda p: rk3d.RK3DSlab(np.ones((8, 8, 8), np.uint8), 0, 8, p), lambda p: rk2d.RK2DSolver(np.ones((8, 8), np.uint8), p)):
        for p in (dict(inlet="Periodic", outlet="Periodic"), dict(inlet="Periodic"), dict(outlet="Periodic")):
            with pytest.raises((ValueError, KeyError)):
                make(p)


# ------------------------------------------------------------------------------------------------ the ini readers and the drivers
def _periodic_ini(tmp_path, inlet="'Periodic'", outlet="'Periodic'", csf=True, **kw):
    from ini_fixtures import write_rk3d, write_rk3d_csf
    d = str(tmp_path)
    (write_rk3d_csf if csf else write_rk3d)(d, **kw)
    ini = tmp_path / "RKtwophasesetup3D.ini"
    text = ini.read_text()
    assert "BoundaryTypeInlet = 'Neumann'" in text and "BoundaryTypeOutlet = 'Dirichlet'" in text
    ini.write_text(text.replace("BoundaryTypeInlet = 'Neumann'", "BoundaryTypeInlet = " + inlet).replace("BoundaryTypeOutlet = 'Dirichlet'", "BoundaryTypeOutlet = " + outlet))
    return d, ini


def test_read_rk3d(tmp_path):
    from openlbmpm_amd import config
    d, ini = _periodic_ini(tmp_path, nx=8, ny=8, nz=12, steps=4, relax="MRT")
    p = config.read_rk3d(d)
    assert p["periodic_z"] is True and p["inlet"] == "Periodic" and p["outlet"] == "Periodic" and p["tension_type"] == "CSF"
    assert p["velocityZB"] == -1.0e-4 and p["densityRL"] == 1.0e-8          # read as ever, used by nobody
    ini.write_text(ini.read_text().replace("NeumannType = 'ZouHe'", "NeumannType = 'Chang'"))
    assert config.read_rk3d(d)["periodic_z"] is True                        # NeumannType is not looked at
    for inlet, outlet in (("'Periodic'", "'Dirichlet'"), ("'Neumann'", "'Periodic'"), ("'Periodic'", "'Convective'")):
        d, _ = _periodic_ini(tmp_path, inlet, outlet, nx=8, ny=8, nz=12, steps=4)
        with pytest.raises(config.ConfigError, match="Periodic"):
            config.read_rk3d(d)
    d, _ = _periodic_ini(tmp_path, csf=False, nx=8, ny=8, nz=12, steps=4)
    with pytest.raises(config.ConfigError, match="CSF"):
        config.read_rk3d(d)
    d, _ = _periodic_ini(tmp_path, "'Neumann'", "'Dirichlet'", nx=8, ny=8, nz=12, steps=4)
    assert config.read_rk3d(d)["periodic_z"] is False


def test_read_transport3d(tmp_path):
    from ini_fixtures import write_transport
    from openlbmpm_amd import config
    d = str(tmp_path)
    write_transport(d)
    ini = tmp_path / "transportsetup.ini"
    text = ini.read_text()
    assert config.read_transport3d(d)["inlet_type"] == "Dirichlet"          # between open planes: as ever
    with pytest.raises(config.ConfigError, match="periodic"):
        config.read_transport3d(d, periodic_z=True)
    closed = text.replace("InletType = 'Dirichlet'", "InletType = 'Periodic'")
    ini.write_text(closed)
    with pytest.raises(config.ConfigError, match="Freeflow"):
        config.read_transport3d(d, periodic_z=True)
    ini.write_text(text.replace("OutletType = 'Freeflow'", "OutletType = 'VonNeumann'"))
    with pytest.raises(config.ConfigError, match="Dirichlet"):
        config.read_transport3d(d, periodic_z=True)
    ini.write_text(closed.replace("OutletType = 'Freeflow'", "OutletType = 'VonNeumann'"))
    p = config.read_transport3d(d, periodic_z=True)
    assert p["inlet_type"] == "Periodic" and p["outlet_type"] == "VonNeumann"


class _Out:
    def __init__(self):
        self.written = {}

    def write(self, group, name, array):
        self.written["/%s/%s" % (group, name)] = np.array(array)


def test_the_drivers_take_the_mask_as_given_and_mark_the_file(tmp_path, seen, monkeypatch):
    from ini_fixtures import write_transport
    from openlbmpm_amd import RKColorGradientD3Q19 as D, config
    from openlbmpm_amd.Transport3DRK import Transport3DRK
    d, ini = _periodic_ini(tmp_path, nx=8, ny=6, nz=12, steps=4, relax="MRT")
    sim = D.RKColorGradient3D(d, output_dir=str(tmp_path / "out"))
    assert sim.periodic_z is True
    sim.initializeDomainBorder()
    assert np.array_equal(sim.isDomain, D.duct(8, 6, 12))                   # the four side walls, nothing at the ends
    # a voxel file: its side walls, no buffer planes
    vox = np.ones((9, 6, 8), np.uint8); vox[2:4, 2:4, 3:5] = 0
    np.save(tmp_path / "v.npy", vox)
    ini.write_text(ini.read_text().replace("Existance = 'no'", "Existance = 'yes'"))
    img = D.RKColorGradient3D(d, structure_path=str(tmp_path / "v.npy"), num_buffering_layers=5)
    img.initializeDomainBorder()
    from openlbmpm_amd.geometry import voxel_domain
    assert img.isDomain.shape == (9, 6, 8) and np.array_equal(img.isDomain, voxel_domain(vox, 0))
    given = np.ones((10, 6, 8), np.uint8); given[0, 2, 2] = 0               # an array: as given, ends that do not repeat
    arr = D.RKColorGradient3D(d, domain=given)
    arr.initializeDomainBorder()
    assert np.array_equal(arr.isDomain, given)
    # the solver is asked for periodic z, and the result file says so
    h = sim._open_solver()
    assert h.solver.periodic_z is True and seen["inlet_type"] == 2 and seen["outlet_type"] == 2
    made = {}

    class File(_Out):
        def __init__(self, directory, name, groups):
            _Out.__init__(self)
            self.path, made["groups"], made["file"] = "x", list(groups), self
    monkeypatch.setattr(D, "ResultFile", File)
    sim._open_flow_file(h, [], True)
    assert np.array_equal(made["file"].written["/BoundaryCondition/PeriodicZ"], [1]) and "BoundaryCondition" in [g for g, _ in made["groups"]]
    # between open planes the file has no such group
    d2 = tmp_path / "open"; d2.mkdir()
    _periodic_ini(d2, "'Neumann'", "'Dirichlet'", nx=8, ny=6, nz=12, steps=4)
    plain = D.RKColorGradient3D(str(d2))
    plain.initializeDomainBorder()
    plain._open_flow_file(plain._open_solver(), [], True)
    assert plain.periodic_z is False and "/BoundaryCondition/PeriodicZ" not in made["file"].written and "BoundaryCondition" not in [g for g, _ in made["groups"]]
    # the tracers' driver: the shipped transport file asks for the inlet and outlet rules -- refused; without them it runs periodic
    ini.write_text(ini.read_text().replace("Existance = 'yes'", "Existance = 'no'"))
    write_transport(d)
    with pytest.raises(config.ConfigError, match="periodic"):
        Transport3DRK(d)
    tr = tmp_path / "transportsetup.ini"
    tr.write_text(tr.read_text().replace("InletType = 'Dirichlet'", "InletType = 'Periodic'").replace("OutletType = 'Freeflow'", "OutletType = 'VonNeumann'"))
    t = Transport3DRK(d)
    assert t.periodic_z is True and t.tr["inlet_type"] == "Periodic"
    t.initializeDomainBorder()
    t._open_solver()
    assert seen["inlet_type"] == 2 and seen["outlet_type"] == 2
