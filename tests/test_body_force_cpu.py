"""The body force of the 3-D CSF solver, without a GPU: the conditions that make tests/test_rk3d_csf_body_force_gpu.py meaningful.

* the reference recipe (tests/body_force_ref.py, built around the unchanged oracle) with g = 0 IS oracle.run, has no preferred direction in
  the (x, y) plane, stays in the regime at the points the GPU module compares, and feels every one of the six components there;
* the recipe's physics: a hydrostatic column (one and two layers) and the force-driven plane Poiseuille profile;
* plumbing: the three Python classes, the ini keys, the drivers' argument and the command line reach lbmpm_rk3dcsf_set_body_force; the
  force is no configuration parameter."""
import ctypes as C

import numpy as np
import pytest

import body_force_ref as R
import param_points as P
from helpers import rel_err
from oracle.rk3dcsf import RK3DCSFOracle
from test_param_points_cpu import _Capture

TOL_GPU = 1e-10                  # TOL of tests/test_rk3d_csf_gpu.py: what the GPU module holds the kernels to against the recipe
FIELDS = ("fR", "fB", "rhoR", "rhoB", "phi", "vx", "vy", "vz", "Gx", "Gy", "Gz", "Fx", "Fy", "Fz", "K")
POINTS = (("A", "G1"), ("B", "G2"))


def point_params(point, **over):
    return {k: v for k, v in P.params(P.TABLES["rk3dcsf"], point, **over).items() if k != "variant"}


def field_differences(a, b, fl):
    """{field: field-relative difference}, vector components against the vector's largest magnitude"""
    out = {}
    for f in FIELDS:
        scale = None
        if f[0] in "vGF" and len(f) == 2:
            scale = max(max(float(np.max(np.abs(b.field(f[0] + c)[fl]))) for c in "xyz"), 1e-300)
        out[f] = rel_err(a.field(f)[fl], b.field(f)[fl], scale=scale)
    return out


@pytest.mark.parametrize("relax", ["SRT", "MRT"])
@pytest.mark.parametrize("point", ["A", "B"])
def test_without_a_force_the_recipe_is_the_oracle(point, relax):
    dom, rR, rB = P.lattice_csf()
    par = point_params(point, relax=relax)
    a = R.BodyForceRef(dom, rR, rB, par).run(P.STEPS)
    o = RK3DCSFOracle(dom, rR, rB, dict(par, crisp=R.CRISP)).run(P.STEPS)
    d = field_differences(a, o, dom == 1)
    print("recipe with g = 0 against oracle.run, %s %s: %s" % (point, relax, {k: v for k, v in d.items() if v}))
    assert max(d.values()) < 0.1 * TOL_GPU, d


@pytest.mark.parametrize("relax", ["SRT", "MRT"])
def test_exchanging_x_and_y_exchanges_the_fields(relax):
    """as tests/test_oracle_rk3d_csf.py, with the accelerations' x and y exchanged too"""
    dom, rR, rB = P.lattice_csf()
    par = dict(relax=relax, theta=50.0, tauB=0.8)
    gr, gb = R.G_SETS["G1"]
    a = R.BodyForceRef(dom, rR, rB, par, gr, gb).run(25)
    t = lambda f: np.ascontiguousarray(np.swapaxes(f, 1, 2))
    sw = lambda g: (g[1], g[0], g[2])
    b = R.BodyForceRef(t(dom), t(rR), t(rB), par, sw(gr), sw(gb)).run(25)
    for fa, fb in (("rhoR", "rhoR"), ("rhoB", "rhoB"), ("phi", "phi"), ("vx", "vy"), ("vy", "vx"), ("vz", "vz"), ("Gx", "Gy"), ("Gy", "Gx"),
                   ("Gz", "Gz"), ("Fx", "Fy"), ("Fy", "Fx"), ("Fz", "Fz"), ("K", "K")):
        x, y = a.field(fa), t(b.field(fb))
        scale = max(np.max(np.abs(a.field(fa[0] + c))) for c in "xyz") if fa[0] in "vGF" and len(fa) == 2 else None
        assert rel_err(y, x, scale=scale) < 1e-8, (fa, fb)
    plain = RK3DCSFOracle(dom, rR, rB, dict(par, crisp=R.CRISP)).run(25)
    assert rel_err(a.field("vy"), plain.field("vy"), scale=float(np.max(np.abs(plain.field("vz"))))) > 1e-4      # the force is felt


_ref = {}


def reference(point, gset, relax="MRT", drop=None):
    key = (point, gset, relax, drop)
    if key not in _ref:
        dom, rR, rB = P.lattice_csf()
        g = [list(v) for v in R.G_SETS[gset]]
        if drop is not None:
            g[drop // 3][drop % 3] = 0.0
        _ref[key] = R.BodyForceRef(dom, rR, rB, point_params(point, relax=relax), *g).run(P.STEPS)
    return _ref[key]


@pytest.mark.parametrize("relax", ["SRT", "MRT"])
@pytest.mark.parametrize("point,gset", POINTS)
def test_regime(point, gset, relax):
    r = reference(point, gset, relax)
    fl = r.fl
    for f in FIELDS:
        assert np.all(np.isfinite(r.field(f))), f
    u = np.sqrt(sum(r.field(c) ** 2 for c in ("vx", "vy", "vz")))
    assert float(u.max()) < 0.1, float(u.max())
    assert float((r.field("rhoR") + r.field("rhoB"))[fl].min()) > 0.0
    assert float(r.field("rhoR")[fl].min()) >= 0.0 and float(r.field("rhoB")[fl].min()) >= 0.0
    g = np.array(R.G_SETS[gset]).reshape(-1)
    assert len(set(np.abs(g))) == 6 and np.all(g != 0.0) and tuple(R.G_SETS[gset][0]) != tuple(R.G_SETS[gset][1])


@pytest.mark.parametrize("component", range(6), ids=["gRx", "gRy", "gRz", "gBx", "gBy", "gBz"])
@pytest.mark.parametrize("point,gset", POINTS)
def test_every_component_matters(point, gset, component):
    ref, got = reference(point, gset), reference(point, gset, drop=component)
    d = field_differences(got, ref, ref.fl)
    d.pop("K")                   # (ill-conditioned where |G| is small: not counted, as in tests/test_param_points_cpu.py)
    f = max(d, key=d.get)
    print("%s %s: component %d set to zero moves %s by %.2e" % (point, gset, component, f, d[f]))
    assert d[f] >= 1000.0 * TOL_GPU, (f, d[f])


# ------------------------------------------------------------------------------------------------ the recipe's physics
@pytest.mark.parametrize("relax", ["SRT", "MRT"])
@pytest.mark.parametrize("layers", [1, 2])
def test_hydrostatic_column(layers, relax):
    """bound: 0.5 % on the density drop across the gap against 3 sum F_b (tests/body_force_ref.py: hydrostatic_errors).  Measured, recipe and
    GPU alike: 0.338 % (one layer, SRT), 0.323 % (MRT), 0.340 % / 0.327 % (two layers); per pair of cells 0.44 - 0.46 %; max |u| 4.9e-5 and
    1.5e-5 = g / 2 of the fluid at the far wall.  The two layers are run without surface tension (hydrostatic_case says why)"""
    dom, rR, rB, par, g = R.hydrostatic_case(layers, relax)
    r = R.BodyForceRef(dom, rR, rB, par, *g).run(R.HYDROSTATIC_STEPS)
    drop, cell, umax = R.hydrostatic_errors(r.field("rhoR") + r.field("rhoB"), r.body_force_density()[0],
                                            max(float(np.max(np.abs(r.field(c)))) for c in ("vx", "vy", "vz")))
    print("hydrostatic column, %d layer(s), %s: drop off 3 sum F_b by %.3f %%, per cell %.3f %%, max |u| %.2e" % (layers, relax, 100 * drop, 100 * cell, umax))
    assert drop < R.HYDROSTATIC_DROP_BOUND and cell < 2 * R.HYDROSTATIC_DROP_BOUND and umax < 1e-4


@pytest.mark.parametrize("relax", ["SRT", "MRT"])
def test_force_driven_poiseuille(relax):
    """bound: 2 % on the profile.  Measured, recipe and GPU alike: worst 1.08 % (SRT) and 0.74 % (MRT) at the wall cells, 0.13 % and 0.47 % at
    the centre"""
    dom, rR, rB, par, g = R.poiseuille_case(relax)
    r = R.BodyForceRef(dom, rR, rB, par, *g).run(R.POISEUILLE_STEPS)
    worst, centre = R.poiseuille_errors(r.field("vz"))
    print("force-driven Poiseuille, %s: worst deviation %.3f %%, at the centre %.3f %%" % (relax, 100 * worst, 100 * centre))
    assert worst < R.POISEUILLE_BOUND and centre < R.POISEUILLE_BOUND


# ------------------------------------------------------------------------------------------------ plumbing
class _Calls(_Capture):
    """_Capture that also records the six doubles of every lbmpm_rk3dcsf_set_body_force (None: switched off) and hands them back"""

    def __init__(self):
        _Capture.__init__(self)
        self.forces = []

    def __getattr__(self, fn):
        if fn == "lbmpm_rk3dcsf_set_body_force":
            def call(h, gr, gb):
                self.forces.append(None if gr is None and gb is None else (tuple(gr), tuple(gb)))
                return 0
            return call
        if fn == "lbmpm_rk3dcsf_get_body_force":
            def call(h, gr, gb):
                last = (self.forces[-1] if self.forces else None) or ((0., 0., 0.), (0., 0., 0.))
                gr[:], gb[:] = last[0], last[1]
                return 0
            return call
        return _Capture.__getattr__(self, fn)


@pytest.fixture
def calls(monkeypatch):
    from openlbmpm_amd import _lib
    cap = _Calls()
    monkeypatch.setattr(_lib, "lib", lambda: cap)
    return cap


GR, GB = (1.0e-5, -2.0e-5, 3.0e-5), (-2.5e-5, 1.5e-5, -6.0e-5)


def test_the_solver_hands_over_six_doubles(calls):
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    s = RK3DCSFSolver(np.ones((8, 8, 8), np.uint8))
    s.set_body_force(GR)
    s.set_body_force(red=GR, blue=GB)
    s.set_body_force(GR, blue=GB)
    s.set_body_force(blue=GB)
    assert s.body_force == ((0., 0., 0.), GB)
    s.set_body_force(None)
    s.set_body_force()
    assert calls.forces == [(GR, GR), (GR, GB), (GR, GB), ((0., 0., 0.), GB), None, None]
    for bad in ((1., 2.), 3.0, (1., 2., 3., 4.), ((1., 2., 3.),)):
        with pytest.raises(ValueError):
            s.set_body_force(bad)
    with pytest.raises(ValueError):
        s.set_body_force(GR, blue=(1., 2.))
    assert len(calls.forces) == 6


def test_the_cluster_and_the_distributed_class_reach_every_slab(calls):
    from openlbmpm_amd import _lib, rk3dcsf
    c = rk3dcsf.RK3DCSFCluster(np.ones((24, 6, 6), np.uint8), nslabs=3)
    c.set_body_force(red=GR, blue=GB)
    assert calls.forces == [(GR, GB)] * 3 and c.body_force == (GR, GB)
    c.set_body_force(None)
    assert calls.forces[3:] == [None] * 3
    with pytest.raises(_lib.LbmpmError) as e:
        c.set_body_force((0., float("nan"), 0.))              # refused before any slab is changed
    assert e.value.status == _lib.ERR_INVALID and len(calls.forces) == 6
    d = rk3dcsf.RK3DCSFDistributed.__new__(rk3dcsf.RK3DCSFDistributed)      # (one slab per rank: the rank's slab, without a process group)
    d.slab = c.slabs[1]
    d.set_body_force(GB, red=GR)
    assert calls.forces[6:] == [(GR, GB)] and d.body_force == (GR, GB)


def test_the_force_is_no_configuration_parameter():
    from openlbmpm_amd import _lib, rk3dcsf
    assert sorted(rk3dcsf.DEFAULT_PARAMS) == sorted(
        ["sigma", "theta", "wetting", "beta", "delta", "tauR", "tauB", "tautype", "relax", "inlet", "outlet", "velocityZR", "velocityZB", "densityBH",
         "densityRH", "densityBL", "densityRL", "rates", "variant", "bulk_epsilon"])
    assert [f for f, _ in _lib.RK3DCSFConfig._fields_] == [
        "nx", "ny", "nz", "surface_tension", "contact_angle_deg", "beta", "delta", "tau_r", "tau_b", "inlet_velocity_z", "inlet_rho_r", "inlet_rho_b",
        "outlet_rho_total", "wetting_type", "tau_type", "relaxation", "inlet_type", "outlet_type", "device", "variant", "mrt_rates", "bulk_epsilon",
        "ghost_lo", "ghost_hi", "slab_z0", "global_nz"]


BODY_FORCE_INI = """
[BodyForce]
isBodyForce = 'yes'
bodyForceX = 1.0e-5
bodyForceY = -2.0e-5
bodyForceZ = 3.0e-5
"""


class _Out:
    def __init__(self):
        self.written = {}

    def write(self, group, name, array):
        self.written["/%s/%s" % (group, name)] = np.array(array)


def test_the_ini_and_the_drivers_argument_reach_the_solver(tmp_path, calls):
    from ini_fixtures import write_rk3d, write_rk3d_csf, write_transport
    from openlbmpm_amd import config
    from openlbmpm_amd.RKColorGradientD3Q19 import RKColorGradient3D, _CSFSlab, duct
    from openlbmpm_amd.Transport3DRK import Transport3DRK
    d = str(tmp_path)
    write_rk3d_csf(d, nx=8, ny=8, nz=12, steps=4, relax="MRT")
    assert config.read_rk3d(d)["body_force"] is None and RKColorGradient3D(d).body_force is None
    ini = tmp_path / "RKtwophasesetup3D.ini"
    plain = ini.read_text()
    ini.write_text(plain + BODY_FORCE_INI)
    assert config.read_rk3d(d)["body_force"] == dict(red=GR, blue=GR)
    ini.write_text(plain + BODY_FORCE_INI + "bodyForceXB = -2.5e-5\nbodyForceYB = 1.5e-5\nbodyForceZB = -6.0e-5\nbodyForceZR = 3.0e-5\n")
    assert config.read_rk3d(d)["body_force"] == dict(red=GR, blue=GB)
    write_transport(d)
    for make in (RKColorGradient3D, Transport3DRK):
        for arg, want in ((None, (GR, GB)), (GB, (GB, GB)), (dict(red=GB, blue=GR), (GB, GR)), (dict(blue=GR), ((0., 0., 0.), GR))):
            sim = make(d, body_force=arg)
            solver = _CSFSlab(duct(8, 8, 12), sim.par, 0).solver
            out = _Out()
            sim._apply_body_force(solver, out)
            assert calls.forces[-1] == want, (make.__name__, arg)
            assert np.array_equal(out.written["/BodyForce/Acceleration"], np.array(want)) and out.written["/BodyForce/Acceleration"].shape == (2, 3)
        for bad in ((1., 2.), dict(green=GR), "down"):
            with pytest.raises(config.ConfigError):
                make(d, body_force=bad)
    # the perturbation model's solver has no force term
    write_rk3d(d, nx=8, ny=8, nz=12, steps=4)
    with pytest.raises(config.ConfigError):
        RKColorGradient3D(d, body_force=GR)
    with pytest.raises(config.ConfigError):
        Transport3DRK(d, body_force=GR)
    ini.write_text(ini.read_text() + BODY_FORCE_INI)
    with pytest.raises(config.ConfigError):
        config.read_rk3d(d)
    ini.write_text(ini.read_text().replace("isBodyForce = 'yes'", "isBodyForce = 'no'"))
    assert RKColorGradient3D(d).body_force is None


def test_the_2d_drivers_keep_their_refusal(tmp_path):
    from ini_fixtures import write_rk
    from openlbmpm_amd import config
    write_rk(str(tmp_path))
    ini = tmp_path / "RKtwophasesetup2D.ini"
    text = ini.read_text()
    assert "[BodyForce]" in text
    ini.write_text(text.replace("[BodyForce]", "[BodyForce]\nisBodyForce = 'yes'"))
    with pytest.raises(config.ConfigError):
        config.read_rk2d(str(tmp_path))


def test_the_command_line_reaches_the_drivers(monkeypatch):
    from openlbmpm_amd import RKColorGradientD3Q19, Transport3DRK, __main__ as cli
    seen = {}

    class Fake:
        timeSteps, steady_step, voidSpace = 1, None, 1

        def __init__(self, ini, **kw):
            seen.update(kw)

        def runRKColorGradient3D(self):
            return "x"

        def runTransport3DMPMCRK(self):
            return ("x", "y")

    monkeypatch.setattr(RKColorGradientD3Q19, "RKColorGradient3D", Fake)
    monkeypatch.setattr(Transport3DRK, "Transport3DRK", Fake)
    for model in ("rk3d", "tr3d"):
        for argv, want in (([], None), (["--body-force", "1e-5", "-2e-5", "3e-5"], GR),
                           (["--body-force", "1e-5", "-2e-5", "3e-5", "--body-force-blue", "-2.5e-5", "1.5e-5", "-6e-5"], dict(red=GR, blue=GB)),
                           (["--body-force-blue", "-2.5e-5", "1.5e-5", "-6e-5"], dict(red=(0., 0., 0.), blue=GB))):
            seen.clear()
            assert cli.main([model, "somewhere"] + argv) == 0
            assert seen["body_force"] == want, (model, argv)
    with pytest.raises(SystemExit):
        cli.main(["rk", "somewhere", "--body-force", "1e-5", "0", "0"])


# ------------------------------------------------------------------------------------------------ the code object
# (vgpr_count, sgpr_count, scratch bytes per lane) of the two collisions before the body force existed, by template arguments:
# csf3d_collide<FIRST, MRT, DIAG, TR>, csf3d_collide_deep<MRT, DIAG, TR>
BEFORE = {
    "csf3d_collide": {(0, 0, 0, 0): (168, 106, 36), (0, 0, 0, 1): (168, 106, 52), (0, 0, 1, 0): (168, 106, 52), (0, 0, 1, 1): (168, 106, 52),
                      (1, 0, 0, 0): (167, 106, 28), (1, 0, 0, 1): (168, 106, 44), (1, 0, 1, 0): (168, 106, 44), (1, 0, 1, 1): (168, 106, 44),
                      **{(f, 1, d, t): (256, 106, 36) for f in (0, 1) for d in (0, 1) for t in (0, 1)}},
    "csf3d_collide_deep": {(0, 0, 0): (82, 100, 0), (0, 0, 1): (85, 105, 0), (0, 1, 0): (85, 105, 0), (0, 1, 1): (85, 106, 0),
                           (1, 0, 0): (133, 106, 0), (1, 0, 1): (134, 106, 0), (1, 1, 0): (133, 106, 0), (1, 1, 1): (134, 106, 0)},
}


def test_without_a_force_the_step_launches_the_kernels_it_had():
    """the instances with BF = false have the registers, the scratch (hence the occupancy: the launch bounds are the same) of the kernels
    before the body force; the new instances of the deep kernel use no scratch, those of the full path none beyond their twins'"""
    import os
    import re
    from openlbmpm_amd import codeobj
    from test_codeobj import LIB
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    seen = {}
    for name, m in codeobj.kernels(LIB).items():
        k = re.search(r"\d+(csf3d_collide(?:_deep)?)I((?:Lb[01]E)+)E", name)
        if k:
            args = tuple(int(b) for b in re.findall(r"Lb([01])E", k.group(2)))
            seen[(k.group(1), args)] = (m[".vgpr_count"], m[".sgpr_count"], m[".private_segment_fixed_size"])
    assert len(seen) == 2 * 16 + 2 * 8
    for kernel, table in BEFORE.items():
        for args, want in table.items():
            assert seen[(kernel, args + (0,))] == want, (kernel, args, seen[(kernel, args + (0,))], want)
            new = seen[(kernel, args + (1,))]
            print("%s<%s, BF>: %d VGPRs, %d SGPRs, %d bytes of scratch (without: %s)" % (kernel, ", ".join(map(str, args)), new[0], new[1], new[2], want))
            assert new[2] <= want[2] and new[0] <= 256, (kernel, args, new)
