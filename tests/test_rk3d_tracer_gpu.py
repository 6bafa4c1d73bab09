"""D3Q7 tracers advected by the 3-D CSF flow on the GPU (lbmpm_rk3dcsf_tracer_*, csrc/rk3d_tracer.h) through the C ABI.

* against the CPU restatement tests/tr3d_ref.py (pinned by reduction to the 2-D oracle, tests/test_tr3d_ref.py) on fully 3-D lattices:
  concentration and populations, 1e-10 field-relative -- the tolerance tests/test_rk3d_csf_gpu.py holds the 3-D flow to;
* the reduction itself through the HIP kernels: a y-uniform lattice against the 2-D oracle composition (1e-9), under every open plane
  of the flow;
* what the reduction cannot see: exchanging x and y exchanges the flow and the tracers (1e-8);
* the bulk skip stays exact, the flow is untouched, the restart is bit for bit, the tracer is conserved, a Gaussian blob spreads as 2 D t,
  and as D + D^T under a full tensor;
* the refusals."""
import numpy as np
import pytest

from helpers import rel_err
from tr3d_ref import Coupled3DRef, project_g

pytestmark = pytest.mark.gpu

TOL = 1e-10          # (measured over the 20 cases and 200 steps: 6e-15 at worst)
CRISP = 2.0 ** -51           # the library's "one colour alone" rule, which the flow oracle can follow (tests/test_rk3d_csf_gpu.py)


def solver(dom, par, **kw):
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    return RK3DCSFSolver(dom, par, **kw)


def tracer_case(nT, reaction=True, **over):
    """(keyword arguments of RK3DCSFSolver.configure_tracers, the same case for tests/tr3d_ref.py)"""
    dx, dy, dz = (1. / 6., 0.1, 0.2, 0.15)[:nT], (0.12, 0.1, 0.15, 0.2)[:nT], (0.2, 0.08, 0.1, 0.12)[:nT]
    k = dict(num_tracers=nT, diffusion_x=dx, diffusion_y=dy, diffusion_z=dz, diffusion_xy=0.01, diffusion_yx=-0.02, diffusion_xz=0.03, diffusion_zx=0.015,
             diffusion_yz=-0.01, diffusion_zy=0.02, beta_interface=(1.0, 0.5, 0.0, 0.8)[:nT], criteria_rho=0.5, inlet_concentration=(0.8, 0.4, 0.0, 0.2)[:nT],
             dirichlet_inlet=True, free_outlet=True, reaction_rate=0.03 if (nT == 3 and reaction) else 0.0, diffusion_j=(0.0, 0.25, 0.1, 0.0)[:nT])
    k.update(over)
    r = dict(diffX=k["diffusion_x"], diffY=k["diffusion_y"], diffZ=k["diffusion_z"], dXY=k["diffusion_xy"], dYX=k["diffusion_yx"], dXZ=k["diffusion_xz"],
             dZX=k["diffusion_zx"], dYZ=k["diffusion_yz"], dZY=k["diffusion_zy"], beta=k["beta_interface"], crit=k["criteria_rho"],
             inlet_conc=k["inlet_concentration"], free_outlet=k["free_outlet"], dirichlet_inlet=k["dirichlet_inlet"], reaction_rate=k["reaction_rate"],
             diffJ=k["diffusion_j"])
    return k, r


def tracer_point_b(nT, **over):
    """tracer_case at a second point: criteria_rho, the nine entries of D per tracer, beta_interface, inlet_concentration, reaction_rate and
    diffusion_j all differ from tracer_case's values and from the defaults of configure_tracers (1/6, D_y = D_z = D_x, 0, 0.5) and of
    tests/tr3d_ref.py (beta = inlet = 1).  The diagonal of D stays within [0.05, 0.25] and the off-diagonals below 0.035, so that
    1/2 + 3 D is diagonally dominant (>= 0.68 against <= 0.21 per row)"""
    b = dict(diffusion_x=(0.09, 0.14, 0.22, 0.18)[:nT], diffusion_y=(0.17, 0.07, 0.11, 0.13)[:nT], diffusion_z=(0.13, 0.21, 0.06, 0.16)[:nT],
             diffusion_xy=-0.015, diffusion_yx=0.025, diffusion_xz=-0.024, diffusion_zx=0.012, diffusion_yz=0.035, diffusion_zy=-0.03,
             beta_interface=(0.7, 0.3, 0.9, 0.6)[:nT], criteria_rho=0.35, inlet_concentration=(0.6, 0.3, 0.15, 0.45)[:nT],
             reaction_rate=0.05 if nT == 3 else 0.0, diffusion_j=(0.15, 0.35, 0.2, 0.05)[:nT])
    b.update(over)
    return tracer_case(nT, **b)


def concentrations(dom, nT):
    nz, ny, nx = dom.shape
    zz, yy, xx = np.mgrid[0:nz, 0:ny, 0:nx]
    return np.array([(0.5 + 0.3 * np.sin(2 * np.pi * (xx + 2 * k) / nx) * np.cos(2 * np.pi * (yy + k) / ny) * np.cos(2 * np.pi * (zz + 3 * k) / nz)) * (dom == 1)
                     for k in range(nT)])


def obstacle_box():
    """a box with an obstacle with wetting walls and a slanted wall piece (the sample without symmetry of the flow's tests)"""
    from test_oracle_rk3d_csf import blob3
    return blob3()


def porous_box():
    from openlbmpm_amd.geometry import porous_spheres, initial_densities_rk3d
    dom = porous_spheres(32, 20, 36, porosity=0.7, rmin=3.0, rmax=6.0, seed=7, nbuf=5)
    dom[0] = dom[1]; dom[-1] = dom[-2]
    rR, rB = initial_densities_rk3d(dom, 12)
    return dom, rR, rB


def odd_nx_box():
    from test_oracle_rk3d_csf import blob3
    return blob3(nx=17, ny=10, nz=24)


def odd_box(nx, ny, nz):
    """the flow's odd sizes (tests/test_rk3d_csf_gpu.py::test_odd_sizes): one-cell-wide periodic directions, where every +-x or +-y source
    is the cell itself, and a ragged 70 x 3 x 9; one solid box each, both colours everywhere"""
    from test_rk3d_csf_gpu import ODD
    dom = np.ones((nz, ny, nx), dtype=np.uint8)
    dom[ODD[(nx, ny, nz)]] = 0
    zz = np.mgrid[0:nz, 0:ny, 0:nx][0]
    rR = np.where((dom == 1) & (zz < nz // 2), 1.0, 0.02 * (dom == 1)); rB = np.where((dom == 1) & (zz >= nz // 2), 1.0, 0.03 * (dom == 1))
    return dom, rR, rB


ODD_SIZES = {"5 x 1 x 16": (5, 1, 16), "1 x 6 x 12": (1, 6, 12), "70 x 3 x 9": (70, 3, 9)}
# The flow's wetting rule (updateColorGradientOnWettingNew: the oracle's step_a, csf3d_gradient) turns -G / |G| about the solid normal n_s by
# theta = acos(u . n_s) and divides by sin(theta).  Where the interface lies parallel to a wall u . n_s = 1 - O(eps), acos makes sqrt(eps) of
# it and the rule's tangential direction is rounding noise of size one: under the flat initial interface that is every cell on the two
# 40 x 1 faces of the 70 x 3 x 9 box.  There the ORACLE ALONE, started from densities that differ in the last bit, differs from itself by
# 8e-8 after 5 steps and 1e-3 after 200 (tracer, field-relative); no second implementation can follow it to 1e-10.  Without the rule: 7e-16
# after 200 steps.  The one-cell-wide lattices do not meet this (u . n_s = 1 exactly: the rule leaves G alone; 5e-16), nor do the other
# samples.  tests/test_tr3d_ref.py::test_the_cases_of_the_gpu_comparison_are_well_conditioned holds every lattice here to it.
LATTICE_FLOW = {"70 x 3 x 9": dict(wetting=0)}
LATTICES = {"obstacle": obstacle_box, "porous": porous_box, "odd nx": odd_nx_box}
LATTICES.update({k: (lambda v=v: odd_box(*v)) for k, v in ODD_SIZES.items()})
FLOWS = {
    "SRT": dict(relax="SRT"), "MRT": dict(relax="MRT"),
    "SRT tau type 1": dict(relax="SRT", tautype=1, tauB=0.65), "MRT tau type 1": dict(relax="MRT", tautype=1, tauB=0.7),
    "SRT pressure inlet": dict(relax="SRT", inlet="Dirichlet"), "MRT pressure inlet": dict(relax="MRT", inlet="Dirichlet"),
    # the convective outlet: planes 0 .. 2 take plane 3's streamed state, the collision writes rho_R and u for the tracers from that state,
    # and the tracers' free outlet copies plane 1 onto plane 0 (the masks of planes 0 .. 3 must coincide)
    "SRT convective outlet": dict(relax="SRT", outlet="Convective"), "MRT convective outlet": dict(relax="MRT", outlet="Convective"),
    "SRT convective outlet, pressure inlet": dict(relax="SRT", outlet="Convective", inlet="Dirichlet"),
    "MRT convective outlet, pressure inlet": dict(relax="MRT", outlet="Convective", inlet="Dirichlet"),
}
# the tracers' own open planes, one at a time
FLAGS = {"inlet alone": dict(dirichlet_inlet=True, free_outlet=False), "outlet alone": dict(dirichlet_inlet=False, free_outlet=True)}
POINT_B = "point B"          # in the place of the flags: tracer_point_b in the place of tracer_case
CASES = [("obstacle", f, n, None) for f in sorted(FLOWS) if "convective" not in f for n in (1, 3)]
CASES += [(l, f, n, None) for l in ("porous", "odd nx") for f in ("SRT", "MRT") for n in (1, 3)]
CASES += [("obstacle", f, n, None) for f in ("SRT", "MRT") for n in (2, 4)]
CASES += [("obstacle", f, n, None) for f in sorted(FLOWS) if "convective" in f for n in (1, 3)]
CASES += [("obstacle", f, 4, None) for f in ("SRT pressure inlet", "MRT pressure inlet")]
CASES += [("obstacle", f, 3, flags) for f in ("SRT", "MRT") for flags in sorted(FLAGS)]
CASES += [(l, "MRT", n, None) for l in ODD_SIZES for n in (1, 3)]
CASES += [("obstacle", f, 3, POINT_B) for f in ("SRT", "MRT")]
CASE_IDS = ["-".join([l, f, str(n)] + ([flags] if flags else [])) for l, f, n, flags in CASES]
STEPS = 200
# The steps compared, where they are not 1, 2 and STEPS.  From the sharp start the SRT flow on the obstacle box goes through a transient in
# which the reference, started from densities rippled in the last bit, differs from itself by up to 3e-11 (steps 2 .. 5, depending on the
# ripple; 3e-13 at step 10, 7e-14 with MRT).  The cases added at tracer point B are held to a tenth of TOL in that measure at every compared
# step (tests/test_tr3d_features_cpu.py), so the SRT one takes step 10 for step 2.
COMPARED = {("obstacle", "SRT", 3, POINT_B): (1, 10, STEPS)}


def compare_tracers(s, o, fl, nT, what):
    worst = 0.0
    for k in range(nT):
        c, g = s.get_concentration(k), s.get_tracer_pdf(k)
        assert np.all(c[~fl] == 0.0) and np.all(g[~fl] == 0.0)
        ec = rel_err(c[fl], o.C[k][fl])
        eg = rel_err(np.moveaxis(g, -1, 0)[:, fl], o.g[k][:, fl])
        print("%s: tracer %d concentration %.3e populations %.3e" % (what, k, ec, eg))
        assert ec < TOL and eg < TOL, (what, k, ec, eg)
        worst = max(worst, ec, eg)
    return worst


@pytest.mark.parametrize("lattice,flow,nT,flags", CASES, ids=CASE_IDS)
def test_against_the_restatement(lattice, flow, nT, flags):
    dom, rR, rB = LATTICES[lattice]()
    assert np.array_equal(dom[0], dom[1]) and np.array_equal(dom[-1], dom[-2])          # what lbmpm_rk3dcsf_create requires
    assert "convective" not in flow or all(np.array_equal(dom[0], dom[k]) for k in (1, 2, 3))
    par = dict(theta=50.0, tauB=0.8, velocityZR=0.0, velocityZB=-1.0e-2, sigma=0.05); par.update(FLOWS[flow]); par.update(LATTICE_FLOW.get(lattice, {}))
    kw, ref = tracer_point_b(nT) if flags == POINT_B else tracer_case(nT, **(FLAGS[flags] if flags else {}))
    c0 = concentrations(dom, nT)
    s = solver(dom, par)
    s.configure_tracers(**kw)
    s.set_macro(rR, rB)
    for k in range(nT):
        s.set_concentration(k, c0[k])
    o = Coupled3DRef(dom, rR, rB, c0, dict(par, crisp=CRISP), ref)
    fl = dom == 1
    phi0 = s.get("rec_phi")
    for n in COMPARED.get((lattice, flow, nT, flags), (1, 2, STEPS)):
        s.step(n - s.steps_done); o.run(n - o.steps)
        compare_tracers(s, o, fl, nT, "%s, %s, %d tracers%s, step %d" % (lattice, flow, nT, ", " + flags if flags else "", n))
    assert np.max(np.abs(s.get("rec_phi") - phi0)) > 0.5          # the interface has moved
    assert all(np.max(np.abs(o.C[k] - c0[k])) > 1e-2 for k in range(nT))
    s.close()


def _reductions():
    import test_tr3d_ref as R
    return dict(argvalues=R.REDUCTIONS, ids=R.REDUCTION_IDS)


@pytest.mark.parametrize("name,flow", **_reductions())
def test_reduces_to_the_2d_oracle_through_the_kernels(name, flow):
    """a lattice uniform in y against the 2-D composition rk_csf_step_a -> tr_substep -> rk_csf_step_b of tests/test_tr3d_ref.py, under the
    capture's flow (flow = None) and under the flow's convective outlet, its pressure inlet and both"""
    import test_tr3d_ref as R
    ny = 4
    dom2, o2, o3 = R.setup(name, ny=ny, flow=flow)
    assert flow is None or all(o3.flow.p[k] == v for k, v in R.OPEN_PLANES[flow].items())
    t = o3.tr.t
    nT = o3.tr.nT
    s = solver(R.extrude(dom2, ny), {k: v for k, v in o3.flow.p.items() if k != "crisp"})
    s.configure_tracers(num_tracers=nT, diffusion_x=t["diffX"], diffusion_y=t["diffY"], diffusion_z=t["diffZ"], diffusion_xz=t["dXZ"], diffusion_zx=t["dZX"],
                        beta_interface=t["beta"], criteria_rho=t["crit"], inlet_concentration=t["inlet_conc"], dirichlet_inlet=t["dirichlet_inlet"],
                        free_outlet=t["free_outlet"], reaction_rate=t["reaction_rate"], diffusion_j=t["diffJ"] or 0.0)
    f = o3.flow
    s.set_macro(f.field("rhoR"), f.field("rhoB"))
    for k in range(nT):
        s.set_concentration(k, o3.C[k])
    fl = dom2 == 1
    worst = 0.0
    for n in range(1, R.STEPS + 1):
        R.step2(o2)
        if n in (1, 2, 3, 10, 30, R.STEPS):
            s.step(n - s.steps_done)
            for k in range(nT):
                c, g = s.get_concentration(k), np.moveaxis(s.get_tracer_pdf(k), -1, 0)
                assert np.max(np.abs(c - c[:, :1, :])) <= 1e-12 * np.max(np.abs(c))
                worst = max(worst, rel_err(c[:, 0, :][fl], R.dense2(o2, o2.C[k])[fl]), rel_err(project_g(g)[fl], R.dense2(o2, o2.g[k])[fl]))
    print("%s, %s: worst field-relative difference from the 2-D oracle %.3e" % (name, flow or "the capture's flow", worst))
    assert worst < 1e-9, (name, flow, worst)
    s.close()


@pytest.mark.parametrize("relax", ["SRT", "MRT"])
def test_exchanging_x_and_y_exchanges_the_flow_and_the_tracers(relax):
    """What the reduction cannot see, through the kernels: the obstacle box with 3 tracers, the reaction and the full tensor against the
    run on the transposed problem (arrays transposed, D' = P D P^T).  The flow as in tests/test_oracle_rk3d_csf.py's exchange test, the
    concentrations, and the populations with +x <-> +y, -x <-> -y.  1e-8 as there: the flow's sums over 19 directions run in another
    order, and the tracers inherit that through u and G."""
    from test_tr3d_ref import exchange_field, exchange_populations
    x = lambda f: exchange_field(f, "x", "y")
    dom, rR, rB = obstacle_box()
    assert dom.shape[1] != dom.shape[2]          # (a sample that cannot be its own transpose)
    par = dict(relax=relax, theta=50.0, tauB=0.8, velocityZR=0.0, velocityZB=-1.0e-2, sigma=0.05)
    kw, _ = tracer_case(3)
    assert len({kw["diffusion_" + n] for n in ("xy", "yx", "xz", "zx", "yz", "zy")}) == 6 and kw["reaction_rate"] > 0
    kx = dict(kw, diffusion_x=kw["diffusion_y"], diffusion_y=kw["diffusion_x"], diffusion_xy=kw["diffusion_yx"], diffusion_yx=kw["diffusion_xy"],
              diffusion_xz=kw["diffusion_yz"], diffusion_yz=kw["diffusion_xz"], diffusion_zx=kw["diffusion_zy"], diffusion_zy=kw["diffusion_zx"])
    c0 = concentrations(dom, 3)
    a, b = solver(dom, par, diagnostics=True), solver(x(dom), par, diagnostics=True)
    a.configure_tracers(**kw); b.configure_tracers(**kx)
    a.set_macro(rR, rB); b.set_macro(x(rR), x(rB))
    for k in range(3):
        a.set_concentration(k, c0[k]); b.set_concentration(k, x(c0[k]))
    a.step(40); b.step(40)
    worst = 0.0
    for fa, fb in (("rhoR", "rhoR"), ("rhoB", "rhoB"), ("phi", "phi"), ("vx", "vy"), ("vy", "vx"), ("vz", "vz"), ("Gx", "Gy"), ("Gy", "Gx"),
                   ("Gz", "Gz"), ("Fx", "Fy"), ("Fy", "Fx"), ("Fz", "Fz"), ("K", "K")):
        scale = max(np.max(np.abs(a.get(fa[0] + c))) for c in "xyz") if fa[0] in "vGF" and len(fa) == 2 else None
        e = rel_err(x(b.get(fb)), a.get(fa), scale=scale)
        assert e < 1e-8, (fa, fb, e)
        worst = max(worst, e)
    ca = np.array([a.get_concentration(k) for k in range(3)]); cb = np.array([b.get_concentration(k) for k in range(3)])
    ga = np.array([np.moveaxis(a.get_tracer_pdf(k), -1, 0) for k in range(3)]); gb = np.array([np.moveaxis(b.get_tracer_pdf(k), -1, 0) for k in range(3)])
    ec, eg = rel_err(x(cb), ca), rel_err(gb, exchange_populations(ga, "x", "y"))
    print("x <-> y, %s: flow %.3e concentrations %.3e populations %.3e" % (relax, worst, ec, eg))
    assert ec < 1e-8 and eg < 1e-8, (ec, eg)
    assert np.max(np.abs(a.get("K"))) > 1e-3 and np.max(np.abs(a.get("Fy"))) > 1e-7          # the test sees an interface
    assert all(np.max(np.abs(ca[k] - c0[k])) > 1e-2 for k in range(3))                      # and the tracers have moved
    a.close(); b.close()


def front_in_a_duct():
    from openlbmpm_amd.RKColorGradientD3Q19 import duct
    dom = duct(34, 30, 120)
    dom[40:60, 8:20, 10:24] = 0                       # an obstacle with wetting walls inside the red bulk
    zz = np.mgrid[0:120, 0:30, 0:34][0]
    fl = dom == 1
    return dom, np.where(fl & (zz < 84), 1.0, 0.0), np.where(fl & (zz >= 84), 1.0, 0.0)


FLOW_FIELDS = ("fR", "fB", "rhoR", "rhoB", "phi", "Gx", "Gy", "Gz", "Fx", "Fy", "Fz", "rec_vz", "rec_phi")


@pytest.mark.parametrize("relax", ["MRT", "SRT"])
def test_the_bulk_skip_stays_exact_with_tracers(relax):
    """the deep blocks' collision hands rho_R and u to the tracers like the full path's, and G is an exact zero there: variant 0 against the
    run that sends every cell through the full path (variant 1), bit for bit, flow and concentrations, while a front moves"""
    dom, rR, rB = front_in_a_duct()
    par = dict(relax=relax, theta=60.0, tauB=0.8, velocityZR=0.0, velocityZB=-4.0e-3, sigma=0.05)
    kw, _ = tracer_case(3)
    c0 = concentrations(dom, 3)
    a = solver(dom, par); b = solver(dom, dict(par, variant=1))
    for s in (a, b):
        s.configure_tracers(**kw); s.set_macro(rR, rB)
        for k in range(3):
            s.set_concentration(k, c0[k])
    seen = []
    for n in (1, 2, 3, 40, 41, 120):
        a.step(n - a.steps_done); b.step(n - b.steps_done)
        seen.append(a.bulk_cells)
        assert b.bulk_cells == 0
        for f in FLOW_FIELDS:
            assert np.array_equal(a.get(f), b.get(f)), (n, f)
        for k in range(3):
            assert np.array_equal(a.get_concentration(k), b.get_concentration(k)), (n, k)
            assert np.array_equal(a.get_tracer_pdf(k), b.get_tracer_pdf(k)), (n, k)
    assert seen[1] > 0.3 * a.num_fluid_nodes and len(set(seen[1:])) > 1, seen
    a.close(); b.close()


@pytest.mark.parametrize("relax,variant", [("MRT", 0), ("SRT", 0), ("MRT", 1)])
def test_the_flow_is_untouched(relax, variant):
    dom, rR, rB = front_in_a_duct()
    par = dict(relax=relax, theta=60.0, tauB=0.8, velocityZR=0.0, velocityZB=-4.0e-3, sigma=0.05, variant=variant)
    kw, _ = tracer_case(2)
    a = solver(dom, par); b = solver(dom, par)
    a.configure_tracers(**kw)
    c0 = concentrations(dom, 2)
    for s in (a, b):
        s.set_macro(rR, rB)
    for k in range(2):
        a.set_concentration(k, c0[k])
    assert a.device_bytes > b.device_bytes + 2 * 2 * 7 * 8 * a.num_fluid_nodes       # lbmpm_rk3dcsf_device_bytes counts the tracers' buffers
    for n in (1, 2, 50):
        a.step(n - a.steps_done); b.step(n - b.steps_done)
        for f in FLOW_FIELDS:
            assert np.array_equal(a.get(f), b.get(f)), (n, f)
    assert a.bulk_cells == b.bulk_cells
    a.close(); b.close()


def test_restart_bit_for_bit():
    dom, rR, rB = front_in_a_duct()
    par = dict(relax="MRT", theta=60.0, tauB=0.8, velocityZR=0.0, velocityZB=-4.0e-3, sigma=0.05)
    kw, _ = tracer_case(3)
    c0 = concentrations(dom, 3)
    a = solver(dom, par)
    a.configure_tracers(**kw); a.set_macro(rR, rB)
    for k in range(3):
        a.set_concentration(k, c0[k])
    a.step(45)
    c = solver(dom, par)
    c.configure_tracers(**kw)
    c.set_pdf(a.get("fR"), a.get("fB"), force=(a.get("Fx"), a.get("Fy"), a.get("Fz")))
    for k in range(3):
        c.set_tracer_pdf(k, a.get_tracer_pdf(k))
    for k in range(3):
        assert np.array_equal(a.get_concentration(k), c.get_concentration(k))
    a.step(30); c.step(30)
    for f in ("fR", "fB", "phi", "Fz"):
        assert np.array_equal(a.get(f), c.get(f)), f
    for k in range(3):
        assert np.array_equal(a.get_tracer_pdf(k), c.get_tracer_pdf(k)), k
        assert np.array_equal(a.get_concentration(k), c.get_concentration(k)), k
    a.close(); c.close()


@pytest.mark.parametrize("reaction", [False, True])
def test_conservation(reaction):
    """no open plane for the tracers (the lattice wraps z as it wraps x and y; walls bounce back): the collision keeps sum_i g_i, the
    interface term adds cos(e_i, n) over opposite pairs, the streaming moves populations -- sum C over the fluid cells is constant to
    rounding.  The reaction takes k C_0 C_1 from tracers 0 and 1 and gives it to tracer 2: sum (C_0 - C_1) and sum (C_0 + C_2) stay."""
    dom, rR, rB = porous_box()
    par = dict(relax="MRT", theta=50.0, tauB=0.8, velocityZR=0.0, velocityZB=-3.0e-3, sigma=0.05)
    kw, _ = tracer_case(3, reaction=reaction, dirichlet_inlet=False, free_outlet=False)
    c0 = concentrations(dom, 3)
    s = solver(dom, par)
    s.configure_tracers(**kw); s.set_macro(rR, rB)
    for k in range(3):
        s.set_concentration(k, c0[k])
    total = lambda: np.array([float(np.sum(s.get_concentration(k))) for k in range(3)])
    t0 = total()
    s.step(300)
    t1 = total()
    print("conservation (reaction %s): totals %s -> %s" % (reaction, t0, t1))
    # 300 steps of ~ 1e4 cells in double precision: sums of O(1e4) terms each carrying 1e-16 per step
    if not reaction:
        assert np.all(np.abs(t1 - t0) < 1e-11 * np.abs(t0)), (t0, t1)
    else:
        assert abs((t1[0] - t1[1]) - (t0[0] - t0[1])) < 1e-11 * abs(t0[0]) and abs((t1[0] + t1[2]) - (t0[0] + t0[2])) < 1e-11 * abs(t0[0] + t0[2]), (t0, t1)
        assert t0[0] - t1[0] > 1e-3 * t0[0]          # the reaction did consume A
    s.close()


def test_a_gaussian_blob_spreads_as_2_d_t():
    """A Gaussian blob in a uniform single-phase flow along z (all fluid, red alone, plug flow set from the start): its variance grows as
    2 D t per axis with an anisotropic D, its centre moves with the flow.  Slopes between steps 100 and 300.  Measured on the MI355X:
    d var / dt off 2 D by 3e-6 (x), 4.5e-4 (y), 3.0e-4 (z), the drift equal to the flow to six digits; the bound is the 2-D test's 0.3 %."""
    nx, ny, nz = 64, 64, 160
    dom = np.ones((nz, ny, nx), dtype=np.uint8)
    U = -0.01
    D = (0.04, 0.08, 0.12)
    par = dict(relax="MRT", velocityZR=U, velocityZB=0.0, densityRL=1.0, densityBL=0.0, sigma=0.0)
    s = solver(dom, par)
    s.configure_tracers(num_tracers=1, diffusion_x=D[0], diffusion_y=D[1], diffusion_z=D[2], beta_interface=0.0)
    one = np.ones(dom.shape)
    s.set_macro(one, 0.0 * one, vz=U * one)
    zz, yy, xx = np.mgrid[0:nz, 0:ny, 0:nx].astype(np.float64)
    c0 = (31.5, 31.5, 90.0)
    s.set_concentration(0, np.exp(-((xx - c0[0]) ** 2 + (yy - c0[1]) ** 2 + (zz - c0[2]) ** 2) / (2. * 16.)))

    def moments():
        c = s.get_concentration(0)
        m = c.sum()
        out = []
        for a in (xx, yy, zz):
            mu = (c * a).sum() / m
            out.append((mu, (c * (a - mu) ** 2).sum() / m))
        return m, out
    s.step(100); m1, a1 = moments()
    s.step(200); m2, a2 = moments()
    assert abs(m2 - m1) < 1e-10 * m1
    for ax in range(3):
        slope = (a2[ax][1] - a1[ax][1]) / 200.
        err = abs(slope - 2. * D[ax]) / (2. * D[ax])
        print("axis %d: d var / dt = %.6f, 2 D = %.6f, relative error %.3e" % (ax, slope, 2. * D[ax], err))
        assert err < 3e-3, (ax, slope)
    drift = (a2[2][0] - a1[2][0]) / 200.
    print("drift along z %.6f, flow %.6f" % (drift, U))
    assert abs(drift - U) < 3e-3 * abs(U)
    s.close()


def test_a_gaussian_blob_spreads_as_d_plus_d_transposed():
    """The sibling with a full, nonsymmetric tensor: the blob, the tensor, the periodic 48 x 48 cross-section and the window (sub-steps 40 to
    100) of tests/test_tr3d_ref.py::test_a_gaussian_blob_spreads_as_d_plus_d_transposed, in plug flow along z (96 planes: the blob stays
    eight standard deviations from the open planes).  All six d cov_ij / dt against D_ij + D_ji: the analytic law is the reference.  The
    bounds are that test's -- three times what the restatement misses the law by, entry by entry; this flow (0, 0, -0.01) lies between its
    two runs (at rest, and (0.01, -0.02, 0.015)), so each entry takes the larger of the two.
    The same case through the restatement and the flow oracle on the CPU, relative to 0.24: 7.2e-7 (xx), 2.3e-5 (xy), 2.5e-5 (xz), 2.7e-5 (yy),
    2.6e-5 (yz), 3.0e-4 (zz); the centre's velocity within 1.6e-8 of u; the mass to 3e-15."""
    from test_tr3d_ref import BLOB_D, BLOB_MEASURED, BLOB_DRIFT_MEASURED, blob_moments, blob_tracer
    nx, ny, nz = 48, 48, 96
    dom = np.ones((nz, ny, nx), dtype=np.uint8)
    U = -0.01
    t = blob_tracer()
    par = dict(relax="MRT", velocityZR=U, velocityZB=0.0, densityRL=1.0, densityBL=0.0, sigma=0.0)
    s = solver(dom, par)
    s.configure_tracers(num_tracers=1, diffusion_x=t["diffX"], diffusion_y=t["diffY"], diffusion_z=t["diffZ"], diffusion_xy=t["dXY"], diffusion_yx=t["dYX"],
                        diffusion_xz=t["dXZ"], diffusion_zx=t["dZX"], diffusion_yz=t["dYZ"], diffusion_zy=t["dZY"], beta_interface=0.0)
    one = np.ones(dom.shape)
    s.set_macro(one, 0.0 * one, vz=U * one)
    zz, yy, xx = np.mgrid[0:nz, 0:ny, 0:nx].astype(np.float64)
    s.set_concentration(0, np.exp(-((xx - 23.5) ** 2 + (yy - 23.5) ** 2 + (zz - 48.0) ** 2) / (2. * 9.)))
    s.step(40); m1, mu1, cov1 = blob_moments(s.get_concentration(0))
    s.step(60); m2, mu2, cov2 = blob_moments(s.get_concentration(0))
    want = BLOB_D + BLOB_D.T
    err = np.abs((cov2 - cov1) / 60. - want) / np.max(want)
    drift = np.max(np.abs((mu2 - mu1) / 60. - np.array([0., 0., U])))
    print("|d cov / dt - (D + D^T)| / %.2f =\n%s\ndrift off u by %.3e, mass off by %.3e" % (np.max(want), np.array2string(err, precision=3), drift, abs(m2 - m1) / m1))
    assert abs(m2 - m1) < 1e-10 * m1
    assert np.all(err <= 3. * np.maximum(BLOB_MEASURED["at rest"], BLOB_MEASURED["drifting"])), err
    assert drift <= 3. * BLOB_DRIFT_MEASURED, drift
    s.close()


def test_refusals():
    from openlbmpm_amd._lib import LbmpmError, ERR_UNSUPPORTED, ERR_INVALID, ERR_STATE
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster
    dom, rR, rB = obstacle_box()
    s = solver(dom, None)
    with pytest.raises(LbmpmError) as e:
        s.get_concentration(0)
    assert e.value.status == ERR_STATE and "tracer_configure" in str(e.value)
    with pytest.raises(LbmpmError) as e:
        s.configure_tracers(num_tracers=5)
    assert e.value.status == ERR_INVALID and "1 .. 4" in str(e.value)
    with pytest.raises(LbmpmError) as e:
        s.configure_tracers(num_tracers=2, reaction_rate=0.1)
    assert e.value.status == ERR_INVALID and "three tracers" in str(e.value)
    s.set_macro(rR, rB)
    s.step(1)
    with pytest.raises(LbmpmError) as e:
        s.configure_tracers(num_tracers=1)
    assert e.value.status == ERR_STATE and "before the first step" in str(e.value)
    s.close()
    s = solver(dom, None)
    s.configure_tracers(num_tracers=1)
    with pytest.raises(LbmpmError) as e:
        s.set_concentration(1, rR)
    assert e.value.status == ERR_INVALID
    s.close()
    big = np.concatenate([dom, dom[::-1]], axis=0)
    cl = RK3DCSFCluster(big, None, nslabs=2)
    with pytest.raises(LbmpmError) as e:
        cl.slabs[0].configure_tracers(num_tracers=1)       # a context with ghost planes
    assert e.value.status == ERR_UNSUPPORTED and "slabs" in str(e.value)
    with pytest.raises(LbmpmError) as e:
        cl.configure_tracers(num_tracers=1)
    assert e.value.status == ERR_UNSUPPORTED and "slabs" in str(e.value)
    cl.close()
