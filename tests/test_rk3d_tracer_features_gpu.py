"""The D3Q7 tracers of the 3-D CSF solver under what was added to the flow after them: the body force (TR && BF instances of csf3d_collide and
csf3d_collide_deep), periodic z (tr3d_step without a plane rule) and per-cell contact angles (tr3d_step reads G of csf3d_gradient<true>).

The reference is tests/tr3d_ref.Coupled3DRef around tests/body_force_ref.BodyForceRef or tests/periodic_ref.PeriodicRef: the restated tracer
sub-step spliced between the halves of the flow recipe's step, where u carries half the CSF force and half the body force.
tests/test_tr3d_features_cpu.py holds that composition (it is today's with g = 0, the splice sits where step_a() leaves u, the periodic one is
the open-plane one transposed), shows that every case below is well conditioned and that the mistakes a kernel could make here -- u without
F_b / 2, the colours' accelerations exchanged, no wrap of z, a parameter at its default, the other channel's angle -- move a compared field
by >= 1000 TOL.  Comparisons with a reference are at TOL = 1e-10 (compare_tracers of tests/test_rk3d_tracer_gpu.py); identities are
array_equal.
1. body force, parity;  2. body force, bulk path;  3. body force, cuts and restart;  4. periodic z, parity;  5. contact-angle map;
6. everything on.  (Tracer point B between open planes: tests/test_rk3d_tracer_gpu.py::test_against_the_restatement.)
Measured on the MI355X, worst over the compared steps: 2.3e-14 (body force), 7.8e-16 (periodic z), 7.2e-16 (two channels);
docs/EXPERIMENTS_r7.md, section T."""
import numpy as np
import pytest

import body_force_ref as R
import param_points as P
import periodic_ref as PR
from helpers import rel_err
from tr3d_ref import Coupled3DRef
from test_rk3d_tracer_gpu import CRISP, TOL, compare_tracers, concentrations, tracer_case, tracer_point_b

pytestmark = pytest.mark.gpu

FLOW_STATE = ("fR", "fB", "rhoR", "rhoB", "phi", "Gx", "Gy", "Gz", "Fx", "Fy", "Fz", "K", "vx", "vy", "vz", "rec_vx", "rec_vy", "rec_vz", "rec_phi")


def solver(dom, par, **kw):
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    return RK3DCSFSolver(dom, par, **dict(dict(diagnostics=True), **kw))


class Snap:
    """the tracers of a reference at one moment, as compare_tracers reads them"""

    def __init__(self, o):
        self.C, self.g = np.array(o.C), np.array(o.g)


def snapshots(o, steps):
    out = {}
    for n in steps:
        o.run(n - o.steps)
        out[n] = Snap(o)
    return out


def populations(s, nT):
    return [s.get_tracer_pdf(k) for k in range(nT)]


def same_tracers(a, b, nT, what):
    for k in range(nT):
        x, y = a.get_tracer_pdf(k) if hasattr(a, "get_tracer_pdf") else a[k], b.get_tracer_pdf(k) if hasattr(b, "get_tracer_pdf") else b[k]
        assert np.array_equal(x, y), (what, k, float(np.max(np.abs(x - y))))


def start(s, rR, rB, c0, force=None, theta_map=None):
    if force is not None:
        s.set_body_force(red=force[0], blue=force[1])
    if theta_map is not None:
        s.set_contact_angles(theta_map)
    s.set_macro(rR, rB)
    for k in range(len(c0)):
        s.set_concentration(k, c0[k])
    return s


_REFS = {}


def cached(key, make):
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


# ------------------------------------------------------------------------------------------------ 1. body force, parity
# the four blob3 instances of the body-force parity test at the flow's points A (G1) and B (G2), each with three tracers and the
# reaction at tracer point B and with two tracers at tracer_case; one SRT and one MRT case go on to step 40
BF_TRACERS = {"3 at B": lambda: tracer_point_b(3), "2 at tracer_case": lambda: tracer_case(2)}
BF_CASES = [(i, t) for i in range(4) for t in sorted(BF_TRACERS)]
BF_LONG = ((0, "3 at B"), (2, "3 at B"))
BF_LONG_STEPS = 40


def ramp_start(dom):
    """blob3's mask with a start of its own: a slanted interface four cells thick, rho_R falling linearly from 1 to 0 across it and
    rho_B = 1 - rho_R.  From blob3's own sharp, flat start rho_R is 0 or 1 in step 1 and stays off (0.35, 0.5] for ten steps and more: no
    compared step would see criteria_rho, or a sub-step that reads the densities the second half leaves.  Here cells of every rho_R lie
    on either side of both criteria from the first step on (tests/test_tr3d_features_cpu.py measures it).  The slopes are such that
    no cell starts within 1e-4 of a criterion: a cell that sits ON one is switched by the last bit, and no reference can be followed there"""
    nz, ny, nx = dom.shape
    z, y, x = np.mgrid[0:nz, 0:ny, 0:nx]
    red = np.clip(0.5 - (z + 0.3137 * x - 0.2071 * y - (nz - 7.2863)) / 4., 0., 1.)
    fl = dom == 1
    assert all(np.min(np.abs(red[fl] - crit)) > 1e-4 for crit in (0.35, 0.5))
    return np.where(fl, red, 0.0), np.where(fl, 1. - red, 0.0)


def bf_instance(i):
    from test_rk3d_csf_body_force_gpu import PARITY
    lattice, point, gset, inst = PARITY[i]
    assert lattice == "blob3"
    return point, gset, inst


def bf_case(i, tracers):
    point, gset, inst = bf_instance(i)
    dom = P.lattice_csf()[0]
    rR, rB = ramp_start(dom)
    par = P.params(P.TABLES["rk3dcsf"], point, **inst)
    kw, ref = BF_TRACERS[tracers]()
    nT = kw["num_tracers"]
    steps = (1, 2, P.STEPS) + ((BF_LONG_STEPS,) if (i, tracers) in BF_LONG else ())
    return dict(dom=dom, rR=rR, rB=rB, par=par, opar={k: v for k, v in par.items() if k != "variant"}, g=R.G_SETS[gset], kw=kw, ref=ref, nT=nT,
                c0=concentrations(dom, nT), steps=steps, what="blob3 %s %s %s, %s" % (point, gset, ",".join(str(v) for v in inst.values()), tracers))


def bf_reference(c, rR=None, rB=None, g=None, **kw):
    """Coupled3DRef around the body-force recipe for the case c (start and accelerations replaceable; kw: Coupled3DRef's negative controls)"""
    g = c["g"] if g is None else g
    flow = R.BodyForceRef(c["dom"], c["rR"] if rR is None else rR, c["rB"] if rB is None else rB, c["opar"], g[0], g[1])
    return Coupled3DRef(c["dom"], conc0=c["c0"], tracer=c["ref"], flow=flow, **kw)


@pytest.mark.parametrize("i,tracers", BF_CASES, ids=["%d-%s" % c for c in BF_CASES])
def test_body_force_against_the_recipe(i, tracers):
    """concentrations and populations of every tracer after steps 1, 2 and 10 (40); the run without diagnostics leaves the same bits; the
    reference's concentration moved; without the force the tracers end up elsewhere"""
    c = bf_case(i, tracers)
    dom, nT, fl = c["dom"], c["nT"], c["dom"] == 1
    ref = cached(("bf", i, tracers), lambda: snapshots(bf_reference(c), c["steps"]))
    s = start(solver(dom, c["par"], tracers=c["kw"]), c["rR"], c["rB"], c["c0"], c["g"])
    lean = start(solver(dom, c["par"], tracers=c["kw"], diagnostics=False), c["rR"], c["rB"], c["c0"], c["g"])
    plain = start(solver(dom, c["par"], tracers=c["kw"]), c["rR"], c["rB"], c["c0"])
    worst = 0.0
    for n in c["steps"]:
        for x in (s, lean, plain):
            x.step(n - x.steps_done)
        worst = max(worst, compare_tracers(s, ref[n], fl, nT, "%s, step %d" % (c["what"], n)))
        same_tracers(s, lean, nT, "diagnostics off, step %d" % n)
        felt = max(rel_err(plain.get_tracer_pdf(k)[fl], s.get_tracer_pdf(k)[fl]) for k in range(nT))
        assert felt > 1000 * TOL, (n, felt)
    moved = min(float(np.max(np.abs(ref[P.STEPS].C[k] - c["c0"][k]))) for k in range(nT))
    print("%s: worst field-relative difference %.3e; the force moved the tracers by %.3e; the concentrations moved by %.3e" % (c["what"], worst, felt, moved))
    assert moved > 1e-3, moved
    for x in (s, lean, plain):
        x.close()


# ------------------------------------------------------------------------------------------------ 2. body force, bulk path
@pytest.mark.parametrize("relax", ["MRT", "SRT"])
def test_body_force_bulk_path_equals_the_full_path(relax):
    """variant 0 (deep blocks through csf3d_collide_deep<.., TR, BF>) against variant 1 (every cell through csf3d_collide<.., TR, BF>) with
    two tracers and the colours accelerated differently: the tracers' populations bit for bit while a front moves"""
    from test_rk3d_csf_body_force_gpu import bulk_duct
    dom, rR, rB = bulk_duct()
    gr, gb = R.G_SETS["G1"]
    assert gr != gb
    par = dict(relax=relax, theta=55.0, tauB=0.8, velocityZR=0.0, velocityZB=-4.0e-3, sigma=0.05)
    kw, _ = tracer_case(2)
    c0 = concentrations(dom, 2)
    a = start(solver(dom, par, tracers=kw), rR, rB, c0, (gr, gb))
    b = start(solver(dom, dict(par, variant=1), tracers=kw), rR, rB, c0, (gr, gb))
    off = start(solver(dom, par, tracers=kw), rR, rB, c0)
    for n in (1, 2, 3, 40, 41, 42):
        a.step(n - a.steps_done); b.step(n - b.steps_done)
        assert b.bulk_cells == 0
        assert n < 3 or a.bulk_cells > 0, (n, a.bulk_cells)
        same_tracers(a, b, 2, "%s, step %d" % (relax, n))
        for f in FLOW_STATE:
            assert np.array_equal(a.get(f), b.get(f)), (n, f)
    assert a.bulk_cells > 0 and b.bulk_cells == 0
    off.step(42)
    fl = dom == 1
    assert max(rel_err(off.get_tracer_pdf(k)[fl], a.get_tracer_pdf(k)[fl]) for k in range(2)) > 1000 * TOL       # the force is on in these runs
    for x in (a, b, off):
        x.close()


# ------------------------------------------------------------------------------------------------ 3. body force, cuts and restart
SLAB_PARAMS = dict(relax="MRT", theta=55.0, tauB=0.8, velocityZR=0.0, velocityZB=-3.0e-3, sigma=0.06)
SLAB_STEPS, SLAB_AT = 30, 10
SLAB_G = R.G_SETS["G1"]


def slab_tracers():
    return tracer_case(2)[0]


@pytest.fixture(scope="module")
def undivided():
    """_slab_case (22 x 18 x 44) under the force with two tracers: the state after 10 steps, the tracers after 30"""
    from test_rk3d_csf_gpu import _slab_case
    dom, rR, rB = _slab_case()
    c0 = concentrations(dom, 2)
    s = start(solver(dom, SLAB_PARAMS, tracers=slab_tracers()), rR, rB, c0, SLAB_G)
    s.step(SLAB_AT)
    at10 = {f: s.get(f) for f in ("fR", "fB", "Fx", "Fy", "Fz")}
    at10["g"] = populations(s, 2)
    s.step(SLAB_STEPS - SLAB_AT)
    out = dict(dom=dom, rR=rR, rB=rB, c0=c0, at10=at10, g=populations(s, 2), fR=s.get("fR"))
    s.close()
    return out


@pytest.mark.parametrize("cuts", [2, 3, "thinnest"])
def test_body_force_slabs_equal_the_undivided_lattice(undivided, cuts):
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster
    u = undivided
    nz = u["dom"].shape[0]
    kw = dict(cuts=[0, 4, 8, 12, nz - 4, nz]) if cuts == "thinnest" else dict(nslabs=cuts)
    c = RK3DCSFCluster(u["dom"], SLAB_PARAMS, diagnostics=True, tracers=slab_tracers(), **kw)
    start(c, u["rR"], u["rB"], u["c0"], SLAB_G)
    c.step(SLAB_AT)
    same_tracers(c, u["at10"]["g"], 2, "slabs %s, step %d" % (cuts, SLAB_AT))
    c.step(SLAB_STEPS - SLAB_AT)
    same_tracers(c, u["g"], 2, "slabs %s, step %d" % (cuts, SLAB_STEPS))
    assert np.array_equal(c.get("fR"), u["fR"])
    c.close()


def restarted(u, force):
    s = solver(u["dom"], SLAB_PARAMS, tracers=slab_tracers())
    s.set_pdf(u["at10"]["fR"], u["at10"]["fB"], force=(u["at10"]["Fx"], u["at10"]["Fy"], u["at10"]["Fz"]))
    for k in range(2):
        s.set_tracer_pdf(k, u["at10"]["g"][k])
    s.set_body_force(red=force[0], blue=force[1])
    return s


def test_body_force_restart_continues_bit_for_bit(undivided):
    """a new context at step 10: set_pdf, set_tracer_pdf, the force given again"""
    u = undivided
    s = restarted(u, SLAB_G)
    s.step(SLAB_STEPS - SLAB_AT)
    same_tracers(s, u["g"], 2, "restart")
    assert np.array_equal(s.get("fR"), u["fR"])
    s.close()


def test_body_force_changed_mid_run_equals_a_restart_with_the_new_force(undivided):
    u = undivided
    g2 = R.G_SETS["G2"]
    a = start(solver(u["dom"], SLAB_PARAMS, tracers=slab_tracers()), u["rR"], u["rB"], u["c0"], SLAB_G)
    a.step(SLAB_AT)
    same_tracers(a, u["at10"]["g"], 2, "before the change")
    a.set_body_force(red=g2[0], blue=g2[1])
    a.step(SLAB_STEPS - SLAB_AT)
    b = restarted(u, g2)
    b.step(SLAB_STEPS - SLAB_AT)
    same_tracers(a, b, 2, "changed at step %d" % SLAB_AT)
    fl = u["dom"] == 1
    assert max(rel_err(a.get_tracer_pdf(k)[fl], u["g"][k][fl]) for k in range(2)) > 1000 * TOL          # the new force is the one applied
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 4. periodic z, parity
PERIODIC_STEPS = (1, 2, 10)
PERIODIC_FLOWS = [("SRT", 1), ("SRT", 2), ("MRT", 1), ("MRT", 2)]
NO_FORCE = ((0., 0., 0.), (0., 0., 0.))


def periodic_tracers():
    """three tracers with the reaction at tracer point B (a full tensor with six distinct off-diagonals, distinct betas); periodic z takes
    neither of the tracers' open planes"""
    kw, ref = tracer_point_b(3, dirichlet_inlet=False, free_outlet=False)
    assert len({kw["diffusion_" + n] for n in ("xy", "yx", "xz", "zx", "yz", "zy")}) == 6 and len(set(kw["beta_interface"])) == 3 and kw["reaction_rate"] > 0
    return kw, ref


def periodic_concentrations(dom):
    """tracer 0 in the planes nz-2 and nz-1 alone; tracers 1 and 2 vary along z without a symmetry about the seam"""
    nz, ny, nx = dom.shape
    z, y, x = np.mgrid[0:nz, 0:ny, 0:nx]
    c = [np.where(z >= nz - 2, 0.8 + 0.1 * np.cos(2. * np.pi * y / ny), 0.0),
         0.5 + 0.3 * np.sin(2. * np.pi * z / nz + 0.7) + 0.1 * np.cos(4. * np.pi * z / nz + 0.2),
         0.25 + 0.15 * np.cos(2. * np.pi * (2. * z / nz + x / nx) + 1.1)]
    return np.array([np.where(dom == 1, a, 0.0) for a in c])


def periodic_case(relax, tautype, gset):
    dom, rR, rB = PR.parity_lattice()
    kw, ref = periodic_tracers()
    return dict(dom=dom, rR=rR, rB=rB, par=PR.parity_params(relax, tautype), g=R.G_SETS[gset] if gset else NO_FORCE, kw=kw, ref=ref, nT=3,
                c0=periodic_concentrations(dom), steps=PERIODIC_STEPS, what="periodic %s tautype %d %s" % (relax, tautype, gset))


def periodic_reference(c, rR=None, rB=None, **kw):
    flow = PR.PeriodicRef(c["dom"], c["rR"] if rR is None else rR, c["rB"] if rB is None else rB, c["par"], *c["g"])
    return Coupled3DRef(c["dom"], conc0=c["c0"], tracer=c["ref"], flow=flow, **kw)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("gset", ["G1", None])
@pytest.mark.parametrize("relax,tautype", PERIODIC_FLOWS)
def test_periodic_z_against_the_transposed_recipe(relax, tautype, gset, variant):
    c = periodic_case(relax, tautype, gset)
    dom, fl = c["dom"], c["dom"] == 1
    ref = cached(("periodic", relax, tautype, gset), lambda: snapshots(periodic_reference(c), c["steps"]))
    s = solver(dom, dict(c["par"], variant=variant), tracers=c["kw"])
    assert s.periodic_z
    start(s, c["rR"], c["rB"], c["c0"], c["g"] if gset else None)
    worst = 0.0
    for n in c["steps"]:
        s.step(n - s.steps_done)
        worst = max(worst, compare_tracers(s, ref[n], fl, 3, "%s variant %d, step %d" % (c["what"], variant, n)))
    print("%s variant %d: worst field-relative difference %.3e" % (c["what"], variant, worst))
    # the seam carried tracer 0: after two steps it is in the planes 0 and 1, which nothing reaches from plane nz-2 the other way round
    assert np.all(c["c0"][0][:2] == 0.0) and all(float(np.max(ref[2].C[0][z])) > 1e-6 for z in (0, 1))
    assert all(float(np.max(ref[10].C[0][z])) > 1e-6 for z in (0, 1))
    s.close()


# ------------------------------------------------------------------------------------------------ 5. contact-angle map
ANGLES = {"A": 50.0, "B": 130.0}
CHANNEL_STEPS = (1, 30)


def channel_case():
    from test_wettability_cpu import TWO_CHANNEL_PARAMS, two_channels
    dom, rR, rB, A, B = two_channels()
    kw, ref = tracer_case(2)
    assert all(b != 0.0 for b in kw["beta_interface"]) and len(set(kw["beta_interface"])) == 2
    return dict(dom=dom, rR=rR, rB=rB, cells={"A": A, "B": B}, par=dict(TWO_CHANNEL_PARAMS, theta=97.0), kw=kw, ref=ref, nT=2, c0=concentrations(dom, 2),
                steps=CHANNEL_STEPS)


def channel_reference(c, theta, rR=None, rB=None):
    return Coupled3DRef(c["dom"], c["rR"] if rR is None else rR, c["rB"] if rB is None else rB, c["c0"], dict(c["par"], theta=theta, crisp=CRISP), c["ref"])


class TracerChannel:
    """a solver's or a reference's tracers seen through one channel: zero outside it"""

    def __init__(self, inner, cells):
        self.inner, self.cells = inner, cells

    def get_concentration(self, k):
        return np.where(self.cells, self.inner.get_concentration(k), 0.0)

    def get_tracer_pdf(self, k):
        return np.where(self.cells[..., None], self.inner.get_tracer_pdf(k), 0.0)

    C = property(lambda self: np.where(self.cells, self.inner.C, 0.0))
    g = property(lambda self: np.where(self.cells, self.inner.g, 0.0))


def wall_map(dom, par, values):
    """values at the fluid cells next to solid (the solver's kind 3), NaN elsewhere"""
    s = solver(dom, par)
    kind = s.get("kind")
    s.close()
    return np.where(kind == 3, values, np.nan)


@pytest.mark.parametrize("variant", [0, 1])
def test_each_channels_tracers_run_with_its_own_angle(variant):
    """two channels that cannot see each other (tests/test_wettability_cpu.py) under the 50 / 130 map: channel A's tracers are the scalar-50
    run's and channel B's the scalar-130 run's, bit for bit, neither is the other angle's, and each agrees with Coupled3DRef at its angle"""
    c = channel_case()
    dom, fl, nT = c["dom"], c["dom"] == 1, c["nT"]
    par = dict(c["par"], variant=variant)
    theta = wall_map(dom, par, np.where(c["cells"]["A"], ANGLES["A"], ANGLES["B"]))
    m = start(solver(dom, par, tracers=c["kw"]), c["rR"], c["rB"], c["c0"], theta_map=theta)
    scalar = {a: start(solver(dom, dict(par, theta=a), tracers=c["kw"]), c["rR"], c["rB"], c["c0"]) for a in ANGLES.values()}
    refs = {a: cached(("channel", a), lambda a=a: snapshots(channel_reference(c, a), c["steps"])) for a in ANGLES.values()}
    worst = 0.0
    for n in c["steps"]:
        for x in [m] + list(scalar.values()):
            x.step(n - x.steps_done)
        for name, other in (("A", "B"), ("B", "A")):
            cells = c["cells"][name] & fl
            for k in range(nT):
                g = m.get_tracer_pdf(k)[cells]
                assert np.array_equal(g, scalar[ANGLES[name]].get_tracer_pdf(k)[cells]), (name, n, k)
                assert not np.array_equal(g, scalar[ANGLES[other]].get_tracer_pdf(k)[cells]), (name, n, k)
            worst = max(worst, compare_tracers(TracerChannel(m, cells), TracerChannel(refs[ANGLES[name]][n], cells), cells, nT,
                                               "channel %s against the reference at %g, variant %d, step %d" % (name, ANGLES[name], variant, n)))
        for k in range(nT):
            assert np.all(m.get_tracer_pdf(k)[~fl] == 0.0) and np.all(m.get_concentration(k)[~fl] == 0.0)
    print("two channels, variant %d: worst field-relative difference %.3e" % (variant, worst))
    for x in [m] + list(scalar.values()):
        x.close()


def test_the_map_with_slabs_and_tracers_equals_the_undivided_lattice():
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster
    c = channel_case()
    dom = c["dom"]
    theta = wall_map(dom, c["par"], np.where(c["cells"]["A"], ANGLES["A"], ANGLES["B"]))
    one = start(solver(dom, c["par"], tracers=c["kw"]), c["rR"], c["rB"], c["c0"], theta_map=theta)
    cl = RK3DCSFCluster(dom, c["par"], nslabs=3, diagnostics=True, tracers=c["kw"])
    start(cl, c["rR"], c["rB"], c["c0"], theta_map=theta)
    for n in (1, 30):
        done = one.steps_done
        one.step(n - done); cl.step(n - done)
        same_tracers(cl, one, 2, "map, 3 slabs, step %d" % n)
    assert np.array_equal(cl.get("fR"), one.get("fR"))
    one.close(); cl.close()


# ------------------------------------------------------------------------------------------------ 6. everything on
def test_everything_on_a_uniform_map_is_the_scalar_run():
    """periodic z, the body force G1, a uniform angle map and three tracers: every flow and tracer field of the run with the map equals the
    scalar-angle run's, which test_periodic_z_against_the_transposed_recipe holds to the reference (MRT, tautype 2, G1, variant 0)"""
    c = periodic_case("MRT", 2, "G1")
    dom = c["dom"]
    theta = wall_map(dom, c["par"], c["par"]["theta"])
    assert np.isfinite(theta).sum() > 100
    a = start(solver(dom, dict(c["par"], theta=97.0), tracers=c["kw"]), c["rR"], c["rB"], c["c0"], c["g"], theta_map=theta)
    b = start(solver(dom, c["par"], tracers=c["kw"]), c["rR"], c["rB"], c["c0"], c["g"])
    other = start(solver(dom, dict(c["par"], theta=97.0), tracers=c["kw"]), c["rR"], c["rB"], c["c0"], c["g"])
    for n in range(1, 11):
        a.step(1); b.step(1)
        for f in FLOW_STATE:
            assert np.array_equal(a.get(f), b.get(f)), (n, f)
        same_tracers(a, b, 3, "step %d" % n)
        for k in range(3):
            assert np.array_equal(a.get_concentration(k), b.get_concentration(k)), (n, k)
    other.step(10)
    assert not np.array_equal(other.get_tracer_pdf(0), a.get_tracer_pdf(0))          # (the map is what sets the angle: the scalar 97 differs)
    for x in (a, b, other):
        x.close()
