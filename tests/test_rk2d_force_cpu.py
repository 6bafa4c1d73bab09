"""The reference of the 2-D body force and of periodic y (tests/body_force_2d_ref.py) held to its own conditions, on the CPU, and the
plumbing from the ini, the drivers' keyword and the command line down to the library call.

1. g = 0 is RKOracle.run / CoupledOracle.run bit for bit;  2. the transposition the ring's reference rests on: on a sealed box the oracle
   and its transposed run agree (flow and tracers);  3. a rolled ring gives the rolled fields, the colours' masses stay;  4. every
   compared case follows itself from a start rippled in the last bit within a tenth of TOL_2D;  5. F_b / 2 left out of u, the colours'
   accelerations exchanged, g_x <-> g_y and a cut wrap each move a compared field by >= 1000 x TOL_2D;  6. the two-layer case's reference
   figure;  7. plumbing;  8. what the compiler made of the new kernels."""
import os

import numpy as np
import pytest

import body_force_2d_ref as R
import param_points as P

TOL = P.TOL_2D
Z = ((0., 0.), (0., 0.))


def _csf(point, inst):
    p = P.params(P.RK2D_CSF, point, inst)
    p.pop("variant", None)
    return p


def _ring(point="A", **inst):
    return dict(P.RK2D_CSF[point], **inst)


def _worst(name, a, b, drop_K=False):
    d = P.differences(name, a, b)
    if drop_K:
        d.pop("K", None)
    f = max(d, key=d.get)
    return d[f], f


# ------------------------------------------------------------------------------------------------ 1. g = 0
@pytest.mark.parametrize("point", "AB")
def test_zero_force_is_the_oracles_run(point):
    dom, rR, rB = P.lattice_2d()
    for inst in P.RK2D_CSF["instances"]:
        p = _csf(point, inst)
        a, b = P.oracle_run("rk2d-csf", p, (P.STEPS,))[P.STEPS], R.forced_run(dom, p, rR, rB, *Z, (P.STEPS,))[P.STEPS]
        assert all(np.array_equal(a[k], b[k]) for k in a), inst
    for inst in P.RK2D_TR["instances"][::3]:
        p = P.params(P.RK2D_TR, point, inst)
        d, r1, r2 = P.lattice_tr(p["lattice"])
        a = P.oracle_run("rk2d-tr", p, (P.STEPS,))[P.STEPS]
        b = R.forced_run(d, p, r1, r2, *Z, (P.STEPS,), conc=P.concentrations(d, p["tracers"]), tracer=p["tr"])[P.STEPS]
        assert all(np.array_equal(a[k], b[k]) for k in a), inst


# ------------------------------------------------------------------------------------------------ 2. transposition
def _box():
    dom, rR, rB = R.ring_lattice(45)
    box = dom.copy()
    box[:4] = 0; box[-4:] = 0
    return box, rR * (box == 1), rB * (box == 1)


@pytest.mark.parametrize("relax,wetting", [("SRT", 1), ("SRT", 2), ("MRT", 1), ("MRT", 2)])
def test_the_oracle_and_its_transposed_run_agree_on_a_sealed_box(relax, wetting):
    """a box closed on all four sides runs either way round; both inlets, the convective outlet (the pressure outlet's ghost rule picks its
    nodes by compact index and is not symmetric).  Flow and three reacting tracers within a tenth of TOL_2D; K, a quotient by |G| compared
    from |G| = 1e-6 on, within TOL_2D (rounding of G, 1e-16, over 1e-6, times the handful of terms of the curvature stencil)."""
    box, rR, rB = _box()
    conc = P.concentrations(box, 3)
    tr = P.tracer_kwargs(P.TRACER, "A", 3, (False, False))
    for inlet in ("Neumann", "Dirichlet"):
        p = _csf("A", dict(relax=relax, wetting=wetting, tautype=2, inlet=inlet, outlet="Convective"))
        a = R.forced_run(box, p, rR, rB, *R.G_SETS[0], (P.STEPS,), conc=conc, tracer=tr)[P.STEPS]
        b = R.ring_run(box, p, rR, rB, *R.G_SETS[0], (P.STEPS,), conc=conc, tracer=tr)[P.STEPS]
        d = P.differences("rk2d-tr", b, a)
        print(relax, wetting, inlet, {k: "%.1e" % v for k, v in d.items()})
        assert d.pop("K") < TOL and max(d.values()) < 0.1 * TOL, d


# ------------------------------------------------------------------------------------------------ 3. the ring
@pytest.mark.parametrize("ny", [45, 16])
def test_a_rolled_ring_gives_the_rolled_fields_and_keeps_its_masses(ny):
    dom, rR, rB = R.ring_lattice(ny)
    assert R.walls_suffice(dom) and np.any(dom[0] == 0) and np.any(dom[-1] == 0)          # (a disc across the seam)
    p = _ring("A", relax="MRT", wetting=2, tautype=2)
    roll = lambda a: np.ascontiguousarray(np.roll(a, 7, axis=0))
    a = R.RingOracle(dom, p, rR, rB, *R.G_SETS[0]).run(P.STEPS)
    b = R.RingOracle(roll(dom), p, roll(rR), roll(rB), *R.G_SETS[0]).run(P.STEPS)
    fa, fb = a.fields(), b.fields()
    sel, selr = dom.reshape(-1) == 1, roll(dom).reshape(-1) == 1
    for k in R.FLOW_FIELDS:
        da = np.zeros((dom.size,) + fa[k].shape[1:]); da[sel] = fa[k]
        db = np.zeros((dom.size,) + fb[k].shape[1:]); db[selr] = fb[k]
        assert np.array_equal(roll(da.reshape(dom.shape + fa[k].shape[1:])), db.reshape(dom.shape + fb[k].shape[1:])), k
    for c, r0 in (("rhoR", rR), ("rhoB", rB)):
        e = abs(fa[c].sum() / r0.sum() - 1.)
        print("ny %d: %s drifts by %.1e in %d steps" % (ny, c, e, P.STEPS))
        assert e < 1e-14
    # the inlet and outlet values are idle
    q = dict(p, **{k: P.RK2D_CSF["B"][k] for k in ("vyR", "vyB", "rhoRH", "rhoBH", "rhoRL", "rhoBL")})
    fq = R.RingOracle(dom, q, rR, rB, *R.G_SETS[0]).run(P.STEPS).fields()
    assert all(np.array_equal(fq[k], fa[k]) for k in R.FLOW_FIELDS)


# ------------------------------------------------------------------------------------------------ 4. conditioning
def _ripple(*arrays):
    return [P.last_bit(a, float(i)) for i, a in enumerate(arrays)]


@pytest.mark.parametrize("point,gset", [("A", 0), ("B", 1)])
def test_the_open_row_cases_follow_a_last_bit_ripple(point, gset):
    dom, rR, rB = P.lattice_2d()
    for inst in P.RK2D_CSF["instances"]:
        p = _csf(point, inst)
        a = R.forced_run(dom, p, rR, rB, *R.G_SETS[gset], (P.STEPS,))[P.STEPS]
        b = R.forced_run(dom, p, *_ripple(rR, rB), *R.G_SETS[gset], (P.STEPS,))[P.STEPS]
        e, f = _worst("rk2d-csf", b, a)
        assert np.all(np.isfinite(a["fR"])) and max(np.abs(a["vx"]).max(), np.abs(a["vy"]).max()) < 0.05
        assert e < 0.1 * TOL, (inst, f, e)
    for inst in P.RK2D_TR["instances"]:
        p = P.params(P.RK2D_TR, point, inst)
        d, r1, r2 = P.lattice_tr(p["lattice"])
        conc = P.concentrations(d, p["tracers"])
        a = R.forced_run(d, p, r1, r2, *R.G_SETS[gset], (P.STEPS,), conc=conc, tracer=p["tr"])[P.STEPS]
        b = R.forced_run(d, p, *_ripple(r1, r2), *R.G_SETS[gset], (P.STEPS,), conc=conc, tracer=p["tr"])[P.STEPS]
        e, f = _worst("rk2d-tr", b, a)
        assert e < 0.1 * TOL, (inst, f, e)


@pytest.mark.parametrize("ny", [45, 16])
def test_the_ring_cases_follow_a_last_bit_ripple(ny):
    """... and a second rounding of the same step, the lattice mirrored in x: the wetting rules' branches must not hang on the order of a
    sum (a colour gradient built from phase-field values +-1 alone meets their ties exactly; ring_lattice says what it does about it)"""
    dom, rR, rB = R.ring_lattice(ny)
    m = lambda a: np.ascontiguousarray(a[..., ::-1])
    MX = [0, 3, 2, 1, 4, 6, 5, 8, 7]
    sel, selm = dom.reshape(-1) == 1, m(dom).reshape(-1) == 1
    for relax, wetting, tautype, g in (("SRT", 1, 1, R.G_SETS[0]), ("MRT", 2, 2, R.G_SETS[1]), ("MRT", 1, 2, Z), ("SRT", 2, 1, Z)):
        p = _ring("A", relax=relax, wetting=wetting, tautype=tautype)
        for n in (1, P.STEPS):
            a = R.ring_run(dom, p, rR, rB, *g, (n,))[n]
            b = R.ring_run(dom, p, *_ripple(rR, rB), *g, (n,))[n]
            e, f = _worst("rk2d-csf", b, a)
            assert e < 0.1 * TOL, (relax, wetting, n, f, e)
            c = R.ring_run(m(dom), p, m(rR), m(rB), (-g[0][0], g[0][1]), (-g[1][0], g[1][1]), (n,))[n]
            back = {}
            for k in R.FLOW_FIELDS:
                d = np.zeros((dom.size,) + c[k].shape[1:]); d[selm] = c[k]
                back[k] = np.ascontiguousarray(d.reshape(dom.shape + c[k].shape[1:])[:, ::-1]).reshape((-1,) + c[k].shape[1:])[sel]
            back["fR"], back["fB"] = back["fR"][:, MX], back["fB"][:, MX]
            for k in ("vx", "Gx", "Fx"):
                back[k] = -back[k]
            e, f = _worst("rk2d-csf", back, a)
            assert e < 0.1 * TOL, ("mirrored", relax, wetting, n, f, e)


# ------------------------------------------------------------------------------------------------ 5. sensitivity
@pytest.mark.parametrize("point,gset", [("A", 0), ("B", 1)])
def test_every_part_of_the_force_matters(point, gset):
    dom, rR, rB = P.lattice_2d()
    gR, gB = R.G_SETS[gset]
    for inst in P.RK2D_CSF["instances"]:
        p = _csf(point, inst)
        ref = R.forced_run(dom, p, rR, rB, gR, gB, (P.STEPS,))[P.STEPS]
        for what, run in (("no force", R.forced_run(dom, p, rR, rB, *Z, (P.STEPS,))),
                          ("F_b / 2 left out of u", R.forced_run(dom, p, rR, rB, gR, gB, (P.STEPS,), half_in_u=False)),
                          ("colours exchanged", R.forced_run(dom, p, rR, rB, gB, gR, (P.STEPS,))),
                          ("gx <-> gy", R.forced_run(dom, p, rR, rB, gR[::-1], gB[::-1], (P.STEPS,)))):
            e, f = _worst("rk2d-csf", run[P.STEPS], ref, drop_K=True)
            print("%s %s: %s moves %s by %.2e" % (point, P.TABLES["rk2d-csf"]["name"], what, f, e))
            assert e >= 1000 * TOL, (inst, what, f, e)


def test_a_cut_wrap_matters():
    """the ring against the same lattice with a wall across the seam (row 0 solid): the nodes both have"""
    dom, rR, rB = R.ring_lattice(16)
    cut = dom.copy(); cut[0] = 0
    p = _ring("A", relax="MRT", wetting=2, tautype=2)
    a = R.ring_run(dom, p, rR, rB, *R.G_SETS[0], (P.STEPS,))[P.STEPS]
    b = R.ring_run(cut, p, rR * (cut == 1), rB * (cut == 1), *R.G_SETS[0], (P.STEPS,))[P.STEPS]
    both = (cut == 1).reshape(-1)[dom.reshape(-1) == 1]
    e = max(P.rel_err(b[k], a[k][both]) for k in ("fR", "fB", "rhoR", "rhoB"))
    assert e >= 1000 * TOL, e


# ------------------------------------------------------------------------------------------------ 6. physics
def test_the_two_layer_reference_figure():
    """SRT, the 16 000 steps of the GPU test: the CPU reference is 1.319 % of the peak off the analytic two-viscosity profile (MRT:
    1.278 %); body_force_2d_ref.TWO_LAYER_BOUND is 1.5 times that"""
    t = R.TWO_LAYER
    dom, rR, rB = R.two_layer_lattice()
    o = R.RingOracle(dom, dict(t["params"], relax="SRT"), rR, rB, t["gR"], t["gB"]).run(t["steps"])
    d = np.zeros(dom.size); d[dom.reshape(-1) == 1] = o.rec()["vy"]
    e = R.two_layer_error(d.reshape(dom.shape)[3, t["wall"]:-t["wall"]])
    print("two layers, SRT: %.4f %% of the peak" % (100 * e))
    assert abs(e / R.TWO_LAYER_REFERENCE["SRT"] - 1.) < 1e-2 and R.TWO_LAYER_BOUND == 1.5 * max(R.TWO_LAYER_REFERENCE.values())


# ------------------------------------------------------------------------------------------------ 7. plumbing
GR, GB = (1.0e-5, -2.0e-5), (-2.5e-5, 1.5e-5)


class _Calls:
    """stands in for the loaded library: records the config handed to lbmpm_rk2d_create / _tracer_configure and the doubles of every
    lbmpm_rk2d_set_body_force (None: switched off), and hands them back"""

    def __init__(self):
        self.forces, self.seen = [], {}

    def __getattr__(self, fn):
        def call(*args):
            if fn == "lbmpm_rk2d_set_body_force":
                self.forces.append(None if args[1] is None and args[2] is None else (tuple(args[1]), tuple(args[2])))
            elif fn == "lbmpm_rk2d_get_body_force":
                last = (self.forces[-1] if self.forces else None) or Z
                args[1][:], args[2][:] = last[0], last[1]
            elif fn.endswith("_create") or fn.endswith("_tracer_configure"):
                cfg = args[0 if fn.endswith("_create") else 1]._obj
                self.seen.update({f: getattr(cfg, f) for f, _ in cfg._fields_})
            return 0
        return call


@pytest.fixture
def calls(monkeypatch):
    from openlbmpm_amd import _lib
    cap = _Calls()
    monkeypatch.setattr(_lib, "lib", lambda: cap)
    return cap


def test_the_solver_hands_over_four_doubles(calls):
    from openlbmpm_amd.rk2d import DEFAULT_PARAMS, RK2DSolver
    from openlbmpm_amd import _lib
    s = RK2DSolver(np.ones((8, 8), np.uint8))
    assert not s.periodic_y and (calls.seen["inlet_type"], calls.seen["outlet_type"]) == (0, 0)
    s.set_body_force(GR)
    s.set_body_force(red=GR, blue=GB)
    s.set_body_force(blue=GB)
    assert s.body_force == ((0., 0.), GB)
    s.set_body_force(None)
    assert calls.forces == [(GR, GR), (GR, GB), ((0., 0.), GB), None]
    for bad in ((1., 2., 3.), 3.0, ((1., 2.),)):
        with pytest.raises(ValueError):
            s.set_body_force(bad)
    ring = RK2DSolver(np.ones((8, 8), np.uint8), periodic_y=True)
    assert ring.periodic_y and (calls.seen["inlet_type"], calls.seen["outlet_type"]) == (2, 2)
    # 'Periodic' is no kind of open row: the parameters keep refusing the word, one alone or both
    for word in (dict(inlet="Periodic"), dict(outlet="Periodic"), dict(inlet="Periodic", outlet="Convective"), dict(inlet="Periodic", outlet="Periodic")):
        with pytest.raises(ValueError):
            RK2DSolver(np.ones((8, 8), np.uint8), word)
    with pytest.raises(ValueError):
        RK2DSolver(np.ones((8, 8), np.uint8), periodic_y=True, perturbation=dict(AkR=1e-3, AkB=1e-3))
    # the force is neither a parameter nor a configuration field
    assert "body_force" not in DEFAULT_PARAMS and not [f for f, _ in _lib.RK2DConfig._fields_ if "force" in f or "accel" in f]


class _Out:
    def __init__(self):
        self.written = {}

    def write(self, group, name, array):
        self.written["/%s/%s" % (group, name)] = np.array(array)


def test_the_ini_and_the_drivers_argument_reach_the_solver(tmp_path, calls, monkeypatch):
    from ini_fixtures import write_rk, write_transport
    from openlbmpm_amd import RKD2Q9, config
    from openlbmpm_amd.RKD2Q9 import RKColorGradientLBM
    from openlbmpm_amd.Transport2DRK import Transport2DRK
    from openlbmpm_amd.rk2d import RK2DSolver
    d = str(tmp_path)
    write_rk(d)
    write_transport(d)
    files = []

    class FakeFile(_Out):
        def __init__(self, directory, name, groups):
            _Out.__init__(self)
            self.path, self.groups = name, tuple(groups)
            files.append(self)
    monkeypatch.setattr(RKD2Q9, "ResultFile", FakeFile)
    assert config.read_rk2d(d)["periodic_y"] is False
    for make in (RKColorGradientLBM, Transport2DRK):
        for arg, want in ((GR, (GR, GR)), (dict(red=GB, blue=GR), (GB, GR)), (dict(blue=GR), ((0., 0.), GR))):
            sim = make(d, body_force=arg)
            assert not sim.periodic_y
            out = sim._open_flow_file(RK2DSolver(np.ones((8, 8), np.uint8)))
            assert calls.forces[-1] == want, (make.__name__, arg)
            assert np.array_equal(out.written["/BodyForce/Acceleration"], np.array(want)) and out.written["/BodyForce/Acceleration"].shape == (2, 2)
            assert ("BodyForce", "Acceleration") in out.groups and "/BoundaryCondition/PeriodicY" not in out.written
        n = len(calls.forces)
        out = make(d)._open_flow_file(RK2DSolver(np.ones((8, 8), np.uint8)))          # without either feature the file is what it was
        assert out.groups == RKD2Q9._FLOW_GROUPS and not out.written and len(calls.forces) == n
        for bad in ((1., 2., 3.), dict(green=GR), "down"):
            with pytest.raises(config.ConfigError):
                make(d, body_force=bad)
    # periodic y from the ini
    ini = tmp_path / "RKtwophasesetup2D.ini"
    plain = ini.read_text()
    ring = plain.replace("BoundaryTypeInlet = 'Neumann'", "BoundaryTypeInlet = 'Periodic'").replace("BoundaryTypeOutlet = 'Dirichlet'", "BoundaryTypeOutlet = 'Periodic'")
    assert ring.count("'Periodic'") == 2
    for half in (plain.replace("BoundaryTypeInlet = 'Neumann'", "BoundaryTypeInlet = 'Periodic'"),
                 plain.replace("BoundaryTypeOutlet = 'Dirichlet'", "BoundaryTypeOutlet = 'Periodic'"),
                 ring.replace("SurfaceTensionType = 'CSF'", "SurfaceTensionType = 'Perturbation'")):
        ini.write_text(half)
        with pytest.raises(config.ConfigError):
            config.read_rk2d(d)
    ini.write_text(ring)
    assert config.read_rk2d(d)["periodic_y"] is True
    sim = RKColorGradientLBM(d, body_force=GR)
    keys = ("sigma", "inlet", "outlet", "vyR")
    assert sim._solver_params(keys) == dict(sigma=sim.par["sigma"], vyR=sim.par["vyR"])          # the word goes into the keyword, not the parameters
    out = sim._open_flow_file(RK2DSolver(np.ones((8, 8), np.uint8), sim._solver_params(keys), periodic_y=sim.periodic_y))
    assert (calls.seen["inlet_type"], calls.seen["outlet_type"]) == (2, 2)
    assert out.written["/BoundaryCondition/PeriodicY"].tolist() == [1] and "/BodyForce/Acceleration" in out.written
    # an image gets its side walls and no buffer rows
    img = np.full((12, 9), 255.0); img[0, 0] = img[-1, -1] = img[5, 4] = 0.0
    sim = RKColorGradientLBM(d, image=img)
    sim.par["image"] = True
    sim.initializeDomainBorder()
    assert sim.isDomain.shape == (12, 9) and not sim.isDomain[:, 0].any() and not sim.isDomain[:, -1].any()
    # the tracers' ends name rows that are not special on a ring (the fixture's transportsetup.ini has both)
    with pytest.raises(config.ConfigError):
        Transport2DRK(d)
    # the perturbation model has no force term; the ini's own [BodyForce] stays refused (tests/test_body_force_cpu.py)
    ini.write_text(plain.replace("SurfaceTensionType = 'CSF'", "SurfaceTensionType = 'Perturbation'"))
    try:
        config.read_rk2d(d)
    except config.ConfigError:
        pass                    # (the fixture lacks the perturbation model's keys: nothing to refuse a force on)
    else:
        with pytest.raises(config.ConfigError):
            RKColorGradientLBM(d, body_force=GR)


def test_the_command_line_reaches_the_drivers(monkeypatch):
    from openlbmpm_amd import RKD2Q9, Transport2DRK, __main__ as cli
    seen = {}

    class Fake:
        timeSteps, voidSpace = 1, 1

        def __init__(self, ini, **kw):
            seen.update(kw)

        def runRKColorGradient2D(self):
            return "x"

        def runTransport2DMPMCRKNew(self):
            return ("x", "y")

    monkeypatch.setattr(RKD2Q9, "RKColorGradientLBM", Fake)
    monkeypatch.setattr(Transport2DRK, "Transport2DRK", Fake)
    for model in ("rk", "tr"):
        for argv, want in (([], None), (["--body-force", "1e-5", "-2e-5"], GR),
                           (["--body-force", "1e-5", "-2e-5", "--body-force-blue", "-2.5e-5", "1.5e-5"], dict(red=GR, blue=GB)),
                           (["--body-force-blue", "-2.5e-5", "1.5e-5"], dict(red=(0., 0.), blue=GB))):
            seen.clear()
            assert cli.main([model, "somewhere"] + argv) == 0
            assert seen["body_force"] == want, (model, argv)
        for argv in (["--body-force", "1e-5", "0", "0"], ["--body-force", "1e-5"], ["--body-force", "1e-5", "0", "--body-force-blue", "1", "2", "3"]):
            with pytest.raises(SystemExit):
                cli.main([model, "somewhere"] + argv)
    with pytest.raises(SystemExit):
        cli.main(["sc", "somewhere", "--body-force", "1e-5", "0"])
    with pytest.raises(SystemExit):
        cli.main(["rk3d", "somewhere", "--body-force", "1e-5", "0"])


# ------------------------------------------------------------------------------------------------ 8. the code object
def test_the_new_kernels_and_the_old_counts():
    """the forced family exists in the shapes the launcher reaches (64 x 8 and 64 x 4: SRT / MRT x plain / tracers x ring / open rows, and the
    two-copy tracer launch), each within the 128 registers that let two 512-thread workgroups share a CU, without scratch or spills; its
    names hold neither of the strings tests/test_codeobj.py counts the unforced instances by"""
    from openlbmpm_amd import codeobj
    from test_codeobj import LIB
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    k = codeobj.kernels(LIB)
    forced = {n: m for n, m in k.items() if "rk2d_forcedI" in n}
    two = {n: m for n, m in k.items() if "rk2d_forced_tracerI" in n}
    assert len(forced) == 16 and len(two) == 4, (sorted(forced), sorted(two))
    for shape in ("FusedShapeILi8ELi1", "FusedShapeILi4ELi1"):
        assert sum(shape in n for n in forced) == 8 and sum(shape in n for n in two) == 2
    for n, m in list(forced.items()) + list(two.items()):
        print("%s: %d VGPRs, %d SGPRs" % (n, m[".vgpr_count"], m[".sgpr_count"]))
        assert m[".vgpr_count"] <= 128 and m[".private_segment_fixed_size"] == 0 and m[".vgpr_spill_count"] == 0, n
        assert "rk2d_fused" not in n
    # the unforced family is what it was: four shapes x SRT / MRT, the single-launch tracer step in two shapes, the two-copy launch in two
    # (tests/test_codeobj.py counts the ten of the twelve that hold asm loads: all but the shape with two nodes per lane)
    assert sum("rk2d_fusedI" in n for n in k) == 12 and sum("rk2d_fused_tracerI" in n for n in k) == 4
    assert sum("rk2d_fusedI" in n and "FusedShapeILi16ELi2" not in n for n in k) == 10
    assert sum("rk2d_collide_stream_forcedI" in n for n in k) == 4 and sum("rk2d_observe_forcedI" in n for n in k) == 2
    assert sum("rk2d_phase_field_ring" in n for n in k) == 1
