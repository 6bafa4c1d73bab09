"""The 2-D CSF solver under a per-colour body force and on a lattice periodic in y (lbmpm_rk2d_set_body_force, periodic_y=True)
against the recipe of tests/body_force_2d_ref.py around the unchanged oracle: every field of param_points.COMPARED after step 1 and
step 10 at TOL_2D.

1. open rows with force: the six rk2d-csf instances (both schedules among them) and the sixteen rk2d-tr instances (both copies of the
   two-copy launch, the single launch) at A with the first acceleration set and at B with the second;  2. bit-for-bit: force off again,
   force changed mid-run, g = 0;  3. the ring: a sealed lattice with a disc across the seam at ny = 45 (a partial tile row at the seam) and
   ny = 16, both wetting rules, SRT / MRT, both schedules, with and without force, with tracers; rolled lattices; the colours' masses; the
   idle inlet parameters; the record view;  4. refusals;  5. two layers of different viscosity against the analytic profile."""
import numpy as np
import pytest

import body_force_2d_ref as R
import param_points as P

pytestmark = pytest.mark.gpu

CHECKPOINTS = (1, P.STEPS)
_FLOW = R.FLOW_FIELDS
_SETS = (("A", 0), ("B", 1))          # (parameter point, acceleration set)


def _id(v):
    return ",".join(str(x) for x in v.values()) if isinstance(v, dict) else str(v)


def _hold(name, got, ref, what):
    d = P.differences(name, got, ref)
    for f, e in d.items():
        print("%s: %s %.2e" % (what, f, e))
        assert e < P.TOL_2D, "%s: %s off the reference by %.3e" % (what, f, e)
    return max(d.values())


def _solver(dom, p, rR, rB, variant=0, force=None):
    from openlbmpm_amd.rk2d import DEFAULT_PARAMS, RK2DSolver
    s = RK2DSolver(dom, {k: p[k] for k in DEFAULT_PARAMS if k in p}, diagnostics=True, variant=variant, periodic_y=bool(p.get("ring")))
    s.set_macro(rR, rB)
    if force is not None:
        s.set_body_force(red=force[0], blue=force[1])
    return s


def _got(s, nT=0):
    got = {f: s.get_compact(f) for f in _FLOW}
    got.update({"C%d" % k: s.get_tracer(k, compact=True) for k in range(nT)})
    return got


# ------------------------------------------------------------------------------------------------ 1. open rows
@pytest.mark.parametrize("point,gset,inst", [(pt, g, i) for pt, g in _SETS for i in P.RK2D_CSF["instances"]] +
                         [("A", 1, dict(P.RK2D_CSF["base"], variant=1))], ids=_id)
def test_forced_csf(point, gset, inst):
    p = P.params(P.RK2D_CSF, point, inst)
    variant = p.pop("variant", None)
    dom, rR, rB = P.lattice_2d()
    gR, gB = R.G_SETS[gset]
    ref = R.forced_run(dom, p, rR, rB, gR, gB, CHECKPOINTS)
    s = _solver(dom, p, rR, rB, variant, (gR, gB))
    assert s.body_force == (gR, gB)
    for n in CHECKPOINTS:
        s.step(n - s.steps_done)
        _hold("rk2d-csf", _got(s), ref[n], "%s set %d [%s] step %d" % (point, gset, _id(inst), n))
    s.close()


@pytest.mark.parametrize("point,gset,inst", [(pt, g, i) for pt, g in _SETS for i in P.RK2D_TR["instances"]], ids=_id)
def test_forced_tracers(point, gset, inst):
    """rk2d_forced_tracer on the tall lattice (both copies of node_finish), rk2d_forced<., true, ., true> on the short one"""
    p = P.params(P.RK2D_TR, point, inst)
    dom, rR, rB = P.lattice_tr(p["lattice"])
    nT = p["tracers"]
    conc = P.concentrations(dom, nT)
    gR, gB = R.G_SETS[gset]
    ref = R.forced_run(dom, p, rR, rB, gR, gB, CHECKPOINTS, conc=conc, tracer=p["tr"])
    s = _solver(dom, p, rR, rB, 0, (gR, gB))
    s.configure_tracers(**p["tr"])
    for k in range(nT):
        s.set_tracer(k, conc[k])
    for n in CHECKPOINTS:
        s.step(n - s.steps_done)
        _hold("rk2d-tr", _got(s, nT), ref[n], "%s set %d [%s] step %d" % (point, gset, _id(inst), n))
    s.close()


def test_the_record_carries_the_forced_velocity():
    """rec_* after n steps = what step n + 1 of the recipe holds after its boundary rows and its velocity, F_b / 2 included"""
    p = P.params(P.RK2D_CSF, "A")
    p.pop("variant", None)
    dom, rR, rB = P.lattice_2d()
    gR, gB = R.G_SETS[0]
    o = R.ForcedOracle(dom, p, rR, rB, gR, gB).run(P.STEPS + 1)
    s = _solver(dom, p, rR, rB, 0, (gR, gB))
    s.step(P.STEPS)
    scale = max(np.abs(o.rec["vx"]).max(), np.abs(o.rec["vy"]).max())
    for f in ("fR", "fB", "rhoR", "rhoB", "vx", "vy"):
        e = P.rel_err(s.get_compact("rec_" + f), o.rec[f], scale=scale if f[0] == "v" else None)
        print("rec_%s %.2e" % (f, e))
        assert e < P.TOL_2D, (f, e)
    s.close()


# ------------------------------------------------------------------------------------------------ 2. bit for bit
def _state(s):
    return {f: s.get(f) for f in ("fR", "fB", "vx", "vy", "Fx", "Fy", "phi")}


def _same(a, b, what):
    for f in a:
        assert np.array_equal(a[f], b[f]), "%s: %s differs (max %.3e)" % (what, f, np.abs(a[f] - b[f]).max())


@pytest.mark.parametrize("relax,variant", [("MRT", 0), ("SRT", 1)])
def test_force_off_and_force_changed_mid_run(relax, variant):
    """a context whose force is changed (or switched off) in mid-run equals two contexts joined by set_pdf.  set_pdf clears the lagged CSF
    force, so the one context passes its own state through set_pdf as well; it keeps its force across that call."""
    p = P.params(P.RK2D_CSF, "A", dict(P.RK2D_CSF["base"], relax=relax))
    p.pop("variant", None)
    dom, rR, rB = P.lattice_2d()
    g1, g2 = R.G_SETS
    for second in (g2, None):
        a = _solver(dom, p, rR, rB, variant, g1)
        a.step(5)
        fR, fB = a.get("fR"), a.get("fB")
        a.set_pdf(fR, fB)
        assert a.body_force == g1
        a.set_body_force(None) if second is None else a.set_body_force(red=second[0], blue=second[1])
        assert a.body_force == (second or ((0., 0.), (0., 0.)))
        a.step(5)
        b = _solver(dom, p, rR, rB, variant, second)
        b.set_pdf(fR, fB)
        b.step(5)
        _same(_state(a), _state(b), "second stretch %r" % (second,))
        assert np.abs(a.get("vx")).max() > 0
        a.close(); b.close()


@pytest.mark.parametrize("variant", [0, 1])
def test_zero_accelerations_equal_no_call(variant):
    """the forced kernels add exact zeros"""
    p = P.params(P.RK2D_CSF, "B")
    p.pop("variant", None)
    dom, rR, rB = P.lattice_2d()
    out = []
    for force in (None, ((0., 0.), (0., 0.))):
        s = _solver(dom, p, rR, rB, variant, force)
        s.step(P.STEPS)
        out.append(dict(_state(s), rec_vx=s.get("rec_vx"), rec_vy=s.get("rec_vy")))
        s.close()
    _same(out[0], out[1], "g = 0")


# ------------------------------------------------------------------------------------------------ 3. the ring
_RING = dict(ring=True)          # (no solver parameter: _solver turns it into periodic_y=True)
# (ny, relax, wetting, tautype, variant, acceleration set or None): every value of every axis with both heights and both schedules
_RING_CASES = [(45, "SRT", 1, 1, 0, 0), (45, "MRT", 2, 2, 1, 1), (16, "MRT", 1, 2, 0, None), (16, "SRT", 2, 1, 1, 0), (45, "MRT", 2, 1, 0, None),
               (16, "SRT", 1, 2, 1, None), (45, "SRT", 2, 2, 1, None), (16, "MRT", 2, 1, 0, 1)]


def _ring_params(point, **inst):
    return dict(P.RK2D_CSF[point], **dict(_RING, **inst))


@pytest.mark.parametrize("ny,relax,wetting,tautype,variant,gset", _RING_CASES)
def test_ring_against_the_transposed_oracle(ny, relax, wetting, tautype, variant, gset):
    p = _ring_params("A", relax=relax, wetting=wetting, tautype=tautype)
    dom, rR, rB = R.ring_lattice(ny)
    gR, gB = R.G_SETS[gset] if gset is not None else ((0., 0.), (0., 0.))
    ref = R.ring_run(dom, p, rR, rB, gR, gB, CHECKPOINTS)
    s = _solver(dom, p, rR, rB, variant, None if gset is None else (gR, gB))
    assert s.periodic_y
    for n in CHECKPOINTS:
        s.step(n - s.steps_done)
        _hold("rk2d-csf", _got(s), ref[n], "ring ny %d %s w%d t%d v%d set %s step %d" % (ny, relax, wetting, tautype, variant, gset, n))
    s.close()


@pytest.mark.parametrize("ny,relax,nT", [(45, "MRT", 3), (16, "SRT", 4)])
def test_ring_with_tracers(ny, relax, nT):
    """both ends off: the tracers wrap in y with the flow (rk2d_forced<., true, ., false>)"""
    p = _ring_params("B", relax=relax, wetting=2, tautype=2)
    dom, rR, rB = R.ring_lattice(ny)
    conc = P.concentrations(dom, nT)
    tr = P.tracer_kwargs(P.TRACER, "A", nT, (False, False))
    gR, gB = R.G_SETS[1]
    ref = R.ring_run(dom, p, rR, rB, gR, gB, CHECKPOINTS, conc=conc, tracer=tr)
    s = _solver(dom, p, rR, rB, 0, (gR, gB))
    s.configure_tracers(**tr)
    for k in range(nT):
        s.set_tracer(k, conc[k])
    for n in CHECKPOINTS:
        s.step(n - s.steps_done)
        _hold("rk2d-tr", _got(s, nT), ref[n], "ring tracers ny %d %s step %d" % (ny, relax, n))
    mass = [float(s.get_tracer(k).sum() / conc[k].sum() - 1.) for k in range(nT)]
    print("tracer masses", mass)
    if nT == 4:                      # (no reaction: every tracer keeps its mass, to the 1e-11 of test_param_points_gpu.py)
        assert max(abs(m) for m in mass) < 1e-11, mass
    s.close()


@pytest.mark.parametrize("ny,variant", [(45, 0), (16, 0), (45, 1)])
def test_a_rolled_lattice_gives_the_rolled_fields(ny, variant):
    """no row is special: the lattice rolled by 7 rows gives the rolled fields bit for bit, the record view included"""
    p = _ring_params("A", relax="MRT", wetting=2, tautype=2)
    dom, rR, rB = R.ring_lattice(ny)
    force = R.G_SETS[0]
    out = []
    for k in (0, 7):
        roll = lambda a: np.ascontiguousarray(np.roll(a, k, axis=0))
        s = _solver(roll(dom), p, roll(rR), roll(rB), variant, force)
        s.step(P.STEPS)
        out.append({f: np.roll(s.get(f), -k, axis=0) for f in ("fR", "fB", "vx", "vy", "Fx", "Fy", "K", "rec_fR", "rec_vy", "rec_rhoB")})
        s.close()
    _same(out[0], out[1], "rolled by 7")
    assert np.abs(out[0]["vy"]).max() > 1e-5


@pytest.mark.parametrize("relax,variant", [("MRT", 0), ("SRT", 1)])
def test_the_colours_masses_are_conserved(relax, variant):
    p = _ring_params("B", relax=relax, wetting=2, tautype=2)
    dom, rR, rB = R.ring_lattice(45)
    s = _solver(dom, p, rR, rB, variant, R.G_SETS[1])
    m0 = (s.get("rhoR").sum(), s.get("rhoB").sum())
    s.step(200)
    m1 = (s.get("rhoR").sum(), s.get("rhoB").sum())
    e = [abs(b / a - 1.) for a, b in zip(m0, m1)]
    print("%s variant %d: red mass drifts by %.2e, blue by %.2e in 200 steps" % (relax, variant, e[0], e[1]))
    assert np.isfinite(m1).all() and max(e) < 1e-12, e
    s.close()


def test_the_inlet_parameters_are_idle_on_a_ring():
    dom, rR, rB = R.ring_lattice(16)
    out = []
    for point in "AB":
        p = _ring_params("A", relax="MRT", wetting=2, tautype=2)
        p.update({k: P.RK2D_CSF[point][k] for k in ("vyR", "vyB", "rhoRH", "rhoBH", "rhoRL", "rhoBL")})
        s = _solver(dom, p, rR, rB, 0, R.G_SETS[0])
        s.step(P.STEPS)
        out.append(_state(s))
        s.close()
    _same(out[0], out[1], "inlet / outlet values of A and of B")


def test_the_ring_records_without_row_rules():
    p = _ring_params("A", relax="SRT", wetting=2, tautype=2)
    dom, rR, rB = R.ring_lattice(16)
    gR, gB = R.G_SETS[0]
    o = R.RingOracle(dom, p, rR, rB, gR, gB).run(P.STEPS + 1)
    rec = o.rec()
    s = _solver(dom, p, rR, rB, 0, (gR, gB))
    s.step(P.STEPS)
    scale = max(np.abs(rec["vx"]).max(), np.abs(rec["vy"]).max())
    for f in ("fR", "fB", "rhoR", "rhoB", "vx", "vy"):
        e = P.rel_err(s.get_compact("rec_" + f), rec[f], scale=scale if f[0] == "v" else None)
        print("ring rec_%s %.2e" % (f, e))
        assert e < P.TOL_2D, (f, e)
    s.close()


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals():
    import ctypes as C
    from openlbmpm_amd import _lib
    from openlbmpm_amd._lib import LbmpmError
    from openlbmpm_amd.rk2d import RK2DSolver
    dom, rR, rB = R.ring_lattice(16)
    # 'Periodic' is no kind of open row: params["inlet"] / ["outlet"] keep refusing it, one alone or both (the ring is periodic_y=True)
    for word in (dict(inlet="Periodic"), dict(outlet="Periodic"), dict(inlet="Periodic", outlet="Periodic")):
        with pytest.raises(ValueError):
            RK2DSolver(dom, word)
    # the library's own check of half a pair
    cfg = _lib.RK2DConfig()
    s = RK2DSolver(dom, periodic_y=True)
    L = s._L
    for a, b in ((2, 0), (1, 2)):
        cfg.nx, cfg.ny, cfg.wetting_type, cfg.tau_type, cfg.tau_r, cfg.tau_b, cfg.relaxation = dom.shape[1], dom.shape[0], 2, 2, 1.0, 1.0, 1
        cfg.inlet_type, cfg.outlet_type = a, b
        h = C.c_void_p()
        assert L.lbmpm_rk2d_create(C.byref(cfg), dom.ctypes.data_as(_lib.U8P), C.byref(h)) == _lib.ERR_INVALID and not h
    # tracer ends on a ring
    for ends in ((True, False), (False, True), (True, True)):
        with pytest.raises(LbmpmError) as e:
            s.configure_tracers(dirichlet_inlet=ends[0], free_outlet=ends[1])
        assert e.value.status == _lib.ERR_INVALID
    s.configure_tracers(dirichlet_inlet=False, free_outlet=False)
    # values that are not finite, half a pair of accelerations, a wrong shape
    for bad in ((float("nan"), 0.), (0., float("inf"))):
        with pytest.raises(LbmpmError) as e:
            s.set_body_force(red=bad, blue=(0., 0.))
        assert e.value.status == _lib.ERR_INVALID
    assert s.body_force == ((0., 0.), (0., 0.))
    assert L.lbmpm_rk2d_set_body_force(s._h, (C.c_double * 2)(1e-5, 0.), None) == _lib.ERR_INVALID
    with pytest.raises(ValueError):
        s.set_body_force((1e-5, 0., 0.))
    s.close()
    # the perturbation model: on a ring, after a force, and a force after it
    pert = dict(AkR=7e-3, AkB=7e-3, solidPhi=1.0)
    with pytest.raises(ValueError):
        RK2DSolver(dom, periodic_y=True, perturbation=pert)
    box = np.ones((24, 40), dtype=np.uint8)
    box[8:16, 0] = 0; box[8:16, -1] = 0
    s = RK2DSolver(box)
    s.set_body_force((1e-5, 0.))
    q = _lib.RK2DPerturbation()
    q.ak_r, q.ak_b, q.solid_phi, q.outlet_rho_r, q.outlet_rho_b = 7e-3, 7e-3, 1.0, 1.0, 1.0
    assert L.lbmpm_rk2d_set_perturbation(s._h, C.byref(q)) == _lib.ERR_UNSUPPORTED
    s.close()
    s = RK2DSolver(box, perturbation=pert)
    with pytest.raises(LbmpmError) as e:
        s.set_body_force((1e-5, 0.))
    assert e.value.status == _lib.ERR_UNSUPPORTED
    s.close()
    ring = RK2DSolver(dom, periodic_y=True)
    assert L.lbmpm_rk2d_set_perturbation(ring._h, C.byref(q)) == _lib.ERR_UNSUPPORTED
    ring.close()


# ------------------------------------------------------------------------------------------------ 5. physics
@pytest.mark.parametrize("relax", ["MRT", "SRT"])
def test_two_layer_force_driven_flow(relax):
    """two layers of different viscosity between walls 32 nodes apart on a ring, each colour driven by its own g_y: rec_vy against the
    analytic two-viscosity profile, within 1.5 x what the CPU reference shows for the same case and steps (body_force_2d_ref.TWO_LAYER)"""
    t = R.TWO_LAYER
    dom, rR, rB = R.two_layer_lattice()
    s = _solver(dom, dict(t["params"], relax=relax), rR, rB, 0, (t["gR"], t["gB"]))
    s.step(t["steps"])
    vy = s.get("rec_vy")
    assert np.abs(vy - vy[0]).max() < 1e-12 * np.abs(vy).max()          # (uniform along y)
    e = R.two_layer_error(vy[3, t["wall"]:-t["wall"]])
    print("%s: profile off the analytic one by %.4f %% of the peak (CPU reference: %.4f %%)" % (relax, 100 * e, 100 * R.TWO_LAYER_REFERENCE[relax]))
    assert e < R.TWO_LAYER_BOUND, e
    s.close()
