"""Every fused solver against its oracle at the two off-default parameter points A and B of tests/param_points.py, in every kernel
instance, after step 1 and after the last step, at the standing tolerance (1e-9 in 2-D, 1e-10 in 3-D, field-relative, vector components
against the vector's magnitude).  tests/test_param_points_cpu.py proves that at these points every parameter, every colour swap and
every rate moves the oracle by >= 1000 x that tolerance, and that the oracle follows itself within a tenth of it: a kernel that ignores a
config field, hard-codes its default or swaps two fields fails here by three orders of magnitude.

The 2-D CSF step with tracers fused into it (table rk2d-tr) is its own instantiation of the fused tile: sixteen instances that pair every
value of relaxation, wetting rule, tautype, inlet, outlet, tracer set (1, 2, 3 with the reaction, 4), tracer ends and launch path (tall
lattice: rk2d_fused_tracer with both copies of node_finish; short lattice: the single launch) with every value of every other axis.

At A also the paths that carry a parameter outside the step kernel: slabs (face pack / unpack), get_pdf and set_pdf of the 23-value
storage (beta enters its records), the 3-D CSF slabs and the bulk kernel csf3d_collide_deep (the MRT rates a second time)."""
import numpy as np
import pytest

import param_points as P
from helpers import rel_err

pytestmark = pytest.mark.gpu

CHECKPOINTS = (1, P.STEPS)


def _id(v):
    return ",".join(str(x) for x in v.values()) if isinstance(v, dict) else str(v)


def _cases(name):
    return [(point, inst) for point in "AB" for inst in P.TABLES[name]["instances"]]


def _hold(name, got, ref, what):
    d = P.differences(name, got, ref)
    for f, e in d.items():
        assert e < P.TABLES[name]["tol"], "%s: %s off the oracle by %.3e" % (what, f, e)
    return max(d.values())


def _report(name, point, inst, worst):
    print("%s %s [%s]: worst field-relative difference to the oracle %.2e" % (name, point, _id(inst), worst))


# ------------------------------------------------------------------------------------------------ 2-D
@pytest.mark.parametrize("point,inst", _cases("rk2d-csf"), ids=_id)
def test_rk2d_csf(point, inst):
    from openlbmpm_amd.rk2d import RK2DSolver
    t = P.RK2D_CSF
    p = P.params(t, point, inst)
    variant = p.pop("variant")
    dom, rR, rB = P.lattice_2d()
    ref = P.oracle_run("rk2d-csf", p, CHECKPOINTS)
    s = RK2DSolver(dom, p, diagnostics=True, variant=variant)
    s.set_macro(rR, rB)
    worst = 0.0
    for n in CHECKPOINTS:
        s.step(n - s.steps_done)
        got = {f: s.get_compact(f) for f in ("fR", "fB", "rhoR", "rhoB", "phi", "vx", "vy", "Gx", "Gy", "Fx", "Fy", "K")}
        worst = max(worst, _hold("rk2d-csf", got, ref[n], "%s %s step %d" % (point, _id(inst), n)))
    s.close()
    _report("rk2d-csf", point, inst, worst)


_FLOW_2D = ("fR", "fB", "rhoR", "rhoB", "phi", "vx", "vy", "Gx", "Gy", "Fx", "Fy", "K")


def _tracer_solver(p):
    """RK2DSolver with the tracers of p["tr"] on the lattice of the instance, started as the oracle of P.oracle_run("rk2d-tr", p) is"""
    from openlbmpm_amd.rk2d import DEFAULT_PARAMS, RK2DSolver
    dom, rR, rB = P.lattice_tr(p["lattice"])
    conc = P.concentrations(dom, p["tracers"])
    s = RK2DSolver(dom, {k: p[k] for k in DEFAULT_PARAMS}, diagnostics=True)
    s.set_macro(rR, rB)
    s.configure_tracers(**p["tr"])
    for k in range(p["tracers"]):
        s.set_tracer(k, conc[k])
    return s, conc


@pytest.mark.parametrize("point,inst", _cases("rk2d-tr"), ids=_id)
def test_rk2d_tracers(point, inst):
    """the CSF step with D2Q5 tracers fused into it -- rk2d_fused_tracer<MRT, SH> on the tall lattice, rk2d_fused<MRT, true, SH, 1> on the
    short one (launch_fused_tracer) -- against oracle.tr.CoupledOracle: every tracer's concentration and the flow fields of the CSF table"""
    p = P.params(P.RK2D_TR, point, inst)
    assert P.tracer_launch(P.lattice_tr(p["lattice"])[0].shape[0])[3] == (p["lattice"] == "short")
    ref = P.oracle_run("rk2d-tr", p, CHECKPOINTS)
    s, _ = _tracer_solver(p)
    worst = 0.0
    for n in CHECKPOINTS:
        s.step(n - s.steps_done)
        got = {f: s.get_compact(f) for f in _FLOW_2D}
        got.update({"C%d" % k: s.get_tracer(k, compact=True) for k in range(p["tracers"])})
        assert all("C%d" % k in ref[n] for k in range(p["tracers"]))
        worst = max(worst, _hold("rk2d-tr", got, ref[n], "%s %s step %d" % (point, _id(inst), n)))
    s.close()
    _report("rk2d-tr", point, inst, worst)


@pytest.mark.parametrize("relax,lattice", [("SRT", "tall"), ("MRT", "short")])
def test_rk2d_tracers_are_passive(relax, lattice):
    """the flow part of the tracer kernel sees neither the number of tracers nor their parameters: one tracer at A and four at B leave
    the same populations, bit for bit"""
    t = P.RK2D_TR
    out = []
    for point, nT in (("A", 1), ("B", 4)):
        p = P.params(t, "A", dict(t["base"], relax=relax, lattice=lattice, tracers=nT))
        p["tr"] = P.tracer_kwargs(t["tracer"], point, nT, p["ends"])
        s, _ = _tracer_solver(p)
        s.step(P.STEPS)
        out.append((s.get("fR"), s.get("fB")))
        s.close()
    for name, a, b in (("fR", out[0][0], out[1][0]), ("fB", out[0][1], out[1][1])):
        rows = np.flatnonzero(np.any(a != b, axis=(1, 2)))
        assert rows.size == 0, "%s differs between one tracer at A and four at B on the rows %s" % (name, rows.tolist())
    assert np.all(np.isfinite(out[0][0])) and np.abs(out[0][0]).max() > 0


@pytest.mark.parametrize("relax", ["SRT", "MRT"])
def test_rk2d_tracers_keep_their_mass_between_closed_ends(relax):
    """both ends off (the tracers' streaming wraps in y, walls bounce back), four tracers at A on the tall lattice: the summed concentration
    of every tracer stays, to the 1e-11 of test_tracer_gpu.py::test_tracer_mass_conserved_without_open_boundaries"""
    t = P.RK2D_TR
    p = P.params(t, "A", dict(t["base"], relax=relax, tracers=4, ends=(False, False)))
    s, conc = _tracer_solver(p)
    s.step(P.STEPS)
    for k in range(4):
        c = s.get_tracer(k)
        e = abs(c.sum() - conc[k].sum()) / conc[k].sum()
        print("rk2d-tr %s: tracer %d keeps its mass to %.2e" % (relax, k, e))
        assert np.isfinite(c).all() and e < 1e-11, (k, e)
    assert np.abs(s.get_tracer(0) - conc[0]).max() > 1e-3        # (and moved)
    s.close()


def _pert_solver(p, **more):
    from openlbmpm_amd.rk2d import RK2DSolver
    pert = {k: p[k] for k in ("AkR", "AkB", "solidPhi")}
    return RK2DSolver(P.lattice_2d_mixed()[0], dict({k: v for k, v in p.items() if k not in pert}, **more), diagnostics=True, perturbation=pert)


@pytest.mark.parametrize("point,inst", _cases("rk2d-pert"), ids=_id)
def test_rk2d_perturbation(point, inst):
    p = P.params(P.RK2D_PERT, point, inst)
    dom, rR, rB = P.lattice_2d_mixed()
    ref = P.oracle_run("rk2d-pert", p, CHECKPOINTS)
    s = _pert_solver(p)
    assert s.model == "Perturbation"
    if "fR" in ref[1]:
        s.set_macro(rR, rB)
    else:               # the reference by reduction to the 3-D oracle: the step that streams first starts one streaming earlier
        s.set_pdf(*P.pert_unstreamed(dom, rR, rB))
    worst = 0.0
    for n in CHECKPOINTS:
        s.step(n - s.steps_done)
        got = {f: s.get_compact(f) for f in ("fR", "fB", "rhoR", "rhoB", "phi", "vx", "vy")}
        worst = max(worst, _hold("rk2d-pert", got, ref[n], "%s %s step %d" % (point, _id(inst), n)))
    s.close()
    _report("rk2d-pert", point, inst, worst)


def test_rk2d_perturbation_does_not_read_the_csf_parameters():
    """the keys of RK2DSolver's parameters that the table of the perturbation step leaves out as unread: moved, they leave the run bit-equal"""
    p = P.params(P.RK2D_PERT, "A")
    _, rR, rB = P.lattice_2d_mixed()
    out = []
    for more in ({}, dict(sigma=0.23, theta=31.0, delta=0.5, tautype=1, wetting=1)):
        s = _pert_solver(p, **more)
        s.set_macro(rR, rB); s.step(P.STEPS)
        out.append({f: s.get(f) for f in ("fR", "fB", "rhoR", "rhoB", "phi", "vx", "vy")})
        s.close()
    for f in out[0]:
        assert np.array_equal(out[0][f], out[1][f]), f


@pytest.mark.parametrize("name,point,inst", [(n, pt, i) for n in ("sc2d-efs", "sc2d-original") for pt, i in _cases(n)], ids=_id)
def test_sc2d(name, point, inst):
    from openlbmpm_amd.sc2d import SC2DSolver
    p = P.params(P.TABLES[name], point, inst)
    dom, r0, r1 = P.lattice_sc()
    ref = P.oracle_run(name, p, CHECKPOINTS)
    f0 = P.sc_populations(dom, r0, r1)
    s = SC2DSolver(dom, p, diagnostics=True)
    s.set_pdf(f0[0], f0[1])
    names = [f for f in P.COMPARED[name]["scalars"]] + [c for vec in P.COMPARED[name]["vectors"] for c in vec]
    worst = 0.0
    for n in CHECKPOINTS:
        s.step(n - s.steps_done)
        worst = max(worst, _hold(name, {f: s.get_compact(f) for f in names}, ref[n], "%s %s step %d" % (point, _id(inst), n)))
    s.close()
    _report(name, point, inst, worst)


# ------------------------------------------------------------------------------------------------ 3-D perturbation model
_STORAGE_ENV = {"q23": {}, "dense": {"LBMPM_RK3D_LAYOUT": "dense"}, "compact38": {"LBMPM_RK3D_STORAGE": "38"}, "split": {}}
_STORAGE_KERNEL = {"q23": "rk3dq_fused", "dense": "rk3d_fused", "compact38": "rk3dc_fused", "split": "rk3dq_fused"}
_FIELDS_3D = ("rhoR", "rhoB", "phi", "vx", "vy", "vz")
_PARTS = [(0, 8), (8, 7), (15, 7)]


def _rk3d_env(monkeypatch, storage):
    for k in ("LBMPM_RK3D_LAYOUT", "LBMPM_RK3D_STORAGE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in _STORAGE_ENV[storage].items():
        monkeypatch.setenv(k, v)


def _rk3d_par(point, inst):
    p = P.params(P.RK3D, point, inst)
    return {k: v for k, v in p.items() if k not in ("storage", "nx")}


@pytest.mark.parametrize("point,inst", _cases("rk3d"), ids=_id)
def test_rk3d(point, inst, monkeypatch, knobs):
    from openlbmpm_amd.rk3d import RK3DCluster, RK3DSlab
    storage, nx = inst["storage"], inst["nx"]
    par = _rk3d_par(point, inst)
    dom, rR, rB = P.lattice_3d(nx)
    ref = P.oracle_run("rk3d", par, CHECKPOINTS, nx=nx)
    _rk3d_env(monkeypatch, storage)
    worst = 0.0
    if storage == "split":
        from test_rk3d_gpu import _threaded_slab_run
        knobs({"LBMPM_RK3D_SLAB_SCHEDULE": "split"})
        probe = RK3DSlab(dom, *_PARTS[1], par)
        assert probe.dominant_kernel == "rk3dq_fused" and probe.one_exchange
        probe.close()
        for n in CHECKPOINTS:
            got, _ = _threaded_slab_run(dom, rR, rB, _PARTS, par, [1, n - 1] if n > 1 else [1], fields=_FIELDS_3D)
            worst = max(worst, _hold("rk3d", got, ref[n], "%s %s step %d" % (point, _id(inst), n)))
    else:
        c = RK3DCluster(dom, 1, par)
        assert c.slabs[0].dominant_kernel == _STORAGE_KERNEL[storage]
        c.set_density(rR, rB)
        for n in CHECKPOINTS:
            c.step(n - c.slabs[0].steps_done); c.observe()
            worst = max(worst, _hold("rk3d", {f: c.get(f) for f in _FIELDS_3D}, ref[n], "%s %s step %d" % (point, _id(inst), n)))
        c.close()
    _report("rk3d", point, inst, worst)


_Q23_AT_A = [dict(nx=70, relax="MRT", **P._VP), dict(nx=64, relax="SRT", **P._PC)]


@pytest.mark.parametrize("inst", _Q23_AT_A, ids=_id)
def test_rk3d_q23_three_slabs_equal_the_single_domain_at_A(inst):
    """beta and the solid phi enter the face pack and unpack of the 23-value storage (csrc/rk3dq.h: the records travel, the colours are
    rebuilt on the other side): three slabs, bit for bit"""
    from openlbmpm_amd.rk3d import RK3DCluster
    par = _rk3d_par("A", inst)
    dom, rR, rB = P.lattice_3d(inst["nx"])
    ref = RK3DCluster(dom, 1, par); c = RK3DCluster(dom, 3, par)
    assert c.slabs[0].dominant_kernel == "rk3dq_fused" and c.slabs[0].one_exchange
    ref.set_density(rR, rB); c.set_density(rR, rB)
    for n in CHECKPOINTS:
        ref.step(n - ref.slabs[0].steps_done); ref.observe(); c.step(n - c.slabs[0].steps_done); c.observe()
        for f in _FIELDS_3D:
            assert np.array_equal(ref.get(f), c.get(f)), (f, n)
    ref.close(); c.close()


@pytest.mark.parametrize("inst", _Q23_AT_A, ids=_id)
def test_rk3d_q23_get_pdf_streamed_is_the_oracles_population_array_at_A(inst):
    """get_pdf rebuilds both colours from the 19 colour-blind populations and the record with beta (rk3dq.h); the mask of
    test_rk3d_state_gpu.py::test_get_pdf_streamed_is_the_oracles_population_array"""
    from openlbmpm_amd.rk3d import RK3DCluster
    from test_rk3d_state_gpu import CZ, stream
    par = _rk3d_par("A", inst)
    dom, rR, rB = P.lattice_3d(inst["nx"])
    o = P.oracle_run("rk3d", par, (P.STEPS,), nx=inst["nx"])[P.STEPS]
    c = RK3DCluster(dom, 1, par)
    c.set_density(rR, rB); c.step(P.STEPS)
    fR, fB = c.get_pdf()
    c.close()
    scale = float(np.max(np.abs(o["fR"] + o["fB"])))
    keep = np.ones(dom.shape + (19,), dtype=bool)
    keep[0] = keep[-1] = False
    keep[1][..., CZ == 1] = False
    keep[-2][..., CZ == -1] = False
    if inst["outlet"] == "Convective":
        # by the same argument the planes 1, 2 are no part of it: the head of the next step overwrites them, every direction, with the
        # streamed populations of plane 3 (the storage holds what the copied state collided to; rk3dq.h, "convective outlet")
        keep[1:3] = False
    for got, name in ((fR, "fR"), (fB, "fB")):
        diff = np.abs(np.where(keep, stream(got, dom) - o[name], 0.0)) / scale
        e = rel_err(np.where(keep, stream(got, dom), 0.0), np.where(keep, o[name], 0.0), scale=scale)
        print("get_pdf at A [%s] %s: %.2e" % (_id(inst), name, e))
        assert e < 1e-10, (name, e, "per plane: %s" % " ".join("%.1e" % v for v in diff.reshape(dom.shape[0], -1).max(axis=1)))


@pytest.mark.parametrize("inst", _Q23_AT_A, ids=_id)
def test_rk3d_q23_a_run_continues_through_get_pdf_and_set_pdf_at_A(inst):
    """set_pdf makes the records of the 23-value storage from the two colours with beta, get_pdf undoes it: a run continued through
    the pair follows the uninterrupted one to 1e-12"""
    from openlbmpm_amd.rk3d import RK3DCluster
    par = _rk3d_par("A", inst)
    dom, rR, rB = P.lattice_3d(inst["nx"])
    half = P.STEPS // 2
    a = RK3DCluster(dom, 1, par)
    a.set_density(rR, rB); a.step(half)
    fR, fB = a.get_pdf()
    a.step(P.STEPS - half); a.observe()
    want = {f: a.get(f) for f in _FIELDS_3D}
    a.close()
    b = RK3DCluster(dom, 1, par)
    b.set_pdf(fR, fB); b.step(P.STEPS - half); b.observe()
    got = {f: b.get(f) for f in _FIELDS_3D}
    b.close()
    d = P.differences("rk3d", got, want)
    print("continued through get_pdf -> set_pdf at A [%s]: %.2e" % (_id(inst), max(d.values())))
    for f, e in d.items():
        assert e < 1e-12, (f, e)


# ------------------------------------------------------------------------------------------------ 3-D CSF model
_CSF_FIELDS = ("fR", "fB", "rhoR", "rhoB", "phi", "vx", "vy", "vz", "Gx", "Gy", "Gz", "Fx", "Fy", "Fz", "K")
_CSF_SLAB_FIELDS = _CSF_FIELDS + ("rec_rhoR", "rec_rhoB", "rec_vz", "rec_phi")


@pytest.mark.parametrize("point,inst", _cases("rk3dcsf"), ids=_id)
def test_rk3dcsf(point, inst):
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    p = P.params(P.RK3D_CSF, point, inst)
    dom, rR, rB = P.lattice_csf()
    fl = dom == 1
    ref = P.oracle_run("rk3dcsf", p, CHECKPOINTS)
    s = RK3DCSFSolver(dom, p, diagnostics=True)
    s.set_macro(rR, rB)
    worst = 0.0
    for n in CHECKPOINTS:
        s.step(n - s.steps_done)
        what = "%s %s step %d" % (point, _id(inst), n)
        worst = max(worst, _hold("rk3dcsf", {f: s.get(f)[fl] for f in _CSF_FIELDS}, ref[n], what))
        assert np.all(s.get("fR")[~fl] == 0.0) and np.all(s.get("fB")[~fl] == 0.0)
        wet = ref[n]["kind"] == 2                       # phi on the wetting solids
        assert wet.any() and rel_err(s.get("phi")[wet], ref[n]["phi_dense"][wet]) < P.TOL_3D, what
    s.close()
    _report("rk3dcsf", point, inst, worst)


@pytest.mark.parametrize("relax", ["MRT", "SRT"])
def test_rk3dcsf_three_slabs_equal_the_undivided_lattice_at_A(relax):
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster, RK3DCSFSolver
    p = P.params(P.RK3D_CSF, "A", dict(P.RK3D_CSF["base"], relax=relax))
    dom, rR, rB = P.lattice_csf_slabs()
    a = RK3DCSFSolver(dom, p, diagnostics=True); c = RK3DCSFCluster(dom, p, nslabs=3, diagnostics=True)
    a.set_macro(rR, rB); c.set_macro(rR, rB)
    for n in CHECKPOINTS:
        a.step(n - a.steps_done); c.step(n - c.steps_done)
        for f in _CSF_SLAB_FIELDS:
            assert np.array_equal(a.get(f), c.get(f)), (n, f)
    assert np.all(np.isfinite(a.get("vz"))) and np.abs(a.get("Fz")).max() > 0
    a.close(); c.close()


def test_rk3dcsf_the_bulk_kernel_at_A():
    """csf3d_collide_deep (blocks of 256 cells deep inside one colour) holds the rate-to-moment map a second time: at A, with six distinct
    rates, the build that sends every cell through csf3d_collide (variant 1) leaves the same bits, while a front moves through the duct
    and the bulk kernel runs"""
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    p = P.params(P.RK3D_CSF, "A")
    dom, rR, rB = P.lattice_csf_slabs()
    a = RK3DCSFSolver(dom, dict(p, variant=0), diagnostics=True); b = RK3DCSFSolver(dom, dict(p, variant=1), diagnostics=True)
    a.set_macro(rR, rB); b.set_macro(rR, rB)
    seen = []
    for n in (1, 2, 20, 40):
        a.step(n - a.steps_done); b.step(n - b.steps_done)
        seen.append(a.bulk_cells)
        assert b.bulk_cells == 0
        for f in _CSF_SLAB_FIELDS:
            assert np.array_equal(a.get(f), b.get(f)), (n, f)
    assert max(seen) > 0, seen
    assert np.all(np.isfinite(a.get("vz")))
    a.close(); b.close()
