"""Periodic z of the 3-D CSF solver (inlet = outlet = 'Periodic': LBMPM_INLET_PERIODIC with LBMPM_OUTLET_NONE) on the GPU.

The reference is tests/periodic_ref.py -- the unchanged oracle on the lattice with x and z exchanged -- whose own conditions
tests/test_rk3d_csf_periodic_cpu.py holds.
1. parity with it;  2. a lattice rolled along z gives the rolled fields, bit for bit, and the same bulk count;  3. the bulk path against
the full path across the seam;  4. a state uniform along z stays so;  5. slabs, two processes;  6. conservation;  7. the two-layer
force-driven flow against its analytic profile;  8. refusals."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import body_force_ref as R
import periodic_ref as PR
from helpers import rel_err
from test_rk3d_csf_gpu import TOL, compare_all, solver
from test_rk3d_gpu import _free_port

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERIODIC = dict(inlet="Periodic", outlet="Periodic")
NO_FORCE = ((0., 0., 0.), (0., 0., 0.))
STATE = ("fR", "fB", "rhoR", "rhoB", "phi", "Gx", "Gy", "Gz", "Fx", "Fy", "Fz", "K", "vx", "vy", "vz",
         "rec_fR", "rec_rhoR", "rec_rhoB", "rec_vx", "rec_vy", "rec_vz", "rec_phi")


def fields_of(s, names=STATE):
    out = {f: s.get(f) for f in names}
    for t in range(getattr(s, "num_tracers", 0)):
        out["tracer %d" % t] = s.get_tracer_pdf(t)
    return out


def same(a, b, what):
    for f in a:
        assert np.array_equal(a[f], b[f]), (what, f, float(np.max(np.abs(a[f] - b[f]))))


# ------------------------------------------------------------------------------------------------ 1. parity
_REFS = {}


def reference(relax, tautype, gset):
    """snapshots of the reference after step 1 and step 10, each with its record view (what the next step's first half makes of it)"""
    key = (relax, tautype, gset)
    if key not in _REFS:
        dom, rR, rB = PR.parity_lattice()
        par = PR.parity_params(relax, tautype)
        g = R.G_SETS[gset] if gset else NO_FORCE
        a = PR.PeriodicRef(dom, rR, rB, par, *g).run(1)
        s1 = PR.Snapshot(a)
        r1 = PR.Snapshot(PR.PeriodicRef(dom, rR, rB, par, *g).run(1).step_a())
        s10 = PR.Snapshot(a.run(9))
        r10 = PR.Snapshot(a.step_a())
        _REFS[key] = (s1, r1, s10, r10)
    return _REFS[key]


def check_record(s, rec, what):
    fl = rec.fl
    umax = max(float(np.max(np.abs(rec.field(c)[fl]))) for c in ("vx", "vy", "vz"))
    for f in ("fR", "fB", "rhoR", "rhoB", "vx", "vy", "vz", "phi"):
        e = rel_err(s.get("rec_" + f)[fl], rec.field(f)[fl], scale=umax if f[0] == "v" else None)
        assert e < TOL, "record view %s: %s %.3e" % (what, f, e)
    # the totals of integrals(): sums over what rec_* hand out
    want, got = PR.totals_of(rec), s.integrals()
    mass = want["mass_R"] + want["mass_B"]
    scale = dict(mass_R=mass, mass_B=mass, flux_R=umax * mass, flux_B=umax * mass, mom_x=umax * mass, mom_y=umax * mass,
                 uz_R=umax * want["cells"], uz_B=umax * want["cells"], umax2=umax * umax)
    for c, w in want.items():
        if c in scale:
            assert abs(got.total(c) - w) < TOL * scale[c], "integrals %s: %s %r != %r" % (what, c, got.total(c), w)
        else:
            assert got.total(c) == w, "integrals %s: %s %r != %r" % (what, c, got.total(c), w)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("gset", ["G1", None])
@pytest.mark.parametrize("relax,tautype", [("SRT", 1), ("SRT", 2), ("MRT", 1), ("MRT", 2)])
def test_against_the_transposed_oracle(relax, tautype, gset, variant):
    """the fields, the tolerance and the treatment of K of tests/test_rk3d_csf_gpu.py against the crisp oracle, after step 1 and
    step 10; the record view, the totals of integrals() and the set-up tables (a grain lies across the seam)"""
    dom, rR, rB = PR.parity_lattice()
    s1, r1, s10, r10 = reference(relax, tautype, gset)
    s = solver(dom, PR.parity_params(relax, tautype, variant=variant))
    assert s.periodic_z
    if gset:
        s.set_body_force(red=R.G_SETS[gset][0], blue=R.G_SETS[gset][1])
    s.set_macro(rR, rB)
    assert np.array_equal(s.get("kind").astype(np.uint8), s1.field("kind")) and s.num_fluid_nodes == int(dom.sum())
    for c in ("nsx", "nsy", "nsz"):
        assert rel_err(s.get(c), s1.field(c)) < TOL, c
    what = "%s tautype %d %s variant %d" % (relax, tautype, gset, variant)
    s.step(1)
    w1 = compare_all(s, s1, what + ", step 1")
    check_record(s, r1, what + ", after step 1")
    s.step(9)
    w10 = compare_all(s, s10, what + ", step 10")
    check_record(s, r10, what + ", after step 10")
    print("%s: worst field-relative difference %.2e after step 1, %.2e after step 10" % (what, w1, w10))
    assert np.max(np.abs(s10.field("K"))) > 1e-3
    s.close()


# ------------------------------------------------------------------------------------------------ 2. translation, 3. the bulk path
TRACERS = dict(num_tracers=3, diffusion_x=(0.12, 0.1, 0.15), beta_interface=(0.4, 0.0, 0.2), reaction_rate=0.03, diffusion_j=(0.0, 0.25, 0.1),
               dirichlet_inlet=False, free_outlet=False)
ROLL_STEPS = 12
_FREE = {}


def free_solver(k, variant):
    """a solver on the 16^3 lattice of tests/periodic_ref.py rolled by k planes along z, three tracers, before the first step"""
    dom, rR, rB = (np.roll(a, k, axis=0) for a in PR.free_lattice())
    z, y, x = np.mgrid[0:16, 0:16, 0:16]
    s = solver(dom, dict(PR.FREE_PARAMS, variant=variant), tracers=TRACERS)
    s.set_macro(rR, rB)
    for t in range(3):
        conc = (0.2 + 0.1 * t + 0.1 * np.cos(2. * np.pi * ((z + 3 * t) / 16. + y / 16.)) * np.sin(2. * np.pi * x / 16.)) * (t < 2)
        s.set_concentration(t, np.roll(np.where(PR.free_lattice()[0] == 1, conc, 0.0), k, axis=0))
    return s


def free_run(k, variant):
    """... after ROLL_STEPS steps: (fields, bulk_cells)"""
    if (k, variant) not in _FREE:
        s = free_solver(k, variant)
        s.step(ROLL_STEPS)
        _FREE[(k, variant)] = (fields_of(s), s.bulk_cells)
        s.close()
    return _FREE[(k, variant)]


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("k", PR.ROLLS)
def test_a_rolled_lattice_gives_the_rolled_fields(k, variant):
    """no plane is special: mask and initial state rolled by k planes give every field of the unrolled run rolled by k, bit for bit,
    the tracers' populations among them.  The rolled lattice's blocks of 256 cells are the unrolled one's (tests/periodic_ref.py), and
    the ranges of the blocks next to z = 0 cross the seam in one run and not in the other: the same bulk count says they are handled
    alike"""
    base, bulk0 = free_run(0, variant)
    got, bulk = free_run(k, variant)
    same({f: np.roll(a, k, axis=0) for f, a in base.items()}, got, "rolled by %d, variant %d" % (k, variant))
    assert bulk == bulk0, (k, bulk, bulk0)
    assert (bulk0 > 0) if variant == 0 else (bulk0 == 0)
    assert np.max(np.abs(base["vz"])) > 1e-6 and np.max(np.abs(base["K"])) > 1e-4


def test_the_bulk_path_equals_the_full_path_across_the_seam():
    """variant 0 against variant 1, bit for bit over 30 steps, with the one-colour core of the red body on the seam: from step 3 on
    blocks are deep, and those around z = 0 are deep through ranges that cross the seam"""
    dom, rR, rB = PR.free_lattice()
    a, b = solver(dom, PR.FREE_PARAMS), solver(dom, dict(PR.FREE_PARAMS, variant=1))
    a.set_macro(rR, rB); b.set_macro(rR, rB)
    counts = []
    for k in range(1, 31):
        a.step(1); b.step(1)
        counts.append(a.bulk_cells)
        assert b.bulk_cells == 0
        if k in (1, 2, 3, 4, 10, 20, 30):
            same(fields_of(a), fields_of(b), "step %d" % k)
    print("bulk cells per step:", counts)
    assert all(c > 0 for c in counts[2:]), counts
    # the deep blocks lie on the seam: both planes next to it hold red alone, with exact zeros where a deep block writes them
    assert np.all(a.get("rhoB")[[15, 0]] == 0.0) and np.all(a.get("Gz")[[15, 0]] == 0.0)
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 4. uniformity
def test_a_state_uniform_along_z_stays_uniform():
    """two layers in a walled gap, uniform along z, driven along z: after 200 steps every plane equals plane 0 bit for bit (between
    open planes it does not: the planes next to them differ)"""
    dom, rR, rB = PR.gap_lattice(8, 4, 16)
    s = solver(dom, dict(PERIODIC, relax="MRT", tauB=0.7, sigma=0.05, theta=90.0))
    s.set_body_force(red=(0., 0., 2.0e-5), blue=(0., 0., 1.0e-5))
    s.set_macro(rR, rB)
    s.step(200)
    got = fields_of(s)
    for f, a in got.items():
        assert np.array_equal(a, np.broadcast_to(a[0], a.shape)), f
    assert np.min(got["vz"][dom == 1]) > 1e-5 and np.all(np.isfinite(got["fR"]))
    s.close()


# ------------------------------------------------------------------------------------------------ 5. slabs
SLAB_FIELDS = ("fR", "fB", "rhoR", "rhoB", "phi", "Gx", "Gy", "Gz", "Fx", "Fy", "Fz", "K", "vx", "vy", "vz", "rec_rhoR", "rec_rhoB", "rec_vz", "rec_phi")
SLAB_PARAMS = dict(PERIODIC, relax="MRT", theta=55.0, tauB=0.8, sigma=0.06)
SLAB_TRACER = dict(num_tracers=2, diffusion_x=(0.12, 0.2), beta_interface=(0.3, 0.0))
SLAB_STEPS = 20
SLAB_G = ((1.0e-5, -2.0e-5, 3.0e-5), (-2.5e-5, 1.5e-5, 6.0e-5))


def slab_lattice():
    """12 planes of 10 x 12: cuts at 4, 6 and 8; a grain across the seam, one across the cut at 4 and 6; a red blob across the seam and
    the cut at 4 (nothing here is special at z = 0 or z = 11)"""
    shape = (12, 10, 12)
    dom = np.ones(shape, dtype=np.uint8)
    dom[[11, 0], 2:4, 3:6] = 0
    dom[3:7, 6:8, 7:9] = 0
    z, y, x = np.mgrid[0:12, 0:10, 0:12]
    blob = (PR._wrapped(z, 1.5, 12) / 3.6) ** 2 + (PR._wrapped(y, 4.5, 10) / 3.2) ** 2 + (PR._wrapped(x, 5.5, 12) / 3.8) ** 2 < 1.
    fl = dom == 1
    return dom, np.where(fl & blob, PR._ripple(shape, 0.02, (1, 1, 1)), 0.0), np.where(fl & ~blob, 0.95 * PR._ripple(shape, 0.02, (2, 0, 1)), 0.0)


def _slab_conc(dom):
    z, y, x = np.mgrid[0:dom.shape[0], 0:dom.shape[1], 0:dom.shape[2]]
    return [np.where(dom == 1, 0.3 + 0.2 * np.cos(2. * np.pi * (z / 12. + t * x / 12.)), 0.0) for t in range(2)]


_UNDIVIDED = {}


def undivided(tracers):
    if tracers not in _UNDIVIDED:
        dom, rR, rB = slab_lattice()
        s = solver(dom, SLAB_PARAMS, **(dict(tracers=SLAB_TRACER) if tracers else {}))
        s.set_body_force(red=SLAB_G[0], blue=SLAB_G[1])
        s.set_macro(rR, rB)
        if tracers:
            for t, c in enumerate(_slab_conc(dom)):
                s.set_concentration(t, c)
        s.step(SLAB_STEPS)
        _UNDIVIDED[tracers] = fields_of(s, SLAB_FIELDS)
        s.close()
    return _UNDIVIDED[tracers]


@pytest.mark.parametrize("tracers", [False, True])
@pytest.mark.parametrize("nslabs", [2, 3])
def test_slabs_equal_the_undivided_periodic_lattice(nslabs, tracers):
    """the ring of slabs with the seam as one more face: bit-equal to the undivided lattice, with and without tracers"""
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster
    dom, rR, rB = slab_lattice()
    c = RK3DCSFCluster(dom, SLAB_PARAMS, nslabs=nslabs, diagnostics=True, **(dict(tracers=SLAB_TRACER) if tracers else {}))
    assert c.periodic_z and len(c.slabs) == nslabs
    c.set_body_force(red=SLAB_G[0], blue=SLAB_G[1])
    c.set_macro(rR, rB)
    if tracers:
        for t, conc in enumerate(_slab_conc(dom)):
            c.set_concentration(t, conc)
    c.step(SLAB_STEPS)
    c.sync()
    same(undivided(tracers), fields_of(c, SLAB_FIELDS), "%d slabs" % nslabs)
    c.close()


_SCRIPT = '''
import json, os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np, torch, torch.distributed as dist
from test_rk3d_csf_periodic_gpu import slab_lattice, _slab_conc, SLAB_PARAMS, SLAB_TRACER, SLAB_FIELDS, SLAB_STEPS, SLAB_G
from openlbmpm_amd.rk3dcsf import RK3DCSFDistributed
torch.cuda.set_device(0)
dist.init_process_group("gloo")
rank = dist.get_rank()
dom, rR, rB = slab_lattice()
d = RK3DCSFDistributed(dom, SLAB_PARAMS, device=0, diagnostics=True, transport="ipc", tracers=SLAB_TRACER)
assert d.periodic_z
d.set_body_force(red=SLAB_G[0], blue=SLAB_G[1])
d.set_macro(rR, rB)
for t, c in enumerate(_slab_conc(dom)):
    d.set_concentration(t, c)
d.step(SLAB_STEPS)
d.sync()
for f in SLAB_FIELDS + ("tracer 0", "tracer 1"):
    g = d.gather(d.get_tracer_pdf(int(f[-1])) if f.startswith("tracer") else d.get(f))
    if rank == 0:
        np.save(os.path.join(%(out)r, f.replace(" ", "_") + ".npy"), g)
dist.barrier()
if rank == 0:
    json.dump(dict(transport=d.transport), open(os.path.join(%(out)r, "transport.json"), "w"))
d.close()
dist.barrier()
dist.destroy_process_group()
'''


def test_two_processes_over_the_librarys_transport_equal_the_undivided_periodic_lattice(tmp_path):
    """two OS processes on this GPU, the face messages over the library's IPC transport (one run, under a time limit): the seam is
    the face between the second rank's high end and the first rank's low end"""
    script = tmp_path / "w.py"
    script.write_text(_SCRIPT % dict(root=ROOT, out=str(tmp_path)))
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(script)], timeout=600)
    assert json.load(open(tmp_path / "transport.json"))["transport"].startswith("ipc")
    want = undivided(True)
    for f, a in want.items():
        got = np.load(tmp_path / (f.replace(" ", "_") + ".npy"))
        assert np.array_equal(a, got), (f, float(np.max(np.abs(a - got))))


# ------------------------------------------------------------------------------------------------ 6. conservation
def test_the_colours_masses_are_conserved():
    """no inlet re-injects a colour, no outlet fixes a density: 200 steps without a force keep the sum of either colour's density to
    1e-12 (the exact model: bulk_epsilon 0)"""
    dom, rR, rB = PR.free_lattice()
    s = solver(dom, dict(PR.FREE_PARAMS, bulk_epsilon=0.0))
    s.set_macro(rR, rB)
    start = s.integrals()
    s.step(200)
    end = s.integrals()
    dR, dB = end.mass_R / start.mass_R - 1., end.mass_B / start.mass_B - 1.
    print("relative change of the masses after 200 steps: red %.3e, blue %.3e" % (dR, dB))
    assert start.mass_R == pytest.approx(float(rR.sum()), rel=1e-13) and end.nonfinite == 0
    assert abs(dR) < 1e-12 and abs(dB) < 1e-12
    assert np.max(np.abs(s.get("rec_vz"))) > 1e-6          # (something moved)
    s.close()


def test_a_force_along_z_adds_its_momentum_every_step():
    """without solids nothing takes momentum out: the sum of rho u_z over the lattice (integrals(): flux_R + flux_B) grows by
    (sum of rho) g_z per step, to 1e-10.  Two flat layers, so that the CSF force has no share in the balance"""
    dom = np.ones(PR.FREE_SHAPE, dtype=np.uint8)
    z = np.mgrid[0:16, 0:16, 0:16][0]
    blue = (z == 8) | (z == 9)
    g = 1.0e-5
    s = solver(dom, dict(PERIODIC, relax="MRT", tauB=0.8, sigma=0.05))
    s.set_body_force((0., 0., g))
    s.set_macro(np.where(blue, 0.0, 1.0), np.where(blue, 1.0, 0.0))
    t = s.integrals()
    last, mass = t.total("flux_R") + t.total("flux_B"), t.mass_R + t.mass_B
    assert last == pytest.approx(0.5 * mass * g, rel=1e-12)        # the state at rest, seen with half the force
    for k in range(1, 11):
        s.step(1)
        t = s.integrals()
        now = t.total("flux_R") + t.total("flux_B")
        assert abs((now - last) / (mass * g) - 1.) < 1e-10, (k, now - last, mass * g)
        assert abs((t.mass_R + t.mass_B) / mass - 1.) < 1e-13
        last = now
    s.close()


# ------------------------------------------------------------------------------------------------ 7. physics
@pytest.mark.parametrize("relax", ["MRT", "SRT"])
def test_two_layer_force_driven_flow(relax):
    """the analytic relative-permeability case (tests/periodic_ref.py): red and blue side by side in a gap, driven along the periodic
    axis by g_z alone; rec_vz against the two-viscosity Poiseuille profile"""
    T = PR.TWO_LAYER
    dom, rR, rB = PR.gap_lattice(T["nz"], T["ny"], T["gap"], T["wall"])
    assert dom.shape == (4, 2, 36)
    s = solver(dom, dict(T["params"], relax=relax))
    s.set_body_force((0., 0., T["g_z"]))
    s.set_macro(rR, rB)
    s.step(T["steps"])
    vz = s.get("rec_vz")
    eR, eB, eP = PR.two_layer_errors(vz[1, 0, T["wall"]:T["wall"] + T["gap"]])
    print("%s: flow rate of red %+.4f %%, of blue %+.4f %%, profile %.4f %% of the peak" % (relax, 100 * eR, 100 * eB, 100 * eP))
    assert np.array_equal(vz, np.broadcast_to(vz[0, 0], vz.shape))
    assert abs(eR) < PR.FLOW_RATE_BOUND and abs(eB) < PR.FLOW_RATE_BOUND and eP < PR.PROFILE_BOUND, (eR, eB, eP)
    i = s.integrals()
    assert i.saturation_R == 0.5 and i.darcy_uz_R > 0. and i.darcy_uz_B > 0.
    s.close()


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals(monkeypatch):
    from openlbmpm_amd import _lib, rk2d, rk3d, rk3dcsf
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver, _SlabGeometry
    dom = np.ones((8, 6, 6), np.uint8)
    for one in (dict(inlet="Periodic"), dict(outlet="Periodic")):
        with pytest.raises(ValueError, match="Periodic"):
            RK3DCSFSolver(dom, one)
    # ... and the library itself, whoever calls it: one of the pair alone is invalid, and the message names both fields
    for table, name in ((rk3dcsf._INLETS, "Neumann"), (rk3dcsf._OUTLETS, "Dirichlet")):
        with monkeypatch.context() as m:
            m.setitem(table, name, 2)
            with pytest.raises(_lib.LbmpmError) as e:
                RK3DCSFSolver(dom)
            assert e.value.status == _lib.ERR_INVALID and "inlet_type" in str(e.value) and "outlet_type" in str(e.value)
    # the perturbation model and the 2-D solvers keep their open ends: in Python, and in the library's range checks
    for make in (lambda p: rk3d.RK3DSlab(np.ones((8, 8, 8), np.uint8), 0, 8, p), lambda p: rk2d.RK2DSolver(np.ones((8, 8), np.uint8), p)):
        with pytest.raises(ValueError):
            make(PERIODIC)
    L = _lib.lib()
    import ctypes as C
    for cls, create, mask in ((_lib.RK3DConfig, "lbmpm_rk3d_create", np.ones((8, 8, 8), np.uint8)), (_lib.RK2DConfig, "lbmpm_rk2d_create", np.ones((8, 8), np.uint8))):
        for field in ("inlet_type", "outlet_type"):
            seen = {}

            def capture(cfg_ref, *rest, seen=seen):
                cfg = cfg_ref._obj
                setattr(cfg, field, 2)
                seen["rc"] = getattr(L, create)(C.byref(cfg), *rest)
                return seen["rc"]

            class Lib:
                def __getattr__(self, fn):
                    return capture if fn == create else getattr(L, fn)
            with monkeypatch.context() as m:
                m.setattr(_lib, "lib", lambda: Lib())
                with pytest.raises(_lib.LbmpmError):
                    (rk3d.RK3DSlab(mask, 0, 8) if cls is _lib.RK3DConfig else rk2d.RK2DSolver(mask))
            assert seen["rc"] == _lib.ERR_INVALID, (create, field)
    # the tracers' inlet and outlet rules name planes that are not special any more: undivided and slab
    per = RK3DCSFSolver(np.ones((8, 6, 6), np.uint8), PERIODIC)
    for rule in (dict(dirichlet_inlet=True), dict(free_outlet=True)):
        with pytest.raises(_lib.LbmpmError) as e:
            per.configure_tracers(num_tracers=1, **rule)
        assert e.value.status == _lib.ERR_INVALID and "periodic" in str(e.value)
        g = _SlabGeometry(12, 0, 6)
        with pytest.raises(_lib.LbmpmError) as e:
            RK3DCSFSolver(g.cut(np.ones((12, 6, 6), np.uint8)), PERIODIC, slab=g.slab, tracers=dict(num_tracers=1, **rule))
        assert e.value.status == _lib.ERR_INVALID and "periodic" in str(e.value)
    per.configure_tracers(num_tracers=1)
    per.close()
    # four planes are enough, three are not
    RK3DCSFSolver(np.ones((4, 3, 5), np.uint8), PERIODIC).close()
    with pytest.raises(_lib.LbmpmError) as e:
        RK3DCSFSolver(np.ones((3, 3, 5), np.uint8), PERIODIC)
    assert e.value.status == _lib.ERR_INVALID
    with pytest.raises(_lib.LbmpmError):            # between open planes eight stay the least
        RK3DCSFSolver(np.ones((4, 3, 5), np.uint8))
