"""Whole runs of the 3-D CSF solver on a periodic context (inlet = outlet = 'Periodic') on the GPU: what include/lbmpm.h says "stays as it
is" there -- restart, the contact-angle map, the drivers -- held to the identities the open-plane tests hold them to
(tests/test_rk3d_csf_body_force_gpu.py, test_rk3d_csf_wettability_gpu.py, test_tr3d_driver_gpu.py).  Every comparison is bit for bit.

4. set_pdf / set_tracer_pdf after ten steps continue like the uninterrupted run, the bulk path's blocks across the seam included;
5. a uniform contact-angle map is the scalar angle, a map with two angles on the grain across the seam rolls with the lattice, cuts into
slabs and is refused like anywhere else;  6. RKColorGradient3D with every periodic analysis on, in one process and under two ranks,
stopped and resumed, and Transport3DRK, against the solver class stepped by hand.
(1. - 3., the observers: tests/test_rk3d_csf_periodic_observers_gpu.py.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

import body_force_ref as R
import periodic_ref as PR
from test_rk3d_csf_gpu import TOL, solver
from test_rk3d_csf_periodic_cpu import _periodic_ini
from test_rk3d_csf_periodic_gpu import STATE, TRACERS, fields_of, free_solver, same
from test_rk3d_gpu import _free_port

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GR, GB = R.G_SETS["G1"]


# ------------------------------------------------------------------------------------------------ 4. restart
def stored(s):
    """what a restart hands over: the streamed populations with the force of the last step, and the tracers' populations"""
    return dict(fR=s.get("fR"), fB=s.get("fB"), force=tuple(s.get(c) for c in ("Fx", "Fy", "Fz")),
                g=[s.get_tracer_pdf(t) for t in range(s.num_tracers)])


def restore(s, st):
    s.set_pdf(st["fR"], st["fB"], force=st["force"])
    for t, g in enumerate(st["g"]):
        s.set_tracer_pdf(t, g)


_RING = {}


def ring_run(variant):
    """the ring box with the ganglion across the seam and one tracer: what ten steps leave to a restart, and the fields after twenty"""
    if variant not in _RING:
        dom = PR.ring_box()
        s = solver(dom, dict(PR.RING_PARAMS, variant=variant), tracers=PR.RING_TRACER)
        s.set_macro(*PR.ring_densities(PR.SEAM, dom))
        s.set_concentration(0, PR.ring_concentration(dom))
        s.step(10)
        st = stored(s)
        s.step(10)
        _RING[variant] = (st, fields_of(s))
        s.close()
    return _RING[variant]


@pytest.mark.parametrize("case", ["variant 0", "variant 1", "3 slabs"])
def test_a_restart_continues_bit_for_bit(case):
    """no plane of a periodic context copies another, so set_pdf has nothing to repair at the ends: a fresh context that takes the state
    of step 10 ends step 20 in the bits of the uninterrupted run -- undivided on both paths, and cut into the smallest ring of three"""
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster
    variant = 1 if case == "variant 1" else 0
    st, want = ring_run(variant)
    dom = PR.ring_box()
    par = dict(PR.RING_PARAMS, variant=variant)
    if case == "3 slabs":
        s = RK3DCSFCluster(dom, par, nslabs=3, diagnostics=True, tracers=PR.RING_TRACER)
        assert s.cuts == [0, 4, 8, 12]
    else:
        s = solver(dom, par, tracers=PR.RING_TRACER)
    assert s.periodic_z
    restore(s, st)
    s.step(10)
    same(want, fields_of(s), case)
    assert not np.array_equal(st["fR"], want["fR"]) and np.max(np.abs(want["K"])) > 1e-3       # (something happened after step 10)
    s.close()


def test_a_restart_rebuilds_the_deep_blocks_across_the_seam():
    """the 16^3 lattice of tests/periodic_ref.py with bulk_epsilon 1e-3: the red body's one-colour core lies on the seam, and the blocks
    around z = 0 are deep through ranges that cross it.  After the restart the same blocks are deep again"""
    a = free_solver(0, 0)
    a.step(10)
    st = stored(a)
    a.step(10)
    want, bulk = fields_of(a), a.bulk_cells
    a.close()
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    b = RK3DCSFSolver(PR.free_lattice()[0], PR.FREE_PARAMS, diagnostics=True, tracers=TRACERS)
    restore(b, st)
    b.step(10)
    assert b.bulk_cells == bulk > 0, (b.bulk_cells, bulk)
    same(want, fields_of(b), "bulk_epsilon 1e-3")
    assert np.all(want["rhoB"][[15, 0]] == 0.0)                  # (the deep blocks lie on the seam)
    b.close()


# ------------------------------------------------------------------------------------------------ 5. the contact-angle map
SET_UP = ("kind", "nsx", "nsy", "nsz", "theta")
ANGLE_STEPS = 10
ANGLE_PARAMS = PR.parity_params("MRT", 2, theta=97.0)


def two_angle_map(k=0):
    """the sealed parity lattice rolled by k planes, and the wall angles of a mineral map that gives the grain across the seam 30 degrees
    in plane 9 and 150 in plane 0 (everything else: the scalar 97)"""
    from openlbmpm_amd.geometry import wall_contact_angles
    dom, rR, rB = PR.parity_lattice()
    mineral = np.full(dom.shape, np.nan)
    assert not (dom[[9, 0], 1:3, 3:5] == 1).any()
    mineral[9, 1:3, 3:5], mineral[0, 1:3, 3:5] = 30.0, 150.0
    theta = wall_contact_angles(dom, mineral, 97.0)
    return tuple(np.roll(a, k, axis=0) for a in (dom, rR, rB, theta))


def angle_run(dom, rR, rB, theta, par=ANGLE_PARAMS, make=solver, **kw):
    s = make(dom, par, **kw)
    if theta is not None:
        s.set_contact_angles(theta)
    s.set_macro(rR, rB)
    s.step(ANGLE_STEPS)
    return s


_ANGLES = {}


def two_angle_fields(k):
    if k not in _ANGLES:
        dom, rR, rB, theta = two_angle_map(k)
        s = angle_run(dom, rR, rB, theta)
        _ANGLES[k] = fields_of(s, STATE + SET_UP)
        s.close()
    return _ANGLES[k]


def test_a_uniform_map_equals_the_scalar_angle_on_a_periodic_context():
    from openlbmpm_amd.geometry import wall_contact_angles
    dom, rR, rB = PR.parity_lattice()
    uniform = wall_contact_angles(dom, np.full(dom.shape, 50.0), 97.0)
    a50 = angle_run(dom, rR, rB, None, dict(ANGLE_PARAMS, theta=50.0))
    a97 = angle_run(dom, rR, rB, None)
    s = angle_run(dom, rR, rB, uniform)
    # the map covers the fluid cells next to solid as a periodic context sees them: z wraps, the grain's cells of plane 0 are next to plane 9
    assert np.array_equal(np.isfinite(uniform), s.get("kind") == 3) and np.isfinite(uniform[[9, 0]]).any()
    assert np.all(uniform[np.isfinite(uniform)] == 50.0)
    same(fields_of(a50, STATE), fields_of(s, STATE), "uniform map 50 against theta = 50")
    assert not np.array_equal(a50.get("Gx"), a97.get("Gx"))          # (the angle matters here)
    for x in (a50, a97, s):
        x.close()


@pytest.mark.parametrize("k", PR.ROLLS)
def test_a_map_rolled_with_the_lattice_gives_the_rolled_fields(k):
    """two angles on the grain across the seam: rolled by k planes the grain lies inside the lattice, and every field -- the wetting
    solids' set-up among them -- is the unrolled one rolled by k, bit for bit"""
    base, got = two_angle_fields(0), two_angle_fields(k)
    same({f: np.roll(a, k, axis=0) for f, a in base.items()}, got, "rolled by %d" % k)
    theta, wall = base["theta"], base["kind"] == 3
    assert {30.0, 150.0} <= set(theta[[8, 9, 0, 1], 0:4, 3:7].reshape(-1).tolist())     # both angles arrived, each on its side of the seam
    assert theta[[8, 9]][wall[[8, 9]]].max() == 97.0 and theta[[0, 1]][wall[[0, 1]]].min() == 97.0


def test_the_two_angles_act_and_cut_into_slabs():
    """against the scalar angle the phase field next to the grain moves by far more than rounding; two slabs of five planes (the cut
    and the seam both next to the grain's neighbours) give the undivided bits"""
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster
    dom, rR, rB, theta = two_angle_map()
    plain = angle_run(dom, rR, rB, None)
    grain = np.zeros(dom.shape, dtype=bool)
    grain[[8, 9, 0, 1], 0:4, 2:7] = True
    d = np.abs(plain.get("phi") - two_angle_fields(0)["phi"])[grain & (dom == 1)]
    print("two angles against the scalar one: phi next to the grain moves by up to %.3e" % d.max())
    assert d.max() > 1000 * TOL
    plain.close()
    c = angle_run(dom, rR, rB, theta, make=RK3DCSFCluster, nslabs=2, diagnostics=True)
    assert c.periodic_z and c.cuts == [0, 5, 10]
    c.sync()
    want = two_angle_fields(0)
    same({f: want[f] for f in STATE + ("theta",)}, fields_of(c, STATE + ("theta",)), "2 slabs")
    c.close()


def test_an_ill_shaped_map_is_refused_and_leaves_the_run_as_it_was():
    """tests/test_rk3d_csf_wettability_gpu.py::test_refusals_leave_the_run_as_it_was on a periodic context, the bad angle at a cell of
    plane 0 whose solid neighbour lies in plane 9"""
    from openlbmpm_amd._lib import ERR_INVALID, LbmpmError
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster
    dom, rR, rB, theta = two_angle_map()
    z, y, x = 1, 1, 4                                     # over the grain's cell (0, 1, 4); (8, 1, 4) lies under its cell (9, 1, 4)
    assert dom[z, y, x] == 1 and dom[0, y, x] == 0 and theta[z, y, x] == 150.0 and theta[8, y, x] == 30.0
    never, s = angle_run(dom, rR, rB, theta), angle_run(dom, rR, rB, theta)
    for bad in (np.nan, 180.5, -1.0, np.inf):
        for cell in ((z, y, x), (8, y, x)):
            t = theta.copy(); t[cell] = bad
            with pytest.raises(LbmpmError) as e:
                s.set_contact_angles(t)
            assert e.value.status == ERR_INVALID and "(%d, %d, %d)" % cell in str(e.value), str(e.value)
            assert np.array_equal(s.get("theta"), never.get("theta"), equal_nan=True)
    for shape in (theta[:, :, 1:], theta[1:], theta.reshape(-1)):
        with pytest.raises(ValueError):
            s.set_contact_angles(shape)
    assert s.steps_done == ANGLE_STEPS
    s.step(5); never.step(5)
    same(fields_of(never, STATE + SET_UP), fields_of(s, STATE + SET_UP), "after refused calls")
    # slabs: checked on every slab before any is changed
    c = angle_run(dom, rR, rB, theta, make=RK3DCSFCluster, nslabs=2, diagnostics=True)
    t = theta.copy(); t[z, y, x] = np.nan
    with pytest.raises(LbmpmError) as e:
        c.set_contact_angles(t)
    assert e.value.status == ERR_INVALID
    with pytest.raises(ValueError):
        c.set_contact_angles(theta[1:])
    c.step(5)
    same(fields_of(never, STATE + ("theta",)), fields_of(c, STATE + ("theta",)), "slabs after refused calls")
    for q in (s, never, c):
        q.close()


# ------------------------------------------------------------------------------------------------ 6. the drivers
NX, NY, NZ, STEPS, EVERY, RECORD = 16, 8, 18, 20, 5, 10
VISITS = [0, 5, 10, 15, 20]
DRIVER_KW = dict(record_every=RECORD, integrals_every=EVERY, clusters_every=EVERY, clusters_props=True, clusters_connectivity=18, morphology_every=EVERY,
                 morphology_phi_cut=0.3, steady_every=EVERY, body_force=dict(red=GR, blue=GB))


def write_ini(tmp_path):
    return _periodic_ini(tmp_path, nx=NX, ny=NY, nz=NZ, steps=STEPS, relax="MRT")[0]


def by_hand(d, tracer_ini=None):
    """the solver class with the driver's set-up, stepped by hand to every visit: the datasets a run must hold"""
    from openlbmpm_amd import config
    from openlbmpm_amd.RKColorGradientD3Q19 import _CSFSlab, duct
    from openlbmpm_amd.geometry import initial_densities_rk3d
    p = config.read_rk3d(d)
    assert p["periodic_z"]
    dom = duct(NX, NY, NZ)
    s = _CSFSlab(dom, p, 0).solver
    assert s.periodic_z
    s.set_body_force(red=GR, blue=GB)
    s.set_macro(*initial_densities_rk3d(dom, min(10, NZ // 4), p["rho0R"], p["rho0B"]))
    out = {}
    for k in VISITS:
        s.step(k - s.steps_done)
        if k == 0:
            s.mark_change()
        else:
            out["/Steady/PlanesAtStep%d" % k] = s.change().planes
        out["/Integrals/PlanesAtStep%d" % k] = s.integrals().planes
        c = s.clusters(connectivity=18, props=True)
        out["/Clusters/TableAtStep%d" % k], out["/Clusters/PropsAtStep%d" % k] = c.table, c.props
        out["/Morphology/PlanesAtStep%d" % k] = s.morphology(0.3).planes
        if k % RECORD == 0:
            r = k // RECORD
            out["/FluidMacro/FluidDensityRin%d" % r], out["/FluidMacro/FluidDensityBin%d" % r] = s.get("rec_rhoR"), s.get("rec_rhoB")
            for ax in "XYZ":
                out["/FluidVelocity/FluidVelocity%sAt%d" % (ax, r)] = s.get("rec_v" + ax.lower())
    s.close()
    return out


def check_file(res, want, what):
    assert np.array_equal(res["/BoundaryCondition/PeriodicZ"], [1]), what
    assert np.array_equal(res["/BodyForce/Acceleration"], np.array([GR, GB])), what
    for group in ("Integrals", "Clusters", "Morphology"):
        assert res["/%s/Steps" % group].tolist() == VISITS, (what, group)
    assert res["/Steady/Steps"].tolist() == VISITS[1:], what
    for key, a in want.items():
        assert res[key].dtype == a.dtype and np.array_equal(res[key], a), (what, key)


@pytest.fixture(scope="module")
def driven(tmp_path_factory):
    """one run of RKColorGradient3D with every periodic analysis on and a checkpoint at step 10, and what the solver class gives by hand"""
    from openlbmpm_amd.RKColorGradientD3Q19 import RKColorGradient3D
    from openlbmpm_amd.results import load_results
    tmp = tmp_path_factory.mktemp("periodic_driver")
    d = write_ini(tmp)
    sim = RKColorGradient3D(d, output_dir=str(tmp / "out"), checkpoint_every=10, **DRIVER_KW)
    res = load_results(sim.runRKColorGradient3D())
    return dict(dir=d, tmp=tmp, sim=sim, res=res, want=by_hand(d))


def test_the_driver_records_what_the_solver_class_gives_by_hand(driven):
    sim, res, want = driven["sim"], driven["res"], driven["want"]
    assert sim.periodic_z and sim.records == 3 and sim.steady_step is None
    check_file(res, want, "one process")
    # the state is not trivial: a flow along z, an interface, a cluster table of more than one row, cells in the band
    assert np.max(np.abs(res["/FluidVelocity/FluidVelocityZAt2"])) > 1e-6 and res["/Clusters/TableAtStep20"].shape[0] >= 2
    from openlbmpm_amd.morphology import COLUMNS
    assert res["/Morphology/PlanesAtStep20"][:, COLUMNS.index("cells_N")].sum() > 0
    # z does not wrap in the tables: red fills the planes 0 .. 13 and blue 14 .. 17, so red touches the first plane and blue the last
    t = res["/Clusters/TableAtStep0"]
    assert t[t[:, 1] == 1][:, 3:].tolist() == [[0, 13]] and t[t[:, 1] == 2][:, 3:].tolist() == [[14, 17]]


def test_a_run_resumed_from_a_checkpoint_ends_in_the_same_bits(driven):
    from openlbmpm_amd.RKColorGradientD3Q19 import RKColorGradient3D
    from openlbmpm_amd.results import load_results
    sim, res = driven["sim"], driven["res"]
    again = RKColorGradient3D(driven["dir"], output_dir=str(driven["tmp"] / "resumed"), restart_from=sim.checkpoint_path, **DRIVER_KW)
    got = load_results(again.runRKColorGradient3D())
    assert again.records == sim.records and np.array_equal(got["/BoundaryCondition/PeriodicZ"], [1])
    late = [k for k in res if k.endswith(("AtStep15", "AtStep20", "in2", "At2"))]
    assert len(late) == 2 * 5 + 5
    for key in late:
        assert np.array_equal(got[key], res[key]), key
    assert np.array_equal(again.solver.get_state()[0], sim.solver.get_state()[0])


_DRIVER_WORKER = '''
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import torch, torch.distributed as dist
from openlbmpm_amd.RKColorGradientD3Q19 import RKColorGradient3D
from test_rk3d_csf_periodic_runs_gpu import DRIVER_KW
dist.init_process_group("gloo")
torch.cuda.set_device(0)
sim = RKColorGradient3D(%(ini)r, output_dir=%(out)r, device=0, **DRIVER_KW)
sim.runRKColorGradient3D()
assert sim.periodic_z and (sim.integrals is None) == (dist.get_rank() != 0)
dist.destroy_process_group()
'''


def test_two_ranks_write_the_single_runs_file(driven, tmp_path):
    """the driver under two ranks on this GPU (fresh child processes, under a time limit): rank 0's file holds the datasets of the
    single run, the analyses' tables -- gathered, joined as a chain -- among them"""
    from openlbmpm_amd.results import load_results
    script = tmp_path / "w.py"
    script.write_text(_DRIVER_WORKER % dict(root=ROOT, ini=driven["dir"], out=str(tmp_path / "out2")))
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(script)], env=dict(os.environ), timeout=300)
    files = os.listdir(tmp_path / "out2")
    assert len(files) == 1 and files[0].startswith("SimulationResultsRK3D."), files
    got = load_results(str(tmp_path / "out2" / files[0]))
    check_file(got, driven["want"], "two ranks")
    assert set(got) == set(driven["res"])
    for key, a in driven["res"].items():
        assert np.array_equal(got[key], a), key


def test_the_tracers_driver_on_a_periodic_lattice(tmp_path):
    """Transport3DRK with InletType = 'Periodic', OutletType = 'VonNeumann': a record holds the flow at the start of a step and the
    concentrations after it (tests/test_tr3d_driver_gpu.py), here of tracers that leave through plane 17 and come back through plane 0"""
    from ini_fixtures import TRANSPORT_INI
    from test_tr3d_driver_gpu import Z_KEYS
    from openlbmpm_amd import config
    from openlbmpm_amd.RKColorGradientD3Q19 import duct
    from openlbmpm_amd.Transport3DRK import Transport3DRK, _CSFTracerSlab
    from openlbmpm_amd.geometry import initial_densities_rk3d
    from openlbmpm_amd.results import load_results
    d = write_ini(tmp_path)
    text = (TRANSPORT_INI + Z_KEYS).replace("InletType = 'Dirichlet'", "InletType = 'Periodic'").replace("OutletType = 'Freeflow'", "OutletType = 'VonNeumann'")
    (tmp_path / "transportsetup.ini").write_text(text)
    sim = Transport3DRK(d, output_dir=str(tmp_path / "out"), record_every=RECORD, body_force=dict(red=GR, blue=GB))
    flow, conc = sim.runTransport3DMPMCRK()
    res = dict(load_results(flow)); res.update(load_results(conc))
    assert sim.periodic_z and sim.records == 3 and np.array_equal(res["/BoundaryCondition/PeriodicZ"], [1])
    # by hand
    p = config.read_rk3d(d)
    dom = duct(NX, NY, NZ)
    s = _CSFTracerSlab(dom, p, config.read_transport3d(d, periodic_z=True), 0).solver
    assert s.periodic_z and s.num_tracers == 2
    s.set_body_force(red=GR, blue=GB)
    s.set_macro(*initial_densities_rk3d(dom, min(10, NZ // 4), p["rho0R"], p["rho0B"]))
    zz = np.arange(NZ)[:, None, None]
    first = np.where((dom == 1) & (zz <= NZ - 10), 1.0, 0.0)
    s.set_concentration(0, first)
    s.set_concentration(1, np.zeros(dom.shape))
    for k in range(3):
        s.step(k * RECORD - s.steps_done)
        assert np.array_equal(res["/FluidMacro/FluidDensityRin%d" % k], s.get("rec_rhoR")), k
        assert np.array_equal(res["/FluidVelocity/FluidVelocityZAt%d" % k], s.get("rec_vz")), k
        if k * RECORD < STEPS:
            s.step(1)
        for i in range(2):
            assert np.array_equal(res["/TransportMacro/TracerConcType%din%d" % (i, k)], s.get_concentration(i)), (k, i)
    last = res["/TransportMacro/TracerConcType0in2"]
    assert last[NZ - 9:].max() > 1e-6 and not np.array_equal(last, first)       # (the tracer spread beyond where it was set)
    s.close()
