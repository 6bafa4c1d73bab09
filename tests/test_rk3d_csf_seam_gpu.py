"""wrap_z=True of clusters() and morphology() on the 3-D CSF classes, on the GPU: the seam of a lattice that is periodic in z, closed.

The device runs the launches it runs by default; what is new is on the host (clusters.close_seam, the ring joins of analysis.py) and in
which planes the contexts hand each other.  Held to the CPU closure of tests/test_seam_cpu.py -- cpu_label and cluster_props_ref on the
classes of get("rec_phi"), closed by close_seam, which that file holds against a cell-by-cell search -- on the ring box of
tests/periodic_ref.py: 1. the solver against the closure;  2. rolled lattices;  3. slabs;  4. two processes;  5. the driver;  6. refusals.

Integers, and tables of one device against another's: array_equal.  The morphology's two density sums against numpy keep the bound of
tests/test_morphology_gpu.compare (2 (n - 1) 2^-53 sum|term|: numpy adds a plane's cells in another order); they must be, bit for bit, the
sums of the default call, which wrap_z does not touch.

Four slabs: a slab owns at least four planes (include/lbmpm.h), so the twelve planes of the ring box make two or three slabs and no more.
The four-slab case runs on the ring box with four planes put in at its middle (ring16), against the undivided solver on that lattice.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_props_ref as ref
import periodic_ref as PR
from openlbmpm_amd.clusters import CLASS, ZMAX, close_seam, relabel
from test_clusters_cpu import classify, cpu_label
from test_morphology_cpu import C, cpu_morphology
from test_morphology_gpu import classes as morphology_classes, compare as morphology_compare
from test_rk3d_csf_gpu import solver
from test_rk3d_csf_periodic_cpu import UPWARDS, _periodic_ini
from test_rk3d_csf_periodic_observers_gpu import PROP_FIELDS, props_equal, record_fields, ring_solver
from test_rk3d_gpu import _free_port
from test_seam_cpu import multiset

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 7
CUTS, CONNS = (0.0, 0.3), (6, 18)
RHO = [C["rho_R"], C["rho_B"]]
UP = [C[n] for n in UPWARDS]


def wrapped(s):
    """every wrapped table of a solver (collective on RK3DCSFDistributed: rank 0 holds the whole lattice's, the others {})"""
    out = {}
    for conn in CONNS:
        c = s.clusters(connectivity=conn, labels=True, props=True, wrap_z=True)
        if c is not None:
            assert c.wrap_z
            out.update({"clusters %d" % conn: c.table, "winding %d" % conn: c.winding, "labels %d" % conn: c.labels, "props %d" % conn: c.props})
    for cut in CUTS:
        m = s.morphology(cut, wrap_z=True)
        if m is not None:
            out["morphology %g" % cut] = m.planes
    return out


def same_tables(got, want, what):
    assert set(got) == set(want), what
    for k, v in want.items():
        assert got[k].dtype == v.dtype and got[k].shape == v.shape and np.array_equal(got[k], v), (what, k)


# ------------------------------------------------------------------------------------------------ 1. against the CPU closure
def check_closure(s, dom, what, across):
    f = record_fields(s)
    fields = {k: f[n] for k, n in PROP_FIELDS}
    rho = f["rhoR"] + f["rhoB"]
    seen = dict(winds=0, across=0, joined=0)
    for cut in CUTS:
        cls = classify(f["phi"], dom, cut)
        cf = ref.class_field(dom, cls)
        for conn in CONNS:
            w = "%s cut %g conn %d" % (what, cut, conn)
            got = s.clusters(phi_cut=cut, connectivity=conn, labels=True, props=True, wrap_z=True)
            lab, tab = cpu_label(cls, conn)
            parts = ref.props(cf, lab, below=cf[-1], above=cf[0], **fields)
            t, wind, mapping, p = close_seam(tab, np.stack([lab[0], lab[-1]]), np.stack([cls[0], cls[-1]]), 70, 33, 12, conn, parts)
            assert got.wrap_z and got.table.dtype == np.int64 and got.table.shape == t.shape and np.array_equal(got.table, t), w
            assert got.winding.dtype == np.int64 and np.array_equal(got.winding, wind), w
            assert got.labels.dtype == np.uint32 and np.array_equal(got.labels, relabel(lab, mapping)), w
            props_equal(got.props, p, t, w)
            seen["winds"] += int(np.count_nonzero(wind))
            seen["across"] += int(np.count_nonzero((wind == 0) & (t[:, ZMAX] >= 12)))
            seen["joined"] += tab.shape[0] - t.shape[0]
            # the default call is what it was: the open table, no winding
            plain = s.clusters(phi_cut=cut, connectivity=conn, props=True)
            assert not plain.wrap_z and plain.winding is None and np.array_equal(plain.table, tab), w
        mc = morphology_classes(f["phi"], f["rhoR"], f["rhoB"], dom, cut)
        g = s.morphology(cut, wrap_z=True)
        assert g.planes.shape == (12, 28)
        T = morphology_compare(g.planes, mc, rho, "%s cut %g" % (what, cut), above=mc[0])
        plain = s.morphology(cut).planes
        assert np.array_equal(g.planes[:, RHO], plain[:, RHO]) and np.array_equal(g.planes[:11], plain[:11])
        assert not np.array_equal(T[11, UP], plain[11, UP]), what          # (row 11 gained what reaches up into plane 0)
    # (the reference alone: clusters that wind, open rows that the seam joins, and -- where asked for -- a ganglion across the seam)
    assert seen["winds"] > 0 and seen["joined"] > 0 and (seen["across"] > 0 or not across), (what, seen)


@pytest.mark.parametrize("name", [PR.SEAM, "serpentine", "random"])
def test_the_solver_against_the_cpu_closure(name):
    """the pattern prescribed, checked at step 0, stepped seven times (MRT) and checked again: table, winding, labels, property table and
    the morphology across the seam, at both cuts and both connectivities"""
    dom, s = ring_solver(name, "MRT")
    check_closure(s, dom, name + " step 0", True)
    s.step(STEPS)
    check_closure(s, dom, name + " step 7", name == PR.SEAM)
    s.close()


# ------------------------------------------------------------------------------------------------ 2. rolls
_STATE = {}


def stepped_state():
    """what seven steps from the ganglion across the seam leave: populations and force (the ring box, no tracers)"""
    if not _STATE:
        dom = PR.ring_box()
        s = solver(dom, PR.RING_PARAMS)
        s.set_macro(*PR.ring_densities(PR.SEAM, dom))
        s.step(STEPS)
        _STATE.update(dom=dom, fR=s.get("fR"), fB=s.get("fB"), force=tuple(s.get(c) for c in ("Fx", "Fy", "Fz")))
        s.close()
    return _STATE


_ROLLED = {}


def rolled_tables(k):
    """the wrapped tables of a solver that holds the lattice and the state of stepped_state, both rolled by k planes"""
    if k not in _ROLLED:
        st = stepped_state()
        roll = lambda a: np.ascontiguousarray(np.roll(a, k, axis=0))
        s = solver(roll(st["dom"]), PR.RING_PARAMS)
        s.set_pdf(roll(st["fR"]), roll(st["fB"]), force=tuple(roll(c) for c in st["force"]))
        _ROLLED[k] = wrapped(s)
        s.close()
    return _ROLLED[k]


@pytest.mark.parametrize("k", PR.ROLLS)
def test_a_rolled_lattice_gives_the_rolled_wrapped_tables(k):
    """with the seam closed no plane is an end: the morphology table of the rolled lattice is the rolled table in all 28 columns of all
    12 rows, bit for bit -- the columns that reach upwards in the last plane included --, and the clusters are the same clusters: the same
    multiset of (class, cells, extent, winding, the property columns that name no plane, the centre moved by k)"""
    base, got = rolled_tables(0), rolled_tables(k)
    for cut in CUTS:
        a, b = base["morphology %g" % cut], got["morphology %g" % cut]
        assert np.array_equal(np.roll(a, k, axis=0), b), (k, cut)
        assert a[11, UP].any() and b[11, UP].any()
    assert base["morphology 0.3"][:, C["cells_N"]].sum() > 0
    for conn in CONNS:
        t, w, p = (base["%s %d" % (n, conn)] for n in ("clusters", "winding", "props"))
        rt, rw, rp = (got["%s %d" % (n, conn)] for n in ("clusters", "winding", "props"))
        assert multiset(rt, rw, rp) == multiset(t, w, p, k), (k, conn)
        assert np.count_nonzero(w) and np.any((w == 0) & (t[:, ZMAX] >= 12)), conn          # a cluster that winds, the ganglion across the seam


# ------------------------------------------------------------------------------------------------ 3. slabs
_UNDIVIDED = {}


def run_ring(s):
    s.step(STEPS)
    return s


def undivided():
    if not _UNDIVIDED:
        dom, s = ring_solver(PR.SEAM)
        _UNDIVIDED.update(wrapped(run_ring(s)))
        s.close()
    return _UNDIVIDED


@pytest.mark.parametrize("nslabs", [2, 3])
def test_slabs_give_the_undivided_wrapped_tables(nslabs):
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster
    dom, c = ring_solver(PR.SEAM, cls=RK3DCSFCluster, nslabs=nslabs)
    assert c.periodic_z and len(c.slabs) == nslabs
    run_ring(c)
    c.sync()
    same_tables(wrapped(c), undivided(), "%d slabs" % nslabs)
    with pytest.raises(ValueError):
        c.slabs[0].clusters(wrap_z=True)                   # one slab of a cut lattice: the seam is closed where the slabs are joined
    with pytest.raises(ValueError):
        c.slabs[-1].morphology(wrap_z=True)
    c.close()


def ring16():
    """the ring box with four planes (copies of the planes 6, 7, 6, 7) put in between plane 7 and plane 8, and the ganglion across its seam"""
    planes = list(range(8)) + [6, 7, 6, 7] + list(range(8, 12))
    dom = PR.ring_box()
    rR, rB = PR.ring_densities(PR.SEAM, dom)
    return tuple(np.ascontiguousarray(a[planes]) for a in (dom, rR, rB))


def test_four_slabs_give_the_undivided_wrapped_tables():
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster
    dom, rR, rB = ring16()
    tables = []
    for make in (lambda: solver(dom, PR.RING_PARAMS), lambda: RK3DCSFCluster(dom, PR.RING_PARAMS, nslabs=4)):
        s = make()
        s.set_macro(rR, rB)
        run_ring(s)
        s.sync()
        tables.append(wrapped(s))
        s.close()
    same_tables(tables[1], tables[0], "4 slabs")
    t, w = tables[0]["clusters 6"], tables[0]["winding 6"]
    red = t[:, CLASS] == 1
    assert np.count_nonzero(w) and np.any(red & (w == 0) & (t[:, ZMAX] >= 16))


# ------------------------------------------------------------------------------------------------ 4. two processes
_SCRIPT = '''
import json, os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np, torch, torch.distributed as dist
import test_rk3d_csf_seam_gpu as T
from openlbmpm_amd.rk3dcsf import RK3DCSFDistributed
torch.cuda.set_device(0)
dist.init_process_group("gloo")
dom, d = T.ring_solver(T.PR.SEAM, cls=RK3DCSFDistributed, device=0, transport="ipc")
assert d.periodic_z
T.run_ring(d)
d.sync()
got = T.wrapped(d)
assert bool(got) == (dist.get_rank() == 0)
if got:
    np.savez(os.path.join(%(out)r, "tables.npz"), **got)
    json.dump(dict(transport=d.transport), open(os.path.join(%(out)r, "transport.json"), "w"))
dist.barrier()
d.close()
dist.barrier()
dist.destroy_process_group()
'''


def test_two_processes_give_the_undivided_wrapped_tables(tmp_path):
    """two OS processes on this GPU (fresh child processes, one run under a time limit), the face messages over the library's IPC
    transport: the gathered joins take the ranks as a ring -- the one all_gather of either analysis hands rank 0 the last rank's plane
    and the last rank rank 0's -- and rank 0 closes the seam"""
    script = tmp_path / "w.py"
    script.write_text(_SCRIPT % dict(root=ROOT, out=str(tmp_path)))
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(script)], timeout=300)
    assert json.load(open(tmp_path / "transport.json"))["transport"].startswith("ipc")
    got = np.load(str(tmp_path / "tables.npz"))
    same_tables({k: got[k] for k in got.files}, undivided(), "two processes")


# ------------------------------------------------------------------------------------------------ 5. the driver
EVERY, RUN = 4, 8
VISITS = [0, 4, 8]


def _driver(tmp_path, out, **kw):
    """the driver on the ring box.  Its own initial state is layered along z -- red below, blue in the top planes -- and has nothing across
    the seam, so the run starts from the ganglion across the seam instead: the one method that makes the initial densities is replaced"""
    from openlbmpm_amd.RKColorGradientD3Q19 import RKColorGradient3D

    class FromTheGanglion(RKColorGradient3D):
        def initializeDomainCondition(self, z0=0, nzl=None):
            nzl = self.zDomain if nzl is None else nzl
            rR, rB = PR.ring_densities(PR.SEAM, self.isDomain)
            self.fluidsRhoR, self.fluidsRhoB = rR[z0:z0 + nzl], rB[z0:z0 + nzl]
    d = _periodic_ini(tmp_path, nx=70, ny=33, nz=12, steps=RUN, relax="MRT")[0]
    return d, FromTheGanglion(d, output_dir=str(tmp_path / out), domain=PR.ring_box(), record_every=RUN, clusters_every=EVERY, clusters_props=True,
                              morphology_every=EVERY, morphology_phi_cut=0.3, **kw)


def test_the_driver_writes_the_wrapped_tables(tmp_path, caplog):
    import logging
    from openlbmpm_amd import config
    from openlbmpm_amd.RKColorGradientD3Q19 import _CSFSlab
    from openlbmpm_amd.results import load_results
    d, sim = _driver(tmp_path, "wrapped", analyses_wrap_z=True)
    with caplog.at_level(logging.INFO):
        res = load_results(sim.runRKColorGradient3D())
    assert sim.periodic_z and sim.clusters.wrap_z and "winding_R=" in caplog.text
    assert np.array_equal(res["/Clusters/WrapZ"], [1]) and np.array_equal(res["/Morphology/WrapZ"], [1])
    assert res["/Clusters/Steps"].tolist() == VISITS and res["/Morphology/Steps"].tolist() == VISITS
    # by hand: the solver class with the driver's set-up, the direct wrapped calls at the visits
    p = config.read_rk3d(d)
    dom = PR.ring_box()
    s = _CSFSlab(dom, p, 0).solver
    s.set_macro(*PR.ring_densities(PR.SEAM, dom))
    for k in VISITS:
        s.step(k - s.steps_done)
        c = s.clusters(props=True, wrap_z=True)
        for name, a in (("Table", c.table), ("Winding", c.winding), ("Props", c.props)):
            got = res["/Clusters/%sAtStep%d" % (name, k)]
            assert got.dtype == np.int64 and np.array_equal(got, a), (name, k)
        assert np.array_equal(res["/Morphology/PlanesAtStep%d" % k], s.morphology(0.3, wrap_z=True).planes), k
    plain = s.clusters(props=True)
    # (the state shows something: a cluster that winds, a ganglion across the seam, fewer rows than the open table, another morphology)
    assert np.count_nonzero(c.winding) and np.any((c.winding == 0) & (c.table[:, ZMAX] >= 12)) and c.table.shape[0] < plain.table.shape[0]
    assert not np.array_equal(s.morphology(0.3).planes, s.morphology(0.3, wrap_z=True).planes)
    s.close()
    # the same run without the flag: no Winding, no WrapZ, the open tables
    _, sim = _driver(tmp_path, "plain")
    res = load_results(sim.runRKColorGradient3D())
    assert not [k for k in res if "Winding" in k or "WrapZ" in k], sorted(res)
    assert np.array_equal(res["/Clusters/TableAtStep%d" % RUN], plain.table) and np.array_equal(res["/Clusters/PropsAtStep%d" % RUN], plain.props)
    assert sim.clusters.winding is None and not sim.clusters.wrap_z


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(tmp_path):
    from openlbmpm_amd import config
    from openlbmpm_amd.RKColorGradientD3Q19 import RKColorGradient3D
    from openlbmpm_amd.Transport3DRK import Transport3DRK
    from openlbmpm_amd.rk3d import RK3DSlab
    from test_clusters_gpu import CSF_PAR, PERT_PAR, _box
    dom, rR, rB = _box()
    s = solver(dom, CSF_PAR)                               # open planes
    s.set_macro(rR, rB)
    p = RK3DSlab(dom, 0, dom.shape[0], PERT_PAR)           # the perturbation model has no periodic z
    p.set_density(rR, rB)
    for q in (s, p):
        before = q.device_bytes
        for call in (lambda: q.clusters(wrap_z=True), lambda: q.clusters(props=True, labels=True, wrap_z=True), lambda: q.morphology(wrap_z=True),
                     lambda: q.morphology(0.3, wrap_z=True)):
            with pytest.raises(ValueError, match="periodic"):
                call()
        assert q.device_bytes == before                    # before any launch: the analyses' memory comes with their first call
        q.close()
    dom, r = ring_solver(PR.SEAM)
    c = r.clusters(wrap_z=True)
    with pytest.raises(ValueError):
        c.connected_cells("R")
    with pytest.raises(ValueError):
        c.trapped_cells("R", z_lo=1)
    with pytest.raises(ValueError):
        c.centre_z()                                       # (no property table was asked for: as ever)
    assert c.percolates("B") and not c.percolates("R") and c.trapped_cells("R") == 360 and c.summary()["winding_B"] == 1
    r.close()
    # the drivers: the flag belongs to a run that is periodic in z
    d2 = tmp_path / "open"; d2.mkdir()
    d = _periodic_ini(d2, "'Neumann'", "'Dirichlet'", nx=8, ny=6, nz=12, steps=4)[0]
    for make in (RKColorGradient3D, Transport3DRK):
        with pytest.raises(config.ConfigError, match="periodic"):
            make(d, analyses_wrap_z=True)
    assert RKColorGradient3D(d).analyses_wrap_z is False
    from openlbmpm_amd.__main__ import parser
    assert parser().parse_args(["rk3d", d, "--wrap-z"]).wrap_z is True and parser().parse_args(["rk3d", d]).wrap_z is False
