"""The observers of the 3-D CSF solver on a periodic context (inlet = outlet = 'Periodic') on the GPU: what include/lbmpm.h promises for
them -- they read the pulled state with no plane rule, and clusters, cluster properties and morphology do NOT wrap z -- against the CPU
restatements the open-plane tests use (tests/test_integrals_gpu.py, change_ref.py, test_clusters_cpu.py, cluster_props_ref.py,
test_morphology_cpu.py, test_tracer_integrals_gpu.py), from the fields get("rec_*") hands out (tests/test_rk3d_csf_periodic_gpu.py ties those
to the oracle).

1. every observer against its restatement on the ring box of tests/periodic_ref.py, at step 0 and after seven steps;  2. a lattice rolled
along z gives the rolled per-plane tables, bit for bit;  3. slabs and two processes give the undivided lattice's tables, the ganglion
across the seam still two clusters.

Integer tables: array_equal.  Float sums: 2 (n - 1) 2^-53 sum|term| per plane (derived at the top of tests/test_integrals_gpu.py).  Rolls,
slabs and ranks: array_equal.  What the references must show for these tests to see anything -- tests/test_rk3d_csf_periodic_cpu.py holds
it for the prescribed states -- is asserted on the reference side after the steps: the labelling that does not wrap has more clusters than
the one of the classes rolled by six planes, with a red row that starts at plane 0 and one that ends at plane 11; morphology's row 11
changes with plane 0 above it; the end rows of the integrals and the rows 0 and 3 of the change table lie further apart than the bound;
at phi_cut 0.3 the band holds cells.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import body_force_ref as R
import change_ref
import cluster_props_ref as ref
import periodic_ref as PR
import test_integrals_gpu as TI
import test_tracer_integrals_gpu as TT
from test_clusters_cpu import classify, cpu_label
from test_clusters_gpu import SHARP
from test_morphology_cpu import C, cpu_morphology
from test_morphology_gpu import classes as morphology_classes, compare as morphology_compare
from test_rk3d_csf_gpu import solver
from test_rk3d_csf_periodic_cpu import UPWARDS, rows_differ, seam_rows
from test_rk3d_csf_periodic_gpu import ROLL_STEPS, free_solver
from test_rk3d_gpu import _free_port

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = SHARP + (PR.SEAM,)
MARK_AT, STEPS = 3, 7
UP = [C[n] for n in UPWARDS]
FLAT = [c for c in range(28) if c not in UP]
PROP_FIELDS = (("rhoR", "rhoR"), ("rhoB", "rhoB"), ("ux", "vx"), ("uy", "vy"), ("uz", "vz"))


def record_fields(s):
    return {k: s.get("rec_" + k) for k in TI.FIELDS}


def ring_solver(name, relax="MRT", cls=None, **kw):
    """a solver on the ring box with the pattern `name` prescribed and one tracer, before the first step"""
    dom = PR.ring_box()
    s = (cls or solver)(dom, dict(PR.RING_PARAMS, relax=relax), tracers=PR.RING_TRACER, **kw)
    s.set_macro(*PR.ring_densities(name, dom))
    s.set_concentration(0, PR.ring_concentration(dom))
    return dom, s


# ------------------------------------------------------------------------------------------------ 1. against the restatements
def props_equal(got, want, table, what):
    """the property table, every column, equal; what differs is reported apart for the rows that touch plane 0 or plane 11"""
    assert got.dtype == np.int64 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(np.any(got != want, axis=1))[0]
    ends = [int(i) for i in bad if table[i, 3] == 0 or table[i, 4] == 11]
    rest = [int(i) for i in bad if int(i) not in ends]
    diff = np.abs(got - want)
    print("%s: %d clusters, worst difference of MASS / MOM_* %d quanta" % (what, want.shape[0], diff[:, ref.MASS:ref.CLIPPED].max() if diff.size else 0))
    assert bad.size == 0, "%s: rows that touch plane 0 or plane 11 differ: %s (columns %s); other rows differ: %s (columns %s)" % (
        what, ends, sorted(set(np.nonzero(diff[ends])[1].tolist())), rest, sorted(set(np.nonzero(diff[rest])[1].tolist())))


def check_integrals(s, dom, f, what, every_sum):
    g = s.integrals()
    assert g.planes.shape == (12, 12) and (g.nx, g.ny) == (70, 33)
    T = TI.compare(g.planes, dom, f, what)
    assert T[5, 0] == 5 and T[:, 11].sum() == 0
    A = TI.restate(dom, f)[1]
    for a, b in ((0, 1), (10, 11)):        # (the reference alone: an open plane redirected to its neighbour would repeat a row)
        far = rows_differ(T, A, a, b, range(2, 10))
        assert T[a, 0] != T[b, 0] and (set(far) == set(range(2, 10)) if every_sum else far), (what, a, b, far)
    return g


def check_clusters(s, dom, f, cut, what, seam):
    cls = classify(f["phi"], dom, cut)
    fields = {k: f[n] for k, n in PROP_FIELDS}
    for conn in (6, 18):
        got = s.clusters(phi_cut=cut, connectivity=conn, labels=True, props=True)
        lab, tab = cpu_label(cls, conn)
        assert got.table.dtype == np.int64 and got.table.shape == tab.shape, (what, conn, got.table.shape, tab.shape)
        assert np.array_equal(got.table, tab), (what, conn)
        assert got.labels.dtype == np.uint32 and np.array_equal(got.labels, lab), (what, conn)
        props_equal(got.props, ref.props(ref.class_field(dom, cls), lab, below=None, above=None, **fields), tab, "%s conn %d" % (what, conn))
        if seam:                           # (the reference alone: a labelling that wrapped z would hand out another table)
            low, high = seam_rows(tab)
            assert low.shape[0] and low[:, 2].max() >= 50 and high.shape[0] and high[:, 2].max() >= 50, (what, conn, low, high)
            assert tab.shape[0] > cpu_label(np.roll(cls, 6, axis=0), conn)[1].shape[0], (what, conn)
    return cls


def check_morphology(s, dom, f, cut, what):
    cls = morphology_classes(f["phi"], f["rhoR"], f["rhoB"], dom, cut)
    rho = f["rhoR"] + f["rhoB"]
    g = s.morphology(phi_cut=cut)
    assert g.planes.shape == (12, 28)
    T = morphology_compare(g.planes, cls, rho, what)
    joined = cpu_morphology(cls, np.where((cls == 1) | (cls == 2), rho, 0.0), above=cls[0])
    assert np.array_equal(joined[:11], T[:11]) and np.array_equal(joined[11, FLAT], T[11, FLAT])
    assert not np.array_equal(joined[11, UP], T[11, UP]), what       # (the reference alone: a count that wrapped z would show in row 11)
    return T


def check_all(s, dom, what, cuts, seam, every_sum):
    f = record_fields(s)
    check_integrals(s, dom, f, what, every_sum)
    for cut in cuts:
        check_clusters(s, dom, f, cut, "%s cut %g" % (what, cut), seam)
        T = check_morphology(s, dom, f, cut, "%s cut %g" % (what, cut))
    t = TT.compare_with_fields(s, dom, 1, what)
    assert t.nonfinite == 0 and t.planes[5, 0, TT.CELLS] == 5
    return f, T


@pytest.mark.parametrize("relax", ["MRT", "SRT"])
@pytest.mark.parametrize("name", PATTERNS)
def test_every_observer_against_its_restatement(name, relax):
    """the sharp patterns of tests/test_clusters_gpu.py and the ganglion across the seam, prescribed, checked at step 0, stepped seven
    times (the change table's snapshot taken after three) and checked again at phi_cut 0 and 0.3"""
    dom, s = ring_solver(name, relax)
    what = "%s %s" % (name, relax)
    seam = name == PR.SEAM
    f, _ = check_all(s, dom, what + " step 0", (0.0,), seam, False)
    # the pattern arrived in every plane: none belongs to a boundary condition
    rR, rB = PR.ring_densities(name, dom)
    assert np.array_equal(classify(f["phi"], dom), np.where(dom == 1, np.where(rR > rB, 1, 2), 0))
    s.step(MARK_AT)
    s.mark_change()
    old = record_fields(s)
    s.step(STEPS - MARK_AT)
    f, T = check_all(s, dom, what + " step 7", (0.0, 0.3), seam, seam)
    if name == "one_phase":                # red throughout as prescribed: no interface to cut a band from
        assert T[:, C["cells_B"]].sum() == 0 and T[:, C["cells_N"]].sum() == 0
    else:
        assert T[:, C["cells_N"]].sum() > 0, "no cell in the band: the case shows nothing"
    g = s.change()
    assert g.steps == STEPS - MARK_AT and g.planes.shape == (12, 11)
    T = change_ref.compare(g.planes, dom, f, old, what + " change")
    A = change_ref.restate(dom, f, old)[1]
    far = rows_differ(T, A, 0, 3, change_ref.SUMS)
    assert T[0, 0] != T[3, 0] and (set(far) == set(change_ref.SUMS) if seam else name == "one_phase" or far), (what, far)
    s.close()


@pytest.mark.parametrize("relax", ["MRT", "SRT"])
def test_a_body_force_along_z_is_in_what_the_observers_read(relax):
    """with g_z set, integrals() and the momentum columns of the cluster properties still match the restatement from rec_v*, which
    carry the force's half"""
    dom, s = ring_solver(PR.SEAM, relax)
    s.set_body_force(red=R.G_SETS["G1"][0], blue=R.G_SETS["G1"][1])
    s.step(STEPS)
    f = record_fields(s)
    assert not np.array_equal(f["vz"], s.get("vz")) and R.G_SETS["G1"][0][2] != 0.0       # (the half is there to be missed)
    check_integrals(s, dom, f, "body force " + relax, True)
    check_clusters(s, dom, f, 0.0, "body force " + relax, True)
    assert np.any(s.clusters(props=True).props[:, ref.MOM_Z] != 0)
    s.close()


# ------------------------------------------------------------------------------------------------ 2. roll equivariance
_ROLLED = {}


def rolled_tables(k):
    """the per-plane tables of the 16^3 lattice of tests/periodic_ref.py rolled by k planes, after ROLL_STEPS steps (marked after MARK_AT)"""
    if k not in _ROLLED:
        s = free_solver(k, 0)
        s.step(MARK_AT)
        s.mark_change()
        s.step(ROLL_STEPS - MARK_AT)
        out = dict(integrals=s.integrals().planes, change=s.change().planes, tracers=s.tracer_integrals().planes, phi=s.get("rec_phi"))
        for cut in (0.0, 0.3):
            out["morphology %g" % cut] = s.morphology(cut).planes
        for conn in (6, 18):
            out["clusters %d" % conn] = s.clusters(connectivity=conn).table
        _ROLLED[k] = out
        s.close()
    return _ROLLED[k]


@pytest.mark.parametrize("k", PR.ROLLS)
def test_a_rolled_lattice_gives_the_rolled_tables(k):
    """no plane is special to an observer either.  The reducer's order within a plane depends on (nx, ny) and the plane's cells alone, so
    the rows of integrals(), change() and tracer_integrals() are the unrolled rows rolled by k, bit for bit; so are morphology's columns
    that do not reach upwards, and those that do (tests/test_morphology_gpu.py::test_the_plane_above lists them) in every plane but the
    one that is last in either lattice.  clusters(): the table of the rolled classes"""
    base, got = rolled_tables(0), rolled_tables(k)
    roll = lambda a: np.roll(a, k, axis=0)
    for name in ("integrals", "change", "tracers"):
        assert np.array_equal(roll(base[name]), got[name]), (k, name)
    assert base["tracers"].shape == (16, 3, 9) and not np.array_equal(base["integrals"][0], base["integrals"][1])
    inner = [z for z in range(16) if z not in (15, k - 1)]
    for cut in (0.0, 0.3):
        a, b = roll(base["morphology %g" % cut]), got["morphology %g" % cut]
        assert np.array_equal(a[:, FLAT], b[:, FLAT]), (k, cut)
        assert np.array_equal(a[inner][:, UP], b[inner][:, UP]), (k, cut)
        # the last plane of either lattice anchors nothing upwards, and the same plane of the other lattice does
        assert not b[15, UP].any() and not a[k - 1, UP].any() and a[15, UP].any() and b[k - 1, UP].any(), (k, cut)
    assert base["morphology 0.3"][:, C["cells_N"]].sum() > 0
    cls = roll(classify(base["phi"], PR.free_lattice()[0]))
    for conn in (6, 18):
        t0, t = base["clusters %d" % conn], got["clusters %d" % conn]
        assert np.array_equal(t, cpu_label(cls, conn)[1]), (k, conn)
        for c in (1, 2):
            assert t0[t0[:, 1] == c, 2].sum() == t[t[:, 1] == c, 2].sum() > 0, (k, conn, c)
        low, high = seam_rows(t0, 16)
        assert low.shape[0] == 1 and high.shape[0] == 1            # the red body across the seam of the unrolled lattice: two clusters
        if k == 8:                                                 # ... and one where the roll has carried the blue film to the seam:
            assert int((t[:, 1] == 1).sum()) == 1 and t.shape[0] != t0.shape[0]        # a labelling that wrapped z would count alike under every roll


# ------------------------------------------------------------------------------------------------ 3. slabs and ranks
def tables(s):
    """every observer's table after the run of run_ring (collective on RK3DCSFDistributed: rank 0 holds the whole lattice's, the others {})"""
    out = {"integrals": s.integrals(), "change": s.change(), "tracer integrals": s.tracer_integrals()}
    for conn in (6, 18):
        out["clusters %d" % conn] = s.clusters(connectivity=conn, labels=True, props=True)
    for cut in (0.0, 0.3):
        out["morphology %g" % cut] = s.morphology(cut)
    if out["integrals"] is None:
        return {}
    flat = {k: v.planes for k, v in out.items() if not k.startswith("clusters")}
    for conn in (6, 18):
        c = out["clusters %d" % conn]
        flat.update({"clusters %d" % conn: c.table, "labels %d" % conn: c.labels, "cluster props %d" % conn: c.props})
    return flat


def run_ring(s):
    s.step(MARK_AT)
    s.mark_change()
    s.step(STEPS - MARK_AT)
    return s


_UNDIVIDED = {}


def undivided():
    if not _UNDIVIDED:
        dom, s = ring_solver(PR.SEAM)
        run_ring(s)
        cls = classify(s.get("rec_phi"), dom)
        _UNDIVIDED.update(tables=tables(s), counts={conn: cpu_label(cls, conn)[1].shape[0] for conn in (6, 18)})
        s.close()
    return _UNDIVIDED


def equal_to_the_undivided(got, what):
    u = undivided()
    assert set(got) == set(u["tables"])
    for k, v in u["tables"].items():
        assert got[k].dtype == v.dtype and np.array_equal(got[k], v, equal_nan=True), (what, k)
    for conn in (6, 18):
        # the ring's extra face between the last and the first slab joins nothing: the ganglion's halves stay two rows
        t = got["clusters %d" % conn]
        low, high = seam_rows(t)
        assert t.shape[0] == u["counts"][conn] and low.shape[0] and high.shape[0] and int((t[:, 1] == 1).sum()) >= 2, (what, conn, t.shape[0], u["counts"][conn])
        assert not np.any((t[:, 1] == 1) & (t[:, 3] == 0) & (t[:, 4] == 11)), (what, conn)
        assert got["cluster props %d" % conn].shape == (t.shape[0], 14)


@pytest.mark.parametrize("nslabs", [2, 3])
def test_slabs_give_the_undivided_tables(nslabs):
    """the population message travels round a ring of slabs; the observers' joins treat the stack as a chain (clusters.merged,
    stacked_props, morphology.stacked).  Three slabs of four own planes are the smallest ring of three"""
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster
    dom, c = ring_solver(PR.SEAM, cls=RK3DCSFCluster, nslabs=nslabs)
    assert c.periodic_z and c.cuts == ([0, 6, 12] if nslabs == 2 else [0, 4, 8, 12])
    run_ring(c)
    c.sync()
    equal_to_the_undivided(tables(c), "%d slabs" % nslabs)
    c.close()


_SCRIPT = '''
import json, os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np, torch, torch.distributed as dist
import test_rk3d_csf_periodic_observers_gpu as T
from openlbmpm_amd.rk3dcsf import RK3DCSFDistributed
torch.cuda.set_device(0)
dist.init_process_group("gloo")
dom, d = T.ring_solver(T.PR.SEAM, cls=RK3DCSFDistributed, device=0, transport="ipc")
assert d.periodic_z
T.run_ring(d)
d.sync()
got = T.tables(d)
assert bool(got) == (dist.get_rank() == 0)
if got:
    np.savez(os.path.join(%(out)r, "tables.npz"), **got)
    json.dump(dict(transport=d.transport), open(os.path.join(%(out)r, "transport.json"), "w"))
dist.barrier()
d.close()
dist.barrier()
dist.destroy_process_group()
'''


def test_two_processes_over_the_librarys_transport_give_the_undivided_tables(tmp_path):
    """two OS processes on this GPU, the face messages over the library's IPC transport (one run, under a time limit): the gathered joins
    (clusters.gather_merged, faces_from_neighbours, morphology.face_from_above) take the ranks as a chain, too"""
    script = tmp_path / "w.py"
    script.write_text(_SCRIPT % dict(root=ROOT, out=str(tmp_path)))
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(script)], timeout=300)
    assert json.load(open(tmp_path / "transport.json"))["transport"].startswith("ipc")
    got = np.load(str(tmp_path / "tables.npz"))
    equal_to_the_undivided({k: got[k] for k in got.files}, "two processes")
