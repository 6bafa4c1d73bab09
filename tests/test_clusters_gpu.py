"""Phase clusters labelled on the device (lbmpm_rk3d_clusters / lbmpm_rk3dcsf_clusters, csrc/rk3d_clusters.h) against the CPU labeller of
tests/test_clusters_cpu.py: the table, the whole label field, connectivity 6 and 18.  The phases are prescribed through set_density /
set_macro at step 0, so the pattern and not the dynamics is under test; the classes the CPU labeller starts from are taken from the
phase field the solver hands out (get("phi") / get("rec_phi")) by the definition of include/lbmpm.h.  Integers throughout: every
comparison is array_equal.

The lattice is the 70 x 33 x 12 porous box of tests/test_integrals_gpu.py: rows of two segments (64 + 6 cells), 33 rows = eight tiles of
four and one ragged, 12 planes = three tiles, 27720 cells = 27 whole chunks and a ragged one, a plane with five fluid cells.
"""
import os

import numpy as np
import pytest

from test_clusters_cpu import classify, cpu_label
from test_drivers_gpu import _free_port
from test_rk3d_csf_gpu import _slab_case

pytestmark = pytest.mark.gpu

CSF_PAR = dict(relax="MRT", theta=55.0, tauB=0.8, velocityZR=0.0, velocityZB=-3.0e-3, sigma=0.06)
PERT_PAR = dict(relax="MRT", tauB=0.8)
NONE = 0xFFFFFFFF
SHARP = ("random", "checkerboard", "serpentine", "wrap_stripes", "segment_boundary", "one_phase")


def _box(nx=70, ny=33, nz=12, seed=17):
    """the porous box of tests/test_integrals_gpu.py::_box, rebuilt: open planes at either end, seeded blocks in between, row y = 7 all
    solid and plane 5 with five fluid cells"""
    rng = np.random.default_rng(seed)
    dom = np.ones((nz, ny, nx), dtype=np.uint8)
    for _ in range(60):
        z, y, x = rng.integers(4, nz - 3), rng.integers(0, ny - 3), rng.integers(0, nx - 4)
        dom[z:z + 2, y:y + 3, x:x + 4] = 0
    dom[4:nz - 2, 7, :] = 0
    dom[5] = 0
    dom[5, 20, 30:33] = 1
    dom[5, 3, 68:70] = 1
    assert int((dom[5] == 1).sum()) == 5 and not (dom[6, 7] == 1).any()
    from openlbmpm_amd.geometry import initial_densities_rk3d
    rR, rB = initial_densities_rk3d(dom, 3)
    return dom, rR, rB


def red_cells(name, shape):
    """where a sharp pattern is R (everywhere else B)"""
    nz, ny, nx = shape
    z, y, x = np.mgrid[0:nz, 0:ny, 0:nx]
    if name == "random":                  # many tiny clusters
        return np.random.default_rng(11).random(shape) < 0.5
    if name == "checkerboard":            # every cell its own cluster under 6
        return (x + y + z) % 2 == 0
    if name == "serpentine":              # one cell wide: rows 1, 3, .. of the planes 0, 2, .., turning at alternate ends, one cell up per plane
        inside = (x >= 1) & (x <= nx - 2)
        row = (z % 2 == 0) & (y % 2 == 1) & inside
        turn = (z % 2 == 0) & (y % 2 == 0) & (y >= 2) & (y <= ny - 3) & (x == np.where((y // 2) % 2 == 1, nx - 2, 1))
        up = (z % 2 == 1) & (y == np.where((z // 2) % 2 == 0, ny - 2 - (ny % 2 == 0), 1)) & (x == 1)
        return row | turn | up
    if name == "wrap_stripes":            # a stripe that closes only through the x wrap, one only through the y wrap
        return (((x < 3) | (x >= nx - 3)) & (y >= 10) & (y < 14)) | (((y < 2) | (y >= ny - 2)) & (x >= 20) & (x < 40))
    if name == "segment_boundary":        # two halves that meet only across x = 63 | 64, in one row
        return ((x >= 50) & (x <= 63) & (y >= 16) & (y <= 18) & (z >= 1) & (z <= 2)) | ((x >= 64) & (x <= 68) & (y == 18) & (z >= 2) & (z <= 3))
    if name == "one_phase":               # one cluster per pore body
        return np.ones(shape, dtype=bool)
    raise KeyError(name)


def densities(name, dom):
    fl = dom == 1
    if name == "graded":                  # phi runs from -1 to 1 along x
        phi = np.broadcast_to(np.linspace(-1.0, 1.0, dom.shape[2]), dom.shape)
        return np.where(fl, 0.5 * (1.0 + phi), 0.0), np.where(fl, 0.5 * (1.0 - phi), 0.0)
    red = red_cells(name, dom.shape)
    return np.where(fl & red, 1.0, 0.0), np.where(fl & ~red, 1.0, 0.0)


_REF = {}


def reference(cls, conn):
    """cpu_label, computed once per class field and connectivity"""
    key = (cls.shape, cls.tobytes(), conn)
    if key not in _REF:
        _REF[key] = cpu_label(cls, conn)
    return _REF[key]


def same(got, cls, conn, what):
    lab, tab = reference(cls, conn)
    assert got.table.dtype == np.int64 and got.table.shape == tab.shape, (what, got.table.shape, tab.shape)
    assert np.array_equal(got.table, tab), (what, got.table[:8], tab[:8])
    assert got.labels.dtype == np.uint32 and np.array_equal(got.labels, lab), what
    return tab


class _Pert:
    """the perturbation model on a lattice: prescribe, read phi back, label"""
    def __init__(self, dom):
        from openlbmpm_amd.rk3d import RK3DSlab
        self.dom, self.s = dom, RK3DSlab(dom, 0, dom.shape[0], PERT_PAR)

    def prescribe(self, rR, rB):
        self.s.set_density(rR, rB)
        self.s.phase_field(diagnostics=True)

    def step(self, n):
        self.s.step_single(n)
        self.s.phase_field(diagnostics=True)

    def phi(self):
        return self.s.get("phi")


class _Csf:
    def __init__(self, dom):
        from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
        self.dom, self.s = dom, RK3DCSFSolver(dom, CSF_PAR)

    def prescribe(self, rR, rB):
        self.s.set_macro(rR, rB)

    def step(self, n):
        self.s.step(n)

    def phi(self):
        return self.s.get("rec_phi")


@pytest.fixture(scope="module")
def box():
    return _box()


@pytest.fixture(scope="module", params=["perturbation", "csf"])
def model(request, box):
    m = (_Pert if request.param == "perturbation" else _Csf)(box[0])
    yield m
    m.s.close()


# ---------------------------------------------------------------------------------------------- 1. prescribed patterns
@pytest.mark.parametrize("name", SHARP)
def test_prescribed_pattern(model, name):
    dom = model.dom
    model.prescribe(*densities(name, dom))
    cls = classify(model.phi(), dom)
    want = np.where(dom == 1, np.where(red_cells(name, dom.shape), 1, 2), 0)
    assert np.array_equal(cls[2:-2], want[2:-2])          # the pattern arrived (the planes next to the open ends belong to the boundary conditions)
    for conn in (6, 18):
        got = model.s.clusters(connectivity=conn, labels=True)
        tab = same(got, cls, conn, (name, conn))
        print("%s conn %d: %d clusters, largest %d" % (name, conn, tab.shape[0], tab[:, 2].max()))
        if name == "checkerboard" and conn == 6:           # away from the ends and from the y wrap (33 rows: 32 | 0 are one colour) every cell is its own cluster
            own = np.arange(dom.size, dtype=np.uint32).reshape(dom.shape)
            inner = np.zeros(dom.shape, dtype=bool)
            inner[3:-3, 1:-1] = dom[3:-3, 1:-1] == 1
            assert np.array_equal(got.labels[inner], own[inner])
        if name == "segment_boundary":                     # the halves meet across x = 63 | 64
            assert got.labels[2, 18, 63] == got.labels[2, 18, 64] == got.labels[3, 18, 68] == got.labels[2, 16, 50] != NONE


def test_the_serpentine_is_one_long_cluster():
    shape = (12, 33, 70)
    red = red_cells("serpentine", shape)
    t = cpu_label(np.where(red, 1, 0).astype(np.uint8), 6)[1]
    assert t.shape[0] == 1 and t[0, 2] == int(red.sum()) and t[0, 3] == 0 and t[0, 4] == 11
    # one cell wide: every cell has at most two neighbours in it
    n = sum(np.roll(red, s, axis=a) for a in (1, 2) for s in (1, -1)).astype(int)
    n[1:] += red[:-1]; n[:-1] += red[1:]
    assert n[red].max() == 2


def test_graded_density_with_a_band(model):
    dom = model.dom
    model.prescribe(*densities("graded", dom))
    phi = model.phi()
    cls = classify(phi, dom, 0.5)
    assert (cls[dom == 1] == 0).sum() > 1000 and (cls == 1).any() and (cls == 2).any()      # the band is in no cluster
    for conn in (6, 18):
        got = model.s.clusters(phi_cut=0.5, connectivity=conn, labels=True)
        same(got, cls, conn, ("graded", conn))
        assert np.all(got.labels[cls == 0] == NONE)
    same(model.s.clusters(labels=True), classify(phi, dom), 6, "graded, no band")


def test_a_bad_cell_is_in_no_cluster(model):
    """R in the three fluid cells of row 20 of plane 5 alone; a NaN in the density of the middle one splits the cluster in two"""
    dom = model.dom
    fl = dom == 1
    red = np.zeros(dom.shape, dtype=bool)
    red[5, 20, 30:33] = True
    rR, rB = np.where(fl & red, 1.0, 0.0), np.where(fl & ~red, 1.0, 0.0)
    model.prescribe(rR, rB)
    clean = model.s.clusters(connectivity=18, labels=True)
    same(clean, classify(model.phi(), dom), 18, "before the nan")
    in5 = lambda c: c.rows("R")[c.rows("R")[:, 3] == 5]           # (the planes at the open ends belong to the boundary conditions)
    assert np.array_equal(in5(clean), [[(5 * 33 + 20) * 70 + 30, 1, 3, 5, 5]])
    bad = rR.copy()
    bad[5, 20, 31] = np.nan
    model.prescribe(bad, rB)
    cls = classify(model.phi(), dom)
    assert cls[5, 20, 31] == 0 and int((cls != 0).sum()) == int(fl.sum()) - 1
    for conn in (6, 18):
        got = model.s.clusters(connectivity=conn, labels=True)
        same(got, cls, conn, ("nan", conn))
        assert got.labels[5, 20, 31] == NONE
        assert np.array_equal(in5(got), [[(5 * 33 + 20) * 70 + 30, 1, 1, 5, 5], [(5 * 33 + 20) * 70 + 32, 1, 1, 5, 5]])


# ---------------------------------------------------------------------------------------------- 2. after real steps
def test_after_real_steps(model, box):
    dom, rR, rB = box
    model.prescribe(rR, rB)
    model.step(5)
    cls = classify(model.phi(), dom)
    for conn in (6, 18):
        got = model.s.clusters(connectivity=conn, labels=True)
        tab = same(got, cls, conn, ("steps", conn))
        again = model.s.clusters(connectivity=conn, labels=True)
        assert np.array_equal(again.table, got.table) and np.array_equal(again.labels, got.labels)      # the same call twice: the same bits
        assert tab[tab[:, 1] == 1, 2].sum() == model.s.integrals().total("cells_R")
        assert got.count("R") + got.count("B") == tab.shape[0] and got.nz == 12


# ---------------------------------------------------------------------------------------------- 3. cut independence
@pytest.mark.parametrize("state", ["random", "steps"])
def test_perturbation_slabs_give_the_undivided_clusters(box, state):
    from openlbmpm_amd.rk3d import RK3DCluster
    dom, rR, rB = box
    if state == "random":
        rR, rB = densities("random", dom)
    m = _Pert(dom)
    m.prescribe(rR, rB)
    if state == "steps":
        m.step(4)
    ref = {conn: m.s.clusters(connectivity=conn, labels=True) for conn in (6, 18)}
    cls = classify(m.phi(), dom)
    m.s.close()
    for conn in (6, 18):
        same(ref[conn], cls, conn, (state, conn))
    for k in (2, 3):
        c = RK3DCluster(dom, k, PERT_PAR)
        c.set_density(rR, rB)
        if state == "steps":
            c.step(4)
        for conn in (6, 18):
            got = c.clusters(connectivity=conn, labels=True)             # (stale: observes first)
            assert np.array_equal(got.table, ref[conn].table), (k, conn)
            assert np.array_equal(got.labels, ref[conn].labels), (k, conn)
        c.close()


@pytest.mark.parametrize("state", ["random", "steps"])
def test_csf_slabs_give_the_undivided_clusters(state):
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster
    dom, rR, rB = _slab_case()
    if state == "random":
        rR, rB = densities("random", dom)
    m = _Csf(dom)
    m.prescribe(rR, rB)
    if state == "steps":
        m.step(4)
    ref = {conn: m.s.clusters(connectivity=conn, labels=True) for conn in (6, 18)}
    cls = classify(m.phi(), dom)
    m.s.close()
    for conn in (6, 18):
        same(ref[conn], cls, conn, (state, conn))
    for kw in (dict(nslabs=4), dict(cuts=[0, 9, 23, 44])):
        c = RK3DCSFCluster(dom, CSF_PAR, **kw)
        c.set_macro(rR, rB)
        if state == "steps":
            c.step(4)
        for conn in (6, 18):
            got = c.clusters(connectivity=conn, labels=True)
            assert np.array_equal(got.table, ref[conn].table), (kw, conn)
            assert np.array_equal(got.labels, ref[conn].labels), (kw, conn)
        c.close()


_WORKER = '''
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
import torch, torch.distributed as dist
import test_clusters_gpu as T
dist.init_process_group("gloo")
torch.cuda.set_device(0)
rank = dist.get_rank()
out = {}
if %(tension)r == "CSF":
    from openlbmpm_amd.rk3dcsf import RK3DCSFDistributed
    dom, _, _ = T._slab_case()
    d = RK3DCSFDistributed(dom, T.CSF_PAR, device=0)
    d.set_macro(*T.densities("random", dom))
else:
    from openlbmpm_amd.rk3d import RK3DDistributed
    dom, _, _ = T._box()
    d = RK3DDistributed(dom, T.PERT_PAR, device=0, transport="callback")
    d.set_density(*T.densities("random", dom))
d.step(3)
d.sync()
for conn in (6, 18):
    c = d.clusters(connectivity=conn, labels=True)
    assert (c is None) == (rank != 0)
    if c is not None:
        out["table%%d" %% conn], out["labels%%d" %% conn] = c.table, c.labels
    assert (d.clusters(connectivity=conn) is None) == (rank != 0)
if rank == 0:
    np.savez(%(npz)r, **out)
if hasattr(d, "close"):
    d.close()
from openlbmpm_amd.RKColorGradientD3Q19 import RKColorGradient3D
sim = RKColorGradient3D(%(ini)r, output_dir=%(out2)r, record_every=6, device=0, clusters_every=5, clusters_connectivity=18)
sim.calibrate_partition = False
sim.runRKColorGradient3D()
assert (sim.clusters is None) == (rank != 0)
dist.destroy_process_group()
'''


@pytest.mark.parametrize("tension", ["perturbation", "CSF"])
def test_two_ranks_give_the_undivided_clusters_and_the_drivers_group(tmp_path, tension, caplog):
    """two ranks on this GPU over gloo: the distributed class against one context (a random pattern, three steps), then the driver's
    /Clusters group against the single run's"""
    import logging
    import subprocess
    import sys
    from ini_fixtures import write_rk3d, write_rk3d_csf
    from openlbmpm_amd.RKColorGradientD3Q19 import RKColorGradient3D
    from openlbmpm_amd.clusters import COLUMNS
    from openlbmpm_amd.integrals import column_names
    from openlbmpm_amd.results import load_results
    tests = os.path.dirname(os.path.abspath(__file__))
    (write_rk3d_csf if tension == "CSF" else write_rk3d)(str(tmp_path), steps=12)
    script = tmp_path / "w.py"
    script.write_text(_WORKER % dict(root=os.path.dirname(tests), tests=tests, tension=tension, npz=str(tmp_path / "two.npz"),
                                     ini=str(tmp_path), out2=str(tmp_path / "out2")))
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(script)], env=dict(os.environ), timeout=600)
    two = np.load(str(tmp_path / "two.npz"))
    if tension == "CSF":
        dom = _slab_case()[0]
        m = _Csf(dom)
    else:
        dom = _box()[0]
        m = _Pert(dom)
    m.prescribe(*densities("random", dom))
    m.step(3)
    cls = classify(m.phi(), dom)
    for conn in (6, 18):
        one = m.s.clusters(connectivity=conn, labels=True)
        same(one, cls, conn, (tension, conn))
        assert np.array_equal(two["table%d" % conn], one.table) and two["table%d" % conn].dtype == np.int64, conn
        assert np.array_equal(two["labels%d" % conn], one.labels) and two["labels%d" % conn].dtype == np.uint32, conn
    m.s.close()
    # the driver
    with caplog.at_level(logging.INFO, logger="openlbmpm_amd"):
        single = RKColorGradient3D(str(tmp_path), output_dir=str(tmp_path / "out1"), record_every=6, clusters_every=5, clusters_connectivity=18)
        ref = load_results(single.runRKColorGradient3D())
    steps = [0, 5, 10, 12]
    assert single.cluster_steps == steps and np.array_equal(ref["/Clusters/Steps"], np.array(steps, dtype=np.int64))
    assert column_names(ref["/Clusters/Columns"]) == COLUMNS
    assert sorted(k for k in ref if k.startswith("/Clusters/")) == sorted(["/Clusters/Steps", "/Clusters/Columns"] + ["/Clusters/TableAtStep%d" % k for k in steps])
    t = ref["/Clusters/TableAtStep12"]
    assert t.dtype == np.int64 and t.ndim == 2 and t.shape[1] == 5 and np.array_equal(t, single.clusters.table) and t.shape[0] >= 2
    lines = [r.getMessage() for r in caplog.records if " clusters step " in r.getMessage()]
    assert len(lines) == len(steps) and all(w in lines[-1] for w in ("clusters_R", "largest_B", "percolates_R", "trapped_B")), lines
    files = os.listdir(tmp_path / "out2")
    assert len(files) == 1, files
    got = load_results(str(tmp_path / "out2" / files[0]))
    assert set(got) == set(ref)
    for key in ref:
        assert np.array_equal(got[key], ref[key]), key
    plain = load_results(RKColorGradient3D(str(tmp_path), output_dir=str(tmp_path / "plain"), record_every=6).runRKColorGradient3D())
    assert not any(k.startswith("/Clusters") for k in plain) and set(plain) == {k for k in ref if not k.startswith("/Clusters/")}


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_refusals(box):
    import ctypes as C
    from openlbmpm_amd import _lib
    from openlbmpm_amd._lib import ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED, I64P, LbmpmError
    dom, rR, rB = box
    L = _lib.lib()
    for m, prefix in ((_Pert(dom), "lbmpm_rk3d"), (_Csf(dom), "lbmpm_rk3dcsf")):
        s = m.s
        table = np.zeros((64, 5), dtype=np.int64)
        labels = np.zeros(dom.shape, dtype=np.uint32)
        faces, classes = np.zeros((2,) + dom.shape[1:], dtype=np.uint32), np.zeros((2,) + dom.shape[1:], dtype=np.uint8)
        raw = dict(table=lambda: getattr(L, prefix + "_clusters_table")(s._h, table.ctypes.data_as(I64P)),
                   labels=lambda: getattr(L, prefix + "_clusters_labels")(s._h, labels.ctypes.data_as(_lib.U32P)),
                   faces=lambda: getattr(L, prefix + "_clusters_faces")(s._h, faces.ctypes.data_as(_lib.U32P), classes.ctypes.data_as(_lib.U8P)))
        m.prescribe(rR, rB)
        for name, call in raw.items():
            assert call() == ERR_STATE, (prefix, name, "before the first _clusters")
        with pytest.raises(LbmpmError) as e:
            s.clusters(connectivity=26)
        assert e.value.status == ERR_UNSUPPORTED
        with pytest.raises(LbmpmError) as e:
            s.clusters(phi_cut=-0.1)
        assert e.value.status == ERR_INVALID
        got = s.clusters()
        assert got.table.shape[0] <= 64
        for name, call in raw.items():
            assert call() == 0, (prefix, name)
        assert np.array_equal(table[:got.table.shape[0]], got.table)
        assert np.array_equal(faces[0], labels[0]) and np.array_equal(faces[1], labels[-1])
        assert np.array_equal(classes[0], classify(m.phi(), dom)[0]) and np.array_equal(classes[1], classify(m.phi(), dom)[-1])
        (s.step_single if prefix == "lbmpm_rk3d" else s.step)(1)
        for name, call in raw.items():
            assert call() == ERR_STATE, (prefix, name, "after a step")
        if prefix == "lbmpm_rk3d":
            with pytest.raises(LbmpmError) as e:
                s.clusters()                               # a step since the last phase_field(diagnostics=True)
            assert e.value.status == ERR_STATE and "stale" in str(e.value)
            s.phase_field(diagnostics=True)
        s.clusters()
        assert raw["table"]() == 0
        m.prescribe(rR, rB)                                # a new state
        assert raw["table"]() == ERR_STATE, prefix
        s.close()
    c = _Csf(dom)
    with pytest.raises(LbmpmError) as e:
        c.s.clusters()                                     # before set_macro / set_pdf
    assert e.value.status == ERR_STATE
    c.s.close()


# ---------------------------------------------------------------------------------------------- 5. memory
def test_memory_is_allocated_by_the_first_call_only(box):
    dom, rR, rB = box
    N = dom.size
    for make in (_Pert, _Csf):
        quiet, m = make(dom), make(dom)
        for k in (quiet, m):
            k.prescribe(rR, rB)
            k.step(2)
            k.s.integrals()
        before = m.s.device_bytes
        assert quiet.s.device_bytes == before              # a context that never asks for clusters holds what it held
        m.s.clusters()
        grown = m.s.device_bytes - before
        assert 0 < grown <= 20 * N, (grown, 20 * N)
        m.s.clusters(connectivity=18, labels=True)
        m.step(1)
        m.s.clusters(phi_cut=0.25)
        assert m.s.device_bytes - before == grown          # allocated once
        quiet.step(1)
        assert quiet.s.device_bytes == before
        quiet.s.close(); m.s.close()
