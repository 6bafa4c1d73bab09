"""openlbmpm_amd/analysis.py without a GPU: every analysis method is defined once per role and shared by the two models; the calls a
context makes into the library, by symbol and argument count, with the shapes that come back; the refresh of stale slabs."""
import ctypes as C

import numpy as np
import pytest

from openlbmpm_amd import _lib, analysis, change, clusters, integrals, morphology
from openlbmpm_amd.rk3d import RK3DCluster, RK3DDistributed, RK3DSlab
from openlbmpm_amd.rk3dcsf import RK3DCSFCluster, RK3DCSFDistributed, RK3DCSFSolver

SLAB_METHODS = ("integrals", "mark_change", "change_part", "change", "clusters_part", "cluster_props_face", "cluster_props_part", "clusters",
                "morphology_face", "morphology_part", "morphology")
WHOLE_METHODS = ("integrals", "mark_change", "change", "clusters", "morphology")
ROLES = ((analysis.SlabAnalysisCalls, SLAB_METHODS, (RK3DSlab, RK3DCSFSolver)),
         (analysis.StackedAnalysis, WHOLE_METHODS, (RK3DCluster, RK3DCSFCluster)),
         (analysis.GatheredAnalysis, WHOLE_METHODS, (RK3DDistributed, RK3DCSFDistributed)))


@pytest.mark.parametrize("role,names,classes", ROLES, ids=[r[0].__name__ for r in ROLES])
def test_single_definition(role, names, classes):
    for name in names:
        fns = [getattr(cls, name) for cls in classes]
        for cls, fn in zip(classes, fns):
            assert callable(fn) and fn.__module__ == "openlbmpm_amd.analysis", "%s.%s is defined in %s" % (cls.__name__, name, fn.__module__)
        assert fns[0] is fns[1] is getattr(role, name), "%s: the two models do not share one function" % name


# ---- calls: nx = 3, ny = 2, 6 stored planes of which 4 are own (ghost 1 + 1), a lattice of 9 planes
NX, NY, STORED, GHOST, LATTICE_NZ, COUNT = 3, 2, 6, (1, 1), 9, 3
OWN = STORED - GHOST[0] - GHOST[1]
TABLE_ROWS = [(20 + i, 1 + i % 2, 5 + i, i, i + 1) for i in range(COUNT)]


def _fill(ptr, n, value):
    for i in range(n):
        ptr[i] = value


class StubLibrary:
    """records (symbol, argument count) and writes a recognisable value into every output array"""

    def __init__(self, prefix):
        self.prefix, self.calls = prefix, []

    def __getattr__(self, name):
        if not name.startswith(self.prefix + "_"):
            raise AttributeError(name)
        what = name[len(self.prefix) + 1:]

        def call(*args):
            self.calls.append((name, len(args)))
            getattr(self, "_" + what)(*args[1:])
            return 0
        return call

    def _integrals(self, out):
        _fill(out, OWN * len(integrals.COLUMNS), 1.5)

    def _change_mark(self):
        pass

    def _change(self, remark, steps, out):
        steps._obj.value = 7
        _fill(out, OWN * len(change.COLUMNS), 2.5)

    def _clusters(self, cfg, count):
        count._obj.value = COUNT

    def _clusters_table(self, out):
        for i, row in enumerate(TABLE_ROWS):
            for j, v in enumerate(row):
                out[i * 5 + j] = v

    def _clusters_labels(self, out):
        _fill(out, OWN * NY * NX, 20)

    def _clusters_faces(self, labels, classes):
        _fill(labels, 2 * NY * NX, 21)
        _fill(classes, 2 * NY * NX, 1)

    def _cluster_props_face(self, out):
        _fill(out, 2 * NY * NX, 2)

    def _cluster_props(self, below, above, out):
        for i, row in enumerate(TABLE_ROWS):
            for j in range(len(clusters.PROP_COLUMNS)):
                out[i * len(clusters.PROP_COLUMNS) + j] = row[j] if j < 3 else 40 + j

    def _morphology_face(self, cfg, out):
        _fill(out, NY * NX, 3)

    def _morphology(self, cfg, above, out):
        _fill(out, OWN * len(morphology.COLUMNS), 3.5)


class OneContext(analysis.SlabAnalysisCalls):
    nx, ny, own_planes, lattice_nz = NX, NY, OWN, LATTICE_NZ

    def __init__(self, prefix):
        self._C_PREFIX, self._L, self._h = prefix, StubLibrary(prefix), C.c_void_p(1)

    def called(self, method, *args, **kwargs):
        del self._L.calls[:]
        got = getattr(self, method)(*args, **kwargs)
        return got, [(name[len(self._C_PREFIX) + 1:], n) for name, n in self._L.calls]


@pytest.mark.parametrize("prefix", ["lbmpm_rk3d", "lbmpm_rk3dcsf"])
def test_calls_of_one_context(prefix, monkeypatch):
    built = []
    real = clusters.Clusters

    class Recorded(real):
        def __init__(self, table, nx, ny, nz, labels=None, props=None):
            built.append((nx, ny, nz))
            real.__init__(self, table, nx, ny, nz, labels, props)
    monkeypatch.setattr(clusters, "Clusters", Recorded)
    s = OneContext(prefix)

    g, calls = s.called("integrals")
    assert calls == [("integrals", 2)]
    assert isinstance(g, integrals.Integrals) and g.planes.shape == (OWN, len(integrals.COLUMNS)) and np.all(g.planes == 1.5) and (g.nx, g.ny) == (NX, NY)

    g, calls = s.called("mark_change")
    assert calls == [("change_mark", 1)] and g is None
    (t, steps), calls = s.called("change_part", remark=False)
    assert calls == [("change", 4)] and t.shape == (OWN, len(change.COLUMNS)) and np.all(t == 2.5) and steps == 7
    g, calls = s.called("change")
    assert calls == [("change", 4)]
    assert isinstance(g, change.Change) and g.planes.shape == (OWN, len(change.COLUMNS)) and g.steps == 7 and (g.nx, g.ny) == (NX, NY)

    g, calls = s.called("clusters_part", labels=True)
    assert calls == [("clusters", 3), ("clusters_table", 2), ("clusters_labels", 2), ("clusters_faces", 3)]
    assert g["table"].tolist() == [list(r) for r in TABLE_ROWS]
    assert g["labels"].shape == (OWN, NY, NX) and np.all(g["labels"] == 20)
    assert g["face_labels"].shape == (2, NY, NX) and g["face_classes"].shape == (2, NY, NX) and np.all(g["face_labels"] == 21)
    g, calls = s.called("cluster_props_face")
    assert calls == [("cluster_props_face", 2)] and g.shape == (2, NY, NX) and g.dtype == np.uint8 and np.all(g == 2)
    g, calls = s.called("cluster_props_part", COUNT, below=np.ones((NY, NX), dtype=np.uint8))
    assert calls == [("cluster_props", 4)] and g.shape == (COUNT, len(clusters.PROP_COLUMNS)) and g[:, :3].tolist() == [list(r[:3]) for r in TABLE_ROWS]
    g, calls = s.called("clusters")
    assert calls == [("clusters", 3), ("clusters_table", 2)] and g.props is None and g.labels is None
    g, calls = s.called("clusters", labels=True, props=True)
    assert calls == [("clusters", 3), ("clusters_table", 2), ("clusters_labels", 2), ("cluster_props", 4)]
    assert g.table.shape == (COUNT, 5) and g.props.shape == (COUNT, len(clusters.PROP_COLUMNS)) and g.labels.shape == (OWN, NY, NX)
    assert built == [(NX, NY, LATTICE_NZ)] * 2 and g.nz == LATTICE_NZ      # the lattice's planes, not the 4 own or the 6 stored ones

    g, calls = s.called("morphology_face", 0.25)
    assert calls == [("morphology_face", 3)] and g.shape == (NY, NX) and g.dtype == np.uint8 and np.all(g == 3)
    g, calls = s.called("morphology_part", above=np.ones((NY, NX), dtype=np.uint8))
    assert calls == [("morphology", 4)] and g.shape == (OWN, len(morphology.COLUMNS)) and np.all(g == 3.5)
    g, calls = s.called("morphology")
    assert calls == [("morphology", 4)]
    assert isinstance(g, morphology.Morphology) and g.planes.shape == (OWN, len(morphology.COLUMNS)) and (g.nx, g.ny) == (NX, NY)


# ---- refresh: two slabs whose first integrals() fails
class StaleSlab:
    def __init__(self, value, status):
        self.value, self.status, self.asked = value, status, 0

    def integrals(self):
        self.asked += 1
        if self.asked == 1:
            raise _lib.LbmpmError("stale", status=self.status)
        return integrals.Integrals(np.full((2, len(integrals.COLUMNS)), self.value), NX, NY)


class Stack(analysis.StackedAnalysis):
    nx, ny, nz = NX, NY, 4

    def __init__(self, status, refresh):
        self.slabs, self.refreshed = [StaleSlab(1.0, status), StaleSlab(2.0, status)], 0
        if refresh:
            self._refresh = self.refresh

    def refresh(self):
        self.refreshed += 1
        for s in self.slabs:
            s.asked = max(s.asked, 1)


def test_refresh_once_then_the_planes_in_order():
    c = Stack(_lib.ERR_STATE, True)
    g = c.integrals()
    assert c.refreshed == 1
    assert g.planes[:, 0].tolist() == [1.0, 1.0, 2.0, 2.0] and (g.nx, g.ny) == (NX, NY)


def test_without_refresh_the_error_propagates():
    c = Stack(_lib.ERR_STATE, False)
    assert c._refresh is None
    with pytest.raises(_lib.LbmpmError) as e:
        c.integrals()
    assert e.value.status == _lib.ERR_STATE
    assert [s.asked for s in c.slabs] == [1, 0] and c.refreshed == 0      # nothing is retried


@pytest.mark.parametrize("refresh", [True, False])
def test_another_status_propagates_without_refresh(refresh):
    c = Stack(_lib.ERR_INVALID, refresh)
    with pytest.raises(_lib.LbmpmError) as e:
        c.integrals()
    assert e.value.status == _lib.ERR_INVALID
    assert [s.asked for s in c.slabs] == [1, 0] and c.refreshed == 0
