"""The on-device analyses of the 3-D solvers -- plane integrals, the steady-state monitor, phase clusters, per-cluster properties, phase
morphology -- as the two models' classes share them.  Three roles, each a mixin in the style of _lib.SlabTransportCalls:

    SlabAnalysisCalls   one context                    RK3DSlab, RK3DCSFSolver
    StackedAnalysis     the slabs of one process       RK3DCluster, RK3DCSFCluster
    GatheredAnalysis    one slab per rank              RK3DDistributed, RK3DCSFDistributed

The tables and what is read from them: integrals.py, change.py, clusters.py, morphology.py.  What the analyses read (and whether it can be
stale) is the model's: see the class that mixes a role in.  A new analysis is one method per role here.
"""
import numpy as np

from .integrals import fresh


def ring_asked(self, wrap_z, whole=True):
    """wrap_z of clusters() / morphology() as a bool; ValueError, before anything is launched, unless the object is periodic in z
    (periodic_z: the 3-D CSF classes say so) and -- one context -- holds the whole lattice"""
    if not wrap_z:
        return False
    if not getattr(self, "periodic_z", False):
        raise ValueError("wrap_z=True closes the seam of a lattice that is periodic in z (3-D CSF, inlet = outlet = 'Periodic'): %s is not" % type(self).__name__)
    if not whole:
        raise ValueError("wrap_z=True on one slab of a cut lattice: the seam is closed where the slabs are joined (the cluster's or the distributed class)")
    return True


class SlabAnalysisCalls:
    """One context.  The class has the library in _L, its context in _h, the C prefix in _C_PREFIX ("lbmpm_rk3d" | "lbmpm_rk3dcsf"), the
    plane's extent in nx, ny, the number of its own planes in own_planes (a slab: without ghost or halo planes) and the planes of the
    whole lattice in lattice_nz.  Every table covers the own planes.  LbmpmError (LBMPM_ERR_STATE) where the model calls its fields stale."""

    def integrals(self):
        """integrals.Integrals of the own planes, reduced on the device (lbmpm_*_integrals)"""
        from .integrals import Integrals, table
        return Integrals(table(self._L, self._C_PREFIX, self._h, self.own_planes), self.nx, self.ny)

    def mark_change(self):
        """the snapshot change() compares with: u and phi of the own planes, kept on the device (32 bytes per own lattice cell, allocated
        by the first call)"""
        from .change import mark
        mark(self._L, self._C_PREFIX, self._h)

    def change_part(self, remark=True):
        """([own planes][11], steps since the mark): the change table of this context alone"""
        from .change import table
        return table(self._L, self._C_PREFIX, self._h, self.own_planes, remark)

    def change(self, remark=True):
        """change.Change of the own planes: the fields against the snapshot, reduced on the device (lbmpm_*_change); remark: they replace
        the snapshot in the same pass.  LbmpmError (LBMPM_ERR_STATE) before mark_change() and after a set_* since the mark"""
        from .change import Change
        t, steps = self.change_part(remark)
        return Change(t, self.nx, self.ny, steps)

    def clusters_part(self, phi_cut=0.0, connectivity=6, labels=False, faces=True):
        """clusters.take of the own planes: the table (and labels, faces) of this context alone, for clusters.merge_slabs"""
        from .clusters import take
        return take(self._L, self._C_PREFIX, self._h, self.own_planes, self.ny, self.nx, phi_cut, connectivity, labels, faces)

    def cluster_props_face(self):
        """[2][ny][nx] uint8: the class bytes of the lowest and the highest own plane under the last clusters_part -- what the slabs beside
        this one pass to cluster_props_part"""
        from .clusters import props_face
        return props_face(self._L, self._C_PREFIX, self._h, self.ny, self.nx)

    def cluster_props_part(self, count, below=None, above=None):
        """[count][14] int64: the properties of the clusters of the last clusters_part (count: its rows), reduced on the device
        (lbmpm_*_cluster_props); below / above: the class planes of the slabs beside this one (None: the lattice ends there)"""
        from .clusters import props_table
        return props_table(self._L, self._C_PREFIX, self._h, count, self.ny, self.nx, below, above)

    def clusters(self, phi_cut=0.0, connectivity=6, labels=False, props=False, wrap_z=False):
        """clusters.Clusters of the own planes: the connected cells of each phase of phi, labelled on the device (lbmpm_*_clusters).
        props=True: with the property table (faces, elements, plane sum, mass and momentum per cluster), reduced on the device.
        wrap_z=True (periodic z, the whole lattice in this context; else ValueError): the seam between plane nz - 1 and plane 0 is
        closed -- the same launches, the property table reduced with the context's own face planes beside it, then clusters.close_seam
        on the table and the two face planes: a cluster across the seam is one row, every row has its winding"""
        from .clusters import Clusters, close_seam, relabel
        if not ring_asked(self, wrap_z, self.own_planes == self.lattice_nz):
            got = self.clusters_part(phi_cut, connectivity, labels, faces=False)
            table = self.cluster_props_part(got["table"].shape[0]) if props else None
            return Clusters(got["table"], self.nx, self.ny, self.lattice_nz, got.get("labels"), table)
        got = self.clusters_part(phi_cut, connectivity, labels, faces=True)
        opened = None
        if props:
            own = self.cluster_props_face()
            opened = self.cluster_props_part(got["table"].shape[0], below=own[1], above=own[0])
        table, winding, mapping, closed = close_seam(got["table"], got["face_labels"], got["face_classes"], self.nx, self.ny, self.lattice_nz,
                                                     connectivity, opened)
        return Clusters(table, self.nx, self.ny, self.lattice_nz, relabel(got["labels"], mapping) if labels else None, closed,
                        winding=winding, wrap_z=True)

    def morphology_face(self, phi_cut=0.0):
        """[ny][nx] uint8: the classes of the lowest own plane -- what the slab below passes to morphology_part as `above`"""
        from .morphology import face
        return face(self._L, self._C_PREFIX, self._h, self.ny, self.nx, phi_cut)

    def morphology_part(self, phi_cut=0.0, above=None):
        """[own planes][28]: the morphology table of this context alone; above: the morphology_face of the slab over it (None: the highest
        own plane anchors nothing that reaches upwards)"""
        from .morphology import table
        return table(self._L, self._C_PREFIX, self._h, self.own_planes, self.ny, self.nx, phi_cut, above)

    def morphology(self, phi_cut=0.0, wrap_z=False):
        """morphology.Morphology of the own planes: cells, class pairs, squares and cubes, counted on the device (lbmpm_*_morphology).
        wrap_z=True (periodic z, the whole lattice in this context; else ValueError): plane 0 is the plane above plane nz - 1"""
        from .morphology import Morphology
        above = self.morphology_face(phi_cut) if ring_asked(self, wrap_z, self.own_planes == self.lattice_nz) else None
        return Morphology(self.morphology_part(phi_cut, above), self.nx, self.ny)


class StackedAnalysis:
    """The slabs of one process, lowest first, in `slabs` (each a SlabAnalysisCalls); the whole lattice's extent in nx, ny, nz.  _refresh:
    what makes stale fields current again -- called once when a slab answers LBMPM_ERR_STATE, then the take is repeated -- or None for a
    model whose analyses are never stale.  Every result is bit-equal to the undivided lattice's."""
    _refresh = None

    def integrals(self):
        """the slabs' tables in plane order"""
        from .integrals import Integrals
        return Integrals(fresh(lambda: np.concatenate([s.integrals().planes for s in self.slabs], axis=0), self._refresh), self.nx, self.ny)

    def mark_change(self):
        """every slab's snapshot for change()"""
        fresh(lambda: [s.mark_change() for s in self.slabs], self._refresh)

    def change(self, remark=True):
        """change.Change of the whole lattice: the slabs' tables in plane order, each against its own snapshot"""
        from .change import Change, stacked
        t, steps = fresh(lambda: stacked(self.slabs, remark), self._refresh)
        return Change(t, self.nx, self.ny, steps)

    def clusters(self, phi_cut=0.0, connectivity=6, labels=False, props=False, wrap_z=False):
        """clusters.Clusters of the whole lattice: the slabs' tables joined through their face planes.  props=True: with the property
        table -- the slabs hand each other their class planes, every slab reduces its own rows, the rows are added.  wrap_z=True
        (periodic z; else ValueError): the stack is a ring -- the end slabs hand each other their planes too, and the seam is closed on
        the joined table (clusters.close_seam)"""
        from .clusters import merged, stacked_props
        ring = ring_asked(self, wrap_z)

        def take():
            parts = [s.clusters_part(phi_cut, connectivity, labels) for s in self.slabs]
            return stacked_props(self.slabs, parts, ring) if props else parts
        return merged(fresh(take, self._refresh), self.nx, self.ny, self.nz, connectivity, labels, ring)

    def morphology(self, phi_cut=0.0, wrap_z=False):
        """morphology.Morphology of the whole lattice: every slab joins the lowest own plane of the slab over it on its device, the top
        slab nothing -- or, with wrap_z=True (periodic z; else ValueError), the lowest plane of the bottom slab"""
        from .morphology import Morphology, stacked
        ring = ring_asked(self, wrap_z)
        return Morphology(fresh(lambda: stacked(self.slabs, phi_cut, ring), self._refresh), self.nx, self.ny)


class GatheredAnalysis:
    """One slab per rank of torch.distributed: this rank's in `slab` (a SlabAnalysisCalls), gather(array of the own planes) -> the whole
    lattice's on rank 0, rank, world, group (None: the default group), device_index (the slab's GPU: the class planes travel through it
    under nccl), the whole lattice's extent in nx, ny, nz, and _refresh as in StackedAnalysis (every rank is stale, or none: they step
    together).  Every method is collective: rank 0 returns the result of the whole lattice, the others None."""
    _refresh = None

    def integrals(self):
        """the ranks' tables through gather()"""
        from .integrals import Integrals
        t = self.gather(fresh(lambda: self.slab.integrals().planes, self._refresh))
        return None if t is None else Integrals(t, self.nx, self.ny)

    def mark_change(self):
        """every rank: the snapshot of its slab for change() (nothing is returned)"""
        fresh(self.slab.mark_change, self._refresh)

    def change(self, remark=True):
        """change.Change of the whole lattice: every rank against its own snapshot, the tables through gather()"""
        from .change import Change
        part, steps = fresh(lambda: self.slab.change_part(remark), self._refresh)
        t = self.gather(part)
        return None if t is None else Change(t, self.nx, self.ny, steps)

    def clusters(self, phi_cut=0.0, connectivity=6, labels=False, props=False, wrap_z=False):
        """clusters.Clusters of the whole lattice: the ranks' tables and face planes, joined on rank 0 (with labels=True the label planes
        too).  props=True: with the property table -- one all_gather of 2 ny nx class bytes first, every rank reduces its own rows, rank
        0 adds them.  wrap_z=True (periodic z; else ValueError on every rank): the ranks are a ring -- the same all_gather hands rank 0
        the last rank's plane and the last rank rank 0's, and rank 0 closes the seam on the joined table (clusters.close_seam)"""
        from .clusters import faces_from_neighbours, gather_merged
        ring = ring_asked(self, wrap_z)

        def take():
            part = self.slab.clusters_part(phi_cut, connectivity, labels)
            if props:
                part["props_face"] = self.slab.cluster_props_face()
            return part
        part = fresh(take, self._refresh)
        if props:
            below, above = faces_from_neighbours(part.pop("props_face"), self.rank, self.world, self.group, self.device_index, ring)
            part["props"] = self.slab.cluster_props_part(part["table"].shape[0], below, above)
        return gather_merged(part, self.rank, self.world, self.group, self.nx, self.ny, self.nz, connectivity, labels, ring)

    def morphology(self, phi_cut=0.0, wrap_z=False):
        """morphology.Morphology of the whole lattice: every rank takes the lowest class plane of the rank above it (one all_gather of
        [ny][nx] bytes) and joins on its device; the tables through gather().  wrap_z=True (periodic z; else ValueError on every rank):
        the last rank takes rank 0's plane out of the same all_gather"""
        from .morphology import Morphology, face_from_above
        ring = ring_asked(self, wrap_z)
        mine = fresh(lambda: self.slab.morphology_face(phi_cut), self._refresh)
        above = face_from_above(mine, self.rank, self.world, self.group, self.device_index, ring)
        t = self.gather(self.slab.morphology_part(phi_cut, above))
        return None if t is None else Morphology(t, self.nx, self.ny)
