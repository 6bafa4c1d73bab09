"""Phase clusters of the 3-D solvers: the table of lbmpm_rk3d_clusters / lbmpm_rk3dcsf_clusters (include/lbmpm.h holds the definition)
and what a drainage or imbibition run is read through -- has a phase broken through, how much of it is still connected to an open
plane, how much is trapped in ganglia.

The library labels the connected cells of each phase on the device; a label is the global cell number of a cluster's smallest cell,
so a table is the same bit for bit however the lattice was cut into slabs.  A slab's table is that of the slab alone: `merge_slabs`
joins the tables of consecutive slabs through the labels and classes of their face planes.
"""
import numpy as np

# the columns, in the order of LBMPM_CL_* (include/lbmpm.h)
COLUMNS = ("label", "class", "cells", "zmin", "zmax")
LABEL, CLASS, CELLS, ZMIN, ZMAX = range(5)
NONE = 0xFFFFFFFF                     # LBMPM_CLUSTER_NONE: a cell in no cluster
PHASES = {"R": 1, "B": 2}

# the neighbour offsets (dx, dy) of a cell in the plane above it: faces, and the D3Q19 links that cross z
_UP = {6: ((0, 0),), 18: ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1))}


class Clusters:
    """table: [n][5] int64, one row per cluster by ascending label (label, class 1 = R / 2 = B, cells, lowest and highest plane);
    nx, ny, nz: the lattice; labels: [nz][ny][nx] uint32 or None (NONE: solid, interface band or not finite)"""
    COLUMNS = COLUMNS

    def __init__(self, table, nx, ny, nz, labels=None):
        a = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, len(COLUMNS)) if np.size(table) else np.zeros((0, len(COLUMNS)), dtype=np.int64)
        self.table, self.nx, self.ny, self.nz = a, int(nx), int(ny), int(nz)
        self.labels = labels

    def rows(self, phase):
        """the rows of one phase ('R' or 'B')"""
        return self.table[self.table[:, CLASS] == PHASES[phase]]

    def count(self, phase):
        return int(self.rows(phase).shape[0])

    def cells(self, phase):
        """the cells of a phase that lie in clusters (all of them)"""
        return int(self.rows(phase)[:, CELLS].sum())

    def sizes(self, phase):
        """cluster sizes, descending"""
        return np.sort(self.rows(phase)[:, CELLS])[::-1]

    def largest(self, phase):
        s = self.sizes(phase)
        return int(s[0]) if s.size else 0

    def _planes(self, z_lo, z_hi):
        return (1 if z_lo is None else int(z_lo)), (self.nz - 2 if z_hi is None else int(z_hi))

    def spanning(self, phase, z_lo=None, z_hi=None):
        """the rows that reach from plane z_lo (default 1, the outlet plane) to plane z_hi (default nz - 2, the inlet plane)"""
        lo, hi = self._planes(z_lo, z_hi)
        r = self.rows(phase)
        return r[(r[:, ZMIN] <= lo) & (r[:, ZMAX] >= hi)]

    def percolates(self, phase, z_lo=None, z_hi=None):
        return bool(self.spanning(phase, z_lo, z_hi).shape[0])

    def connected_cells(self, phase, to="inlet", z_lo=None, z_hi=None):
        """cells in clusters that touch the inlet plane (high z) or the outlet plane (low z)"""
        if to not in ("inlet", "outlet"):
            raise ValueError("to must be 'inlet' or 'outlet'")
        lo, hi = self._planes(z_lo, z_hi)
        r = self.rows(phase)
        return int(r[r[:, ZMAX] >= hi, CELLS].sum() if to == "inlet" else r[r[:, ZMIN] <= lo, CELLS].sum())

    def trapped_cells(self, phase, z_lo=None, z_hi=None):
        """cells in clusters that touch neither open plane: the ganglia"""
        lo, hi = self._planes(z_lo, z_hi)
        r = self.rows(phase)
        return int(r[(r[:, ZMIN] > lo) & (r[:, ZMAX] < hi), CELLS].sum())

    def trapped_fraction(self, phase, z_lo=None, z_hi=None):
        """the share of the phase's cells that is trapped (the residual saturation, as a share of the phase)"""
        n = self.cells(phase)
        return self.trapped_cells(phase, z_lo, z_hi) / n if n else float("nan")

    def summary(self):
        """the numbers a log line carries"""
        out = {}
        for p in ("R", "B"):
            out["clusters_" + p], out["largest_" + p] = self.count(p), self.largest(p)
            out["percolates_" + p], out["trapped_" + p] = self.percolates(p), self.trapped_cells(p)
        return out


def _name_bytes():
    width = max(len(c) for c in COLUMNS)
    return np.array([list(c.encode().ljust(width, b"\0")) for c in COLUMNS], dtype=np.uint8)


def column_bytes():
    """COLUMNS as a [5][width] uint8 array, zero-padded: /Clusters/Columns of a result file (integrals.column_names reads it back)"""
    return _name_bytes()


def merge_slabs(tables, face_labels, face_classes, nx, ny, connectivity=6):
    """Join the tables of consecutive slabs (lowest first).  tables[s]: [n_s][5]; face_labels[s], face_classes[s]: [2][ny][nx], the
    lowest and the highest own plane of slab s.  Across every cut the clusters whose face cells are neighbours of one class are joined
    (the offsets that cross z; x and y wrap): a union-find over the rows.  A merged row has the smallest label, the class, the summed
    cells, the smallest zmin and the largest zmax.  Returns (table [m][5] by ascending label, mapping [n][2] int64: old label -> merged
    label, by ascending old label; `relabel` applies it to a label field)."""
    if connectivity not in _UP:
        raise ValueError("connectivity must be 6 or 18")
    parts = [np.asarray(t, dtype=np.int64).reshape(-1, len(COLUMNS)) for t in tables]
    rows = np.concatenate(parts, axis=0) if parts else np.zeros((0, len(COLUMNS)), dtype=np.int64)
    order = np.argsort(rows[:, LABEL], kind="stable")
    rows = rows[order]
    old = rows[:, LABEL].copy()
    if np.any(old[1:] == old[:-1]):
        raise ValueError("the slabs' tables share a label: labels are global cell numbers of each slab's own cells")
    pairs = []
    for s in range(len(parts) - 1):
        la, ca = np.asarray(face_labels[s])[1].reshape(ny, nx), np.asarray(face_classes[s])[1].reshape(ny, nx)
        lb, cb = np.asarray(face_labels[s + 1])[0].reshape(ny, nx), np.asarray(face_classes[s + 1])[0].reshape(ny, nx)
        for dx, dy in _UP[connectivity]:
            lbs, cbs = np.roll(lb, (-dy, -dx), axis=(0, 1)), np.roll(cb, (-dy, -dx), axis=(0, 1))      # [y][x] = the upper cell (x + dx, y + dy)
            m = (ca != 0) & (ca == cbs)
            if m.any():
                pairs.append(np.unique(np.stack([la[m].astype(np.int64), lbs[m].astype(np.int64)], axis=1), axis=0))
    parent = np.arange(rows.shape[0])

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    if pairs:
        pq = np.unique(np.concatenate(pairs, axis=0), axis=0)
        ia, ib = np.searchsorted(old, pq[:, 0]), np.searchsorted(old, pq[:, 1])
        if ia.size and (np.any(old[np.minimum(ia, old.size - 1)] != pq[:, 0]) or np.any(old[np.minimum(ib, old.size - 1)] != pq[:, 1])):
            raise ValueError("a face label has no row in its slab's table")
        for a, b in zip(ia.tolist(), ib.tolist()):
            ra, rb = find(a), find(b)
            if ra != rb:                     # rows ascend by label: the smaller index is the smaller label
                parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(i) for i in range(rows.shape[0])], dtype=np.int64)
    keep = root == np.arange(rows.shape[0])
    out = rows[keep].copy()
    slot = np.cumsum(keep) - 1               # row index -> index in `out` (valid at roots)
    tgt = slot[root]
    out[:, CELLS] = 0
    np.add.at(out[:, CELLS], tgt, rows[:, CELLS])
    np.minimum.at(out[:, ZMIN], tgt, rows[:, ZMIN])
    np.maximum.at(out[:, ZMAX], tgt, rows[:, ZMAX])
    return out, np.stack([old, old[root]], axis=1)


def relabel(labels, mapping):
    """a label field (uint32, NONE where no cluster) rewritten through merge_slabs' mapping"""
    lab = np.asarray(labels, dtype=np.uint32)
    out = lab.copy()
    m = lab != NONE
    if m.any():
        old = mapping[:, 0]
        i = np.searchsorted(old, lab[m].astype(np.int64))
        out[m] = mapping[i, 1].astype(np.uint32)
    return out


def merged(parts, nx, ny, nz, connectivity, labels):
    """Clusters of the whole lattice from the slabs' `take` results, lowest slab first"""
    table, mapping = merge_slabs([p["table"] for p in parts], [p["face_labels"] for p in parts], [p["face_classes"] for p in parts],
                                 nx, ny, connectivity)
    field = relabel(np.concatenate([p["labels"] for p in parts], axis=0), mapping) if labels else None
    return Clusters(table, nx, ny, nz, field)


def take(L, prefix, handle, planes, ny, nx, phi_cut=0.0, connectivity=6, labels=False, faces=False):
    """One context through lbmpm_<prefix>_clusters*: dict(table [n][5] int64, labels [planes][ny][nx] uint32 when asked for, face_labels /
    face_classes [2][ny][nx] when asked for)"""
    import ctypes as C
    from ._lib import I64P, U8P, U32P, ClustersConfig, check
    cfg = ClustersConfig(float(phi_cut), int(connectivity), 0)
    n = C.c_int64(0)
    name = "lbmpm_%s_clusters" % prefix
    check(getattr(L, name)(handle, C.byref(cfg), C.byref(n)), name)
    out = dict(table=np.zeros((n.value, len(COLUMNS)), dtype=np.int64))
    if n.value:
        check(getattr(L, name + "_table")(handle, out["table"].ctypes.data_as(I64P)), name + "_table")
    if labels:
        out["labels"] = np.empty((int(planes), int(ny), int(nx)), dtype=np.uint32)
        check(getattr(L, name + "_labels")(handle, out["labels"].ctypes.data_as(U32P)), name + "_labels")
    if faces:
        out["face_labels"] = np.empty((2, int(ny), int(nx)), dtype=np.uint32)
        out["face_classes"] = np.empty((2, int(ny), int(nx)), dtype=np.uint8)
        check(getattr(L, name + "_faces")(handle, out["face_labels"].ctypes.data_as(U32P), out["face_classes"].ctypes.data_as(U8P)), name + "_faces")
    return out


def gather_merged(part, rank, world, group, nx, ny, nz, connectivity, labels):
    """collective: the ranks' `take` results (rank order = slab order, lowest first) to rank 0, which merges; None elsewhere"""
    import torch.distributed as dist
    got = [None] * world if rank == 0 else None
    dist.gather_object(part, got, dst=0 if group is None else dist.get_global_rank(group, 0), group=group)
    return merged(got, nx, ny, nz, connectivity, labels) if rank == 0 else None
