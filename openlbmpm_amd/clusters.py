"""Phase clusters of the 3-D solvers: the table of lbmpm_rk3d_clusters / lbmpm_rk3dcsf_clusters (include/lbmpm.h holds the definition)
and what a drainage or imbibition run is read through -- has a phase broken through, how much of it is still connected to an open
plane, how much is trapped in ganglia.

The library labels the connected cells of each phase on the device; a label is the global cell number of a cluster's smallest cell,
so a table is the same bit for bit however the lattice was cut into slabs.  A slab's table is that of the slab alone: `merge_slabs`
joins the tables of consecutive slabs through the labels and classes of their face planes.  On a lattice that is periodic in z the seam
between plane nz - 1 and plane 0 is one more such cut: `close_seam` closes it (wrap_z=True of the solvers' clusters()) and gives every
cluster its winding, the number of periods along z by which it is connected to its own image.

Beside the table the library reduces a second one on request (lbmpm_*_cluster_props, `props=True`): per cluster the faces towards the
other phase and towards the solid, the pairs, squares and cubes of its cells, the sum of its plane numbers, and mass and momentum as
fixed-point integer sums -- interfacial and wetted area, Euler number, centre, mean density and velocity of every ganglion without a
field leaving the device.  Integers throughout: `merge_props` adds the slabs' rows, and the result is the undivided lattice's bit for bit.
"""
import numpy as np

# the columns, in the order of LBMPM_CL_* (include/lbmpm.h)
COLUMNS = ("label", "class", "cells", "zmin", "zmax")
LABEL, CLASS, CELLS, ZMIN, ZMAX = range(5)
NONE = 0xFFFFFFFF                     # LBMPM_CLUSTER_NONE: a cell in no cluster
PHASES = {"R": 1, "B": 2}
# the columns of the property table, in the order of LBMPM_CP_* (include/lbmpm.h); the first three are the table's own
PROP_COLUMNS = ("label", "class", "cells", "faces_fluid", "faces_solid", "pairs", "squares", "cubes", "sum_z", "mass", "mom_x", "mom_y", "mom_z",
                "clipped")
P_FACES_FLUID, P_FACES_SOLID, P_PAIRS, P_SQUARES, P_CUBES, P_SUM_Z, P_MASS, P_MOM_X, P_MOM_Y, P_MOM_Z, P_CLIPPED = range(3, 14)
MASS_BITS, MOM_BITS = 24, 30          # LBMPM_CP_MASS_BITS, LBMPM_CP_MOM_BITS: MASS in units of 2^-24, MOM_* in units of 2^-30
MOBILE_SPEED = 1e-6                   # summary(): a ganglion counts as mobile above this |velocity| (lattice units)

# the neighbour offsets (dx, dy) of a cell in the plane above it: faces, and the D3Q19 links that cross z
_UP = {6: ((0, 0),), 18: ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1))}


class Clusters:
    """table: [n][5] int64, one row per cluster by ascending label (label, class 1 = R / 2 = B, cells, lowest and highest plane);
    nx, ny, nz: the lattice; labels: [nz][ny][nx] uint32 or None (NONE: solid, interface band or not finite); props: [n][14] int64, the
    property table row by row beside `table` (PROP_COLUMNS), or None.
    wrap_z: the table is one of a lattice that is periodic in z with the seam between plane nz - 1 and plane 0 closed (`close_seam`);
    winding: [n] int64 beside `table` then -- 0: a ganglion, its planes zmin .. zmax counted on without a break (zmax may exceed nz - 1:
    it lies across the seam); w > 0: the cluster is connected to its own image w periods further along z (zmin = 0, zmax = nz - 1).
    Windings along x and y are not computed.  With wrap_z there are no open planes: what the methods below define through them they
    define through `winding`, as each says"""
    COLUMNS = COLUMNS
    PROP_COLUMNS = PROP_COLUMNS

    def __init__(self, table, nx, ny, nz, labels=None, props=None, *, winding=None, wrap_z=False):
        a = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, len(COLUMNS)) if np.size(table) else np.zeros((0, len(COLUMNS)), dtype=np.int64)
        self.table, self.nx, self.ny, self.nz = a, int(nx), int(ny), int(nz)
        self.labels = labels
        self.wrap_z = bool(wrap_z)
        self.winding = None if winding is None else np.ascontiguousarray(winding, dtype=np.int64).reshape(-1)
        if self.wrap_z and self.winding is None:
            raise ValueError("wrap_z: the winding of every cluster (clusters.close_seam) belongs to the table")
        if self.winding is not None and self.winding.shape[0] != a.shape[0]:
            raise ValueError("winding and table are not row by row the same clusters")
        self.props = None
        if props is not None:
            b = np.ascontiguousarray(props, dtype=np.int64).reshape(-1, len(PROP_COLUMNS)) if np.size(props) else np.zeros((0, len(PROP_COLUMNS)), dtype=np.int64)
            if b.shape[0] != a.shape[0] or not np.array_equal(b[:, :3], a[:, :3]):
                raise ValueError("props and table are not row by row the same clusters (label, class, cells)")
            self.props = b

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

    def _winds(self, phase, z_lo, z_hi):
        """wrap_z: which rows of the phase are connected to their own image"""
        if z_lo is not None or z_hi is not None:
            raise ValueError("wrap_z: a ring has no open planes, z_lo / z_hi have no meaning")
        return self.winding[self.table[:, CLASS] == PHASES[phase]] != 0

    def _free(self, phase, z_lo, z_hi):
        """which rows of the phase are ganglia: they touch neither open plane; wrap_z: they are not connected to their own image"""
        if self.wrap_z:
            return ~self._winds(phase, z_lo, z_hi)
        lo, hi = self._planes(z_lo, z_hi)
        r = self.rows(phase)
        return (r[:, ZMIN] > lo) & (r[:, ZMAX] < hi)

    def extent(self, phase=None):
        """zmax - zmin + 1 of every row (of the phase's rows): the planes a cluster reaches over -- with wrap_z across the seam too"""
        r = self.table if phase is None else self.rows(phase)
        return r[:, ZMAX] - r[:, ZMIN] + 1

    def spanning(self, phase, z_lo=None, z_hi=None):
        """the rows that reach from plane z_lo (default 1, the outlet plane) to plane z_hi (default nz - 2, the inlet plane); wrap_z:
        the rows with winding != 0, which conduct round the ring"""
        if self.wrap_z:
            return self.rows(phase)[self._winds(phase, z_lo, z_hi)]
        lo, hi = self._planes(z_lo, z_hi)
        r = self.rows(phase)
        return r[(r[:, ZMIN] <= lo) & (r[:, ZMAX] >= hi)]

    def percolates(self, phase, z_lo=None, z_hi=None):
        return bool(self.spanning(phase, z_lo, z_hi).shape[0])

    def connected_cells(self, phase, to="inlet", z_lo=None, z_hi=None):
        """cells in clusters that touch the inlet plane (high z) or the outlet plane (low z)"""
        if to not in ("inlet", "outlet"):
            raise ValueError("to must be 'inlet' or 'outlet'")
        if self.wrap_z:
            raise ValueError("wrap_z: a ring has neither inlet nor outlet; spanning() holds the clusters that conduct")
        lo, hi = self._planes(z_lo, z_hi)
        r = self.rows(phase)
        return int(r[r[:, ZMAX] >= hi, CELLS].sum() if to == "inlet" else r[r[:, ZMIN] <= lo, CELLS].sum())

    def trapped_cells(self, phase, z_lo=None, z_hi=None):
        """cells in clusters that touch neither open plane: the ganglia (wrap_z: in clusters with winding 0)"""
        return int(self.rows(phase)[self._free(phase, z_lo, z_hi), CELLS].sum())

    def trapped_fraction(self, phase, z_lo=None, z_hi=None):
        """the share of the phase's cells that is trapped (the residual saturation, as a share of the phase)"""
        n = self.cells(phase)
        return self.trapped_cells(phase, z_lo, z_hi) / n if n else float("nan")

    def summary(self, speed=MOBILE_SPEED):
        """the numbers a log line carries; with props also the ganglia of each phase and those of them faster than `speed`; wrap_z:
        also the largest winding of each phase"""
        out = {}
        for p in ("R", "B"):
            out["clusters_" + p], out["largest_" + p] = self.count(p), self.largest(p)
            out["percolates_" + p], out["trapped_" + p] = self.percolates(p), self.trapped_cells(p)
        if self.wrap_z:
            for p in ("R", "B"):
                w = self.winding[self.table[:, CLASS] == PHASES[p]]
                out["winding_" + p] = int(w.max()) if w.size else 0
        if self.props is not None:
            for p in ("R", "B"):
                g = self.ganglia(p)
                out["ganglia_" + p] = int(g.shape[0])
                out["mobile_" + p] = int(np.count_nonzero(np.sqrt((g["velocity"] ** 2).sum(axis=1)) > speed)) if g.shape[0] else 0
        return out

    # ---- the property table: every accessor returns an array row by row beside .table, or beside rows(phase) when a phase is given
    def prop_rows(self, phase=None):
        if self.props is None:
            raise ValueError("no property table: ask for clusters(props=True)")
        return self.props if phase is None else self.props[self.props[:, CLASS] == PHASES[phase]]

    def interfacial_area(self, phase=None):
        """2/3 of the faces towards the other phase: the three-direction Cauchy-Crofton estimate of morphology.Morphology.area"""
        return 2.0 * self.prop_rows(phase)[:, P_FACES_FLUID] / 3.0

    def wetted_area(self, phase=None):
        """2/3 of the faces towards the solid, the same estimate"""
        return 2.0 * self.prop_rows(phase)[:, P_FACES_SOLID] / 3.0

    def euler(self, phase=None):
        """chi_6 = cells - pairs + squares - cubes of every cluster (int64): 1 for a blob, 0 for a ring"""
        r = self.prop_rows(phase)
        return r[:, CELLS] - r[:, P_PAIRS] + r[:, P_SQUARES] - r[:, P_CUBES]

    def centre_z(self, phase=None):
        """the mean plane number of the cluster's cells; wrap_z: of the planes counted on across the seam, taken mod nz, and NaN for a
        cluster with winding != 0, which has no centre on a ring"""
        r = self.prop_rows(phase)
        if not self.wrap_z:
            return r[:, P_SUM_Z] / r[:, CELLS]
        w = self.winding if phase is None else self.winding[self.table[:, CLASS] == PHASES[phase]]
        return np.where(w == 0, np.mod(r[:, P_SUM_Z] / r[:, CELLS], self.nz), np.nan)

    def clipped(self, phase=None):
        """cells that are in no mass or momentum sum (not finite, or out of the fixed-point range)"""
        return self.prop_rows(phase)[:, P_CLIPPED]

    def mass(self, phase=None):
        """the sum of rho_R + rho_B over the cluster's cells that are not clipped"""
        return self.prop_rows(phase)[:, P_MASS] * 2.0 ** -MASS_BITS

    def mean_density(self, phase=None):
        """mass per cell that is not clipped; NaN without one"""
        r = self.prop_rows(phase)
        n = (r[:, CELLS] - r[:, P_CLIPPED]).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(n > 0, self.mass(phase) / n, np.nan)

    def momentum(self, phase=None):
        """[n][3]: the sum of (rho_R + rho_B) u over the cluster's cells that are not clipped"""
        return self.prop_rows(phase)[:, P_MOM_X:P_MOM_Z + 1] * 2.0 ** -MOM_BITS

    def velocity(self, phase=None):
        """[n][3]: momentum / mass, the mass-weighted mean velocity; NaN where the mass is 0"""
        m = self.mass(phase)[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(m != 0, self.momentum(phase) / m, np.nan)

    GANGLION = np.dtype([("label", np.int64), ("volume", np.int64), ("area", np.float64), ("wetted_area", np.float64), ("euler", np.int64),
                         ("centre_z", np.float64), ("velocity", np.float64, (3,))])

    def ganglia(self, phase, z_lo=None, z_hi=None):
        """a structured array (GANGLION) of the clusters of the phase that touch neither open plane (wrap_z: with winding 0), by
        ascending label"""
        r = self.rows(phase)
        m = self._free(phase, z_lo, z_hi)
        out = np.zeros(int(m.sum()), dtype=self.GANGLION)
        out["label"], out["volume"] = r[m, LABEL], r[m, CELLS]
        out["area"], out["wetted_area"] = self.interfacial_area(phase)[m], self.wetted_area(phase)[m]
        out["euler"], out["centre_z"], out["velocity"] = self.euler(phase)[m], self.centre_z(phase)[m], self.velocity(phase)[m]
        return out

    def mobile_cells(self, phase, speed, z_lo=None, z_hi=None):
        """the cells in ganglia whose |velocity| exceeds `speed`"""
        g = self.ganglia(phase, z_lo, z_hi)
        return int(g["volume"][np.sqrt((g["velocity"] ** 2).sum(axis=1)) > speed].sum()) if g.shape[0] else 0


def _name_bytes():
    width = max(len(c) for c in COLUMNS)
    return np.array([list(c.encode().ljust(width, b"\0")) for c in COLUMNS], dtype=np.uint8)


def column_bytes():
    """COLUMNS as a [5][width] uint8 array, zero-padded: /Clusters/Columns of a result file (integrals.column_names reads it back)"""
    return _name_bytes()


def prop_column_bytes():
    """PROP_COLUMNS as a [14][width] uint8 array, zero-padded: /Clusters/PropColumns of a result file"""
    width = max(len(c) for c in PROP_COLUMNS)
    return np.array([list(c.encode().ljust(width, b"\0")) for c in PROP_COLUMNS], dtype=np.uint8)


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


def merge_props(props_parts, mapping):
    """The property tables of consecutive slabs ([n_s][14] each) joined through merge_slabs' mapping: every row goes to its merged
    label; the accumulated columns and the cells are summed (integers: the undivided lattice's bits), label and class are the merged
    cluster's.  Returns [m][14] by ascending label, row by row beside merge_slabs' table."""
    parts = [np.asarray(t, dtype=np.int64).reshape(-1, len(PROP_COLUMNS)) for t in props_parts]
    rows = np.concatenate(parts, axis=0) if parts else np.zeros((0, len(PROP_COLUMNS)), dtype=np.int64)
    rows = rows[np.argsort(rows[:, LABEL], kind="stable")]
    mapping = np.asarray(mapping, dtype=np.int64).reshape(-1, 2)
    if rows.shape[0] != mapping.shape[0] or not np.array_equal(rows[:, LABEL], mapping[:, 0]):
        raise ValueError("the property tables and the mapping do not hold the same labels")
    new, tgt = np.unique(mapping[:, 1], return_inverse=True)
    out = np.zeros((new.shape[0], len(PROP_COLUMNS)), dtype=np.int64)
    np.add.at(out, tgt.reshape(-1), rows)
    out[:, LABEL] = new
    keep = mapping[:, 0] == mapping[:, 1]                  # the row that gave the merged cluster its label: its class is the cluster's
    out[:, CLASS] = rows[keep, CLASS]
    return out


def _seam_links(old, face_labels, face_classes, nx, ny, connectivity):
    """the links across the seam as unique pairs of row indices (cluster of a cell of plane nz - 1, cluster of its neighbour in plane 0),
    taken as merge_slabs takes a cut's; a pair of one row with itself stays"""
    la, ca = np.asarray(face_labels)[1].reshape(ny, nx), np.asarray(face_classes)[1].reshape(ny, nx)
    lb, cb = np.asarray(face_labels)[0].reshape(ny, nx), np.asarray(face_classes)[0].reshape(ny, nx)
    pairs = []                                # a pair as one number, (upper label << 32) | lower label: labels are uint32
    for dx, dy in _UP[connectivity]:
        lbs, cbs = np.roll(lb, (-dy, -dx), axis=(0, 1)), np.roll(cb, (-dy, -dx), axis=(0, 1))          # [y][x] = the cell (x + dx, y + dy) of plane 0
        m = (ca != 0) & (ca == cbs)
        if m.any():
            pairs.append(np.unique((la[m].astype(np.uint64) << np.uint64(32)) | lbs[m].astype(np.uint64)))
    if not pairs:
        return np.zeros((0, 2), dtype=np.int64)
    pq = np.unique(np.concatenate(pairs))
    upper, lower = (pq >> np.uint64(32)).astype(np.int64), (pq & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ia, ib = np.searchsorted(old, upper), np.searchsorted(old, lower)
    if np.any(old[np.minimum(ia, old.size - 1)] != upper) or np.any(old[np.minimum(ib, old.size - 1)] != lower):
        raise ValueError("a face label has no row in the table")
    return np.stack([ia, ib], axis=1)


def close_seam(table, face_labels, face_classes, nx, ny, nz, connectivity=6, props=None):
    """Close the seam of a lattice that is periodic in z.  table: [n][5], the open table of the whole lattice (one context's, or
    merge_slabs'); face_labels, face_classes: [2][ny][nx], plane 0 and plane nz - 1; props: [n][14] beside the table, or None.

    A link across the seam joins a cell of plane nz - 1 to a neighbour of its class in plane 0 (the offsets that cross z; x and y wrap):
    a directed edge from the upper cell's open cluster to the lower cell's, one period long.  Every connected component of that graph is
    one cluster of the ring.  A walk gives each open cluster an integer potential -- the periods by which it lies above the one the walk
    began with, pot[b] = pot[a] + 1 along an edge -- and an edge that finds another potential than it brings closes a loop that many
    periods long: the component's winding is the gcd of those, 0 without one.  winding w > 0: the cluster is connected to its own image
    w periods on and occupies every plane (zmin = 0, zmax = nz - 1).  winding 0: a ganglion; zmin = min(zmin_i + pot_i nz), zmax likewise,
    both moved by a multiple of nz so that 0 <= zmin < nz -- zmax may exceed nz - 1.  Integers throughout; the result does not depend
    on where the ring was cut or on the order of the walk (the potentials are fixed up to a constant, which the move takes out).

    Returns (table [m][5] by ascending label: the smallest label, the class, the summed cells, the extent; winding [m] int64; mapping
    [n][2] as merge_slabs' -- `relabel` and `merge_props` take it; props [m][14] with sum_z counted on across the seam for winding 0,
    the plain sum otherwise, or None)."""
    if connectivity not in _UP:
        raise ValueError("connectivity must be 6 or 18")
    from math import gcd
    nz = int(nz)
    rows = np.asarray(table, dtype=np.int64).reshape(-1, len(COLUMNS))
    old = rows[:, LABEL].copy()
    if np.any(old[1:] <= old[:-1]):
        raise ValueError("the table's rows must ascend by label")
    n = rows.shape[0]
    edges = _seam_links(old, face_labels, face_classes, int(nx), int(ny), connectivity).tolist() if n else []
    # only the rows with a link walk: every other row is a component of its own, at potential 0
    near = {}                                 # row -> [(the row at the other end, the step in potential towards it)]
    for a, b in edges:
        near.setdefault(a, []).append((b, 1))
        near.setdefault(b, []).append((a, -1))
    pot, root, wind = np.zeros(n, dtype=np.int64), np.arange(n, dtype=np.int64), np.zeros(n, dtype=np.int64)       # wind: at the root's index
    at = {}
    for i in sorted(near):                    # rows ascend by label: a walk begins at its component's smallest label
        if i in at:
            continue
        at[i], todo = 0, [i]
        while todo:
            a = todo.pop()
            for b, step in near[a]:
                if b not in at:
                    at[b], root[b] = at[a] + step, i
                    todo.append(b)
    for a, b in edges:
        wind[root[a]] = gcd(int(wind[root[a]]), abs(at[a] + 1 - at[b]))
    if at:
        pot[list(at)] = list(at.values())
    keep = root == np.arange(n)
    tgt = (np.cumsum(keep) - 1)[root]
    out = rows[keep].copy()
    winding = wind[keep]
    big = np.iinfo(np.int64).max
    lo, hi = np.full(out.shape[0], big), np.full(out.shape[0], -big)
    np.minimum.at(lo, tgt, rows[:, ZMIN] + pot * nz)
    np.maximum.at(hi, tgt, rows[:, ZMAX] + pot * nz)
    shift = np.where(winding == 0, np.floor_divide(lo, nz), 0)         # whole periods to take out
    out[:, CELLS] = 0
    np.add.at(out[:, CELLS], tgt, rows[:, CELLS])
    out[:, ZMIN] = np.where(winding == 0, lo - shift * nz, 0)
    out[:, ZMAX] = np.where(winding == 0, hi - shift * nz, nz - 1)
    mapping = np.stack([old, old[root]], axis=1)
    if props is None:
        return out, winding, mapping, None
    # merge_props' sums (merge_props([props], mapping) is this table but for sum_z), added row by row for the few rows that move only
    parts = np.asarray(props, dtype=np.int64).reshape(-1, len(PROP_COLUMNS))
    if parts.shape[0] != n or not np.array_equal(parts[:, LABEL], old):
        raise ValueError("the property table and the table do not hold the same labels")
    joined = parts[keep].copy()
    moved = np.nonzero(~keep)[0]
    np.add.at(joined, tgt[moved], parts[moved])
    joined[:, LABEL], joined[:, CLASS] = out[:, LABEL], out[:, CLASS]
    walked = np.array(sorted(at), dtype=np.int64).reshape(-1)                # the rows off potential 0 are among these
    walked = walked[(winding == 0)[tgt[walked]]]
    np.add.at(joined[:, P_SUM_Z], tgt[walked], (pot[walked] - shift[tgt[walked]]) * nz * parts[walked, CELLS])
    return out, winding, mapping, joined


def merged(parts, nx, ny, nz, connectivity, labels, ring=False):
    """Clusters of the whole lattice from the slabs' `take` results, lowest slab first (with the property table where every part has one).
    ring: the lattice is periodic in z and the seam between the last slab's highest and the first slab's lowest plane is closed too
    (close_seam on the chain's table; the slabs' property tables were then reduced with the planes across the seam beside them)"""
    table, mapping = merge_slabs([p["table"] for p in parts], [p["face_labels"] for p in parts], [p["face_classes"] for p in parts],
                                 nx, ny, connectivity)
    field = relabel(np.concatenate([p["labels"] for p in parts], axis=0), mapping) if labels else None
    props = merge_props([p["props"] for p in parts], mapping) if parts and all("props" in p for p in parts) else None
    if not ring:
        return Clusters(table, nx, ny, nz, field, props)
    ends = lambda key: np.stack([np.asarray(parts[0][key])[0], np.asarray(parts[-1][key])[1]])
    table, winding, seam, props = close_seam(table, relabel(ends("face_labels"), mapping), ends("face_classes"), nx, ny, nz, connectivity, props)
    return Clusters(table, nx, ny, nz, relabel(field, seam) if labels else None, props, winding=winding, wrap_z=True)


def _class_plane(a, ny, nx, what):
    if a is None:
        return None
    p = np.ascontiguousarray(a, dtype=np.uint8)
    if p.shape != (int(ny), int(nx)):
        raise TypeError("%s must have shape [ny][nx]" % what)
    return p


def props_face(L, prefix, handle, ny, nx):
    """[2][ny][nx] uint8: the class bytes (0 S, 1 R, 2 B, 3 N) of the lowest and the highest own plane of one context, those of its last
    <prefix>_clusters call -- what the slab below takes as `above` ([0]) and the slab above as `below` ([1])"""
    from ._lib import U8P, check
    out = np.empty((2, int(ny), int(nx)), dtype=np.uint8)
    name = prefix + "_cluster_props_face"
    check(getattr(L, name)(handle, out.ctypes.data_as(U8P)), name)
    return out


def props_table(L, prefix, handle, count, ny, nx, below=None, above=None):
    """[count][14] int64 of one context through <prefix>_cluster_props: the properties of the clusters of its last
    <prefix>_clusters call (count: that call's); below / above: [ny][nx] class planes of the neighbouring slabs, None at the
    lattice's ends"""
    from ._lib import I64P, U8P, check
    dn, up = _class_plane(below, ny, nx, "below"), _class_plane(above, ny, nx, "above")
    out = np.zeros((int(count), len(PROP_COLUMNS)), dtype=np.int64)
    name = prefix + "_cluster_props"
    check(getattr(L, name)(handle, None if dn is None else dn.ctypes.data_as(U8P), None if up is None else up.ctypes.data_as(U8P),
                           out.ctypes.data_as(I64P)), name)
    return out


def stacked_props(slabs, parts, ring=False):
    """the slabs of one process, lowest first, after every one's clusters_part (parts): the slabs hand their face planes to each other
    and every part gains its property table.  ring: the lowest slab takes the highest slab's highest plane as `below` and the highest
    slab the lowest slab's lowest plane as `above` (one slab: its own)"""
    faces = [s.cluster_props_face() for s in slabs]
    n = len(slabs)
    for k, (s, part) in enumerate(zip(slabs, parts)):
        below = faces[k - 1][1] if k or ring else None
        above = faces[(k + 1) % n][0] if k + 1 < n or ring else None
        part["props"] = s.cluster_props_part(part["table"].shape[0], below, above)
    return parts


def faces_from_neighbours(mine, rank, world, group, device, ring=False):
    """collective: every rank gives the [2][ny][nx] class planes of its slab and takes (below, above): the highest plane of rank - 1 and
    the lowest of rank + 1 (None at the ends; ring: rank 0 takes the last rank's highest plane and the last rank rank 0's lowest).  One
    all_gather of 2 * ny * nx bytes, through device memory under nccl, host memory under gloo; a world of one: none (ring: its own planes)"""
    if world == 1:
        return (np.asarray(mine)[1], np.asarray(mine)[0]) if ring else (None, None)
    import torch
    import torch.distributed as dist
    dev = torch.device("cuda", device) if dist.get_backend(group) == "nccl" else torch.device("cpu")
    t = torch.from_numpy(np.ascontiguousarray(mine, dtype=np.uint8)).to(dev)
    every = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(every, t, group=group)
    return (every[rank - 1][1].cpu().numpy() if rank or ring else None), (every[(rank + 1) % world][0].cpu().numpy() if rank + 1 < world or ring else None)


def take(L, prefix, handle, planes, ny, nx, phi_cut=0.0, connectivity=6, labels=False, faces=False, props=False, below=None, above=None):
    """One context through <prefix>_clusters*: dict(table [n][5] int64, labels [planes][ny][nx] uint32 when asked for, face_labels /
    face_classes [2][ny][nx] when asked for, props [n][14] int64 when asked for -- with below / above, the class planes of the
    neighbouring slabs, where there are such)"""
    import ctypes as C
    from ._lib import I64P, U8P, U32P, ClustersConfig, check
    cfg = ClustersConfig(float(phi_cut), int(connectivity), 0)
    n = C.c_int64(0)
    name = prefix + "_clusters"
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
    if props:
        out["props"] = props_table(L, prefix, handle, n.value, ny, nx, below, above)
    return out


def gather_merged(part, rank, world, group, nx, ny, nz, connectivity, labels, ring=False):
    """collective: the ranks' `take` results (rank order = slab order, lowest first) to rank 0, which merges (ring: and closes the seam);
    None elsewhere"""
    import torch.distributed as dist
    got = [None] * world if rank == 0 else None
    dist.gather_object(part, got, dst=0 if group is None else dist.get_global_rank(group, 0), group=group)
    return merged(got, nx, ny, nz, connectivity, labels, ring) if rank == 0 else None
