"""Phase clusters without a GPU: the CPU labeller the cluster tests compare the device with (a plain union-find over numpy arrays, kept
here and tested on patterns with known answers), clusters.merge_slabs against it (a lattice labelled slab by slab and joined must give
the undivided table and labels), and the derived numbers of clusters.Clusters on a hand-written table.  Integers throughout: every
comparison is array_equal.
"""
import numpy as np
import pytest

from openlbmpm_amd.clusters import NONE, Clusters, merge_slabs, relabel

# one of every pair of opposite neighbour offsets (dx, dy, dz), dz >= 0: the faces, then the other D3Q19 links
HALF = {6: ((1, 0, 0), (0, 1, 0), (0, 0, 1)),
        18: ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, -1, 0), (1, 0, 1), (-1, 0, 1), (0, 1, 1), (0, -1, 1))}


def classify(phi, dom, phi_cut=0.0):
    """the definition of include/lbmpm.h: 1 where phi > cut, 2 where phi <= -cut, 0 for solid, not finite, the band"""
    phi = np.asarray(phi, dtype=np.float64)
    fin = np.isfinite(phi) & (np.asarray(dom) == 1)
    safe = np.where(fin, phi, 0.0)
    return np.where(fin & (safe > phi_cut), 1, np.where(fin & (safe <= -phi_cut), 2, 0)).astype(np.uint8)


def cpu_label(cls, connectivity, z0=0):
    """cls: [nz][ny][nx] classes (0: in no cluster) of the planes z0 .. of a lattice; x and y wrap, z does not.  Returns (labels uint32
    [nz][ny][nx] -- the global number of the cluster's smallest cell, NONE where class 0 --, table int64 [n][5] by ascending label)"""
    cls = np.asarray(cls, dtype=np.uint8)
    nz, ny, nx = cls.shape
    idx = np.arange(cls.size, dtype=np.int64).reshape(cls.shape)
    pairs = []
    for dx, dy, dz in HALF[connectivity]:
        a_c, a_i = (cls[:nz - 1], idx[:nz - 1]) if dz else (cls, idx)
        b_c, b_i = (cls[1:], idx[1:]) if dz else (cls, idx)
        b_c, b_i = np.roll(b_c, (-dy, -dx), axis=(1, 2)), np.roll(b_i, (-dy, -dx), axis=(1, 2))
        m = (a_c != 0) & (a_c == b_c)
        pairs.append(np.stack([a_i[m], b_i[m]], axis=1))
    parent = list(range(cls.size))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for a, b in np.concatenate(pairs, axis=0).tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(i) for i in range(cls.size)], dtype=np.int64)
    flat = cls.reshape(-1)
    on = flat != 0
    base = z0 * ny * nx
    labels = np.where(on, root + base, NONE).astype(np.uint32).reshape(cls.shape)
    roots, inv, cells = np.unique(root[on], return_inverse=True, return_counts=True)
    z = (np.nonzero(on)[0] // (ny * nx)) + z0
    zmin = np.full(roots.size, np.iinfo(np.int64).max); zmax = np.full(roots.size, -1)
    np.minimum.at(zmin, inv, z); np.maximum.at(zmax, inv, z)
    table = np.stack([roots + base, flat[roots].astype(np.int64), cells.astype(np.int64), zmin, zmax], axis=1).astype(np.int64).reshape(-1, 5)
    return labels, table


def by_slabs(cls, connectivity, cuts):
    """label slab by slab with cpu_label and join with merge_slabs: (labels, table) of the whole lattice"""
    nz, ny, nx = cls.shape
    tabs, fl, fc, labs = [], [], [], []
    for z0, z1 in zip(cuts[:-1], cuts[1:]):
        lab, tab = cpu_label(cls[z0:z1], connectivity, z0)
        tabs.append(tab); labs.append(lab)
        fl.append(np.stack([lab[0], lab[-1]])); fc.append(np.stack([cls[z0], cls[z1 - 1]]))
    table, mapping = merge_slabs(tabs, fl, fc, nx, ny, connectivity)
    return relabel(np.concatenate(labs, axis=0), mapping), table


# ------------------------------------------------------------------------------------------------ the labeller itself
def test_labeller_on_hand_made_patterns():
    c = np.zeros((4, 4, 5), dtype=np.uint8)
    lab, tab = cpu_label(c, 6)
    assert tab.shape == (0, 5) and np.all(lab == NONE)
    c[:] = 1
    lab, tab = cpu_label(c, 6)
    assert np.array_equal(tab, [[0, 1, 80, 0, 3]]) and np.all(lab == 0)
    # two bars of R in plane 1, an isolated B cell in plane 2, the rest class 0
    c[:] = 0
    c[1, 0, 1:3] = 1
    c[1, 2, 0] = 1; c[1, 2, 4] = 1                    # joined through the x wrap
    c[2, 1, 3] = 2
    lab, tab = cpu_label(c, 6)
    assert np.array_equal(tab, [[21, 1, 2, 1, 1], [30, 1, 2, 1, 1], [48, 2, 1, 2, 2]])
    assert lab[1, 2, 4] == 30 and lab[1, 0, 2] == 21 and lab[2, 1, 3] == 48 and lab[0, 0, 0] == NONE
    # y wrap, and z does not wrap
    c[:] = 0
    c[0, 0, 2] = 1; c[0, 3, 2] = 1; c[3, 0, 2] = 1
    lab, tab = cpu_label(c, 6)
    assert np.array_equal(tab, [[2, 1, 2, 0, 0], [62, 1, 1, 3, 3]])
    # a diagonal link joins under 18 only; a body diagonal (not a D3Q19 link) never
    c[:] = 0
    c[1, 1, 1] = 2; c[2, 1, 2] = 2; c[3, 2, 3] = 2
    lab6, tab6 = cpu_label(c, 6)
    lab18, tab18 = cpu_label(c, 18)
    assert tab6.shape[0] == 3
    assert np.array_equal(tab18, [[26, 2, 2, 1, 2], [73, 2, 1, 3, 3]])
    # R next to B: never joined; the offset of a slab's first plane moves labels and planes
    c[:] = 1
    c[:, :, 2:] = 2
    lab, tab = cpu_label(c, 18, z0=5)
    assert np.array_equal(tab, [[100, 1, 32, 5, 8], [102, 2, 48, 5, 8]])


def test_labeller_checkerboard():
    z, y, x = np.mgrid[0:4, 0:4, 0:6]
    c = (1 + (x + y + z) % 2).astype(np.uint8)
    lab, tab = cpu_label(c, 6)
    assert tab.shape[0] == c.size and np.array_equal(lab.reshape(-1), np.arange(c.size))      # every cell is its own cluster
    lab, tab = cpu_label(c, 18)
    assert np.array_equal(tab[:, :3], [[0, 1, 48], [1, 2, 48]])                                # the in-plane diagonals join each colour


# ------------------------------------------------------------------------------------------------ merge_slabs
def _patterns():
    nz, ny, nx = 12, 6, 8
    out = {}
    u = np.zeros((nz, ny, nx), dtype=np.uint8)             # a U: both arms in the low planes, the bend at plane 9
    u[2:10, 2, 1] = 1; u[2:10, 2, 5] = 1; u[9, 2, 1:6] = 1
    u[3, 4, 3] = 2
    out["u_shape"] = (u, 6)
    w = np.zeros((nz, ny, nx), dtype=np.uint8)             # plane 6: a bar that closes through the x wrap only; arms down from both ends
    w[6, 3, 0:2] = 1; w[6, 3, 6:8] = 1
    w[3:6, 3, 1] = 1; w[3:6, 3, 6] = 1
    out["x_wrap_on_the_cut_plane"] = (w, 6)
    d = np.zeros((nz, ny, nx), dtype=np.uint8)             # one cell per plane, each a diagonal link from the last (the x wrap included)
    for z, x in enumerate([0, 7, 0, 7, 6, 5, 4, 3, 2, 1]):
        d[z + 1, 2, x] = 2
    out["diagonal_across_the_cut"] = (d, 18)
    out["diagonal_across_the_cut_6"] = (d, 6)
    yd = np.zeros((nz, ny, nx), dtype=np.uint8)            # the same along y, through the y wrap
    for z, y in enumerate([0, 5, 0, 1, 2, 3, 4, 5, 0, 5]):
        yd[z + 1, y, 4] = 1
    out["y_diagonal"] = (yd, 18)
    rng = np.random.default_rng(3)
    r = rng.integers(0, 3, size=(nz, ny, nx)).astype(np.uint8)
    out["random_6"] = (r, 6); out["random_18"] = (r, 18)
    return out


@pytest.mark.parametrize("name", sorted(_patterns()))
def test_merge_slabs_equals_the_undivided_labelling(name):
    cls, conn = _patterns()[name]
    lab, tab = cpu_label(cls, conn)
    for cuts in ([0, 12], [0, 6, 12], [0, 5, 12], [0, 7, 12], [0, 3, 6, 9, 12], [0, 1, 2, 10, 11, 12], list(range(13))):
        got_lab, got_tab = by_slabs(cls, conn, cuts)
        assert got_tab.dtype == np.int64 and np.array_equal(got_tab, tab), (name, cuts)
        assert got_lab.dtype == np.uint32 and np.array_equal(got_lab, lab), (name, cuts)


def test_the_patterns_are_what_they_claim():
    p = _patterns()
    u, _ = p["u_shape"]
    assert cpu_label(u[:6], 6)[1].shape[0] == 3 and cpu_label(u, 6)[1].shape[0] == 2          # two arms + B below the cut, one U in all
    w, _ = p["x_wrap_on_the_cut_plane"]
    assert cpu_label(w[:6], 6)[1].shape[0] == 2 and cpu_label(w, 6)[1].shape[0] == 1
    ww = w.copy(); ww[6, 3, 0] = 0                                                             # without the wrap's cell: two clusters
    assert cpu_label(ww, 6)[1].shape[0] == 2
    d, _ = p["diagonal_across_the_cut"]
    assert cpu_label(d, 18)[1].shape[0] == 1 and cpu_label(d, 6)[1].shape[0] == 10


def test_merge_slabs_refuses_what_it_cannot_join():
    cls, conn = _patterns()["u_shape"]
    lab, tab = cpu_label(cls[:6], conn, 0)
    faces, classes = np.stack([lab[0], lab[-1]]), np.stack([cls[0], cls[5]])
    with pytest.raises(ValueError):
        merge_slabs([tab, tab], [faces, faces], [classes, classes], 8, 6, conn)               # the same labels twice
    with pytest.raises(ValueError):
        merge_slabs([tab], [faces], [classes], 8, 6, 26)


# ------------------------------------------------------------------------------------------------ Clusters
def test_derived_numbers_on_a_hand_written_table():
    #        label class cells zmin zmax     (nz = 10: outlet plane 1, inlet plane 8)
    t = [[3, 1, 50, 0, 9],                 # R, spans
         [40, 2, 7, 1, 4],                 # B, touches the outlet
         [90, 1, 5, 3, 5],                 # R, trapped
         [120, 2, 30, 2, 8],               # B, touches the inlet
         [150, 1, 2, 6, 9],                # R, touches the inlet
         [200, 2, 11, 4, 6]]               # B, trapped
    c = Clusters(t, 4, 5, 10)
    assert c.table.dtype == np.int64 and c.table.shape == (6, 5)
    assert c.count("R") == 3 and c.count("B") == 3
    assert np.array_equal(c.sizes("R"), [50, 5, 2]) and np.array_equal(c.sizes("B"), [30, 11, 7])
    assert c.largest("R") == 50 and c.largest("B") == 30
    assert np.array_equal(c.spanning("R"), [t[0]]) and c.spanning("B").shape == (0, 5)
    assert c.percolates("R") and not c.percolates("B")
    assert c.percolates("B", z_lo=2, z_hi=8) and not c.percolates("B", z_lo=1, z_hi=8)
    assert c.connected_cells("R", to="inlet") == 52 and c.connected_cells("R", to="outlet") == 50
    assert c.connected_cells("B", to="inlet") == 30 and c.connected_cells("B", to="outlet") == 7
    assert c.trapped_cells("R") == 5 and c.trapped_cells("B") == 11
    assert c.trapped_fraction("R") == 5 / 57 and c.trapped_fraction("B") == 11 / 48
    s = c.summary()
    assert s["clusters_R"] == 3 and s["largest_B"] == 30 and s["percolates_R"] is True and s["trapped_B"] == 11
    with pytest.raises(ValueError):
        c.connected_cells("R", to="side")
    e = Clusters(np.zeros((0, 5)), 4, 5, 10)
    assert e.count("R") == 0 and e.largest("B") == 0 and not e.percolates("R") and np.isnan(e.trapped_fraction("R"))
