"""The seam of a lattice that is periodic in z, closed on the host (clusters.close_seam, Clusters under wrap_z) -- no GPU, no library.

The reference is a search over the cells themselves (`search` below): it walks every cluster of the ring cell by cell and carries an
unwrapped plane number along -- + 1 per step up, - 1 per step down, whatever seam the step crosses.  A cell that is reached a second
time with another number closes a loop round the ring; the gcd of those differences over nz is the winding.  A cluster without one has
the extent min .. max of the numbers, moved by whole periods to 0 <= zmin < nz.  It shares nothing with close_seam, which never looks
at a cell off the two face planes.  Integers throughout: every comparison is exact.
"""
from functools import lru_cache
from math import gcd

import numpy as np
import pytest

import cluster_props_ref as ref
import periodic_ref as PR
from openlbmpm_amd.clusters import CELLS, CLASS, NONE, P_SUM_Z, ZMAX, ZMIN, Clusters, close_seam, relabel
from test_clusters_cpu import HALF, by_slabs, classify, cpu_label
from test_clusters_gpu import SHARP
from test_morphology_cpu import cpu_morphology

PATTERNS = (PR.SEAM,) + SHARP
CASES = [(name, cut, conn) for name in PATTERNS for cut in (0.0, 0.3) for conn in (6, 18)]
NZ = PR.RING_SHAPE[0]


# ------------------------------------------------------------------------------------------------ the reference
def search(cls, conn):
    """(table [m][5], winding [m], sum_z [m], labels [nz][ny][nx] uint32) of the class field on a ring, by a walk over the cells"""
    cls = np.asarray(cls, dtype=np.uint8)
    nz, ny, nx = cls.shape
    plane = ny * nx
    idx = np.arange(cls.size, dtype=np.int64).reshape(cls.shape)
    src, dst, dzs = [], [], []
    for dx, dy, dz in [o for h in HALF[conn] for o in (h, tuple(-c for c in h))]:
        nc, ni = np.roll(cls, (-dz, -dy, -dx), axis=(0, 1, 2)), np.roll(idx, (-dz, -dy, -dx), axis=(0, 1, 2))
        m = (cls != 0) & (cls == nc)
        src.append(idx[m]); dst.append(ni[m]); dzs.append(np.full(int(m.sum()), dz, dtype=np.int64))
    src, dst, dzs = np.concatenate(src), np.concatenate(dst), np.concatenate(dzs)
    order = np.argsort(src, kind="stable")
    first = np.searchsorted(src[order], np.arange(cls.size + 1)).tolist()
    dst, dzs = dst[order].tolist(), dzs[order].tolist()
    flat = cls.reshape(-1).tolist()
    u = [None] * cls.size
    labels = np.full(cls.size, NONE, dtype=np.uint32)
    rows, winding, sums = [], [], []
    for c in range(cls.size):                 # ascending: the first cell of a cluster that the loop meets is its smallest, the label
        if not flat[c] or u[c] is not None:
            continue
        u[c], todo, members, g = c // plane, [c], [c], 0
        while todo:
            a = todo.pop()
            for e in range(first[a], first[a + 1]):
                b, v = dst[e], u[a] + dzs[e]
                if u[b] is None:
                    u[b] = v
                    todo.append(b); members.append(b)
                elif u[b] != v:
                    g = gcd(g, abs(u[b] - v))
        labels[members] = c
        assert g % nz == 0
        if g:
            rows.append([c, flat[c], len(members), 0, nz - 1])
            sums.append(sum(m // plane for m in members))
        else:
            us = [u[m] for m in members]
            shift = min(us) // nz
            rows.append([c, flat[c], len(members), min(us) - shift * nz, max(us) - shift * nz])
            sums.append(sum(us) - shift * nz * len(us))
        winding.append(g // nz)
    return (np.array(rows, dtype=np.int64).reshape(-1, 5), np.array(winding, dtype=np.int64).reshape(-1), np.array(sums, dtype=np.int64).reshape(-1),
            labels.reshape(cls.shape))


@lru_cache(maxsize=None)
def _ring_classes(name, cut):
    """the classes of a pattern on the ring box; cut > 0: of the pattern's phase field averaged over a cell and its six neighbours, so
    that there is a band to cut out"""
    dom = PR.ring_box()
    rR, rB = PR.ring_densities(name, dom)
    phi = np.where(dom == 1, (rR - rB) / np.maximum(rR + rB, 1e-300), 0.0)
    if cut:
        phi = (phi + sum(np.roll(phi, s, axis=a) for a in range(3) for s in (1, -1))) / 7.0
    cls = classify(phi, dom, cut)
    cls.setflags(write=False)
    return dom, cls


@lru_cache(maxsize=None)
def _searched(name, cut, conn):
    return search(_ring_classes(name, cut)[1], conn)


def closed(cls, conn, props=None, cuts=None):
    """close_seam on the CPU labelling of a class field: (table, winding, mapping, props, labels)"""
    nz, ny, nx = cls.shape
    lab, tab = cpu_label(cls, conn) if cuts is None else by_slabs(cls, conn, cuts)
    t, w, mapping, p = close_seam(tab, np.stack([lab[0], lab[-1]]), np.stack([cls[0], cls[-1]]), nx, ny, nz, conn, props)
    return t, w, mapping, p, relabel(lab, mapping)


def _fields(shape):
    """densities and a velocity that differ from cell to cell; some cells clipped (not finite, out of the fixed-point range)"""
    z, y, x = np.mgrid[0:shape[0], 0:shape[1], 0:shape[2]]
    f = dict(rhoR=0.6 + 0.3 * np.sin(0.7 * x + 0.3 * y + z), rhoB=0.5 + 0.2 * np.cos(0.4 * x - 0.9 * y + 2.0 * z),
             ux=1e-3 * np.sin(0.2 * x + z), uy=2e-3 * np.cos(0.5 * y + 0.3 * z), uz=1e-3 * np.sin(0.1 * x + 0.6 * y - z))
    f["rhoR"][0, 15, 35] = np.nan
    f["ux"][11, 17, 36] = 2.0
    return f


def open_props(dom, cls, lab, fields):
    """what the device reduces for the open clusters with the ring's own face planes beside the lattice"""
    cf = ref.class_field(dom, cls)
    return cf, ref.props(cf, lab, below=cf[-1], above=cf[0], **fields)


# ------------------------------------------------------------------------------------------------ 1. against the search
@pytest.mark.parametrize("name,cut,conn", CASES)
def test_close_seam_against_a_search_over_the_cells(name, cut, conn):
    cls = _ring_classes(name, cut)[1]
    table, winding, _, labels = _searched(name, cut, conn)
    t, w, mapping, p, lab = closed(cls, conn)
    assert t.dtype == np.int64 and w.dtype == np.int64 and p is None
    assert t.shape == table.shape and np.array_equal(t, table), (name, cut, conn)
    assert np.array_equal(w, winding), (name, cut, conn)
    assert lab.dtype == np.uint32 and np.array_equal(lab, labels)
    assert mapping.shape == (cpu_label(cls, conn)[1].shape[0], 2) and np.array_equal(np.unique(mapping[:, 1]), t[:, 0])


def test_the_cases_hold_what_the_comparison_is_about():
    """the reference alone: clusters that wind, ganglia across the seam (zmax >= nz), a band at the cut, fewer rows than the open table"""
    winds = across = 0
    for name, cut, conn in CASES:
        table, winding, _, _ = _searched(name, cut, conn)
        winds += int(np.count_nonzero(winding))
        across += int(np.count_nonzero((winding == 0) & (table[:, ZMAX] >= NZ)))
        assert np.all((table[:, ZMIN] >= 0) & (table[:, ZMIN] < NZ))
    assert winds > 0 and across > 0
    table, winding, _, _ = _searched(PR.SEAM, 0.0, 6)
    assert table.shape[0] == 2 and cpu_label(_ring_classes(PR.SEAM, 0.0)[1], 6)[1].shape[0] == 3
    red = table[table[:, CLASS] == 1]
    assert red.shape[0] == 1 and tuple(red[0, 2:]) == (360, 9, 14) and winding[table[:, CLASS] == 1][0] == 0 and winding[table[:, CLASS] == 2][0] == 1
    for name in PATTERNS:
        if name != "one_phase":
            dom, cls = _ring_classes(name, 0.3)
            assert int(((cls == 0) & (dom == 1)).sum()) > 0, name


# ------------------------------------------------------------------------------------------------ 2. a winding of 2
def helix():
    """[4][3][16]: two red strands in row y = 1 that climb two cells in x per plane; after one turn of z each meets the other"""
    cls = np.full((4, 3, 16), 2, dtype=np.uint8)
    for z in range(4):
        for x0 in (2 * z, 8 + 2 * z):
            cls[z, 1, [(x0 + i) % 16 for i in range(3)]] = 1
    return cls


@pytest.mark.parametrize("conn", [6, 18])
@pytest.mark.parametrize("k", range(4))
def test_a_double_helix_has_winding_two(conn, k):
    cls = np.roll(helix(), k, axis=0)
    t, w, _, _, lab = closed(cls, conn)
    assert t.shape[0] == 2
    red, blue = t[:, CLASS] == 1, t[:, CLASS] == 2
    assert tuple(t[red][0, 2:]) == (24, 0, 3) and w[red][0] == 2
    assert tuple(t[blue][0, 2:]) == (4 * 3 * 16 - 24, 0, 3) and w[blue][0] == 1
    table, winding, _, labels = search(cls, conn)
    assert np.array_equal(table, t) and np.array_equal(winding, w) and np.array_equal(labels, lab)


# ------------------------------------------------------------------------------------------------ 3. rolls
ELEMENTS = [ref.FACES_FLUID, ref.FACES_SOLID, ref.PAIRS, ref.SQUARES, ref.CUBES, ref.MASS, ref.MOM_X, ref.MOM_Y, ref.MOM_Z, ref.CLIPPED]


def multiset(t, w, p=None, k=0, nz=NZ):
    """the rows as sorted tuples of what a roll by k planes keeps: class, cells, extent, winding; with props also the columns that do
    not name a plane, and the centre -- sum_z moved by k planes, mod nz cells (an integer form of centre_z mod nz) -- for winding 0"""
    rows = np.stack([t[:, CLASS], t[:, CELLS], t[:, ZMAX] - t[:, ZMIN] + 1, w], axis=1)
    if p is not None:
        centre = np.where(w == 0, np.mod(p[:, P_SUM_Z] + k * p[:, CELLS], nz * p[:, CELLS]), -1)
        rows = np.concatenate([rows, p[:, ELEMENTS], centre[:, None]], axis=1)
    return sorted(map(tuple, rows.tolist()))


@pytest.mark.parametrize("conn", [6, 18])
@pytest.mark.parametrize("name", [PR.SEAM, "serpentine", "random"])
def test_rolled_classes_give_the_same_clusters(name, conn):
    dom, cls = _ring_classes(name, 0.0)
    fields = _fields(cls.shape)
    lab, tab = cpu_label(cls, conn)
    t, w, _, p, _ = closed(cls, conn, open_props(dom, cls, lab, fields)[1])
    open_base = multiset(tab, np.zeros(tab.shape[0], dtype=np.int64))
    open_moves = False
    for k in PR.ROLLS:
        roll = lambda a: np.roll(a, k, axis=0)
        rdom, rcls = roll(dom), roll(cls)
        rlab, rtab = cpu_label(rcls, conn)
        rt, rw, _, rp, _ = closed(rcls, conn, open_props(rdom, rcls, rlab, {n: roll(a) for n, a in fields.items()})[1])
        assert multiset(rt, rw, rp) == multiset(t, w, p, k), (name, conn, k)
        assert multiset(rt, rw) == multiset(t, w), (name, conn, k)
        open_moves = open_moves or multiset(rtab, np.zeros(rtab.shape[0], dtype=np.int64)) != open_base
        if name == PR.SEAM:                    # one red cluster: its centre through Clusters
            a, b = Clusters(t, 70, 33, NZ, props=p, winding=w, wrap_z=True), Clusters(rt, 70, 33, NZ, props=rp, winding=rw, wrap_z=True)
            assert abs(b.centre_z("R")[0] - (a.centre_z("R")[0] + k) % NZ) < 1e-12 and np.isnan(a.centre_z("B")[0])
    assert open_moves, "the open table is the same under every roll: the case shows nothing"


# ------------------------------------------------------------------------------------------------ 4. cuts
@pytest.mark.parametrize("conn", [6, 18])
@pytest.mark.parametrize("name", [PR.SEAM, "serpentine", "random"])
def test_slabs_joined_and_closed_give_the_undivided_closure(name, conn):
    cls = _ring_classes(name, 0.0)[1]
    t, w, _, _, lab = closed(cls, conn)
    for cuts in ((0, 12), (0, 6, 12), (0, 4, 8, 12), (0, 1, 5, 12)):
        st, sw, _, _, slab = closed(cls, conn, cuts=list(cuts))
        assert np.array_equal(st, t) and np.array_equal(sw, w) and np.array_equal(slab, lab), (name, conn, cuts)


# ------------------------------------------------------------------------------------------------ 5. props
@pytest.mark.parametrize("name,cut,conn", [(PR.SEAM, 0.0, 6), (PR.SEAM, 0.3, 18), ("serpentine", 0.0, 18), ("random", 0.0, 6), ("random", 0.3, 18)])
def test_the_merged_property_table(name, cut, conn):
    dom, cls = _ring_classes(name, cut)
    fields = _fields(cls.shape)
    lab, tab = cpu_label(cls, conn)
    cf, parts = open_props(dom, cls, lab, fields)
    t, w, _, p, closed_lab = closed(cls, conn, parts)
    want = ref.props(cf, closed_lab, below=cf[-1], above=cf[0], **fields)
    rest = [c for c in range(ref.COLS) if c != ref.SUM_Z]
    assert p.dtype == np.int64 and p.shape == want.shape and np.array_equal(p[:, rest], want[:, rest]), (name, cut, conn)
    assert np.array_equal(p[:, :3], t[:, :3])
    table, winding, sums, _ = _searched(name, cut, conn)
    assert np.array_equal(p[:, ref.SUM_Z], sums), (name, cut, conn)
    ring = winding != 0
    assert np.array_equal(p[ring, ref.SUM_Z], want[ring, ref.SUM_Z]) and np.any(p[~ring, ref.SUM_Z] != want[~ring, ref.SUM_Z])
    assert cut or p[:, ref.CLIPPED].sum() == 2            # (both bad cells lie in clusters)


# ------------------------------------------------------------------------------------------------ 6. Clusters
def test_clusters_under_wrap_z_on_a_hand_written_table():
    #        label class cells zmin zmax     (nz = 10)
    t = [[3, 1, 50, 0, 9],                 # R, winds
         [40, 2, 7, 1, 4],                 # B, a ganglion
         [90, 1, 6, 8, 11],                # R, a ganglion across the seam
         [120, 2, 30, 0, 9],               # B, winds twice
         [150, 1, 2, 6, 9]]                # R, a ganglion that touches the last plane
    w = [1, 0, 0, 2, 0]
    p = np.zeros((5, 14), dtype=np.int64)
    p[:, :3] = np.array(t)[:, :3]
    p[:, P_SUM_Z] = [225, 20, 6 * 10 + 3, 135, 15]        # the third: six cells, mean plane 10.5 -> 0.5 on the ring
    p[:, ref.MASS] = np.array(t)[:, 2] << 24
    c = Clusters(t, 4, 5, 10, props=p, winding=w, wrap_z=True)
    assert c.wrap_z and c.winding.dtype == np.int64
    assert np.array_equal(c.spanning("R"), [t[0]]) and np.array_equal(c.spanning("B"), [t[3]])
    assert c.percolates("R") and c.percolates("B")
    assert c.trapped_cells("R") == 8 and c.trapped_cells("B") == 7 and c.trapped_fraction("R") == 8 / 58
    g = c.ganglia("R")
    assert np.array_equal(g["label"], [90, 150]) and np.array_equal(g["volume"], [6, 2]) and np.array_equal(g["centre_z"], [0.5, 7.5])
    assert c.mobile_cells("R", 1e-9) == 0
    cz = c.centre_z()
    assert np.isnan(cz[0]) and np.isnan(cz[3]) and cz[1] == 20 / 7 and cz[2] == 0.5 and cz[4] == 7.5
    assert np.array_equal(c.extent(), [10, 4, 4, 10, 4]) and np.array_equal(c.extent("B"), [4, 10])
    s = c.summary()
    assert s["winding_R"] == 1 and s["winding_B"] == 2 and s["percolates_B"] is True and s["trapped_R"] == 8 and s["ganglia_R"] == 2
    with pytest.raises(ValueError):
        c.connected_cells("R")
    for call in (c.trapped_cells, c.trapped_fraction, c.ganglia, c.spanning, c.percolates):
        with pytest.raises(ValueError):
            call("R", z_lo=2)
    with pytest.raises(ValueError):
        c.mobile_cells("R", 1e-9, z_hi=7)
    with pytest.raises(ValueError):
        Clusters(t, 4, 5, 10, wrap_z=True)                 # no winding
    with pytest.raises(ValueError):
        Clusters(t, 4, 5, 10, winding=w[:3], wrap_z=True)
    none = Clusters(np.zeros((0, 5)), 4, 5, 10, winding=[], wrap_z=True)
    assert not none.percolates("R") and none.summary()["winding_R"] == 0
    # the same table without wrap_z: open planes 1 and 8, as ever -- whether a winding is attached or not
    for o in (Clusters(t, 4, 5, 10, props=p), Clusters(t, 4, 5, 10, props=p, winding=w)):
        assert not o.wrap_z and np.array_equal(o.spanning("R"), [t[0]]) and o.connected_cells("R", to="inlet") == 58
        assert o.trapped_cells("R") == 0 and o.trapped_cells("B") == 0 and o.trapped_cells("B", z_lo=0, z_hi=9) == 7
        assert np.array_equal(o.centre_z(), p[:, P_SUM_Z] / p[:, CELLS]) and "winding_R" not in o.summary()
        assert np.array_equal(o.extent(), [10, 4, 4, 10, 4])
    assert Clusters(t, 4, 5, 10).winding is None


# ------------------------------------------------------------------------------------------------ close_seam's own refusals and corners
def test_close_seam_corners():
    e = np.zeros((2, 3, 4), dtype=np.uint8)
    t, w, m, p = close_seam(np.zeros((0, 5)), np.full((2, 3, 4), NONE, dtype=np.uint32), e, 4, 3, 5, 6, np.zeros((0, 14)))
    assert t.shape == (0, 5) and w.shape == (0,) and m.shape == (0, 2) and p.shape == (0, 14)
    with pytest.raises(ValueError):
        close_seam(np.zeros((0, 5)), e, e, 4, 3, 5, 26)
    cls = np.zeros((5, 3, 4), dtype=np.uint8)
    cls[[0, 4], 1, 2] = 1                                  # one cell either side of the seam; another cluster in between
    cls[2, 1, 2] = 1
    lab, tab = cpu_label(cls, 6)
    with pytest.raises(ValueError):
        close_seam(tab[1:], np.stack([lab[0], lab[-1]]), np.stack([cls[0], cls[-1]]), 4, 3, 5)       # a face label without a row
    with pytest.raises(ValueError):
        close_seam(tab[::-1], np.stack([lab[0], lab[-1]]), np.stack([cls[0], cls[-1]]), 4, 3, 5)
    t, w, m, _ = close_seam(tab, np.stack([lab[0], lab[-1]]), np.stack([cls[0], cls[-1]]), 4, 3, 5)
    assert np.array_equal(t, [[6, 1, 2, 4, 5], [30, 1, 1, 2, 2]]) and np.array_equal(w, [0, 0]) and np.array_equal(m, [[6, 6], [30, 30], [54, 6]])


# ------------------------------------------------------------------------------------------------ 7. morphology
@pytest.mark.parametrize("name", PATTERNS)
def test_the_wrapped_morphology_rolls_with_the_lattice(name):
    """with plane 0 as the plane above plane nz - 1 no plane is an end: all 28 columns of all 12 rows roll with the classes, the two
    density sums bit for bit (a plane's cells are added in the same order wherever the plane lies)"""
    dom, cls = _ring_classes(name, 0.3)
    cf = ref.class_field(dom, cls)
    f = _fields(cls.shape)
    rho = np.where((cf == 1) | (cf == 2), np.nan_to_num(f["rhoR"] + f["rhoB"]), 0.0)
    base = cpu_morphology(cf, rho, above=cf[0])
    assert base.shape == (12, 28)
    for k in PR.ROLLS:
        rc = np.roll(cf, k, axis=0)
        assert np.array_equal(cpu_morphology(rc, np.roll(rho, k, axis=0), above=rc[0]), np.roll(base, k, axis=0)), (name, k)
    assert not np.array_equal(cpu_morphology(cf, rho)[11], base[11])          # (the open count: its last row misses what reaches upwards)
