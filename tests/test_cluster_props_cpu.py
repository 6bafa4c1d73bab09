"""Per-cluster properties without a GPU: the NumPy reference (tests/cluster_props_ref.py) on shapes whose answers are counted by hand and
written out here, clusters.merge_props against it (a lattice reduced slab by slab and joined must give the undivided table, bit for bit),
and the accessors of clusters.Clusters on a hand-written property table.  Integers throughout: every comparison of a table is
array_equal.
"""
import numpy as np
import pytest

import cluster_props_ref as ref
from cluster_props_ref import B, N, R, S
from openlbmpm_amd import clusters as cl
from openlbmpm_amd.clusters import Clusters, merge_props, merge_slabs
from test_clusters_cpu import _patterns, cpu_label


def labelled(cls, conn=6, z0=0):
    """(labels, table) of the R and B cells of a four-class field"""
    return cpu_label(np.where((cls == R) | (cls == B), cls, 0).astype(np.uint8), conn, z0)


def row(cls, label, conn=6, **kw):
    lab, _ = labelled(cls, conn)
    t = ref.props(cls, lab, **kw)
    (r,) = t[t[:, ref.LABEL] == label]
    return {name: int(v) for name, v in zip(cl.PROP_COLUMNS, r)}


def chi(r):
    return r["cells"] - r["pairs"] + r["squares"] - r["cubes"]


# ------------------------------------------------------------------------------------------------ known answers
def test_the_columns_are_the_headers():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "lbmpm.h")).read()
    names = re.search(r"enum \{ (LBMPM_CP_LABEL = 0.*?) \};", text, re.S).group(1)
    names = [n.strip().split(" ")[0][len("LBMPM_CP_"):].lower() for n in names.split(",")]
    assert tuple(names) == cl.PROP_COLUMNS and len(cl.PROP_COLUMNS) == ref.COLS == 14
    assert "#define LBMPM_CLUSTER_PROP_COLS 14" in text
    assert re.search(r"#define LBMPM_CP_MASS_BITS\s+24\b", text) and re.search(r"#define LBMPM_CP_MOM_BITS\s+30\b", text)
    assert (cl.MASS_BITS, cl.MOM_BITS) == (ref.MASS_BITS, ref.MOM_BITS) == (24, 30)
    assert (cl.P_FACES_FLUID, cl.P_SUM_Z, cl.P_MASS, cl.P_MOM_Z, cl.P_CLIPPED) == (ref.FACES_FLUID, ref.SUM_Z, ref.MASS, ref.MOM_Z, ref.CLIPPED)


def test_a_single_cell():
    c = np.full((3, 3, 3), B, dtype=np.uint8)
    c[1, 1, 1] = R
    r = row(c, 13)
    assert r == dict(label=13, cells=1, faces_fluid=6, faces_solid=0, pairs=0, squares=0, cubes=0, sum_z=1, mass=0, mom_x=0, mom_y=0,
                     mom_z=0, clipped=0, **{"class": R})
    assert chi(r) == 1
    # the B around it: 26 cells, six faces towards the R cell, no element lost but those through the cell
    b = row(c, 0)
    assert b["class"] == B and b["cells"] == 26 and b["faces_fluid"] == 6
    # in the lowest plane nothing is below: five faces; with a plane below, six again; a solid plane below wets it
    c[:] = B
    c[0, 1, 1] = R
    assert row(c, 4)["faces_fluid"] == 5 and row(c, 4)["sum_z"] == 0
    assert row(c, 4, below=np.full((3, 3), B))["faces_fluid"] == 6
    wet = row(c, 4, below=np.full((3, 3), S))
    assert wet["faces_fluid"] == 5 and wet["faces_solid"] == 1
    # N neighbours are neither
    c[:] = N
    c[1, 1, 1] = B
    assert row(c, 13)["faces_fluid"] == 0 and row(c, 13)["faces_solid"] == 0 and row(c, 13)["class"] == B


def test_a_cube_of_eight():
    c = np.full((4, 4, 4), N, dtype=np.uint8)
    c[1:3, 1:3, 1:3] = R
    r = row(c, 21)
    assert (r["cells"], r["pairs"], r["squares"], r["cubes"]) == (8, 12, 6, 1) and chi(r) == 1
    assert r["faces_fluid"] == 0 and r["sum_z"] == 4 * 1 + 4 * 2
    c[c == N] = B
    assert row(c, 21)["faces_fluid"] == 24
    # the cube on top of the lattice with the slab above given: the elements that reach up are the anchor's
    top = np.full((2, 4, 4), N, dtype=np.uint8)
    top[1, 1:3, 1:3] = R
    above = np.full((4, 4), N, dtype=np.uint8)
    above[1:3, 1:3] = R
    r = row(top, 21, above=above)
    assert (r["cells"], r["pairs"], r["squares"], r["cubes"]) == (4, 4 + 4, 1 + 4, 1)
    r = row(top, 21)
    assert (r["cells"], r["pairs"], r["squares"], r["cubes"]) == (4, 4, 1, 0)


def test_a_ring_of_eight():
    c = np.full((3, 5, 5), B, dtype=np.uint8)
    c[1, 1:4, 1:4] = R
    c[1, 2, 2] = B
    r = row(c, 25 + 6)
    assert (r["cells"], r["pairs"], r["squares"], r["cubes"]) == (8, 8, 0, 0) and chi(r) == 0
    assert r["faces_fluid"] == 16 + 12 + 4              # above and below, the outer rim, the hole


def test_a_plate_on_solid():
    c = np.zeros((3, 3, 4), dtype=np.uint8)
    c[0], c[1], c[2] = S, R, B
    r = row(c, 12)
    assert r["cells"] == 12 and r["faces_solid"] == 12 and r["faces_fluid"] == 12
    assert (r["pairs"], r["squares"], r["cubes"]) == (24, 12, 0) and chi(r) == 0          # it closes through both wraps: a torus
    assert r["sum_z"] == 12


def test_the_wraps_are_literal_for_one_and_two_columns():
    c = np.full((3, 3, 1), R, dtype=np.uint8)            # nx = 1: the cell at x + 1 is the cell itself
    r = row(c, 0)
    assert r["cells"] == 9 and r["faces_fluid"] == 0
    assert (r["pairs"], r["squares"], r["cubes"]) == (9 + 9 + 6, 9 + 6 + 6, 6)
    c = np.array([[[R, B]]], dtype=np.uint8)             # nx = 2, ny = nz = 1: x + 1 and x - 1 are the same cell, each direction counts once
    r = row(c, 0)
    assert r["faces_fluid"] == 2 and (r["pairs"], r["squares"]) == (1, 0)          # the pair along y is the cell with itself
    assert row(c, 1)["faces_fluid"] == 2 and row(c, 1)["class"] == B


def test_fixed_point_sums_and_clipping():
    c = np.full((2, 2, 3), R, dtype=np.uint8)
    rR = np.full(c.shape, 0.75); rB = np.full(c.shape, 0.25 + 2.0 ** -26)       # rho = 1 + 2^-26: a quarter of a quantum, rounded away
    ux = np.full(c.shape, 2.0 ** -31); uy = np.full(c.shape, 3 * 2.0 ** -31); uz = np.full(c.shape, -0.5)       # ties to even: 0 and 2
    r = row(c, 0, rhoR=rR, rhoB=rB, ux=ux, uy=uy, uz=uz)
    assert r["mass"] == 12 << 24 and r["mom_x"] == 12 * 1 and r["mom_y"] == 12 * 2 and r["mom_z"] == -12 * (1 << 29) - 12 * 8
    assert r["clipped"] == 0
    for name, value in (("rhoR", 100.0), ("rhoR", np.nan), ("rhoB", np.inf), ("ux", np.nan), ("uy", 1.5), ("uz", -np.inf), ("rhoR", 63.5)):
        kw = dict(rhoR=rR, rhoB=rB, ux=ux, uy=uy, uz=uz)
        kw[name] = kw[name].copy()
        kw[name][1, 1, 2] = value                        # not finite, |rho| >= 64, or a |p| >= 1
        q = row(c, 0, **kw)
        assert q["clipped"] == 1 and q["cells"] == 12 and q["mass"] == 11 << 24 and q["mom_y"] == 11 * 2, (name, value, q)
    kw = dict(rhoR=rR.copy(), rhoB=rB, ux=ux, uy=uy, uz=uz)
    kw["rhoR"][1, 1, 2] = 62.0                           # rho = 62.25 is in range, p_z = -31.1 is not
    assert row(c, 0, **kw)["clipped"] == 1
    kw["uz"] = np.full(c.shape, -0.01)                   # p_z = -0.62: counted
    assert row(c, 0, **kw)["clipped"] == 0


# ------------------------------------------------------------------------------------------------ merge_props
def _fields(shape, seed):
    rng = np.random.default_rng(seed)
    rR, rB = rng.random(shape), rng.random(shape)
    u = [0.1 * (rng.random(shape) - 0.5) for _ in range(3)]
    rR[rng.random(shape) < 0.02] = 100.0                 # some clipped cells
    u[1][rng.random(shape) < 0.02] = np.nan
    return dict(rhoR=rR, rhoB=rB, ux=u[0], uy=u[1], uz=u[2])


def by_slabs(cls, conn, cuts, fields):
    nz, ny, nx = cls.shape
    tabs, fl, fc, parts = [], [], [], []
    for z0, z1 in zip(cuts[:-1], cuts[1:]):
        lab, tab = labelled(cls[z0:z1], conn, z0)
        tabs.append(tab)
        fl.append(np.stack([lab[0], lab[-1]]))
        fc.append(np.stack([np.where(lab[0] != ref.NONE, cls[z0], 0), np.where(lab[-1] != ref.NONE, cls[z1 - 1], 0)]))
        parts.append(ref.props(cls[z0:z1], lab, below=cls[z0 - 1] if z0 else None, above=cls[z1] if z1 < nz else None, z0=z0,
                               **{k: v[z0:z1] for k, v in fields.items()}))
        assert np.array_equal(parts[-1][:, :3], tab[:, :3])
    table, mapping = merge_slabs(tabs, fl, fc, nx, ny, conn)
    return table, merge_props(parts, mapping)


def _cases():
    out = {}
    for name, (c, conn) in _patterns().items():
        if name.startswith("random"):
            continue
        out[name] = (np.where(c == 0, np.where(np.random.default_rng(5).random(c.shape) < 0.3, S, N), c).astype(np.uint8), conn)
    r = np.random.default_rng(9).integers(0, 4, size=(12, 6, 8)).astype(np.uint8)
    out["random_6"], out["random_18"] = (r, 6), (r, 18)
    two = np.where(np.random.default_rng(10).random((12, 6, 8)) < 0.55, R, B).astype(np.uint8)       # large clusters through every cut
    out["two_phase_6"], out["two_phase_18"] = (two, 6), (two, 18)
    return out


@pytest.mark.parametrize("name", sorted(_cases()))
def test_merge_props_equals_the_undivided_table(name):
    cls, conn = _cases()[name]
    nz = cls.shape[0]
    fields = _fields(cls.shape, 21)
    lab, tab = labelled(cls, conn)
    want = ref.props(cls, lab, **fields)
    assert np.array_equal(want[:, :3], tab[:, :3])
    cuts = [[0, a, nz] for a in range(1, nz)] + [[0, a, b, nz] for a in range(1, nz) for b in range(a + 1, nz)]
    for cut in cuts:
        table, got = by_slabs(cls, conn, cut, fields)
        assert np.array_equal(table, tab), (name, cut)
        assert got.dtype == np.int64 and np.array_equal(got, want), (name, cut)


def test_the_cases_hold_what_they_claim():
    c = _cases()
    u, _ = c["u_shape"]                                   # the U crosses the cuts at 4 and 8 with both arms
    lab, _ = labelled(u)
    assert lab[3, 2, 1] == lab[5, 2, 5] == lab[9, 2, 3] != ref.NONE
    d, conn = c["diagonal_across_the_cut"]                # joined by diagonal links alone: one cluster under 18, ten under 6
    assert conn == 18 and labelled(d, 18)[1].shape[0] == 1 and labelled(d, 6)[1].shape[0] == 10
    t = ref.props(d, labelled(d, 18)[0])
    assert t[0, ref.CELLS] == 10 and t[0, ref.PAIRS] == 0 and t[0, ref.CELLS] - t[0, ref.PAIRS] == 10      # chi_6 counts its face-connected pieces
    with pytest.raises(ValueError):
        merge_props([t], np.array([[1, 1]]))


# ------------------------------------------------------------------------------------------------ Clusters
def test_accessors_on_a_hand_written_table():
    #        label class cells zmin zmax     (nz = 10: outlet plane 1, inlet plane 8)
    t = [[3, 1, 50, 0, 9],
         [40, 2, 8, 1, 4],
         [90, 1, 4, 3, 5],
         [200, 2, 12, 4, 6]]
    q24, q30 = 1 << 24, 1 << 30
    #    label class cells ff  fs  pairs sq cubes sum_z  mass       mom_x     mom_y  mom_z      clipped
    p = [[3, 1, 50, 30, 9, 100, 60, 10, 225, 50 * q24, 0, 0, -q30 // 2, 0],
         [40, 2, 8, 24, 0, 12, 6, 1, 20, 7 * q24, q30 // 4, 0, 0, 1],
         [90, 1, 4, 18, 3, 4, 0, 0, 16, 0, 0, 0, 0, 4],
         [200, 2, 12, 36, 6, 12, 0, 0, 60, 24 * q24, 0, 3 * q30 // 1000, 4 * q30 // 1000, 0]]
    c = Clusters(t, 4, 5, 10, props=p)
    assert c.props.dtype == np.int64 and c.props.shape == (4, 14)
    assert np.array_equal(c.interfacial_area(), [20.0, 16.0, 12.0, 24.0]) and np.array_equal(c.interfacial_area("B"), [16.0, 24.0])
    assert np.array_equal(c.wetted_area(), [6.0, 0.0, 2.0, 4.0])
    assert np.array_equal(c.euler(), [0, 1, 0, 0]) and c.euler().dtype == np.int64 and np.array_equal(c.euler("R"), [0, 0])
    assert np.array_equal(c.centre_z(), [4.5, 2.5, 4.0, 5.0])
    assert np.array_equal(c.mass(), [50.0, 7.0, 0.0, 24.0]) and np.array_equal(c.clipped("B"), [1, 0])
    assert np.array_equal(c.mean_density()[[0, 1, 3]], [1.0, 1.0, 2.0]) and np.isnan(c.mean_density()[2])
    assert np.array_equal(c.momentum()[:2], [[0, 0, -0.5], [0.25, 0, 0]])
    v = c.velocity()
    assert np.array_equal(v[0], [0, 0, -0.01]) and np.array_equal(v[1], [0.25 / 7, 0, 0]) and np.all(np.isnan(v[2]))
    assert np.allclose(v[3], [0, 0.003 / 24, 0.004 / 24], rtol=0, atol=2.0 ** -30)
    g = c.ganglia("B")
    assert g.dtype == Clusters.GANGLION and np.array_equal(g["label"], [200]) and np.array_equal(g["volume"], [12])
    assert g["area"][0] == 24.0 and g["wetted_area"][0] == 4.0 and g["euler"][0] == 0 and g["centre_z"][0] == 5.0
    assert np.array_equal(g["velocity"][0], v[3])
    assert np.array_equal(c.ganglia("R")["label"], [90]) and c.ganglia("B", z_lo=0, z_hi=9).shape[0] == 2
    assert c.mobile_cells("B", 1e-4) == 12 and c.mobile_cells("B", 3e-4) == 0 and c.mobile_cells("R", 0.0) == 0       # NaN moves nowhere
    assert c.mobile_cells("B", 1e-4, z_lo=0, z_hi=9) == 20
    s = c.summary()
    assert s["ganglia_R"] == 1 and s["ganglia_B"] == 1 and s["mobile_B"] == 1 and s["mobile_R"] == 0
    assert c.summary(speed=1e-3)["mobile_B"] == 0
    with pytest.raises(ValueError):
        Clusters(t, 4, 5, 10, props=p[:3])
    bad = [list(r) for r in p]
    bad[1][2] = 9
    with pytest.raises(ValueError):
        Clusters(t, 4, 5, 10, props=bad)
    e = Clusters(np.zeros((0, 5)), 4, 5, 10, props=np.zeros((0, 14)))
    assert e.ganglia("R").shape == (0,) and e.velocity().shape == (0, 3) and e.summary()["mobile_R"] == 0


def test_without_props_everything_is_as_before():
    t = [[3, 1, 50, 0, 9], [40, 2, 7, 1, 4], [90, 1, 5, 3, 5]]
    c = Clusters(t, 4, 5, 10)
    assert c.props is None
    assert c.summary() == dict(clusters_R=2, largest_R=50, percolates_R=True, trapped_R=5, clusters_B=1, largest_B=7, percolates_B=False, trapped_B=0)
    assert list(c.summary()) == ["clusters_R", "largest_R", "percolates_R", "trapped_R", "clusters_B", "largest_B", "percolates_B", "trapped_B"]
    for call in (c.interfacial_area, c.euler, c.velocity, lambda: c.ganglia("R"), lambda: c.mobile_cells("R", 0.0)):
        with pytest.raises(ValueError):
            call()
    assert cl.prop_column_bytes().shape[0] == 14 and bytes(cl.prop_column_bytes()[3]).rstrip(b"\0") == b"faces_fluid"
    assert cl.column_bytes().shape[0] == 5
