"""Phase morphology without a GPU: `cpu_morphology`, a numpy restatement of the definition in include/lbmpm.h that the GPU tests compare
the device's table with (tests/test_morphology_gpu.py), held to known answers here -- balls, a shell, a torus, a bar through the wrap,
a checkerboard; the join across slab cuts on the CPU; every derived number of openlbmpm_amd.morphology.Morphology from a hand-written
table; and the new kernels' code-object metadata (no scratch)."""
import os
import warnings

import numpy as np
import pytest

from openlbmpm_amd.morphology import COLUMNS, Morphology

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, R, B, N = 0, 1, 2, 3
C = {c: i for i, c in enumerate(COLUMNS)}


def cpu_morphology(cls, rho, above=None):
    """[nz][28] from the classes cls [nz][ny][nx] (0 S, 1 R, 2 B, 3 N) and rho = rho_R + rho_B [nz][ny][nx]; above: the class plane
    [ny][nx] over the highest plane, None: none.  Elements are anchored at their lowest corner; x and y wrap (np.roll), z is a shift."""
    cls = np.asarray(cls).astype(np.int64)
    nz = cls.shape[0]
    up = np.full(cls.shape[1:], 4, dtype=np.int64) if above is None else np.asarray(above).astype(np.int64)
    ext = np.concatenate([cls, up[None]], axis=0)                         # [nz + 1]: the plane above belongs to no anchor
    per_plane = lambda m: m[:nz].reshape(nz, -1).sum(axis=1)
    T = np.zeros((nz, len(COLUMNS)))
    for k, name in ((R, "cells_R"), (B, "cells_B"), (N, "cells_N")):
        T[:, C[name]] = per_plane(cls == k)
    for z in range(nz):
        T[z, C["rho_R"]] = np.asarray(rho)[z][cls[z] == R].sum()
        T[z, C["rho_B"]] = np.asarray(rho)[z][cls[z] == B].sum()
    nb = dict(x=np.roll(ext, -1, axis=2), y=np.roll(ext, -1, axis=1), z=np.concatenate([ext[1:], np.full((1,) + ext.shape[1:], 4)], axis=0))
    for a in "xyz":
        p, q = ext, nb[a]
        both = lambda u, v: ((p == u) & (q == v)) | ((p == v) & (q == u))
        for name, (u, v) in dict(RR=(R, R), BB=(B, B), RB=(R, B), RS=(R, S), BS=(B, S)).items():
            T[:, C["%s_%s" % (name, a)]] = per_plane(both(u, v))
    for k, ph in ((R, "R"), (B, "B")):
        m = ext == k
        mx, my = m & np.roll(m, -1, axis=2), m & np.roll(m, -1, axis=1)
        xy = mx & np.roll(mx, -1, axis=1)
        over = lambda t: t & np.concatenate([t[1:], np.zeros((1,) + t.shape[1:], dtype=bool)], axis=0)
        T[:, C["sq_%s_xy" % ph]] = per_plane(xy)
        T[:, C["sq_%s_xz" % ph]] = per_plane(over(mx))
        T[:, C["sq_%s_yz" % ph]] = per_plane(over(my))
        T[:, C["cube_" + ph]] = per_plane(over(xy))
    return T


def _grid(n=40, centre=19.5):
    z, y, x = np.mgrid[0:n, 0:n, 0:n]
    return z - centre, y - centre, x - centre


def _of(red):
    """Morphology of a two-phase field without solid: R where `red`, B elsewhere"""
    cls = np.where(red, R, B)
    return Morphology(cpu_morphology(cls, np.ones(cls.shape)), cls.shape[2], cls.shape[1])


# ---------------------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("r", [6, 10, 15])
def test_a_ball(r):
    z, y, x = _grid()
    red = x * x + y * y + z * z <= r * r
    m = _of(red)
    assert m.euler("R") == 1 and m.cells("R") == int(red.sum())
    for a, axis in (("x", 2), ("y", 1), ("z", 0)):
        assert m.faces("RB", a) == 2 * int(red.any(axis=axis).sum())           # convex: a column enters and leaves once
    ratio = m.area("RB") / (4.0 * np.pi * r * r)
    print("r = %d: 2/3 faces / (4 pi r^2) = %.4f, faces / area = %.4f" % (r, ratio, 1.5 * ratio))
    assert abs(ratio - 1.0) < 0.02
    assert m.specific_area("RB") == m.area("RB") / 40 ** 3


def test_a_ball_complement_is_consistent():
    """the lattice wraps in x and y and is open in z: all of it has cells - pairs + squares - cubes
    = n^3 - (2 n^3 + n^2 (n - 1)) + (n^3 + 2 n^2 (n - 1)) - n^2 (n - 1) = 0, a torus times an interval; a ball taken out of it is a cavity, + 1"""
    z, y, x = _grid()
    full = _of(np.ones((40, 40, 40), dtype=bool))
    assert full.euler("R") == 0
    m = _of(x * x + y * y + z * z <= 100)
    assert m.euler("B") == 1 and m.euler("R") == 1


def test_a_hollow_shell_a_torus_and_a_bar_through_the_wrap():
    z, y, x = _grid()
    r2 = x * x + y * y + z * z
    assert _of((r2 > 25) & (r2 <= 100)).euler("R") == 2
    assert _of((np.sqrt(x * x + y * y) - 10.0) ** 2 + z * z <= 16.0).euler("R") == 0
    bar = (np.abs(y) < 5) & (np.abs(z) < 5)                  # 10 x 10 cells, every x: closes through the x wrap
    assert int(bar[:, :, 0].sum()) == 100
    m = _of(bar)
    assert m.euler("R") == 0 and m.faces("RB", "x") == 0


def test_a_checkerboard():
    z, y, x = np.mgrid[0:40, 0:40, 0:40]
    m = _of((x + y + z) % 2 == 0)
    assert m.euler("R") == m.cells("R") == 32000 and m.euler("B") == m.cells("B") == 32000
    assert sum(m.column("RR_" + a).sum() + m.column("BB_" + a).sum() for a in "xyz") == 0
    assert m.faces("RB") == 2 * 40 ** 3 + 40 * 40 * 39


@pytest.mark.parametrize("classes", [(S, R, B), (S, R, B, N)])
def test_every_anchor_has_one_pair_per_axis(classes):
    rng = np.random.default_rng(3)
    cls = rng.choice(classes, size=(7, 6, 9))
    T = cpu_morphology(cls, np.ones(cls.shape))
    for a, axis in (("x", 2), ("y", 1), ("z", 0)):
        q = np.roll(cls, -1, axis=axis)
        valid = np.ones(cls.shape, dtype=bool)
        if a == "z":
            valid[-1] = False                                 # z does not wrap
        with_n = int((((cls == N) | (q == N)) & valid).sum())
        ss = int(((cls == S) & (q == S) & valid).sum())
        counted = sum(T[:, C["%s_%s" % (p, a)]].sum() for p in ("RR", "BB", "RB", "RS", "BS"))
        assert counted + with_n + ss == int(valid.sum()), a
    if N not in classes:
        assert T[:, C["cells_N"]].sum() == 0


def test_small_extents_are_taken_literally():
    """nx = 1: the +x neighbour of a cell is the cell itself -- one pair (c, c) per anchor and axis, as the definition says"""
    cls = np.full((3, 2, 1), R)
    T = cpu_morphology(cls, np.ones(cls.shape))
    assert np.array_equal(T[:, C["RR_x"]], [2, 2, 2]) and np.array_equal(T[:, C["sq_R_xy"]], [2, 2, 2]) and np.array_equal(T[:, C["cube_R"]], [2, 2, 0])


# ---------------------------------------------------------------------------------------------- slabs
@pytest.mark.parametrize("cuts", [[0, 10, 11], [0, 3, 4, 11], [0, 2, 5, 6, 9, 11]], ids=["2", "3", "5"])
def test_slabs_stack_to_the_undivided_table(cuts):
    """every slab gets the lowest plane of the slab over it as `above`; one slab of every cutting owns a single plane"""
    rng = np.random.default_rng(8)
    cls = rng.choice((S, R, B, N), size=(11, 5, 6), p=(0.2, 0.35, 0.35, 0.1))
    rho = rng.random(cls.shape) + 0.5
    whole = cpu_morphology(cls, rho)
    assert any(b - a == 1 for a, b in zip(cuts[:-1], cuts[1:]))
    parts = [cpu_morphology(cls[a:b], rho[a:b], cls[b] if b < cls.shape[0] else None) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate(parts, axis=0), whole)
    alone = np.concatenate([cpu_morphology(cls[a:b], rho[a:b]) for a, b in zip(cuts[:-1], cuts[1:])], axis=0)
    assert not np.array_equal(alone, whole)                   # without `above` the cut planes lose what reaches upwards


# ---------------------------------------------------------------------------------------------- the Morphology class
def test_derived_numbers_from_a_hand_written_table():
    t = np.zeros((3, 28))
    row = dict(cells_R=10, cells_B=20, cells_N=3, rho_R=11.0, rho_B=19.0, RR_x=4, RR_y=3, RR_z=2, BB_x=9, BB_y=8, BB_z=7, RB_x=5, RB_y=4, RB_z=3,
               RS_x=2, RS_y=1, RS_z=0, BS_x=6, BS_y=5, BS_z=4, sq_R_xy=2, sq_R_xz=1, sq_R_yz=1, sq_B_xy=5, sq_B_xz=4, sq_B_yz=3, cube_R=1, cube_B=2)
    assert set(row) == set(COLUMNS)
    for k, v in row.items():
        t[0, C[k]] = v
    t[1, C["cells_B"]], t[1, C["rho_B"]], t[1, C["BB_x"]] = 5, 6.0, 2          # a plane without R cells; plane 2: no fluid at all
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m = Morphology(t, 7, 5)
        assert m.nz == 3 and m.COLUMNS == COLUMNS and len(COLUMNS) == 28 and np.array_equal(m.column("RB_y"), [4, 0, 0])
        assert m.cells("R") == 10 and m.cells("B") == 25 and m.cells("N") == 3
        assert m.faces("RB") == 12 and m.faces("RB", "y") == 4 and m.faces("RS") == 3 and m.faces("BS", "z") == 4 and m.faces("BS") == 15
        assert m.area("RB") == 8.0 and m.area("RS") == 2.0
        assert m.specific_area("RB") == 8.0 / (7 * 5 * 3)
        assert m.wetted_fraction("R") == 3 / 18 and m.wetted_fraction("B") == 15 / 18
        assert m.euler("R") == 10 - 9 + 4 - 1 and m.euler("B") == 25 - 26 + 12 - 2
        assert m.mean_density("R") == 1.1 and m.mean_density("B") == 1.0
        assert m.capillary_pressure() == (1.1 - 1.0) / 3.0 and m.capillary_pressure(cs2=0.5) == 0.5 * (1.1 - 1.0)
        s = m.summary()
        assert s["areaRB"] == 8.0 and s["eulerR"] == 4 and s["eulerB"] == 9 and s["wettedR"] == 3 / 18 and s["capillaryPressure"] == m.capillary_pressure()
        # nothing of a phase: NaN, not a division by zero
        e = Morphology(t[1:], 7, 5)
        assert e.cells("R") == 0 and np.isnan(e.mean_density("R")) and np.isnan(e.capillary_pressure()) and np.isnan(e.wetted_fraction("R"))
        assert e.euler("R") == 0 and e.area("RB") == 0.0 and e.mean_density("B") == 1.2
        assert np.isnan(Morphology(t[2:], 7, 5).mean_density("B"))
    for bad in (lambda: m.faces("RR"), lambda: m.faces("RB", "w"), lambda: m.euler("N"), lambda: m.cells("S")):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        Morphology(np.zeros((3, 12)), 7, 5)


def test_columns_are_the_headers_enum():
    """COLUMNS in the order of LBMPM_MO_* and LBMPM_MORPH_COLS of include/lbmpm.h; column_bytes reads back"""
    import re
    from openlbmpm_amd.integrals import column_names
    from openlbmpm_amd.morphology import column_bytes
    text = open(os.path.join(ROOT, "include", "lbmpm.h")).read()
    body = re.search(r"enum \{ (LBMPM_MO_CELLS_R = 0.*?) \};", text, flags=re.S).group(1)
    names = [n.strip().split(" ")[0][len("LBMPM_MO_"):] for n in body.split(",")]
    assert [n.lower() for n in names] == [c.lower() for c in COLUMNS]
    assert "#define LBMPM_MORPH_COLS 28" in text
    assert column_names(column_bytes()) == COLUMNS


# ---------------------------------------------------------------------------------------------- the code object
def test_the_morphology_kernels_use_no_scratch_memory():
    """28 accumulators per thread and the flow loader's state: classify, the reducer's two stages, for both models' loaders -- from
    registers and LDS alone (the metadata of the built library, as tests/test_codeobj.py reads it)"""
    lib = os.path.join(ROOT, "openlbmpm_amd", "liblbmpm_hip.so")
    if not os.path.exists(lib):
        import __graft_entry__
        __graft_entry__.build()
    from openlbmpm_amd import codeobj
    k = {n: m for n, m in codeobj.kernels(lib).items() if "morphology_" in n}
    # classify and partial: the perturbation model's loader and the CSF model's <FIRST>; one final
    assert sum("morphology_classify" in n for n in k) == 3 and sum("morphology_partial" in n for n in k) == 3 and sum("morphology_final" in n for n in k) == 1, sorted(k)
    for n, m in k.items():
        assert m[".private_segment_fixed_size"] == 0 and m[".vgpr_spill_count"] == 0, (n, m)
