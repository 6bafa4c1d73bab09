"""integrals.TracerIntegrals on hand-made tables (no GPU): the totals in plane order, the extrema over the planes that have cells, the
moments of a known profile, the shape check, the column names of the result file; Transport3DRK keeps integrals_every."""
import numpy as np
import pytest

from openlbmpm_amd.integrals import TRACER_COLUMNS, TracerIntegrals, column_names, tracer_column_bytes

C = {c: i for i, c in enumerate(TRACER_COLUMNS)}


def _table(nz=5, nT=2):
    """plane 2 is empty (no fluid cell: cmin = cmax = 0 as the library reports it), plane 3 of tracer 1 holds one cell that is not finite
    and no other (the same)"""
    t = np.zeros((nz, nT, 9))
    for z in range(nz):
        for k in range(nT):
            sign = 1.0 if k == 0 else -1.0
            t[z, k] = [4, sign * (z + 1), 0.25 * z, -0.5 * z, sign * 0.125 * (z + 1), (z + 1) ** 2 / 4., sign * 0.2 * (z + 1) - 0.05, sign * 0.2 * (z + 1) + 0.05, 0]
    t[2] = 0.0
    t[3, 1] = [1, 0, 0, 0, 0, 0, 0, 0, 1]
    return t


def test_columns_and_shape():
    assert TRACER_COLUMNS == ("cells", "mass", "flux_x", "flux_y", "flux_z", "sum_c2", "cmin", "cmax", "nonfinite")
    assert TracerIntegrals.COLUMNS == TRACER_COLUMNS
    t = TracerIntegrals(_table(), 7, 3)
    assert (t.nz, t.num_tracers, t.nx, t.ny) == (5, 2, 7, 3) and t.planes.shape == (5, 2, 9) and t.totals.shape == (2, 9)
    assert np.array_equal(t.column("mass", 1), _table()[:, 1, 1])
    for bad in (np.zeros((5, 9)), np.zeros((5, 2, 12)), np.zeros((5, 2, 9, 1))):
        with pytest.raises(TypeError):
            TracerIntegrals(bad, 7, 3)
    b = tracer_column_bytes()
    assert b.dtype == np.uint8 and b.shape == (9, len("nonfinite")) and column_names(b) == TRACER_COLUMNS


def test_totals_are_added_in_plane_order():
    """values whose sum depends on the order: 1 + 2^-53 + 2^-53 is 1 from the left and 1 + 2^-52 from the right"""
    t = np.zeros((3, 1, 9))
    t[:, 0, C["cells"]] = 1
    t[:, 0, C["mass"]] = [1.0, 2.0 ** -53, 2.0 ** -53]
    t[:, 0, C["sum_c2"]] = [2.0 ** -53, 2.0 ** -53, 1.0]
    g = TracerIntegrals(t, 1, 1)
    assert g.mass(0) == 1.0 and g.total("sum_c2", 0) == 1.0 + 2.0 ** -52
    want = [0.0] * 9
    for row in _table()[:, 0].tolist():
        for c in (0, 1, 2, 3, 4, 5, 8):
            want[c] += row[c]
    got = TracerIntegrals(_table(), 7, 3).totals[0]
    assert all(got[c] == want[c] for c in (0, 1, 2, 3, 4, 5, 8))


def test_the_extrema_skip_the_planes_without_finite_cells():
    t = TracerIntegrals(_table(), 7, 3)
    # tracer 0: all positive -- the empty plane's 0 must not become the minimum; tracer 1: all negative -- nor the maximum
    assert t.cmin(0) == 0.2 - 0.05 and t.cmax(0) == 0.2 * 5 + 0.05
    assert t.cmax(1) == -0.2 + 0.05 and t.cmin(1) == -0.2 * 5 - 0.05          # (plane 3 of tracer 1 has no finite cell either)
    assert t.nonfinite == 1 and t.good_cells(1) == 4 * 3 and t.good_cells(0) == 4 * 4
    s = t.summary()
    assert list(s) == ["mass0", "cmin0", "cmax0", "mass1", "cmin1", "cmax1"] and s["mass0"] == t.mass(0) and s["cmax1"] == t.cmax(1)
    empty = TracerIntegrals(np.zeros((4, 1, 9)), 2, 2)
    assert empty.cmin(0) == 0.0 and empty.cmax(0) == 0.0 and np.isnan(empty.mean(0)) and np.isnan(empty.centre_z(0))


def test_mean_variance_and_the_moments_along_z():
    nz = 9
    t = np.zeros((nz, 1, 9))
    m = np.array([0, 0, 1, 4, 6, 4, 1, 0, 0], dtype=np.float64)              # binomial about z = 4: variance 1
    t[:, 0, C["cells"]] = 8
    t[:, 0, C["mass"]] = m
    t[:, 0, C["sum_c2"]] = m * m / 8. + 0.5                                   # per plane: 8 cells of m / 8 ... plus a spread
    t[:, 0, C["flux_z"]] = -0.5 * m
    g = TracerIntegrals(t, 4, 2)
    assert g.mass(0) == 16.0 and g.centre_z(0) == 4.0 and g.variance_z(0) == 1.0
    assert g.mean(0) == 16.0 / 72.0
    assert abs(g.variance(0) - ((m * m / 8. + 0.5).sum() / 72.0 - (16.0 / 72.0) ** 2)) < 1e-15
    assert g.flux_z_at(0, 3) == -2.0 and g.flux_z_at(0, 1) == 0.0
    assert "-flux_z_at(k, 1)" in TracerIntegrals.flux_z_at.__doc__
    # shifted by two planes the centre moves, the spread stays
    t2 = np.roll(t, 2, axis=0)
    g2 = TracerIntegrals(t2, 4, 2)
    assert g2.centre_z(0) == 6.0 and g2.variance_z(0) == 1.0


def test_the_driver_keeps_integrals_every(tmp_path):
    from openlbmpm_amd.Transport3DRK import Transport3DRK
    from test_tr3d_driver_gpu import write_ini
    write_ini(tmp_path, nx=14, ny=12, nz=40, steps=12)
    assert Transport3DRK(str(tmp_path), output_dir=str(tmp_path / "o"), integrals_every=5).integrals_every == 5
    assert Transport3DRK(str(tmp_path), output_dir=str(tmp_path / "o")).integrals_every == 0
