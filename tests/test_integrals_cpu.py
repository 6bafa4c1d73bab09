"""openlbmpm_amd.integrals.Integrals on hand-made tables, and the declarations of the two C entry points: no GPU needed."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table():
    """[5][12]: plane 3 holds two cells that are not finite, plane 4 is all solid"""
    from openlbmpm_amd.integrals import COLUMNS
    t = np.zeros((5, len(COLUMNS)))
    #          cells cells_R mass_R mass_B flux_R  flux_B  uz_R   uz_B    mom_x  mom_y   umax2  nonfinite
    t[0] = [10., 4., 4.25, 6.5, 1e-3, -2e-3, 4e-3, -6e-3, 1e-4, -1e-4, 2.5e-5, 0.]
    t[1] = [12., 12., 12.1, 1e-7, 3e-3, 1e-9, 5e-3, 0., 2e-4, 3e-4, 9.0e-6, 0.]
    t[2] = [7., 0., 1e-7, 7.3, 1e-10, -4e-3, 0., -7e-3, -1e-4, 2e-4, 4.9e-5, 0.]
    t[3] = [9., 3., 3.3, 4.1, 2e-3, -1e-3, 3e-3, -4e-3, 5e-5, 6e-5, 1.6e-5, 2.]
    return t


def test_totals_and_derived_numbers():
    from openlbmpm_amd.integrals import COLUMNS, Integrals
    t = _table()
    g = Integrals(t, nx=6, ny=4)
    assert g.COLUMNS == COLUMNS and len(COLUMNS) == 12 and g.planes.shape == (5, 12) and g.nz == 5
    tot = g.totals
    for c, name in enumerate(COLUMNS):
        if name == "umax2":
            assert tot[c] == 4.9e-5                                  # the maximum, not a sum
        else:
            want = 0.0
            for z in range(5):
                want += t[z, c]
            assert tot[c] == want, name
    assert np.array_equal(g.column("mass_B"), t[:, 3])
    # two of the 38 fluid cells are not finite: they are not part of the saturation's denominator
    assert g.nonfinite == 2 and g.total("cells") == 38.0
    assert g.saturation_R == 19.0 / 36.0
    assert g.mass_R == tot[2] and g.mass_B == tot[3] and g.mass_fraction_R == tot[2] / (tot[2] + tot[3])
    assert g.flux_R == tot[4] / 5 and g.flux_B == tot[5] / 5                 # means over the planes
    assert g.darcy_uz_R == tot[6] / (6 * 4 * 5) and g.darcy_uz_B == tot[7] / (6 * 4 * 5)      # the whole volume, solid included
    assert g.max_speed == float(np.sqrt(4.9e-5))
    s = g.summary()
    assert set(s) == {"saturationR", "massR", "massB", "maxSpeed"} and s["massR"] == g.mass_R
    with pytest.raises(TypeError):
        Integrals(np.zeros((5, 11)), 6, 4)


def test_totals_of_concatenated_pieces_are_the_same_bits():
    """the planes are added in plane order by one fixed loop: a table assembled from the slabs' pieces gives the totals of the whole one"""
    from openlbmpm_amd.integrals import Integrals
    rng = np.random.default_rng(11)
    t = rng.standard_normal((37, 12)) * 10.0 ** rng.integers(-12, 6, size=(37, 12))
    t[:, 10] = np.abs(t[:, 10])
    whole = Integrals(t, 9, 7).totals
    for cut in (1, 5, 18, 36):
        pieces = Integrals(np.concatenate([t[:cut].copy(), t[cut:].copy()], axis=0), 9, 7).totals
        assert np.array_equal(whole, pieces), cut
    three = Integrals(np.concatenate([t[:9], t[9:23], t[23:]], axis=0), 9, 7).totals
    assert np.array_equal(whole, three)
    assert whole[10] == t[:, 10].max()


def test_column_names_round_trip_through_their_bytes():
    from openlbmpm_amd.integrals import COLUMNS, column_bytes, column_names
    b = column_bytes()
    assert b.dtype == np.uint8 and b.shape == (12, 9)
    assert column_names(b) == COLUMNS


def test_the_header_declares_both_functions_and_the_columns():
    from openlbmpm_amd import _lib
    from openlbmpm_amd.integrals import COLUMNS
    text = open(os.path.join(ROOT, "include", "lbmpm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+lbmpm_rk3d_integrals\s*\(\s*lbmpm_rk3d\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+lbmpm_rk3dcsf_integrals\s*\(\s*lbmpm_rk3dcsf\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*\)\s*;", text)
    m = re.search(r"#define\s+LBMPM_INTEGRAL_COLS\s+(\d+)", text)
    assert m and int(m.group(1)) == len(COLUMNS)
    # the enum names the columns in the order of COLUMNS
    body = re.search(r"enum\s*\{\s*(LBMPM_INT_CELLS\b.*?)\}", text, flags=re.S).group(1)
    names = [n.strip().split("=")[0].strip() for n in body.split(",") if n.strip()]
    assert [n[len("LBMPM_INT_"):].lower() for n in names] == [c.lower() for c in COLUMNS]
    assert "lbmpm_rk3d_integrals" in _lib._SIGNATURES and "lbmpm_rk3dcsf_integrals" in _lib._SIGNATURES


def test_the_reduction_kernels_run_from_registers_and_lds_alone():
    """what the compiler made of csrc/rk3d_integrals.h, read from the built library: both loaders' instances of stage 1 (the CSF model's
    for the first and for the later steps) and stage 2, no scratch memory, the 4 x 12 doubles of the cross-wave step in LDS"""
    lib = os.path.join(ROOT, "openlbmpm_amd", "liblbmpm_hip.so")
    if not os.path.exists(lib):
        import __graft_entry__
        __graft_entry__.build()
    from openlbmpm_amd import codeobj
    k = {n: m for n, m in codeobj.kernels(lib).items() if "integrals_partial" in n or "integrals_final" in n}
    assert sum("integrals_partial" in n for n in k) == 3 and sum("integrals_final" in n for n in k) == 1, sorted(k)
    for n, m in k.items():
        assert m[".private_segment_fixed_size"] == 0 and m[".vgpr_spill_count"] == 0, n
        assert m[".group_segment_fixed_size"] == (4 * 12 * 8 if "integrals_partial" in n else 0), n
