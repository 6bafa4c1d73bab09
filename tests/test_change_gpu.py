"""The steady-state monitor on the device (lbmpm_rk3d_change / lbmpm_rk3dcsf_change, csrc/rk3d_change.h) against a numpy restatement
(change_ref.restate) from the fields the solvers already hand out, at the mark and at the call.

Counts and the two maxima (columns 0, 1, 2, 8, 9, 10) are equal exactly: the terms are the same doubles (the library is built with
-ffp-contract=off) and the maximum of identical doubles knows no order.  A sum column (3 .. 7) is within 2 (n - 1) 2^-53 sum|term| per
plane, n the plane's fluid cells: the worst-case distance between two orders of summation of the same rounded terms, as
tests/test_integrals_gpu.py derives it.  The lattice is that test's 70 x 33 x 12 box: 2310 cells per plane = two whole chunks of the
reducer and a ragged third, nx no multiple of 64, a plane with five fluid cells, a row without any.
"""
import numpy as np
import pytest

from change_ref import EXACT, compare, restate
from test_integrals_gpu import CSF_PAR, _box, _fields, _pert, _with_one_nan
from test_rk3d_csf_gpu import _slab_case

pytestmark = pytest.mark.gpu

FLIP_STEPS = 50


@pytest.fixture(scope="module")
def box():
    return _box()


def _snapshot_bytes(dom):
    return 32 * dom.size


def _reducer_bytes(dom):
    """chunk partials + the table of the change reducer: [planes][chunks + 1][11] doubles"""
    nz, ny, nx = dom.shape
    return 8 * nz * ((ny * nx + 1023) // 1024 + 1) * 11


# ---------------------------------------------------------------------------------------------- 1. perturbation model vs its fields
@pytest.mark.parametrize("relax", ["MRT", "SRT"])
def test_perturbation_model_against_its_fields(box, relax):
    dom, rR, rB = box
    s = _pert(dom, relax)
    s.set_density(rR, rB)
    s.phase_field(diagnostics=True)
    old = _fields(s)
    s.mark_change()
    s.step_single(7)
    s.phase_field(diagnostics=True)
    g = s.change()
    assert g.steps == 7 and g.nx == 70 and g.ny == 33 and g.planes.shape == (12, 11)
    T = compare(g.planes, dom, _fields(s), old, "rk3d %s" % relax)
    assert T[5, 0] == 5 and g.nonfinite == 0 and g.total("du2_R") + g.total("du2_B") > 0 and g.velocity_change() > 0
    s.close()


# ---------------------------------------------------------------------------------------------- 2. CSF model vs the rec_* fields
@pytest.mark.parametrize("over", [{}, dict(outlet="Convective")], ids=["default", "convective-outlet"])
def test_csf_model_against_its_record_fields(box, over):
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    dom, rR, rB = box
    s = RK3DCSFSolver(dom, dict(CSF_PAR, **over))
    s.set_macro(rR, rB)
    f0 = _fields(s, "rec_")
    s.mark_change()                     # before the first step: the FIRST instance of the loader
    s.step(5)
    f5 = _fields(s, "rec_")
    g = s.change(remark=True)
    assert g.steps == 5
    compare(g.planes, dom, f5, f0, "csf %s 0 -> 5" % sorted(over))
    s.step(3)
    f8 = _fields(s, "rec_")
    g = s.change()
    assert g.steps == 3                 # against step 5: the call before re-marked
    compare(g.planes, dom, f8, f5, "csf %s 5 -> 8" % sorted(over))
    assert g.velocity_change() > 0 and g.nonfinite == 0
    s.step(2)
    a, b = s.change(remark=False), s.change(remark=False)
    assert a.steps == b.steps == 2 and np.array_equal(a.planes, b.planes)          # the same call twice: the same bits
    compare(a.planes, dom, _fields(s, "rec_"), f8, "csf %s 8 -> 10" % sorted(over))
    s.close()


# ---------------------------------------------------------------------------------------------- 3. nothing in between
def test_no_steps_between_mark_and_change(box):
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    dom, rR, rB = box
    s = _pert(dom)
    s.set_density(rR, rB); s.step_single(3); s.phase_field(diagnostics=True)
    s.mark_change()
    c = RK3DCSFSolver(dom, CSF_PAR)
    c.set_macro(rR, rB); c.step(3)
    c.mark_change()
    for g, f, what in ((s.change(), _fields(s), "rk3d"), (c.change(), _fields(c, "rec_"), "csf")):
        assert g.steps == 0 and not g.is_steady(1.0), what
        for col in (2, 5, 6, 7, 8, 9):
            assert np.array_equal(g.planes[:, col], np.zeros(12)), (what, col)
        compare(g.planes, dom, f, f, what)
        assert g.total("u2_R") + g.total("u2_B") > 0 and g.velocity_change() == 0.0, what
    s.close(); c.close()


# ---------------------------------------------------------------------------------------------- 4. the interface moves
def test_cells_that_change_colour_are_counted(box):
    """50 steps: the smallest multiple of 50 at which the CPU oracle (oracle/rk3dcsf.py, the box with CSF_PAR) has cells whose phi
    changed sign against the initial state -- 458 of them"""
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    dom, rR, rB = box
    s = RK3DCSFSolver(dom, CSF_PAR)
    s.set_macro(rR, rB)
    p0 = s.get("rec_phi")
    s.mark_change()
    s.step(FLIP_STEPS)
    g = s.change()
    p1 = s.get("rec_phi")
    want = np.array([(((p1[z] > 0) != (p0[z] > 0)) & (dom[z] == 1)).sum() for z in range(dom.shape[0])], dtype=np.float64)
    assert want.sum() > 0
    assert np.array_equal(g.column("flipped"), want) and g.flipped == int(want.sum()) and g.steps == FLIP_STEPS
    assert 0 < g.flipped_fraction < 1 and g.max_dphi > 0
    s.close()


# ---------------------------------------------------------------------------------------------- 5. cut-independence, bit for bit
def test_csf_slabs_give_the_bits_of_the_undivided_lattice():
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster, RK3DCSFSolver
    dom, rR, rB = _slab_case()
    a = RK3DCSFSolver(dom, CSF_PAR)
    a.set_macro(rR, rB); a.mark_change(); a.step(6)
    ref = a.change()
    a.close()
    assert ref.total("du2_R") > 0
    for kw in (dict(nslabs=4), dict(cuts=[0, 9, 23, 44])):
        c = RK3DCSFCluster(dom, CSF_PAR, **kw)
        c.set_macro(rR, rB); c.mark_change(); c.step(6)
        got = c.change()
        assert got.steps == 6 and got.planes.shape == ref.planes.shape and np.array_equal(got.planes, ref.planes), kw
        c.close()


def test_perturbation_slabs_give_the_bits_of_the_undivided_lattice(box):
    from openlbmpm_amd.rk3d import RK3DCluster
    dom, rR, rB = box
    s = _pert(dom, "MRT")
    s.set_density(rR, rB); s.phase_field(diagnostics=True); s.mark_change()
    s.step_single(6); s.phase_field(diagnostics=True)
    ref = s.change()
    s.close()
    assert ref.total("du2_R") > 0
    for k in (2, 3):
        c = RK3DCluster(dom, k, dict(relax="MRT", tauB=0.8))
        c.set_density(rR, rB)
        c.mark_change()                          # (stale: observes first)
        c.step(6)
        got = c.change()
        assert got.steps == 6 and np.array_equal(got.planes, ref.planes), k
        c.close()


# ---------------------------------------------------------------------------------------------- 6. bad cells
def _check_marked_nan(g, dom, hole, now, old, what):
    """g: the table against a snapshot whose cell of _with_one_nan is NaN, no step in between"""
    compare(g.planes, dom, now, old, what)
    T, _ = restate(hole, now, old)               # the lattice without that cell ...
    T[4, 0] += 1; T[4, 10] += 1                  # ... and the cell in CELLS and NONFINITE, nowhere else
    for c in EXACT:
        assert np.array_equal(g.planes[:, c], T[:, c]), (what, c)
    assert g.nonfinite == 1 and np.all(np.isfinite(g.planes)), what


def test_a_bad_cell_in_the_marked_state_csf():
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    dom, rR, rB = _slab_case()
    bad, hole = _with_one_nan(dom, rR)
    s = RK3DCSFSolver(dom, CSF_PAR)
    s.set_macro(bad, rB)
    old = _fields(s, "rec_")
    s.mark_change()
    _check_marked_nan(s.change(remark=False), dom, hole, old, old, "csf, no step")
    s.step(2)
    g = s.change()
    T = compare(g.planes, dom, _fields(s, "rec_"), old, "csf, two steps")      # the cells the NaN has reached since: clean at the mark, bad now
    assert g.nonfinite > 1 and T[:, 10].sum() == g.nonfinite and np.all(np.isfinite(g.planes)) and not g.is_steady(1e300)
    s.close()


def test_a_bad_cell_in_the_marked_state_perturbation(box):
    dom, rR, rB = box
    bad, hole = _with_one_nan(dom, rR)
    s = _pert(dom)
    s.set_density(bad, rB); s.phase_field(diagnostics=True)
    old = _fields(s)
    s.mark_change()
    _check_marked_nan(s.change(remark=False), dom, hole, old, old, "rk3d, no step")
    s.step_single(2); s.phase_field(diagnostics=True)
    g = s.change()
    compare(g.planes, dom, _fields(s), old, "rk3d, two steps")
    assert g.nonfinite > 1 and np.all(np.isfinite(g.planes))
    s.close()


def test_a_state_that_went_bad_after_a_clean_mark():
    """sigma = 50 overturns the CSF run within a few steps (the CPU oracle: every cell finite up to step 6, 594 cells not at step 7):
    the mark at step 0 is clean, the state at step 8 is not"""
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    dom, rR, rB = _slab_case()
    s = RK3DCSFSolver(dom, dict(CSF_PAR, sigma=50.0))
    s.set_macro(rR, rB)
    old = _fields(s, "rec_")
    assert all(np.all(np.isfinite(a)) for a in old.values())
    s.mark_change()
    assert s.change(remark=False).nonfinite == 0
    s.step(8)
    g = s.change()
    T = compare(g.planes, dom, _fields(s, "rec_"), old, "csf, went bad")
    assert g.nonfinite > 0 and T[:, 10].sum() == g.nonfinite and not g.is_steady(1e300)
    assert not np.any(np.isnan(g.planes))
    s.close()


# ---------------------------------------------------------------------------------------------- 7. refusals, memory
def test_refusals_perturbation(box):
    from openlbmpm_amd._lib import ERR_STATE, LbmpmError
    dom, rR, rB = box
    s = _pert(dom)
    s.set_density(rR, rB)
    for call in (s.mark_change, s.change):              # never observed
        with pytest.raises(LbmpmError) as e:
            call()
        assert e.value.status == ERR_STATE
    s.phase_field(diagnostics=True)
    before = s.device_bytes
    with pytest.raises(LbmpmError) as e:
        s.change()                                      # before a mark
    assert e.value.status == ERR_STATE and s.device_bytes == before
    s.mark_change()
    assert s.device_bytes - before == _snapshot_bytes(dom) + _reducer_bytes(dom)
    s.change(); s.mark_change()
    assert s.device_bytes - before == _snapshot_bytes(dom) + _reducer_bytes(dom)          # allocated once
    s.step_single(1)
    for call in (s.mark_change, s.change):              # stale diagnostics
        with pytest.raises(LbmpmError) as e:
            call()
        assert e.value.status == ERR_STATE and "stale" in str(e.value)
    s.phase_field(diagnostics=True)
    assert s.change().steps == 1
    s.set_density(rR, rB); s.phase_field(diagnostics=True)
    with pytest.raises(LbmpmError) as e:
        s.change()                                      # set_density voided the snapshot
    assert e.value.status == ERR_STATE
    s.mark_change()
    assert s.change().steps == 0
    s.close()


def test_refusals_csf(box):
    from openlbmpm_amd._lib import ERR_STATE, LbmpmError
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    dom, rR, rB = box
    s = RK3DCSFSolver(dom, CSF_PAR)
    for call in (s.mark_change, s.change):              # before set_macro / set_pdf
        with pytest.raises(LbmpmError) as e:
            call()
        assert e.value.status == ERR_STATE
    s.set_macro(rR, rB)
    s.integrals()
    before = s.device_bytes
    with pytest.raises(LbmpmError) as e:
        s.change()                                      # before a mark
    assert e.value.status == ERR_STATE and s.device_bytes == before
    s.mark_change()
    assert s.device_bytes - before == _snapshot_bytes(dom) + _reducer_bytes(dom)
    s.step(2)
    assert s.change().steps == 2 and s.device_bytes - before == _snapshot_bytes(dom) + _reducer_bytes(dom)
    s.set_macro(rR, rB)
    with pytest.raises(LbmpmError) as e:
        s.change()                                      # set_macro voided the snapshot
    assert e.value.status == ERR_STATE
    s.mark_change(); s.step(1)
    assert s.change().steps == 1
    s.close()
