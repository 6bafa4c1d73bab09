"""The steady-state monitor without a GPU: the arithmetic of change.Change on hand-written tables, the column order against the header,
the numpy restatement the GPU tests compare with against a three-cell example worked by hand, the driver's and the CLI's options."""
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _row(**kw):
    from openlbmpm_amd.change import COLUMNS
    r = [0.0] * len(COLUMNS)
    for k, v in kw.items():
        r[COLUMNS.index(k)] = float(v)
    return r


def test_columns_follow_the_enum_of_the_header():
    from openlbmpm_amd.change import COLUMNS
    text = open(os.path.join(ROOT, "include", "lbmpm.h")).read()
    assert re.search(r"#define\s+LBMPM_CHANGE_COLS\s+11\b", text)
    body = re.search(r"enum\s*\{\s*(LBMPM_CH_CELLS\s*=\s*0[^}]*)\}", text).group(1)
    names = [n.strip().split("=")[0].strip() for n in body.split(",")]
    assert [n[len("LBMPM_CH_"):].lower().replace("_r", "_R").replace("_b", "_B") for n in names] == list(COLUMNS)
    assert len(COLUMNS) == 11


def test_change_arithmetic_on_a_hand_written_table():
    from openlbmpm_amd.change import Change
    planes = [_row(cells=10, cells_R=4, flipped=1, u2_R=4.0, u2_B=12.0, du2_R=1.0, du2_B=3.0, dphi2=0.5, dumax2=0.25, dphimax=0.5),
              _row(cells=6, cells_R=6, flipped=2, u2_R=5.0, u2_B=0.0, du2_R=0.25, du2_B=0.0, dphi2=1.5, dumax2=0.09, dphimax=0.75)]
    c = Change(planes, 5, 2, 40)
    assert c.planes.shape == (2, 11) and c.nz == 2 and c.steps == 40 and (c.nx, c.ny) == (5, 2)
    assert np.array_equal(c.column("flipped"), [1.0, 2.0])
    assert c.total("cells") == 16 and c.total("du2_R") == 1.25
    assert c.total("dumax2") == 0.25 and c.total("dphimax") == 0.75            # the two maxima are joined by max
    assert c.velocity_change() == math.sqrt(4.25 / 21.0)
    assert c.velocity_change("R") == math.sqrt(1.25 / 9.0)
    assert c.velocity_change("B") == math.sqrt(3.0 / 12.0)
    assert c.phase_change() == math.sqrt(2.0 / 16.0)
    assert c.flipped == 3 and c.flipped_fraction == 3.0 / 16.0
    assert c.max_du == 0.5 and c.max_dphi == 0.75 and c.nonfinite == 0
    s = c.summary()
    assert s["steps"] == 40 and s["velocityChange"] == c.velocity_change() and s["phaseChange"] == c.phase_change() and s["flipped"] == 3
    assert c.is_steady(0.5) and not c.is_steady(0.4)                           # velocity 0.4499, phase 0.3536
    assert c.is_steady(0.45, phase_tol=0.36) and not c.is_steady(0.45, phase_tol=0.35)
    with pytest.raises(TypeError):
        Change(np.zeros((2, 12)), 5, 2, 1)
    with pytest.raises(ValueError):
        c.velocity_change("G")


def test_zero_and_infinite_ratios():
    from openlbmpm_amd.change import Change
    rest = Change([_row(cells=8, cells_R=8)], 4, 2, 10)                        # nothing moves, nothing moved
    assert rest.velocity_change() == 0.0 and rest.velocity_change("B") == 0.0 and rest.phase_change() == 0.0
    assert rest.is_steady(0.0)
    started = Change([_row(cells=8, u2_R=0.0, du2_R=1e-6, u2_B=2.0)], 4, 2, 10)      # the red phase has come to rest since the snapshot
    assert started.velocity_change("R") == float("inf") and started.velocity_change("B") == 0.0
    assert started.velocity_change() == math.sqrt(1e-6 / 2.0)
    assert not Change([_row(cells=8, du2_B=1e-6)], 4, 2, 10).is_steady(1e300)  # inf is within no tolerance
    assert math.isnan(Change([_row()], 4, 2, 10).flipped_fraction)


def test_is_steady_needs_steps_and_finite_cells():
    from openlbmpm_amd.change import Change
    quiet = _row(cells=8, cells_R=3, u2_R=1.0, u2_B=1.0)
    assert Change([quiet], 4, 2, 5).is_steady(1e-9)
    assert not Change([quiet], 4, 2, 0).is_steady(1e-9)                         # mark and change at the same step say nothing
    bad = Change([_row(cells=8, cells_R=3, u2_R=1.0, u2_B=1.0, nonfinite=1)], 4, 2, 5)
    assert bad.nonfinite == 1 and not bad.is_steady(1.0)
    assert bad.phase_change() == 0.0 and bad.flipped_fraction == 0.0           # (over the seven finite cells)


def test_column_bytes_round_trip():
    from openlbmpm_amd.change import COLUMNS, CRITERIA_COLUMNS, column_bytes, criteria_column_bytes
    from openlbmpm_amd.integrals import column_names
    assert column_names(column_bytes()) == COLUMNS and column_bytes().dtype == np.uint8 and column_bytes().shape[0] == 11
    assert column_names(criteria_column_bytes()) == CRITERIA_COLUMNS
    assert CRITERIA_COLUMNS == ("step", "steps_between", "velocity_change", "velocity_change_R", "velocity_change_B", "phase_change", "flipped", "max_du")


def test_restate_on_three_cells_worked_by_hand():
    """one plane, four cells of which one is solid.  Cell a: red, stays red; cell b: was blue, is red; cell c: blue, its old phi is NaN"""
    from change_ref import restate
    dom = np.array([[[1, 1, 0, 1]]], dtype=np.uint8)
    f = lambda *v: np.array([[list(v)]], dtype=np.float64)
    nan = float("nan")
    now = dict(rhoR=f(1, 1, 9, 0), rhoB=f(0, 0, 9, 1), vx=f(0.5, 0.0, 9, 1.0), vy=f(0.0, 0.25, 9, 1.0), vz=f(0.0, 0.0, 9, 1.0), phi=f(1.0, 0.5, 9, -1.0))
    old = dict(vx=f(0.25, 0.0, nan, 1.0), vy=f(0.0, 0.0, nan, 1.0), vz=f(0.0, -0.5, nan, 1.0), phi=f(0.5, -0.5, nan, nan))
    T, A = restate(dom, now, old)
    #        cells cells_R flipped u2_R                 u2_B du2_R                          du2_B dphi2        dumax2  dphimax nonfinite
    want = [3.0, 2.0, 1.0, 0.25 + 0.0625, 0.0, 0.0625 + (0.0625 + 0.25), 0.0, 0.25 + 1.0, 0.3125, 1.0, 1.0]
    assert T.shape == (1, 11) and T[0].tolist() == want
    assert A[0, 3] == 0.3125 and A[0, 5] == 0.375 and A[0, 7] == 1.25 and A[0, 4] == 0.0
    # the same cells with a bad current value instead: counted the same way
    now["rhoB"][0, 0, 3], old["phi"][0, 0, 3] = nan, -1.0
    assert restate(dom, now, old)[0][0].tolist() == want


def test_steady_tol_needs_steady_every(tmp_path):
    from ini_fixtures import write_rk3d
    from openlbmpm_amd import config
    from openlbmpm_amd.RKColorGradientD3Q19 import RKColorGradient3D
    write_rk3d(str(tmp_path), nx=16, ny=16, nz=32, steps=10)
    with pytest.raises(config.ConfigError):
        RKColorGradient3D(str(tmp_path), steady_tol=1e-3)
    sim = RKColorGradient3D(str(tmp_path), steady_every=5, steady_tol=1e-3, steady_phase_tol=0.5)
    assert (sim.steady_every, sim.steady_tol, sim.steady_phase_tol, sim.steady_step) == (5, 1e-3, 0.5, None)
    off = RKColorGradient3D(str(tmp_path))
    assert (off.steady_every, off.steady_tol, off.steady_phase_tol) == (0, 0.0, None)


def test_the_cli_takes_the_three_options():
    from openlbmpm_amd.__main__ import parser
    a = parser().parse_args(["rk3d", "somewhere", "--steady-every", "100", "--steady-tol", "1e-4", "--steady-phase-tol", "0.5"])
    assert (a.steady_every, a.steady_tol, a.steady_phase_tol) == (100, 1e-4, 0.5)
    a = parser().parse_args(["rk3d", "somewhere"])
    assert (a.steady_every, a.steady_tol, a.steady_phase_tol) == (0, 0.0, None)
