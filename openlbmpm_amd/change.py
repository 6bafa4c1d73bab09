"""Steady-state monitor of the 3-D solvers: the table of lbmpm_rk3d_change / lbmpm_rk3dcsf_change (include/lbmpm.h holds the definition)
and the criteria a run is stopped on -- how far the velocity and the phase field of the recorded state have moved since the snapshot a
mark_change() or the last change(remark=True) left on the device.

The library reduces every plane on the device in the plane integrals' fixed order, so a table is the same bit for bit however the
lattice was cut into slabs; `totals` keeps that: one loop over the planes in plane order.

Relation to the reference: ShanChenD2Q9.py:831-850 (__calSteadyStateCritiria, written and never called) takes
relativeError = sqrt(sum (|u| - |u0|)^2 / sum |u|^2) of the speeds against a stored record.  velocity_change() here is
sqrt(sum |u - u0|^2 / sum |u|^2) of the vectors.  Since | |u| - |u0| | <= |u - u0| in every cell, the reference's number never exceeds
velocity_change(): a tolerance met here is met there.
"""
import math

import numpy as np

# the columns, in the order of LBMPM_CH_* (csrc/rk3d_change.h is the only other place that knows it)
COLUMNS = ("cells", "cells_R", "flipped", "u2_R", "u2_B", "du2_R", "du2_B", "dphi2", "dumax2", "dphimax", "nonfinite")
_MAX = (COLUMNS.index("dumax2"), COLUMNS.index("dphimax"))
# /Steady/Criteria of a result file, one row per table
CRITERIA_COLUMNS = ("step", "steps_between", "velocity_change", "velocity_change_R", "velocity_change_B", "phase_change", "flipped", "max_du")


def _ratio(num, den):
    """sqrt(num / den); 0.0 when the numerator is 0, inf when only the denominator is"""
    if num == 0.0:
        return 0.0
    if den == 0.0:
        return float("inf")
    return math.sqrt(num / den)


class Change:
    """planes: [nz][11], one row per lattice plane over the plane's fluid cells, the recorded state now against the snapshot (a cell
    that is not finite in either counts in `cells` and `nonfinite` only); nx, ny: the plane's extent; steps: the time steps between
    the snapshot and now"""
    COLUMNS = COLUMNS

    def __init__(self, planes, nx, ny, steps):
        a = np.ascontiguousarray(planes, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != len(COLUMNS):
            raise TypeError("planes must have shape [nz][%d]" % len(COLUMNS))
        self.planes, self.nx, self.ny, self.steps = a, int(nx), int(ny), int(steps)
        self.nz = a.shape[0]
        self._totals = None

    def column(self, name):
        """the profile of one column along z"""
        return self.planes[:, COLUMNS.index(name)]

    @property
    def totals(self):
        """[11]: the planes added in plane order (the maximum for dumax2 and dphimax)"""
        if self._totals is None:
            t = [0.0] * len(COLUMNS)
            for row in self.planes.tolist():
                for c, v in enumerate(row):
                    t[c] = (v if v > t[c] else t[c]) if c in _MAX else t[c] + v
            self._totals = np.array(t, dtype=np.float64)
        return self._totals

    def total(self, name):
        return float(self.totals[COLUMNS.index(name)])

    def velocity_change(self, phase=None):
        """sqrt(sum |u - u0|^2 / sum |u|^2) over the cells that are red now ("R"), blue now ("B") or both (None): the relative L2 change
        of the velocity since the snapshot"""
        if phase not in (None, "R", "B"):
            raise ValueError("phase is None, 'R' or 'B'")
        ph = ("R", "B") if phase is None else (phase,)
        return _ratio(sum(self.total("du2_" + p) for p in ph), sum(self.total("u2_" + p) for p in ph))

    def phase_change(self):
        """sqrt(sum (phi - phi0)^2 / finite cells): the root mean square change of the phase field (phi is of order one already)"""
        return _ratio(self.total("dphi2"), self.total("cells") - self.total("nonfinite"))

    @property
    def flipped(self):
        """cells whose colour (phi > 0) is not the snapshot's"""
        return int(self.total("flipped"))

    @property
    def flipped_fraction(self):
        good = self.total("cells") - self.total("nonfinite")
        return self.total("flipped") / good if good else float("nan")

    @property
    def max_du(self):
        """the largest |u - u0| of a cell"""
        return math.sqrt(self.total("dumax2"))

    @property
    def max_dphi(self):
        return self.total("dphimax")

    @property
    def nonfinite(self):
        return int(self.total("nonfinite"))

    def is_steady(self, tol, phase_tol=None):
        """steps have been taken, every cell is finite, velocity_change() <= tol and phase_change() <= phase_tol (None: tol)"""
        return bool(self.steps > 0 and self.nonfinite == 0 and self.velocity_change() <= tol and
                    self.phase_change() <= (tol if phase_tol is None else phase_tol))

    def criteria(self, step):
        """the row of /Steady/Criteria (CRITERIA_COLUMNS) for the table taken at `step`"""
        return [float(step), float(self.steps), self.velocity_change(), self.velocity_change("R"), self.velocity_change("B"), self.phase_change(),
                float(self.flipped), self.max_du]

    def summary(self):
        """the numbers a log line carries"""
        return dict(steps=self.steps, velocityChange=self.velocity_change(), phaseChange=self.phase_change(), flipped=self.flipped, maxDu=self.max_du)


def column_bytes():
    """COLUMNS as a [11][width] uint8 array, zero-padded: /Steady/Columns of a result file (integrals.column_names reads it back)"""
    from .integrals import _name_bytes
    return _name_bytes(COLUMNS)


def criteria_column_bytes():
    """CRITERIA_COLUMNS the same way: /Steady/CriteriaColumns"""
    from .integrals import _name_bytes
    return _name_bytes(CRITERIA_COLUMNS)


def mark(L, prefix, handle):
    """the snapshot of one context through <prefix>_change_mark"""
    from ._lib import check
    name = prefix + "_change_mark"
    check(getattr(L, name)(handle), name)


def table(L, prefix, handle, planes, remark):
    """([planes][11], steps since the mark) of one context through <prefix>_change"""
    import ctypes as C
    from ._lib import F64P, check
    out = np.empty((int(planes), len(COLUMNS)), dtype=np.float64)
    steps = C.c_int64(0)
    name = prefix + "_change"
    check(getattr(L, name)(handle, 1 if remark else 0, C.byref(steps), out.ctypes.data_as(F64P)), name)
    return out, int(steps.value)


def stacked(slabs, remark):
    """([nz][11], steps) of slabs in plane order: every slab against its own snapshot (they step together: one step count)"""
    parts = [s.change_part(remark) for s in slabs]
    return np.concatenate([p[0] for p in parts], axis=0), parts[0][1]
