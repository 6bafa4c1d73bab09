"""Plane integrals of the 3-D solvers: the table of lbmpm_rk3d_integrals / lbmpm_rk3dcsf_integrals (include/lbmpm.h) and what a
two-phase run is read through -- saturation, masses, fluxes, Darcy velocities, the largest speed, the count of non-finite cells.

The library reduces every plane on the device in a fixed order, so a table is the same bit for bit however the lattice was cut into
slabs; `totals` keeps that: one loop over the planes in plane order, not a reduction whose order numpy may choose.
"""
import numpy as np

# the columns, in the order of LBMPM_INT_* (csrc/rk3d_integrals.h is the only other place that knows it)
COLUMNS = ("cells", "cells_R", "mass_R", "mass_B", "flux_R", "flux_B", "uz_R", "uz_B", "mom_x", "mom_y", "umax2", "nonfinite")
_MAX = COLUMNS.index("umax2")


class Integrals:
    """planes: [nz][12], one row per lattice plane (sums over the plane's fluid cells; a cell that is not finite counts in `cells` and
    `nonfinite` only); nx, ny: the plane's extent (the Darcy velocities divide by the whole volume, solid included)"""
    COLUMNS = COLUMNS

    def __init__(self, planes, nx, ny):
        a = np.ascontiguousarray(planes, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != len(COLUMNS):
            raise TypeError("planes must have shape [nz][%d]" % len(COLUMNS))
        self.planes, self.nx, self.ny = a, int(nx), int(ny)
        self.nz = a.shape[0]
        self._totals = None

    def column(self, name):
        """the profile of one column along z"""
        return self.planes[:, COLUMNS.index(name)]

    @property
    def totals(self):
        """[12]: the planes added in plane order (the maximum for umax2)"""
        if self._totals is None:
            t = [0.0] * len(COLUMNS)
            for row in self.planes.tolist():
                for c, v in enumerate(row):
                    t[c] = (v if v > t[c] else t[c]) if c == _MAX else t[c] + v
            self._totals = np.array(t, dtype=np.float64)
        return self._totals

    def total(self, name):
        return float(self.totals[COLUMNS.index(name)])

    @property
    def good_cells(self):
        return self.total("cells") - self.total("nonfinite")

    @property
    def saturation_R(self):
        """share of the finite fluid cells with phi > 0"""
        return self.total("cells_R") / self.good_cells if self.good_cells else float("nan")

    @property
    def mass_R(self):
        return self.total("mass_R")

    @property
    def mass_B(self):
        return self.total("mass_B")

    @property
    def mass_fraction_R(self):
        m = self.mass_R + self.mass_B
        return self.mass_R / m if m else float("nan")

    @property
    def flux_R(self):
        """mean over the planes of the red mass flux along z"""
        return self.total("flux_R") / self.nz

    @property
    def flux_B(self):
        return self.total("flux_B") / self.nz

    @property
    def darcy_uz_R(self):
        """sum of u_z over the red cells / (nx ny nz): the phase's Darcy velocity, the input of a relative-permeability curve"""
        return self.total("uz_R") / (self.nx * self.ny * self.nz)

    @property
    def darcy_uz_B(self):
        return self.total("uz_B") / (self.nx * self.ny * self.nz)

    @property
    def max_speed(self):
        return float(np.sqrt(self.total("umax2")))

    @property
    def nonfinite(self):
        return int(self.total("nonfinite"))

    def summary(self):
        """the sums a log line carries"""
        return dict(saturationR=self.saturation_R, massR=self.mass_R, massB=self.mass_B, maxSpeed=self.max_speed)


def column_bytes():
    """COLUMNS as a [12][width] uint8 array, zero-padded: what /Integrals/Columns of a result file holds (every backend writes it)"""
    width = max(len(c) for c in COLUMNS)
    return np.array([list(c.encode().ljust(width, b"\0")) for c in COLUMNS], dtype=np.uint8)


def column_names(a):
    """the names back from /Integrals/Columns"""
    return tuple(bytes(bytearray(np.asarray(row, dtype=np.uint8).tolist())).rstrip(b"\0").decode() for row in np.asarray(a))


def fresh(take, observe):
    """take(), after observe() when the perturbation model's diagnostics are stale (LBMPM_ERR_STATE: a step since the last observe)"""
    from ._lib import ERR_STATE, LbmpmError
    try:
        return take()
    except LbmpmError as e:
        if e.status != ERR_STATE:
            raise
    observe()
    return take()


def table(L, fn_name, handle, planes):
    """[planes][12] of one context through lbmpm_*_integrals"""
    from ._lib import F64P, check
    out = np.empty((int(planes), len(COLUMNS)), dtype=np.float64)
    check(getattr(L, fn_name)(handle, out.ctypes.data_as(F64P)), fn_name)
    return out
