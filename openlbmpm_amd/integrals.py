"""Plane integrals of the 3-D solvers: the table of lbmpm_rk3d_integrals / lbmpm_rk3dcsf_integrals (include/lbmpm.h) and what a
two-phase run is read through -- saturation, masses, fluxes, Darcy velocities, the largest speed, the count of non-finite cells; and
the tracers' table of lbmpm_rk3dcsf_tracer_integrals (TracerIntegrals): mass balances, breakthrough, the moments of a plume along z;
and the table of lbmpm_rk3dcsf_tracer_wall_integrals (TracerWallIntegrals): what the tracers' wall reaction took up, per plane and tracer.

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


# the tracers' columns, in the order of LBMPM_TRINT_* (csrc/rk3d_tracer_integrals.h is the only other place that knows it)
TRACER_COLUMNS = ("cells", "mass", "flux_x", "flux_y", "flux_z", "sum_c2", "cmin", "cmax", "nonfinite")
_T = {c: i for i, c in enumerate(TRACER_COLUMNS)}


class TracerIntegrals:
    """planes: [nz][nT][9], one row per lattice plane and tracer over the plane's fluid cells, from the populations g[0..6] that
    get_tracer_pdf hands out and C = their sum (a cell where C or a population is not finite counts in `cells` and `nonfinite` only;
    cmin = cmax = 0 on a plane without finite cells); nx, ny: the plane's extent.  Everything below is computed from the plane
    profile alone."""
    COLUMNS = TRACER_COLUMNS

    def __init__(self, planes, nx, ny):
        a = np.ascontiguousarray(planes, dtype=np.float64)
        if a.ndim != 3 or a.shape[2] != len(TRACER_COLUMNS):
            raise TypeError("planes must have shape [nz][nT][%d]" % len(TRACER_COLUMNS))
        self.planes, self.nx, self.ny = a, int(nx), int(ny)
        self.nz, self.num_tracers = a.shape[0], a.shape[1]
        self._totals = None

    def column(self, name, tracer):
        """the profile of one column of one tracer along z"""
        return self.planes[:, int(tracer), _T[name]]

    @property
    def totals(self):
        """[nT][9]: the planes added in plane order; cmin / cmax: the least / largest over the planes that have finite cells (0 without)"""
        if self._totals is None:
            n = len(TRACER_COLUMNS)
            t = [[0.0] * n for _ in range(self.num_tracers)]
            seen = [False] * self.num_tracers
            for plane in self.planes.tolist():
                for k, row in enumerate(plane):
                    good = row[_T["cells"]] - row[_T["nonfinite"]] > 0
                    for c, v in enumerate(row):
                        if c == _T["cmin"] or c == _T["cmax"]:
                            if good:
                                t[k][c] = v if not seen[k] else (min(t[k][c], v) if c == _T["cmin"] else max(t[k][c], v))
                        else:
                            t[k][c] = t[k][c] + v
                    seen[k] = seen[k] or good
            self._totals = np.array(t, dtype=np.float64).reshape(self.num_tracers, n)
        return self._totals

    def total(self, name, tracer):
        return float(self.totals[int(tracer), _T[name]])

    def good_cells(self, tracer):
        return self.total("cells", tracer) - self.total("nonfinite", tracer)

    def mass(self, tracer):
        """sum of C over the finite fluid cells"""
        return self.total("mass", tracer)

    def mean(self, tracer):
        g = self.good_cells(tracer)
        return self.mass(tracer) / g if g else float("nan")

    def variance(self, tracer):
        """sum C^2 / cells - mean^2: the scalar variance (the mixing state)"""
        g = self.good_cells(tracer)
        return self.total("sum_c2", tracer) / g - self.mean(tracer) ** 2 if g else float("nan")

    def cmin(self, tracer):
        return self.total("cmin", tracer)

    def cmax(self, tracer):
        return self.total("cmax", tracer)

    @property
    def nonfinite(self):
        """cells that are not finite, all tracers together"""
        return int(sum(self.total("nonfinite", k) for k in range(self.num_tracers)))

    def _z_sums(self, tracer):
        """sum m(z), sum z m(z), sum z^2 m(z), added in plane order"""
        s0 = s1 = s2 = 0.0
        for z, m in enumerate(self.column("mass", tracer).tolist()):
            s0 += m
            s1 += z * m
            s2 += z * z * m
        return s0, s1, s2

    def centre_z(self, tracer):
        """sum z m(z) / sum m(z): the plume's centre of mass along the flow axis"""
        s0, s1, _ = self._z_sums(tracer)
        return s1 / s0 if s0 else float("nan")

    def variance_z(self, tracer):
        """the second central moment of the mass profile along z; it grows as 2 D_zz t"""
        s0 = self._z_sums(tracer)[0]
        if not s0:
            return float("nan")
        mu = self.centre_z(tracer)
        v = 0.0
        for z, m in enumerate(self.column("mass", tracer).tolist()):
            v += (z - mu) ** 2 * m
        return v / s0

    def flux_z_at(self, tracer, z):
        """sum of g(+z) - g(-z) over plane z: one entry of the profile.  The flow runs towards -z (inlet on plane nz-1, outlet on plane 0),
        so the breakthrough at the outlet is -flux_z_at(k, 1)"""
        return float(self.planes[int(z), int(tracer), _T["flux_z"]])

    def summary(self):
        """the numbers a log line carries: mass<k>, cmin<k>, cmax<k> per tracer"""
        out = {}
        for k in range(self.num_tracers):
            out["mass%d" % k], out["cmin%d" % k], out["cmax%d" % k] = self.mass(k), self.cmin(k), self.cmax(k)
        return out


# the wall table's columns, in the order of LBMPM_TRWALL_* (csrc/rk3d_tracer_wall.h is the only other place that knows it)
TRACER_WALL_COLUMNS = ("wall_links", "uptake", "wall_c", "nonfinite")
_W = {c: i for i, c in enumerate(TRACER_WALL_COLUMNS)}


class TracerWallIntegrals:
    """planes: [nz][nT][4], one row per lattice plane and tracer over the plane's wall links -- a fluid cell and a direction whose source
    cell is solid: their count, the sum of g_out - g_in (what the walls took out of the tracer in the last completed sub-step), the sum of
    the links' wall concentrations 3 (g_out + g_in), and the cells with a population that is not finite among those read (they count in
    the links and in nothing else).  The mass a run loses from step n - 1 to step n is uptake(k) after step n."""
    COLUMNS = TRACER_WALL_COLUMNS

    def __init__(self, planes, nx, ny):
        a = np.ascontiguousarray(planes, dtype=np.float64)
        if a.ndim != 3 or a.shape[2] != len(TRACER_WALL_COLUMNS):
            raise TypeError("planes must have shape [nz][nT][%d]" % len(TRACER_WALL_COLUMNS))
        self.planes, self.nx, self.ny = a, int(nx), int(ny)
        self.nz, self.num_tracers = a.shape[0], a.shape[1]

    def column(self, name, tracer):
        """the profile of one column of one tracer along z"""
        return self.planes[:, int(tracer), _W[name]]

    def total(self, name, tracer):
        """the planes added in plane order"""
        t = 0.0
        for v in self.column(name, tracer).tolist():
            t += v
        return t

    def uptake(self, tracer):
        """what the walls of the whole lattice took out of the tracer in the last completed sub-step"""
        return self.total("uptake", tracer)

    @property
    def wall_links(self):
        """wall links of the lattice (the same for every tracer)"""
        return int(self.total("wall_links", 0))

    def mean_wall_concentration(self, tracer):
        """sum of the links' wall concentrations / links (all of them: a lattice with non-finite cells reports those in `nonfinite`)"""
        n = self.total("wall_links", tracer)
        return self.total("wall_c", tracer) / n if n else float("nan")

    @property
    def nonfinite(self):
        """cells with a non-finite population at a wall, all tracers together"""
        return int(sum(self.total("nonfinite", k) for k in range(self.num_tracers)))

    def summary(self):
        """the numbers a log line carries: uptake<k>, wallC<k> per tracer"""
        out = {}
        for k in range(self.num_tracers):
            out["uptake%d" % k], out["wallC%d" % k] = self.uptake(k), self.mean_wall_concentration(k)
        return out


def _name_bytes(names):
    width = max(len(c) for c in names)
    return np.array([list(c.encode().ljust(width, b"\0")) for c in names], dtype=np.uint8)


def column_bytes():
    """COLUMNS as a [12][width] uint8 array, zero-padded: what /Integrals/Columns of a result file holds (every backend writes it)"""
    return _name_bytes(COLUMNS)


def tracer_column_bytes():
    """TRACER_COLUMNS the same way: /TracerIntegrals/Columns (column_names reads both)"""
    return _name_bytes(TRACER_COLUMNS)


def tracer_wall_column_bytes():
    """TRACER_WALL_COLUMNS the same way: /TracerWallIntegrals/Columns"""
    return _name_bytes(TRACER_WALL_COLUMNS)


def column_names(a):
    """the names back from /Integrals/Columns"""
    return tuple(bytes(bytearray(np.asarray(row, dtype=np.uint8).tolist())).rstrip(b"\0").decode() for row in np.asarray(a))


def fresh(take, observe):
    """take(), after observe() when the perturbation model's diagnostics are stale (LBMPM_ERR_STATE: a step since the last observe);
    observe = None (a model whose analyses are never stale): just take()"""
    from ._lib import ERR_STATE, LbmpmError
    if observe is None:
        return take()
    try:
        return take()
    except LbmpmError as e:
        if e.status != ERR_STATE:
            raise
    observe()
    return take()


def table(L, prefix, handle, planes):
    """[planes][12] of one context through <prefix>_integrals (prefix: the class's _C_PREFIX, here and in change, clusters, morphology)"""
    from ._lib import F64P, check
    out = np.empty((int(planes), len(COLUMNS)), dtype=np.float64)
    name = prefix + "_integrals"
    check(getattr(L, name)(handle, out.ctypes.data_as(F64P)), name)
    return out


def tracer_table(L, handle, planes, num_tracers):
    """[planes][nT][9] of one context through lbmpm_rk3dcsf_tracer_integrals"""
    from ._lib import F64P, check
    out = np.empty((int(planes), int(num_tracers), len(TRACER_COLUMNS)), dtype=np.float64)
    check(L.lbmpm_rk3dcsf_tracer_integrals(handle, out.ctypes.data_as(F64P)), "lbmpm_rk3dcsf_tracer_integrals")
    return out


def tracer_wall_table(L, handle, planes, num_tracers):
    """[planes][nT][4] of one context through lbmpm_rk3dcsf_tracer_wall_integrals"""
    from ._lib import F64P, check
    out = np.empty((int(planes), int(num_tracers), len(TRACER_WALL_COLUMNS)), dtype=np.float64)
    check(L.lbmpm_rk3dcsf_tracer_wall_integrals(handle, out.ctypes.data_as(F64P)), "lbmpm_rk3dcsf_tracer_wall_integrals")
    return out
