"""Phase morphology of the 3-D solvers: the table of lbmpm_rk3d_morphology / lbmpm_rk3dcsf_morphology (include/lbmpm.h holds the
definition) and the state variables that two-phase theory adds to saturation -- the fluid-fluid interfacial area, the wetted solid
areas, the Euler characteristic of each phase and a phase-averaged pressure difference: a Pc-S-a_nw sample without a field download.

The library classifies every cell (S solid, R, B, N neither) and counts, per plane, the cells, the pairs along every axis by their
classes and the 2 x 2 squares and 2 x 2 x 2 cubes of one phase, each anchored at its lowest corner; x and y wrap, z does not unless
asked to (wrap_z=True on a lattice that is periodic in z: plane 0 is then the plane above plane nz - 1, through the same `above`).  The
counts are integers and the two density sums are added in a fixed order, so a table is the same bit for bit however the lattice was
cut into slabs: a slab passes the classes of its lowest plane (`face`) to the slab below it, which joins on its device.
"""
import numpy as np

PAIRS = ("RR", "BB", "RB", "RS", "BS")
AXES = ("x", "y", "z")
# the columns, in the order of LBMPM_MO_* (csrc/rk3d_morphology.h is the only other place that knows it)
COLUMNS = ("cells_R", "cells_B", "cells_N", "rho_R", "rho_B") + tuple("%s_%s" % (p, a) for a in AXES for p in PAIRS) + \
    tuple("sq_%s_%s" % (p, f) for p in "RB" for f in ("xy", "xz", "yz")) + ("cube_R", "cube_B")
_C = {c: i for i, c in enumerate(COLUMNS)}
S, R, B, N = range(4)                 # LBMPM_MORPH_*: the class bytes


class Morphology:
    """planes: [nz][28], one row per lattice plane (every element counts in the plane of its anchor cell); nx, ny: the plane's extent.
    Everything below is a sum over the planes of integer columns, or a ratio of two such sums."""
    COLUMNS = COLUMNS

    def __init__(self, planes, nx, ny):
        a = np.ascontiguousarray(planes, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != len(COLUMNS):
            raise TypeError("planes must have shape [nz][%d]" % len(COLUMNS))
        self.planes, self.nx, self.ny = a, int(nx), int(ny)
        self.nz = a.shape[0]

    def column(self, name):
        """the profile of one column along z"""
        return self.planes[:, _C[name]]

    def _count(self, name):
        return int(self.column(name).sum())

    @staticmethod
    def _phase(phase):
        if phase not in ("R", "B"):
            raise ValueError("phase must be 'R' or 'B'")
        return phase

    def cells(self, phase):
        """the cells of a class: 'R', 'B' or 'N' (fluid in neither phase: the band of a phi_cut > 0, and cells that are not finite)"""
        if phase not in ("R", "B", "N"):
            raise ValueError("phase must be 'R', 'B' or 'N'")
        return self._count("cells_" + phase)

    def faces(self, pair, axis=None):
        """the cell faces between the two classes of `pair` ('RB', 'RS' or 'BS'), normal to `axis` ('x', 'y', 'z') or to any (None)"""
        if pair not in ("RB", "RS", "BS"):
            raise ValueError("pair must be 'RB', 'RS' or 'BS'")
        if axis is not None and axis not in AXES:
            raise ValueError("axis must be 'x', 'y', 'z' or None")
        return sum(self._count("%s_%s" % (pair, a)) for a in (AXES if axis is None else (axis,)))

    def area(self, pair):
        """2/3 of the face count: the three-direction Cauchy-Crofton estimate of the interface's area (the mean over the three axes
        of the projected face count, times two).  The plain face count is the area of the staircase, which overstates a smooth surface
        -- a sphere by a factor of 1.5; two thirds of it is within a few per cent of 4 pi r^2 from r = 6 on."""
        return 2.0 * self.faces(pair) / 3.0

    def specific_area(self, pair):
        """area(pair) per lattice volume nx ny nz (solid included): a_nw for 'RB'"""
        return self.area(pair) / (self.nx * self.ny * self.nz)

    def wetted_fraction(self, phase):
        """the share of the fluid-solid faces that the phase wets, XS / (RS + BS): cos of an effective contact angle is 2 f_B - 1 with
        B the wetting phase.  NaN without such faces."""
        n = self.faces("RS") + self.faces("BS")
        return self.faces(self._phase(phase) + "S") / n if n else float("nan")

    def euler(self, phase):
        """chi_6 = cells - pairs + squares - cubes of the phase: the Euler characteristic of its cells joined through faces (the
        connectivity clusters() labels by default) = clusters - redundant loops + cavities"""
        p = self._phase(phase)
        return self._count("cells_" + p) - sum(self._count("%s%s_%s" % (p, p, a)) for a in AXES) + \
            sum(self._count("sq_%s_%s" % (p, f)) for f in ("xy", "xz", "yz")) - self._count("cube_" + p)

    def mean_density(self, phase):
        """the mean of rho_R + rho_B over the cells of the phase (the planes added in plane order); NaN without such cells"""
        p = self._phase(phase)
        n = self._count("cells_" + p)
        if not n:
            return float("nan")
        s = 0.0
        for v in self.column("rho_" + p).tolist():
            s += v
        return s / n

    def capillary_pressure(self, cs2=1.0 / 3.0):
        """cs2 (mean_density('R') - mean_density('B')): the phase-averaged pressure difference under p = cs2 rho, the equation of
        state of the CSF model.  On the perturbation model, whose rest equilibria depend on the colour, p is not cs2 rho and this is
        only a density difference."""
        return cs2 * (self.mean_density("R") - self.mean_density("B"))

    def summary(self):
        """the numbers a log line carries"""
        return dict(areaRB=self.area("RB"), wettedR=self.wetted_fraction("R"), eulerR=self.euler("R"), eulerB=self.euler("B"),
                    capillaryPressure=self.capillary_pressure())


def column_bytes():
    """COLUMNS as a [28][width] uint8 array, zero-padded: /Morphology/Columns of a result file (integrals.column_names reads it back)"""
    width = max(len(c) for c in COLUMNS)
    return np.array([list(c.encode().ljust(width, b"\0")) for c in COLUMNS], dtype=np.uint8)


def _config(phi_cut):
    from ._lib import MorphologyConfig
    return MorphologyConfig(float(phi_cut))


def face(L, prefix, handle, ny, nx, phi_cut=0.0):
    """[ny][nx] uint8: the classes of the lowest own plane of one context through <prefix>_morphology_face"""
    import ctypes as C
    from ._lib import U8P, check
    out = np.empty((int(ny), int(nx)), dtype=np.uint8)
    name = prefix + "_morphology_face"
    check(getattr(L, name)(handle, C.byref(_config(phi_cut)), out.ctypes.data_as(U8P)), name)
    return out


def table(L, prefix, handle, planes, ny, nx, phi_cut=0.0, above=None):
    """[planes][28] of one context through <prefix>_morphology; above: [ny][nx] classes of the plane over the highest own plane
    (the `face` of the slab above), None at the lattice's end"""
    import ctypes as C
    from ._lib import F64P, U8P, check
    out = np.empty((int(planes), len(COLUMNS)), dtype=np.float64)
    up = None
    if above is not None:
        up = np.ascontiguousarray(above, dtype=np.uint8)
        if up.shape != (int(ny), int(nx)):
            raise TypeError("above must have shape [ny][nx]")
    name = prefix + "_morphology"
    check(getattr(L, name)(handle, C.byref(_config(phi_cut)), None if up is None else up.ctypes.data_as(U8P), out.ctypes.data_as(F64P)), name)
    return out


def stacked(slabs, phi_cut, ring=False):
    """the slabs of one process, lowest first: every slab gets the face of the slab over it, the top one None (ring: the lowest slab's);
    [nz][28]"""
    faces = [s.morphology_face(phi_cut) for s in slabs[1:]] + [slabs[0].morphology_face(phi_cut) if ring else None]
    return np.concatenate([s.morphology_part(phi_cut, up) for s, up in zip(slabs, faces)], axis=0)


def face_from_above(mine, rank, world, group, device, ring=False):
    """collective: every rank gives the face of its slab and takes that of rank + 1 (None on the last; ring: rank 0's): one all_gather
    of [ny][nx] bytes, through device memory under nccl, host memory under gloo; a world of one: none (ring: its own face)"""
    if world == 1:
        return np.asarray(mine) if ring else None
    import torch
    import torch.distributed as dist
    dev = torch.device("cuda", device) if dist.get_backend(group) == "nccl" else torch.device("cpu")
    t = torch.from_numpy(np.ascontiguousarray(mine, dtype=np.uint8)).to(dev)
    every = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(every, t, group=group)
    return every[(rank + 1) % world].cpu().numpy() if rank + 1 < world or ring else None
