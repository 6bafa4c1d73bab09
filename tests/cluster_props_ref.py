"""The per-cluster property table of include/lbmpm.h (lbmpm_*_cluster_props) restated in NumPy: what the device is compared with, and
what clusters.merge_props is held against.  Nothing here shares code with the library: rolls instead of index arithmetic, np.add.at
instead of atomics.

    cls      [nz][ny][nx] class bytes: 0 S, 1 R, 2 B, 3 N
    labels   [nz][ny][nx] uint32, 0xFFFFFFFF where the cell is in no cluster; a cluster's cells are all R or all B
    rhoR, rhoB, ux, uy, uz   [nz][ny][nx] float64, read at the cluster's cells only
    below, above             [ny][nx] class planes next to the lattice's first and last plane, None: nothing is there
    z0       the global number of the first plane
"""
import numpy as np

S, R, B, N, NOTHING = 0, 1, 2, 3, 4
NONE = 0xFFFFFFFF
COLS = 14
LABEL, CLASS, CELLS, FACES_FLUID, FACES_SOLID, PAIRS, SQUARES, CUBES, SUM_Z, MASS, MOM_X, MOM_Y, MOM_Z, CLIPPED = range(COLS)
MASS_BITS, MOM_BITS = 24, 30


def fixed(x, bits):
    """round-to-nearest-even to a multiple of 2^-bits, as an integer count of quanta"""
    return np.rint(np.asarray(x, dtype=np.float64) * 2.0 ** bits).astype(np.int64)


def class_field(dom, cluster_classes):
    """the class bytes from the mask and the classes of clusters() (1 / 2 in a cluster, 0 otherwise): S where the mask says solid, N for
    a fluid cell in no cluster"""
    dom, c = np.asarray(dom), np.asarray(cluster_classes)
    return np.where(dom != 1, S, np.where(c == 1, R, np.where(c == 2, B, N))).astype(np.uint8)


def props(cls, labels, rhoR=None, rhoB=None, ux=None, uy=None, uz=None, below=None, above=None, z0=0):
    """[n][14] int64 by ascending label"""
    cls = np.asarray(cls, dtype=np.uint8)
    nz, ny, nx = cls.shape
    labels = np.asarray(labels, dtype=np.uint32)
    zero = np.zeros(cls.shape)
    rhoR, rhoB, ux, uy, uz = [zero if a is None else np.asarray(a, dtype=np.float64) for a in (rhoR, rhoB, ux, uy, uz)]
    nothing = np.full((1, ny, nx), NOTHING, dtype=np.uint8)
    lo = nothing if below is None else np.asarray(below, dtype=np.uint8).reshape(1, ny, nx)
    hi = nothing if above is None else np.asarray(above, dtype=np.uint8).reshape(1, ny, nx)
    pad = np.concatenate([lo, cls, hi], axis=0)
    own, dn, up = pad[1:-1], pad[:-2], pad[2:]
    xp = lambda a: np.roll(a, -1, axis=2)         # [z][y][x] = a at x + 1 mod nx
    xm = lambda a: np.roll(a, 1, axis=2)
    yp = lambda a: np.roll(a, -1, axis=1)
    ym = lambda a: np.roll(a, 1, axis=1)
    member = labels != NONE
    assert np.all((own[member] == R) | (own[member] == B)), "a cluster's cell is R or B"
    other = np.where(own == R, B, R)
    six = (xp(own), xm(own), yp(own), ym(own), dn, up)
    faces_fluid = sum((n == other).astype(np.int64) for n in six)
    faces_solid = sum((n == S).astype(np.int64) for n in six)
    px, py, pz = xp(own) == own, yp(own) == own, up == own
    sxy = px & py & (xp(yp(own)) == own)
    sxz = px & pz & (xp(up) == own)
    syz = py & pz & (yp(up) == own)
    cube = sxy & sxz & syz & (xp(yp(up)) == own)
    pairs = px.astype(np.int64) + py + pz
    squares = sxy.astype(np.int64) + sxz + syz
    z = np.broadcast_to(np.arange(z0, z0 + nz, dtype=np.int64)[:, None, None], cls.shape)
    with np.errstate(all="ignore"):
        rho = rhoR + rhoB
        mom = [rho * u for u in (ux, uy, uz)]
        good = np.isfinite(rhoR) & np.isfinite(rhoB) & np.isfinite(ux) & np.isfinite(uy) & np.isfinite(uz)
        good = good & (np.abs(rho) < 64.0) & (np.abs(mom[0]) < 1.0) & (np.abs(mom[1]) < 1.0) & (np.abs(mom[2]) < 1.0)
        mass = fixed(np.where(good, rho, 0.0), MASS_BITS)
        mom = [fixed(np.where(good, m, 0.0), MOM_BITS) for m in mom]
    keys, inv = np.unique(labels[member].astype(np.int64), return_inverse=True)
    inv = inv.reshape(-1)
    out = np.zeros((keys.shape[0], COLS), dtype=np.int64)
    out[:, LABEL] = keys
    out[inv, CLASS] = own[member]
    for col, a in ((CELLS, np.ones(cls.shape, dtype=np.int64)), (FACES_FLUID, faces_fluid), (FACES_SOLID, faces_solid), (PAIRS, pairs),
                   (SQUARES, squares), (CUBES, cube.astype(np.int64)), (SUM_Z, z), (MASS, mass), (MOM_X, mom[0]), (MOM_Y, mom[1]),
                   (MOM_Z, mom[2]), (CLIPPED, (~good).astype(np.int64))):
        np.add.at(out[:, col], inv, np.asarray(a, dtype=np.int64)[member])
    return out
