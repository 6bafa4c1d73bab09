"""Reference for periodic z of the 3-D CSF solver (inlet = outlet = 'Periodic'), built AROUND the unchanged oracle: TEST INFRASTRUCTURE ONLY.

The oracle (oracle/rk3d_csf_oracle.c) has open planes at both ends of z and no periodic mode.  It needs none: the model is symmetric
under a permutation of the axes, the oracle wraps x and y, and its open-plane rules touch fluid cells only.  So a lattice A[z][y][x]
that is periodic in z and SEALED in x -- solid planes at least two thick at either end of x -- has an exact reference: the unchanged
oracle on A.transpose(2, 1, 0).  The solver's x becomes the oracle's z, whose four open planes are solid and do nothing; the solver's
z becomes the oracle's periodic x.  Body forces, vector fields and the D3Q19 directions go through the same exchange of x and z.
tests/test_rk3d_csf_periodic_cpu.py holds the reference's own conditions (the seal, the symmetry, mass).
"""
import numpy as np

import body_force_ref as R

SEAL = 2         # solid planes at either end of x
# direction i of the solver is direction XZ[i] of the transposed oracle: (cx, cy, cz) -> (cz, cy, cx)
XZ = np.array([[j for j in range(19) if (R.CX[j], R.CY[j], R.CZ[j]) == (R.CZ[i], R.CY[i], R.CX[i])][0] for i in range(19)])
_NAMES = dict(vx="vz", vz="vx", Gx="Gz", Gz="Gx", Fx="Fz", Fz="Fx", nsx="nsz", nsz="nsx")
RATES = (1.1, 1.45, 1.25, 1.35, 1.15, 0.9)        # six distinct MRT rates (the conserved moments' among them: it must not matter)
FLOW_KEYS = ("inlet", "outlet", "variant", "bulk_epsilon")      # what the solver's params carry and the oracle's do not


def swap(a):
    """[z][y][x](...) <-> [x][y][z](...)"""
    a = np.asarray(a)
    return np.ascontiguousarray(np.transpose(a, (2, 1, 0) + tuple(range(3, a.ndim))))


def sealed(dom):
    dom = np.asarray(dom)
    return bool(np.all(dom[:, :, :SEAL] != 1) and np.all(dom[:, :, -SEAL:] != 1))


class PeriodicRef:
    """tests/body_force_ref.BodyForceRef on the transposed lattice, seen through the solver's axes: dom, fl, field(name), run(n),
    step_a() (the record view, with the body force's half in u)"""

    def __init__(self, dom, rhoR0, rhoB0, params=None, g_r=(0., 0., 0.), g_b=(0., 0., 0.), crisp=R.CRISP):
        if not sealed(dom):
            raise ValueError("the reference needs solid planes %d thick at both ends of x" % SEAL)
        par = {k: v for k, v in (params or {}).items() if k not in FLOW_KEYS}
        self.dom = np.ascontiguousarray(dom, dtype=np.uint8)
        self.fl = self.dom == 1
        self.g_r, self.g_b = np.asarray(g_r, dtype=np.float64), np.asarray(g_b, dtype=np.float64)
        self.ref = R.BodyForceRef(swap(self.dom), swap(rhoR0), swap(rhoB0), par, tuple(g_r)[::-1], tuple(g_b)[::-1], crisp=crisp)

    def run(self, n, hook=None):
        """hook: BodyForceRef.step's, handed through; when it is called field() gives rhoR, vx .. Gz of that moment in the solver's axes"""
        self.ref.run(n, hook)
        return self

    def step(self, hook=None):
        return self.run(1, hook)

    def step_a(self):
        self.ref.step_a()
        return self

    def field(self, name):
        a = swap(self.ref.field(_NAMES.get(name, name)))
        return np.ascontiguousarray(a[..., XZ]) if a.ndim == 4 else a


class Snapshot:
    """the fields of a reference at one moment, with the calls tests/test_rk3d_csf_gpu.compare_all makes"""
    FIELDS = ("rhoR", "rhoB", "phi", "K", "vx", "vy", "vz", "Gx", "Gy", "Gz", "Fx", "Fy", "Fz", "fR", "fB", "kind", "nsx", "nsy", "nsz")

    def __init__(self, ref):
        self.dom, self.fl = ref.dom, ref.fl
        self._f = {f: ref.field(f) for f in self.FIELDS}

    def field(self, name):
        return self._f[name]


def totals_of(rec):
    """the totals of integrals() (openlbmpm_amd/integrals.COLUMNS) from a Snapshot of the record view"""
    fl = rec.fl
    rR, rB, phi = rec.field("rhoR")[fl], rec.field("rhoB")[fl], rec.field("phi")[fl]
    ux, uy, uz = (rec.field(c)[fl] for c in ("vx", "vy", "vz"))
    red = phi > 0.
    return dict(cells=float(fl.sum()), cells_R=float(red.sum()), mass_R=float(rR.sum()), mass_B=float(rB.sum()), flux_R=float((rR * uz).sum()),
                flux_B=float((rB * uz).sum()), uz_R=float(uz[red].sum()), uz_B=float(uz[~red].sum()), mom_x=float(((rR + rB) * ux).sum()),
                mom_y=float(((rR + rB) * uy).sum()), umax2=float((ux * ux + uy * uy + uz * uz).max()), nonfinite=0.0)


# ------------------------------------------------------------------------------------------------ lattices
def _ripple(shape, a, k):
    z, y, x = np.mgrid[0:shape[0], 0:shape[1], 0:shape[2]]
    return 1. + a * np.sin(2. * np.pi * (k[0] * z / shape[0] + k[1] * y / shape[1] + k[2] * x / shape[2]) + 0.3)


def _wrapped(i, centre, n):
    d = np.abs(i - centre)
    return np.minimum(d, n - d)


def parity_lattice(wall=3):
    """10 x 6 x 14 ([nz][ny][nx]), sealed in x by walls `wall` thick: two grains (one across the seam of z, next to a wall), a red blob
    that lies across the seam, rippled densities.  (dom, rhoR, rhoB)"""
    shape = (10, 6, 14)
    dom = np.ones(shape, dtype=np.uint8)
    dom[:, :, :wall] = 0; dom[:, :, -wall:] = 0
    dom[[9, 0], 1:3, wall:wall + 2] = 0
    dom[4:6, 3:5, 7:9] = 0
    z, y, x = np.mgrid[0:10, 0:6, 0:14]
    blob = (_wrapped(z, 0.5, 10) / 3.2) ** 2 + (_wrapped(y, 2.5, 6) / 2.6) ** 2 + ((x - 6.5) / 3.0) ** 2 < 1.
    fl = dom == 1
    rR = np.where(fl & blob, 1.0 * _ripple(shape, 0.03, (1, 1, 2)), 0.0)
    rB = np.where(fl & ~blob, 0.9 * _ripple(shape, 0.02, (2, 1, 1)), 0.0)
    return dom, rR, rB


def parity_params(relax, tautype, **over):
    return dict(dict(relax=relax, tautype=tautype, theta=50.0, tauR=0.9, tauB=1.3, rates=RATES, inlet="Periodic", outlet="Periodic"), **over)


# Blocks of the bulk path are 256 fluid cells in lattice order; a plane of 16 x 16 is one block.  The four grains are 4 x 4 x 4 each and
# stand side by side in the planes 4 .. 7: those planes hold 192 fluid cells, four of them three blocks, and the grains lie in planes that
# a roll by k <= 8 does not carry across the seam.  So for k = 1 .. 8 the rolled lattice's blocks are the SAME sets of cells, numbered
# k further round the ring: whatever the bulk path decides per block it must decide alike for every k.
# A block is deep when every block within two cells of it holds one colour alone, and a block is a plane here: the one-colour core of
# the red body therefore has to fill whole planes.  Red fills the planes 10 .. 15, 0 .. 7 across the seam (rippled), blue is a film in the
# planes 8, 9; the colours' tails stop where a colour falls below bulk_epsilon = 1e-3 of the density (~ 3.5 cells from the film with
# beta = 1), which leaves the planes around z = 0 red alone for good.
FREE_SHAPE = (16, 16, 16)
FREE_PARAMS = dict(relax="MRT", theta=50.0, tauB=0.8, sigma=0.05, beta=1.0, bulk_epsilon=1.0e-3, inlet="Periodic", outlet="Periodic")
ROLLS = (1, 5, 8)


def free_lattice(grains=True):
    """16 x 16 x 16 without walls (see above).  (dom, rhoR, rhoB)"""
    dom = np.ones(FREE_SHAPE, dtype=np.uint8)
    if grains:
        for y0, x0 in ((1, 2), (9, 3), (3, 10), (10, 11)):
            dom[4:8, y0:y0 + 4, x0:x0 + 4] = 0
    z = np.mgrid[0:16, 0:16, 0:16][0]
    blue = (z == 8) | (z == 9)
    fl = dom == 1
    rR = np.where(fl & ~blue, 1.0 * _ripple(FREE_SHAPE, 0.02, (1, 2, 1)), 0.0)
    rB = np.where(fl & blue, 0.95 * _ripple(FREE_SHAPE, 0.02, (0, 1, 2)), 0.0)
    return dom, rR, rB


# ------------------------------------------------------------------------------------------------ the ring box (observers, restart)
# The 70 x 33 x 12 box of the analyses' tests (tests/test_integrals_gpu.py: rows of 64 + 6 cells, 2310 cells per plane = two chunks of the
# reducer and a ragged one, 12 planes = no multiple of the 4-plane cluster tile) with a mask made for a ring: nothing repeats at the ends of
# z, and what is special lies on the seam between plane 11 and plane 0.
RING_SHAPE = (12, 33, 70)
RING_PARAMS = dict(relax="MRT", theta=55.0, tauB=0.8, sigma=0.06, inlet="Periodic", outlet="Periodic")
RING_TRACER = dict(num_tracers=1, diffusion_x=0.12, beta_interface=0.3, dirichlet_inlet=False, free_outlet=False)
SEAM = "seam_ganglion"


def ring_box(seed=29):
    """the mask [12][33][70]: seeded blocks anywhere round the ring (some across the seam), a grain across the seam, a grain in the planes
    10, 11 under fluid of plane 0 and one in the planes 0, 1 over fluid of plane 11, row y = 7 all solid in the planes 3 .. 8, plane 5 with
    five fluid cells, and room for the ganglion of ring_red_cells"""
    nz, ny, nx = RING_SHAPE
    rng = np.random.default_rng(seed)
    dom = np.ones(RING_SHAPE, dtype=np.uint8)
    for _ in range(60):
        z, y, x = rng.integers(0, nz), rng.integers(0, ny - 3), rng.integers(0, nx - 4)
        for p in (z, (z + 1) % nz):
            dom[p, y:y + 3, x:x + 4] = 0
    dom[3:9, 7, :] = 0
    dom[5] = 0
    dom[5, 20, 30:33] = 1
    dom[5, 3, 68:70] = 1
    dom[[9, 10, 11, 0, 1, 2], 13:23, 29:45] = 1          # the ganglion's room
    dom[[11, 0], 24:28, 8:14] = 0                        # the grain across the seam
    dom[10:12, 2:5, 50:56] = 0; dom[0:2, 2:5, 50:56] = 1
    dom[0:2, 28:31, 20:26] = 0; dom[10:12, 28:31, 20:26] = 1
    return dom


def ring_red_cells():
    """the pattern of its own: one red ganglion across the seam, three planes thick on either side (9 .. 11 and 0 .. 2), whose footprints
    in the planes 11 and 0 differ and overlap (x 34 .. 39, y 16 .. 19); blue everywhere else"""
    red = np.zeros(RING_SHAPE, dtype=bool)
    red[9:12, 14:20, 30:40] = True
    red[0:3, 16:22, 34:44] = True
    return red


def ring_densities(name, dom):
    """(rhoR, rhoB) of the pattern `name`: SEAM, or a pattern of tests/test_clusters_gpu.densities"""
    if name != SEAM:
        from test_clusters_gpu import densities
        return densities(name, dom)
    fl, red = dom == 1, ring_red_cells()
    return np.where(fl & red, 1.0, 0.0), np.where(fl & ~red, 1.0, 0.0)


def ring_concentration(dom):
    nz, ny, nx = dom.shape
    z, y, x = np.mgrid[0:nz, 0:ny, 0:nx]
    return np.where(dom == 1, 0.3 + 0.2 * np.cos(2. * np.pi * (z / nz + x / nx)) + 0.05 * np.sin(2. * np.pi * y / ny), 0.0)


def gap_lattice(nz, ny, gap, wall=2):
    """a gap `gap` cells wide between walls `wall` thick at both ends of x, red in its lower half, blue in the upper one: uniform along z"""
    nx = gap + 2 * wall
    dom = np.ones((nz, ny, nx), dtype=np.uint8)
    dom[:, :, :wall] = 0; dom[:, :, -wall:] = 0
    x = np.mgrid[0:nz, 0:ny, 0:nx][2]
    fl = dom == 1
    return dom, np.where(fl & (x < wall + gap // 2), 1.0, 0.0), np.where(fl & (x >= wall + gap // 2), 1.0, 0.0)


# ------------------------------------------------------------------------------------------------ the two-layer force-driven flow
# Gap of 32 cells between walls 2 thick, lattice 4 x 2 x 36; red in the lower half, blue in the upper one, g_z on both colours.  The
# analytic profile: no slip at the half-way walls (s = 0 and s = 32 with s = x - 3/2), velocity and stress continuous at s = 16.
# The oracle-based reference (PeriodicRef after 20 000 steps, its record view, measured by two_layer_errors below) gave against it, as
# flow-rate errors of red / of blue and the worst deviation of the profile in shares of the peak velocity:
#     MRT  +0.027 %  +0.29 %  0.89 %      SRT  +0.072 %  +0.26 %  0.87 %
# (the case was first run with flow rates summed a little differently: -0.010 % / +0.22 % / 0.89 % and +0.035 % / +0.19 % / 0.87 %).
# The bounds for the GPU run, 0.5 % for either flow rate and 1.5 % of the peak for the profile, are about twice what the reference shows,
# for the half-force term and rounding.
TWO_LAYER = dict(gap=32, wall=2, nz=4, ny=2, steps=20000, g_z=1.0e-6,
                 params=dict(tauR=1.0, tauB=0.7, sigma=0.05, theta=90.0, inlet="Periodic", outlet="Periodic"))
TWO_LAYER_REFERENCE = dict(MRT=(0.027e-2, 0.29e-2, 0.89e-2), SRT=(0.072e-2, 0.26e-2, 0.87e-2))
FLOW_RATE_BOUND, PROFILE_BOUND = 0.5e-2, 1.5e-2


def two_layer_profile(s, g=TWO_LAYER["g_z"], H=32., h=16., tauR=1.0, tauB=0.7):
    """u_z at the distances s from the lower wall: nu_c u'' = -g in either layer (rho = 1), u(0) = u(H) = 0, u and nu u' continuous at h"""
    n1, n2 = (tauR - 0.5) / 3., (tauB - 0.5) / 3.
    # u1 = -g s^2 / (2 n1) + a s;  u2 = -g (s - H)^2 / (2 n2) + b (s - H);  stress: -g h + n1 a = -g (h - H) + n2 b
    # velocity: -g h^2 / (2 n1) + a h = -g (h - H)^2 / (2 n2) + b (h - H)
    A = np.array([[n1, -n2], [h, -(h - H)]])
    rhs = np.array([g * h - g * (h - H), g * h * h / (2. * n1) - g * (h - H) ** 2 / (2. * n2)])
    a, b = np.linalg.solve(A, rhs)
    s = np.asarray(s, dtype=np.float64)
    return np.where(s < h, -g * s * s / (2. * n1) + a * s, -g * (s - H) ** 2 / (2. * n2) + b * (s - H))


def two_layer_errors(vz_row):
    """vz_row: u_z of the 32 cells across the gap.  (flow-rate error of red, of blue, worst deviation / peak) against the analytic
    profile, the flow rates as integrals of it over either layer"""
    s = np.arange(32) + 0.5
    fine = (np.arange(16 * 4096) + 0.5) / 4096.
    qR, qB = float(two_layer_profile(fine).sum() / 4096.), float(two_layer_profile(fine + 16.).sum() / 4096.)
    want = two_layer_profile(s)
    peak = float(two_layer_profile(np.linspace(0., 32., 6401)).max())
    return float(vz_row[:16].sum() / qR - 1.), float(vz_row[16:].sum() / qB - 1.), float(np.max(np.abs(vz_row - want)) / peak)
