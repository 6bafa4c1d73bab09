"""Per-cell contact angles of the 3-D CSF solver (lbmpm_rk3dcsf_set_contact_angles, csf3d_gradient<true>) on the GPU.

No oracle of its own: the angle enters the step in one place, the wetting rule at the fluid cells next to solid, so exact identities
against scalar-angle runs of the same library carry the tests -- a uniform map IS the scalar run; two channels that cannot see each other
(tests/test_wettability_cpu.py shows that on the oracle) each equal the scalar run of their angle, and the oracle at that angle; the
first step's gradient, whose phase field does not depend on the angle yet, equals cell by cell that of the scalar run with the cell's
angle.  Then slabs, both variants, restarts and a map changed mid-run against each other, the refusals, and one sessile-droplet pair."""
import os

import numpy as np
import pytest

from test_oracle_rk3d_csf import blob3
from test_rk3d_csf_gpu import RK3DCSFOracle, _SLAB_FIELDS, compare_all, solver
from test_wettability_cpu import TWO_CHANNEL_PARAMS, two_channels

pytestmark = pytest.mark.gpu

FIELDS = ("fR", "fB", "rhoR", "rhoB", "phi", "Gx", "Gy", "Gz", "Fx", "Fy", "Fz", "K", "vx", "vy", "vz")
PALETTE = (20.0, 75.0, 110.0, 165.0)


def kinds(dom):
    s = solver(dom, None)
    k = s.get("kind")
    s.close()
    return k


def wall_cells(dom):
    return kinds(dom) == 3


def on_walls(dom, values):
    """values at the fluid cells next to solid, NaN elsewhere"""
    return np.where(wall_cells(dom), values, np.nan)


def random_map(dom, seed=11):
    rng = np.random.default_rng(seed)
    return on_walls(dom, rng.choice(np.array(PALETTE), size=dom.shape))


def run(dom, rR, rB, par, steps, theta_map=None):
    s = solver(dom, par)
    if theta_map is not None:
        s.set_contact_angles(theta_map)
    s.set_macro(rR, rB)
    s.step(steps)
    return s


def same(a, b, fields=FIELDS, cells=None, what=""):
    for f in fields:
        x, y = a[f] if isinstance(a, dict) else a.get(f), b[f] if isinstance(b, dict) else b.get(f)
        if cells is not None:
            x, y = x[cells], y[cells]
        assert np.array_equal(x, y), (what, f, float(np.max(np.abs(x - y))))


# ------------------------------------------------------------------------------------------------ 1. a uniform map is the scalar
def test_a_uniform_map_equals_the_scalar_angle_bit_for_bit():
    dom, rR, rB = blob3()
    par = dict(relax="MRT", tauB=0.8, theta=97.0)
    a50 = run(dom, rR, rB, dict(par, theta=50.0), 30)
    a97 = run(dom, rR, rB, par, 30)
    s = solver(dom, par)
    s.set_macro(rR, rB); s.get("rhoR")                            # (the observers' staging array comes with the first get: not the map's)
    before = s.device_bytes
    s.set_contact_angles(on_walls(dom, 50.0))
    grown = s.device_bytes - before
    assert 0 < grown <= 24 * s.num_fluid_nodes, (grown, s.num_fluid_nodes)
    s.set_contact_angles(on_walls(dom, 50.0))                     # again: the same memory
    assert s.device_bytes - before == grown
    s.set_macro(rR, rB)
    assert s.device_bytes - before == grown                       # set_macro keeps the map
    s.step(30)
    same(s, a50, what="uniform map 50 against theta = 50")
    assert not np.array_equal(a50.get("Gx"), a97.get("Gx"))       # (the angle matters here)
    s.set_contact_angles(None)
    assert s.device_bytes == before
    s.set_macro(rR, rB)
    s.step(30)
    same(s, a97, what="back to the scalar 97")
    for x in (s, a50, a97):
        x.close()


# ------------------------------------------------------------------------------------------------ 2. two channels, two angles
class _Channel:
    """a solver or an oracle seen through one channel: compare_all's `dom`, `get` and `field` restricted to it (its walls' faces included)"""

    def __init__(self, inner, dom, ext):
        self.inner, self.ext = inner, ext
        self.dom = np.where(ext, dom, 0).astype(np.uint8)

    def _cut(self, a):
        return np.where(self.ext[..., None] if a.ndim == 4 else self.ext, a, 0)

    def get(self, f):
        return self._cut(self.inner.get(f))

    def field(self, f):
        return self._cut(self.inner.field(f))


def _channel_extents(dom):
    """the channels with the wall faces next to them: A x 3 .. 12, B x 15 .. 23 and 0 (x wraps)"""
    A = np.zeros(dom.shape, dtype=bool); A[:, :, 3:13] = True
    B = np.zeros(dom.shape, dtype=bool); B[:, :, 15:24] = True; B[:, :, 0] = True
    return A, B


@pytest.mark.parametrize("relax,variant,over", [("MRT", 0, {}), ("SRT", 0, {}), ("MRT", 1, {}), ("SRT", 1, {}), ("MRT", 0, dict(outlet="Convective"))])
def test_each_channel_runs_with_its_own_angle(relax, variant, over):
    dom, rR, rB, A, B = two_channels()
    extA, extB = _channel_extents(dom)
    par = dict(TWO_CHANNEL_PARAMS, relax=relax, variant=variant, theta=97.0); par.update(over)
    opar = {k: v for k, v in par.items() if k != "variant"}
    theta = on_walls(dom, np.where(A, 50.0, 130.0))
    wet = kinds(dom) == 2
    m = solver(dom, par); m.set_contact_angles(theta); m.set_macro(rR, rB)
    s50 = solver(dom, dict(par, theta=50.0)); s50.set_macro(rR, rB)
    s130 = solver(dom, dict(par, theta=130.0)); s130.set_macro(rR, rB)
    o50, o130 = RK3DCSFOracle(dom, rR, rB, dict(opar, theta=50.0)), RK3DCSFOracle(dom, rR, rB, dict(opar, theta=130.0))
    done = 0
    for k in (1, 30):
        for x in (m, s50, s130):
            x.step(k - done)
        o50.run(k - done); o130.run(k - done)
        done = k
        fl = dom == 1
        same(m, s50, cells=A & fl, what="channel A, step %d" % k)
        same(m, s130, cells=B & fl, what="channel B, step %d" % k)
        # phi of the wetting solids on each channel's wall faces and around its grain
        same(m, s50, fields=("phi",), cells=extA & wet, what="walls of A, step %d" % k)
        same(m, s130, fields=("phi",), cells=extB & wet, what="walls of B, step %d" % k)
        assert (extA & wet)[:, :, 3].any() and (extA & wet)[:, :, 12].any() and (extB & wet)[:, :, 15].any() and (extB & wet)[:, :, 0].any()
        compare_all(_Channel(m, dom, extA), _Channel(o50, dom, extA), "channel A against the oracle at 50, step %d" % k)
        compare_all(_Channel(m, dom, extB), _Channel(o130, dom, extB), "channel B against the oracle at 130, step %d" % k)
    assert not np.array_equal(m.get("Gx")[A & fl], s130.get("Gx")[A & fl]) and not np.array_equal(m.get("Gx")[B & fl], s50.get("Gx")[B & fl])
    for x in (m, s50, s130):
        x.close()


# ------------------------------------------------------------------------------------------------ 3. cell by cell
def test_the_first_gradient_takes_each_cells_own_angle():
    """phi of step 1 does not depend on the angle, so G of step 1 at a cell next to solid is that of the scalar run with the cell's angle"""
    dom, rR, rB = blob3()
    par = dict(relax="MRT", tauB=0.8, theta=97.0)
    theta = random_map(dom)
    wall = np.isfinite(theta)
    assert all((theta[wall] == v).sum() > 20 for v in PALETTE)
    m = solver(dom, par)
    m.set_contact_angles(theta)
    assert np.array_equal(m.get("theta"), np.where(wall, theta, 0.0))         # before set_macro too
    m.set_macro(rR, rB); m.step(1)
    assert np.array_equal(m.get("theta"), np.where(wall, theta, 0.0))
    scalar = {v: run(dom, rR, rB, dict(par, theta=v), 1) for v in PALETTE}
    moved = 0
    for c in ("Gx", "Gy", "Gz"):
        g = m.get(c)
        for v, s in scalar.items():
            ref = s.get(c)
            assert np.array_equal(g[wall & (theta == v)], ref[wall & (theta == v)]), (c, v)
            assert np.array_equal(g[~wall], ref[~wall]), (c, v)
        moved += int((scalar[20.0].get(c)[wall] != scalar[165.0].get(c)[wall]).sum())
    assert moved > 50                                                          # (the rule acts at step 1: the angles tell the runs apart)
    u = solver(dom, par); u.set_macro(rR, rB)
    assert np.array_equal(u.get("theta"), np.where(wall, 97.0, 0.0))           # no map: the scalar's
    for x in [m, u] + list(scalar.values()):
        x.close()


# ------------------------------------------------------------------------------------------------ 4. cuts and paths
PATH_PARAMS = dict(TWO_CHANNEL_PARAMS, theta=97.0, sigma=0.06, velocityZR=0.0, velocityZB=-3.0e-3)


@pytest.fixture(scope="module")
def undivided():
    """the 16-plane two-channel lattice under the random map: the state after 10 steps, the fields after 20"""
    dom, rR, rB = two_channels()[:3]
    theta = random_map(dom, seed=5)
    s = run(dom, rR, rB, PATH_PARAMS, 10, theta)
    at10 = {f: s.get(f) for f in ("fR", "fB", "Fx", "Fy", "Fz")}
    s.step(10)
    out = dict(dom=dom, rR=rR, rB=rB, theta=theta, at10=at10, at20={f: s.get(f) for f in _SLAB_FIELDS})
    s.close()
    return out


@pytest.mark.parametrize("nslabs", [2, 3])
def test_slabs_equal_the_undivided_lattice(undivided, nslabs):
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster
    u = undivided
    c = RK3DCSFCluster(u["dom"], PATH_PARAMS, nslabs=nslabs, diagnostics=True)
    c.set_contact_angles(u["theta"])
    assert np.array_equal(c.get("theta"), np.where(np.isfinite(u["theta"]), u["theta"], 0.0))
    c.set_macro(u["rR"], u["rB"])
    c.step(20)
    same(c, u["at20"], fields=_SLAB_FIELDS, what="%d slabs" % nslabs)
    with pytest.raises(ValueError):
        c.set_contact_angles(u["theta"][1:])
    c.close()


def test_the_full_path_equals_the_bulk_skip(undivided):
    u = undivided
    s = run(u["dom"], u["rR"], u["rB"], dict(PATH_PARAMS, variant=1), 20, u["theta"])
    same(s, u["at20"], fields=_SLAB_FIELDS, what="variant 1")
    s.close()


def test_a_restart_with_the_map_continues_bit_for_bit(undivided):
    u = undivided
    s = solver(u["dom"], PATH_PARAMS)
    s.set_pdf(u["at10"]["fR"], u["at10"]["fB"], force=(u["at10"]["Fx"], u["at10"]["Fy"], u["at10"]["Fz"]))
    s.set_contact_angles(u["theta"])
    s.step(10)
    same(s, u["at20"], fields=_SLAB_FIELDS, what="restart")
    s.close()


def test_a_map_changed_mid_run_equals_a_restart_with_the_new_map(undivided):
    u = undivided
    new = random_map(u["dom"], seed=23)
    assert not np.array_equal(new, u["theta"], equal_nan=True)
    a = run(u["dom"], u["rR"], u["rB"], PATH_PARAMS, 10, u["theta"])
    a.set_contact_angles(new)
    assert a.steps_done == 10
    a.step(10)
    b = solver(u["dom"], PATH_PARAMS)
    b.set_contact_angles(new)
    b.set_pdf(u["at10"]["fR"], u["at10"]["fB"], force=(u["at10"]["Fx"], u["at10"]["Fy"], u["at10"]["Fz"]))        # set_pdf keeps the map
    b.step(10)
    same(a, b, fields=_SLAB_FIELDS, what="changed at step 10")
    assert not np.array_equal(a.get("Gx"), u["at20"]["Gx"])
    a.close(); b.close()


def test_two_processes_over_torch_distributed_equal_the_undivided_lattice(undivided, tmp_path):
    """started the way tests/test_rk3d_csf_gpu.py starts its two ranks (gloo: both share the one GPU)"""
    import subprocess
    import sys
    from test_rk3d_gpu import _free_port
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    u = undivided
    np.save(tmp_path / "map.npy", u["theta"])
    script = tmp_path / "w.py"
    script.write_text('''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np, torch, torch.distributed as dist
from test_wettability_cpu import two_channels
from test_rk3d_csf_wettability_gpu import PATH_PARAMS
from openlbmpm_amd.rk3dcsf import RK3DCSFDistributed
torch.cuda.set_device(0)
dist.init_process_group("gloo")
dom, rR, rB = two_channels()[:3]
d = RK3DCSFDistributed(dom, PATH_PARAMS, device=0)
d.set_contact_angles(np.load(os.path.join(%r, "map.npy")))
d.set_macro(rR, rB)
d.step(20)
for f in ("fR", "phi", "Gx", "Fz", "rec_vz", "theta"):
    g = d.gather(d.get(f))
    if dist.get_rank() == 0:
        np.save(os.path.join(%r, f + ".npy"), g)
d.close(); dist.destroy_process_group()
''' % (root, root, str(tmp_path), str(tmp_path)))
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(script)], timeout=300)
    for f in ("fR", "phi", "Gx", "Fz", "rec_vz"):
        assert np.array_equal(u["at20"][f], np.load(tmp_path / (f + ".npy"))), f
    assert np.array_equal(np.load(tmp_path / "theta.npy"), np.where(np.isfinite(u["theta"]), u["theta"], 0.0))


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_leave_the_run_as_it_was():
    from openlbmpm_amd._lib import ERR_INVALID, LbmpmError
    dom, rR, rB = blob3()
    par = dict(relax="MRT", tauB=0.8, theta=97.0)
    theta = random_map(dom)
    wall = np.isfinite(theta)
    z, y, x = [int(i[len(i) // 2]) for i in np.nonzero(wall)]
    never = run(dom, rR, rB, par, 5, theta)
    s = run(dom, rR, rB, par, 5, theta)
    for bad in (np.nan, 180.5, -1.0, np.inf):
        t = theta.copy(); t[z, y, x] = bad
        with pytest.raises(LbmpmError) as e:
            s.set_contact_angles(t)
        assert e.value.status == ERR_INVALID and "(%d, %d, %d)" % (z, y, x) in str(e.value), str(e.value)
        assert np.array_equal(s.get("theta"), never.get("theta"))
    with pytest.raises(ValueError):
        s.set_contact_angles(theta[:, :, 1:])
    with pytest.raises(ValueError):
        s.set_contact_angles(theta.reshape(-1))
    assert s.steps_done == 5
    s.step(5); never.step(5)
    same(s, never, what="after refused calls")
    # NaN off the cells next to solid is what the map carries anyway; anything else there is ignored too
    t = np.where(wall, theta, -77.0)
    s.set_contact_angles(t)
    s.step(3); never.step(3)
    same(s, never, what="values off the walls are ignored")
    # 0 and 180 themselves are angles
    t = theta.copy(); t[z, y, x] = 180.0; t[wall & (theta == 20.0)] = 0.0
    s.set_contact_angles(t)
    # without a wetting rule there is nothing to apply the angles to
    w0 = run(dom, rR, rB, dict(par, wetting=0), 5)
    w0_never = run(dom, rR, rB, dict(par, wetting=0), 5)
    for arg in (theta, None):
        with pytest.raises(LbmpmError) as e:
            w0.set_contact_angles(arg)
        assert e.value.status == ERR_INVALID
    w0.step(5); w0_never.step(5)
    same(w0, w0_never, what="wetting 0")
    for q in (s, never, w0, w0_never):
        q.close()


# ------------------------------------------------------------------------------------------------ 6. physics
def test_two_faces_of_a_wall_take_their_own_contact_angles():
    """tests/test_rk3d_csf_gpu.py::test_sessile_droplet_takes_the_prescribed_contact_angle twice in one lattice: a wall four cells thick
    (x 0 .. 3; x wraps) whose faces carry 60 and 120 degrees through geometry.wall_contact_angles, a red cap of radius 14 on each,
    52 fluid cells between the faces (the caps end up 18 and 10 cells high).  Each cap shows 180 - theta of its face, measured as there."""
    from openlbmpm_amd.geometry import wall_contact_angles
    nx, ny, nz = 56, 56, 64
    dom = np.ones((nz, ny, nx), dtype=np.uint8)
    dom[:, :, 0:4] = 0
    zz, yy, xx = np.mgrid[0:nz, 0:ny, 0:nx]
    disc = (zz - nz / 2) ** 2 + (yy - ny / 2) ** 2
    red = (disc + (xx - 4.0) ** 2 <= 14.0 ** 2) | (disc + (xx - 55.0) ** 2 <= 14.0 ** 2)
    fl = dom == 1
    mineral = np.full(dom.shape, np.nan)
    mineral[:, :, 2:4] = 60.0          # the face the fluid at x = 4 sees
    mineral[:, :, 0:2] = 120.0         # the face the fluid at x = 55 sees
    theta = wall_contact_angles(dom, mineral, 90.0)
    assert np.all(theta[:, :, 4] == 60.0) and np.all(theta[:, :, 55] == 120.0) and int(np.isfinite(theta).sum()) == 2 * ny * nz
    par = dict(relax="MRT", sigma=0.03, beta=0.7, theta=90.0, velocityZR=0.0, velocityZB=0.0, densityBL=1.0, densityRL=0.0)
    s = solver(dom, par)
    s.set_contact_angles(theta)
    s.set_macro(np.where(red & fl, 1.0, 0.0), np.where(~red & fl, 1.0, 0.0))
    s.step(12000)
    phi = s.get("phi")
    assert np.all(np.isfinite(phi))
    inside = (phi > 0) & fl
    got = {}
    for want, axis, layer in ((60.0, phi[nz // 2, ny // 2, 4:], 4), (120.0, phi[nz // 2, ny // 2, 55:3:-1], 55)):
        k = int(np.argmax(axis <= 0))
        h = 0.5 + (k - 1) + axis[k - 1] / (axis[k - 1] - axis[k])          # the wall sits half a cell below the first fluid cell
        a = np.sqrt(float(inside[:, :, layer].sum()) / np.pi)
        got[want] = np.degrees(2. * np.arctan(h / a))
        print("face at %g degrees: red cap's angle %.2f (h %.2f, a %.2f)" % (want, got[want], h, a))
    for want, g in got.items():
        assert abs(g - (180. - want)) < 6.0, "red cap's angle %.1f on the face of ContactAngle %.0f" % (g, want)
    assert got[60.0] - got[120.0] > 40.0, got
    s.close()


# ------------------------------------------------------------------------------------------------ 7. the driver
def test_the_driver_applies_the_map_and_records_it(tmp_path):
    """RKColorGradient3D(..., contact_angle_solids=): the run equals a stand-alone solver given wall_contact_angles of the same array, the
    result file holds the angles in force, and a run continued from a checkpoint applies the map again"""
    from ini_fixtures import write_rk3d_csf
    from openlbmpm_amd import config
    from openlbmpm_amd.RKColorGradientD3Q19 import RKColorGradient3D, _CSFSlab, duct
    from openlbmpm_amd.geometry import initial_densities_rk3d, wall_contact_angles
    from openlbmpm_amd.results import load_results
    write_rk3d_csf(str(tmp_path), theta=70.0, nx=14, ny=12, nz=32, steps=12, relax="MRT")
    dom = duct(14, 12, 32)
    mineral = np.full(dom.shape, np.nan)
    mineral[:, 0, :] = 35.0
    mineral[:, :, -1] = 150.0
    np.save(tmp_path / "angles.npy", mineral)
    sim = RKColorGradient3D(str(tmp_path), output_dir=str(tmp_path / "out"), record_every=6, contact_angle_solids=str(tmp_path / "angles.npy"),
                            checkpoint_every=6)
    res = load_results(sim.runRKColorGradient3D())
    p = config.read_rk3d(str(tmp_path))
    wall = wall_contact_angles(dom, mineral, 70.0)
    assert set(np.unique(wall[np.isfinite(wall)])) >= {35.0, 70.0, 150.0}
    assert np.array_equal(res["/Wettability/ContactAngle"], np.where(np.isfinite(wall), wall, 0.0))
    s = _CSFSlab(dom, p, 0).solver
    s.set_contact_angles(wall)
    s.set_macro(*initial_densities_rk3d(dom, 8, p["rho0R"], p["rho0B"]))
    s.step(12)
    last = sim.records - 1
    assert np.array_equal(res["/FluidMacro/FluidDensityRin%d" % last], s.get("rec_rhoR"))
    assert np.array_equal(res["/FluidVelocity/FluidVelocityZAt%d" % last], s.get("rec_vz"))
    plain = _CSFSlab(dom, p, 0).solver
    plain.set_macro(*initial_densities_rk3d(dom, 8, p["rho0R"], p["rho0B"])); plain.step(12)
    assert not np.array_equal(plain.get("rec_vz"), s.get("rec_vz"))          # (the map matters in this run)
    # from the checkpoint at step 6, with the same argument
    again = RKColorGradient3D(str(tmp_path), output_dir=str(tmp_path / "out2"), record_every=6, contact_angle_solids=mineral,
                              restart_from=sim.checkpoint_path)
    res2 = load_results(again.runRKColorGradient3D())
    assert np.array_equal(res2["/Wettability/ContactAngle"], res["/Wettability/ContactAngle"])
    assert np.array_equal(res2["/FluidVelocity/FluidVelocityZAt%d" % (again.records - 1)], s.get("rec_vz"))
    s.close(); plain.close()
