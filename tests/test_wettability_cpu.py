"""Mixed wettability without a GPU: geometry.wall_contact_angles by hand, the driver's option (ini key, command-line flag, framing, the
perturbation model's refusal), and -- on the oracle alone -- the precondition of the separability test of
tests/test_rk3d_csf_wettability_gpu.py: two channels behind walls four cells thick do not see each other."""
import re

import numpy as np
import pytest

from helpers import rel_err
from oracle.rk3dcsf import RK3DCSFOracle
from test_oracle_rk3d_csf import blob3
from test_rk3d_csf_gpu import CRISP, SCALARS, TOL, VECTORS

from openlbmpm_amd import config
from openlbmpm_amd.geometry import wall_contact_angles


# ------------------------------------------------------------------------------------------------ wall_contact_angles
def test_cassie_average_of_an_axis_and_a_diagonal_neighbour():
    """w = 1/18 at 60 degrees, 1/36 at 120: cos = (1/18 * 1/2 - 1/36 * 1/2) / (1/18 + 1/36) = 1/6"""
    dom = np.ones((5, 5, 5), dtype=np.uint8)
    dom[2, 2, 3] = 0          # +x of the cell (2, 2, 2)
    dom[3, 1, 2] = 0          # +z -y
    th = np.full(dom.shape, np.nan)
    th[2, 2, 3], th[3, 1, 2] = 60.0, 120.0
    out = wall_contact_angles(dom, th, 90.0)
    assert abs(out[2, 2, 2] - np.degrees(np.arccos(1.0 / 6.0))) < 1e-12 and abs(out[2, 2, 2] - 80.4059317731) < 1e-9
    # a cell that sees one of them only takes its value as it stands
    assert out[2, 2, 4] == 60.0 and out[4, 0, 2] == 120.0
    # NaN off the fluid cells next to solid: the solids themselves, and fluid further away
    assert np.isnan(out[2, 2, 3]) and np.isnan(out[3, 1, 2]) and np.isnan(out[0, 4, 0])
    near = np.zeros(dom.shape, dtype=bool)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if 1 <= dz * dz + dy * dy + dx * dx <= 2:
                    near |= np.roll(dom == 0, (dz, dy, dx), axis=(0, 1, 2))
    assert np.array_equal(np.isfinite(out), near & (dom == 1))


@pytest.mark.parametrize("value", [50.0, 97.3, 1.0 / 3.0, 180.0, 0.0])
def test_a_uniform_mineral_map_gives_a_uniform_wall_map_bit_for_bit(value):
    dom = blob3()[0]
    out = wall_contact_angles(dom, np.full(dom.shape, value), 33.0)
    assert np.isfinite(out).any() and np.all(out[np.isfinite(out)] == value)
    # ... and so does the default alone
    out = wall_contact_angles(dom, np.full(dom.shape, np.nan), value)
    assert np.all(out[np.isfinite(out)] == value)


def test_nan_entries_take_the_default():
    dom = np.ones((5, 5, 5), dtype=np.uint8)
    dom[2, 2, 3] = dom[2, 2, 1] = 0
    th = np.full(dom.shape, np.nan)
    th[2, 2, 3] = 60.0
    out = wall_contact_angles(dom, th, 120.0)           # the cell between them: both along the axis, cos = (1/2 - 1/2) / 2
    assert abs(out[2, 2, 2] - 90.0) < 1e-12
    assert out[2, 2, 0] == 120.0 and out[2, 2, 4] == 60.0
    th[0, 0, 0] = 500.0                                 # read at solid voxels only
    assert np.array_equal(wall_contact_angles(dom, th, 120.0), out, equal_nan=True)
    th[2, 2, 3] = 181.0
    with pytest.raises(ValueError):
        wall_contact_angles(dom, th, 120.0)
    with pytest.raises(ValueError):
        wall_contact_angles(dom, th[:4], 120.0)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_the_wrap_is_honoured(axis):
    """a solid in the last plane of an axis is the neighbour of the fluid in its first plane"""
    dom = np.ones((6, 5, 7), dtype=np.uint8)
    solid, fluid = [2, 2, 2], [2, 2, 2]
    solid[axis], fluid[axis] = dom.shape[axis] - 1, 0
    dom[tuple(solid)] = 0
    th = np.full(dom.shape, np.nan)
    th[tuple(solid)] = 35.0
    out = wall_contact_angles(dom, th, 90.0)
    assert out[tuple(fluid)] == 35.0
    far = list(fluid); far[axis] = 1
    assert np.isnan(out[tuple(far)])
    assert int(np.isfinite(out).sum()) == 18


def test_the_cells_are_the_oracles_kind_3():
    dom, rR, rB = blob3()
    kind = RK3DCSFOracle(dom, rR, rB).field("kind")
    out = wall_contact_angles(dom, np.full(dom.shape, np.nan), 60.0)
    assert (kind == 3).any() and np.array_equal(np.isfinite(out), kind == 3)


# ------------------------------------------------------------------------------------------------ driver and configuration
def _csf_ini(d, **kw):
    from ini_fixtures import write_rk3d_csf
    write_rk3d_csf(str(d), theta=70.0, **kw)
    return d / "RKtwophasesetup3D.ini"


def test_the_ini_key_and_the_flag(tmp_path):
    from openlbmpm_amd.__main__ import parser
    ini = _csf_ini(tmp_path)
    assert config.read_rk3d(str(tmp_path))["contact_angle_file"] is None
    ini.write_text(ini.read_text() + "ContactAngleFile = '/somewhere/angles.npy'\n")
    assert config.read_rk3d(str(tmp_path))["contact_angle_file"] == "/somewhere/angles.npy"
    for model in ("rk3d", "tr3d"):
        assert parser().parse_args([model, str(tmp_path), "--contact-angles", "a.npy"]).contact_angles == "a.npy"
        assert parser().parse_args([model, str(tmp_path)]).contact_angles is None


def test_the_driver_takes_an_array_a_path_or_the_inis_file(tmp_path):
    from openlbmpm_amd.RKColorGradientD3Q19 import RKColorGradient3D
    ini = _csf_ini(tmp_path, nx=9, ny=8, nz=12)
    a = np.full((12, 8, 9), np.nan)
    a[:, 0, :] = 40.0
    np.save(tmp_path / "angles.npy", a)
    sims = [RKColorGradient3D(str(tmp_path), contact_angle_solids=a), RKColorGradient3D(str(tmp_path), contact_angle_solids=str(tmp_path / "angles.npy"))]
    ini.write_text(ini.read_text() + "ContactAngleFile = '%s'\n" % (tmp_path / "angles.npy"))
    sims.append(RKColorGradient3D(str(tmp_path)))
    for sim in sims:
        sim.initializeDomainBorder()
        assert np.array_equal(sim.solid_contact_angles(), a, equal_nan=True)
    # the wall angles the driver hands on: the duct's wall y = 0 at 40 degrees, the others at the ini's 70, the corners' neighbours between
    wall = wall_contact_angles(sims[0].isDomain, a, sims[0].par["theta"])
    assert wall[5, 1, 4] == 40.0 and wall[5, 6, 4] == 70.0 and wall[5, 4, 1] == 70.0 and 40.0 < wall[5, 1, 1] < 70.0
    with pytest.raises(config.ConfigError, match="shape"):
        s = RKColorGradient3D(str(tmp_path), contact_angle_solids=a[1:]); s.initializeDomainBorder(); s.solid_contact_angles()
    with pytest.raises(config.ConfigError, match="not found"):
        s = RKColorGradient3D(str(tmp_path), contact_angle_solids=str(tmp_path / "none.npy")); s.initializeDomainBorder(); s.solid_contact_angles()


def test_an_image_shaped_file_is_framed_like_the_image(tmp_path):
    from openlbmpm_amd.RKColorGradientD3Q19 import RKColorGradient3D
    from openlbmpm_amd.geometry import voxel_domain
    ini = _csf_ini(tmp_path)
    ini.write_text(re.sub(r"(?m)^Existance\s*=.*$", "Existance = 'yes'", ini.read_text()))
    rng = np.random.default_rng(4)
    vox = (rng.random((9, 7, 8)) < 0.7).astype(np.uint8)          # non-zero = pore
    np.save(tmp_path / "structure3D.npy", vox)
    angles = np.where(vox == 0, 30.0 + 100.0 * rng.random(vox.shape), 11.0)      # (a value on what the file calls pore is not the solid's)
    np.save(tmp_path / "angles.npy", angles)
    sim = RKColorGradient3D(str(tmp_path), structure_path=str(tmp_path / "structure3D.npy"), num_buffering_layers=3,
                            contact_angle_solids=str(tmp_path / "angles.npy"))
    sim.initializeDomainBorder()
    assert np.array_equal(sim.isDomain, voxel_domain(vox, 3)) and sim.isDomain.shape == (15, 7, 8)
    a = sim.solid_contact_angles()
    assert a.shape == sim.isDomain.shape
    assert np.all(np.isnan(a[:3])) and np.all(np.isnan(a[-3:]))                    # the buffer planes
    core = a[3:-3]
    assert np.array_equal(core[vox == 0], angles[vox == 0])                       # the file's solids, plane for plane
    assert np.all(np.isnan(core[vox != 0]))                                       # pores -- the side walls forced solid among them: the ini's angle
    forced = (sim.isDomain[3:-3] == 0) & (vox != 0)
    assert forced.any()
    wall = wall_contact_angles(sim.isDomain, a, sim.par["theta"])
    assert np.nanmin(wall) >= 30.0 and np.nanmax(wall) <= 130.0 and (wall == 70.0).any()      # (70: cells that see forced walls only)
    with pytest.raises(config.ConfigError, match="voxel file"):
        s = RKColorGradient3D(str(tmp_path), structure_path=str(tmp_path / "structure3D.npy"), num_buffering_layers=3,
                              contact_angle_solids=np.zeros(sim.isDomain.shape))
        s.initializeDomainBorder(); s.solid_contact_angles()


def test_the_perturbation_model_refuses_the_option(tmp_path):
    from ini_fixtures import write_rk3d
    from openlbmpm_amd.RKColorGradientD3Q19 import RKColorGradient3D
    from openlbmpm_amd.Transport3DRK import Transport3DRK
    write_rk3d(str(tmp_path), nx=9, ny=8, nz=12)
    with pytest.raises(config.ConfigError, match="SolidRhoR"):
        RKColorGradient3D(str(tmp_path), contact_angle_solids=np.full((12, 8, 9), 60.0))
    ini = tmp_path / "RKtwophasesetup3D.ini"
    text = ini.read_text()
    ini.write_text(text + "\n[SurfaceTension]\nSurfaceTensionType = 'Perturbation'\nContactAngleFile = 'angles.npy'\n")
    with pytest.raises(config.ConfigError, match="SolidRhoR"):
        config.read_rk3d(str(tmp_path))
    ini.write_text(text)
    with pytest.raises(config.ConfigError, match="SolidRhoR"):
        Transport3DRK(str(tmp_path), contact_angle_solids=np.full((12, 8, 9), 60.0))      # (refused before it looks for transportsetup.ini)


# ------------------------------------------------------------------------------------------------ two channels that do not see each other
TWO_CHANNEL_PARAMS = dict(relax="MRT", tauB=0.8)


def two_channels():
    """16 x 8 x 24 (nz, ny, nx): walls four cells thick at x 0..3 and 12..15 (x wraps), channel A x 4..11, channel B x 16..23, a
    spherical grain in each, the plain channel mask on the four planes at either end, red below nz - 6.  1968 fluid cells: 8 blocks."""
    nz, ny, nx = 16, 8, 24
    zz, yy, xx = np.mgrid[0:nz, 0:ny, 0:nx]
    dom = np.ones((nz, ny, nx), dtype=np.uint8)
    dom[:, :, 0:4] = 0
    dom[:, :, 12:16] = 0
    mask = dom.copy()
    dom[(zz - 7.3) ** 2 + (yy - 3.1) ** 2 + (xx - 8.2) ** 2 <= 4.0] = 0
    dom[(zz - 9.2) ** 2 + (yy - 5.7) ** 2 + (xx - 19.9) ** 2 <= 5.0] = 0
    dom[:4] = mask[:4]; dom[-4:] = mask[-4:]
    fl = dom == 1
    rR, rB = np.where(fl & (zz < nz - 6), 1.0, 0.0), np.where(fl & (zz >= nz - 6), 1.0, 0.0)
    A = np.zeros(dom.shape, dtype=bool); A[:, :, 4:12] = True
    B = np.zeros(dom.shape, dtype=bool); B[:, :, 16:24] = True
    return dom, rR, rB, A, B


def channel_changes(a, b, cells):
    """name -> the change of every field compare_all looks at between two oracles, over `cells`, in compare_all's measure"""
    out = {}
    for f in SCALARS + ("fR", "fB"):
        out[f] = rel_err(a.field(f)[cells], b.field(f)[cells])
    for vec in VECTORS:
        scale = max(max(float(np.max(np.abs(b.field(c)[cells]))) for c in vec), 1e-300)
        for c in vec:
            out[c] = rel_err(a.field(c)[cells], b.field(c)[cells], scale=scale)
    return out


def _oracle(dom, rR, rB, theta):
    return RK3DCSFOracle(dom, rR, rB, dict(TWO_CHANNEL_PARAMS, theta=theta, crisp=CRISP)).run(30)


@pytest.fixture(scope="module")
def channels():
    dom, rR, rB, A, B = two_channels()
    return dict(dom=dom, rR=rR, rB=rB, A=A, B=B, o50=_oracle(dom, rR, rB, 50.0), o130=_oracle(dom, rR, rB, 130.0))


def test_the_two_channel_lattice_is_the_one_specified():
    dom, rR, rB, A, B = two_channels()
    assert dom.shape == (16, 8, 24) and int(dom.sum()) == 1968
    assert not dom[:, :, 0:4].any() and not dom[:, :, 12:16].any()
    assert (dom[5:11][A[5:11]] == 0).any() and (dom[5:11][B[5:11]] == 0).any()          # a grain in each
    assert dom[:4][A[:4]].all() and dom[-4:][B[-4:]].all()


def test_a_channel_does_not_see_the_other_channels_state(channels):
    """(a): channel B's colours exchanged and its interface moved -- every field of channel A after 30 steps is the same bit for bit,
    the walls' phi on A's side included"""
    c = channels
    zz = np.mgrid[0:16, 0:8, 0:24][0]
    fl = c["dom"] == 1
    rR = np.where(c["B"], np.where(fl & (zz >= 7), 0.9, 0.0), c["rR"])
    rB = np.where(c["B"], np.where(fl & (zz < 7), 1.1, 0.0), c["rB"])
    other = _oracle(c["dom"], rR, rB, 50.0)
    for f in SCALARS + ("fR", "fB") + tuple(x for v in VECTORS for x in v):
        assert np.array_equal(other.field(f)[c["A"] & fl], c["o50"].field(f)[c["A"] & fl]), f
        assert not np.array_equal(other.field(f)[c["B"] & fl], c["o50"].field(f)[c["B"] & fl]), f
    near_a = np.zeros(c["dom"].shape, dtype=bool); near_a[:, :, 3] = near_a[:, :, 12] = True
    wet = c["o50"].field("kind") == 2
    assert (wet & near_a).any() and np.array_equal(other.field("phi")[wet & near_a], c["o50"].field("phi")[wet & near_a])


def test_the_contact_angle_moves_every_field_of_each_channel(channels):
    """(b): theta 50 -> 130 changes every compared field by >= 1000 TOL in channel A and in channel B: a channel that ran with the other
    channel's angle could not pass for its own"""
    c = channels
    fl = c["dom"] == 1
    for name in ("A", "B"):
        for f, e in channel_changes(c["o130"], c["o50"], c[name] & fl).items():
            assert e >= 1000 * TOL, (name, f, e)


def test_a_ripple_in_the_last_bit_stays_far_below_the_tolerance(channels):
    """(c): initial densities rippled in their last bit move no field by more than TOL / 10 in 30 steps -- the lattice amplifies nothing,
    so TOL against the oracle per channel means what it means on blob3"""
    c = channels
    rng = np.random.default_rng(7)
    ripple = lambda a: a * (1.0 + (rng.integers(-1, 2, a.shape)) * 2.0 ** -52)
    other = _oracle(c["dom"], ripple(c["rR"]), ripple(c["rB"]), 50.0)
    fl = c["dom"] == 1
    assert not np.array_equal(other.field("fR"), c["o50"].field("fR"))
    for f, e in channel_changes(other, c["o50"], fl).items():
        assert e <= TOL / 10, (f, e)
