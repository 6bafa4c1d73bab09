"""The tracers' first-order reaction at solid walls, without a GPU: the CPU restatement tests/wall_reaction_ref.py (Tracer3DRef with the
bounce-back line changed) against Tracer3DRef, against the analytic slit eigenmode and against its own mass balance; the conditioning of
the cases tests/test_rk3d_tracer_wall_gpu.py compares the kernels on and what a mistake there would move; the ini keys, the command
line and the refusals.

The slit: H = 16 fluid cells along x between two reactive plates, fluid at rest, started in the first even eigenmode cos(lambda x) with
lambda tan(lambda H / 2) = k / D; the mass decays as exp(-D lambda^2 t).  Measured with this reference (decay rate from step 200 to
400 / profile at step 400, both relative):
    D = 1/6:  k = 0.05  8.5e-4 / 3.9e-4   k = 1  1.3e-4 / 9.1e-5   k = inf  2.8e-6 / 6.7e-16
    D = 0.05: k = 0.05  1.3e-3 / 4.0e-5   k = 1  1.6e-3 / 2.7e-6   k = inf  1.6e-3 / 3.3e-16
The bounds, 0.5 % and 2e-3, are 3 x and 5 x the worst of them.  The mass balance closes to 1.4e-14 of the initial mass."""
import os

import numpy as np
import pytest

import param_points as P
import wall_cases as W
from helpers import rel_err
from test_tr3d_ref import prescribed_problem
from tr3d_ref import Tracer3DRef
from wall_reaction_ref import WallReactionRef, reflection, slit_case, slit_deviations

TOL = 1e-10                     # what the GPU comparison holds the kernels to (tests/test_rk3d_tracer_gpu.py)
RATE_BOUND, PROFILE_BOUND = 0.5e-2, 2e-3
SLIT = [(k, D) for D in (1. / 6., 0.05) for k in (0.05, 1.0, W.INF)]
FULL = dict(diffX=(1. / 6., 0.1, 0.2), diffY=(0.12, 0.1, 0.15), diffZ=(0.2, 0.08, 0.1), dXY=0.01, dYX=-0.02, dXZ=0.03, dZX=0.015, dYZ=-0.01, dZY=0.02,
            beta=(1.0, 0.5, 0.0), inlet_conc=(0.8, 0.4, 0.0), reaction_rate=0.03, diffJ=(0.0, 0.25, 0.1))


def drive(r, rhoR, v, G, steps):
    for _ in range(steps):
        r.substep(rhoR, v["x"], v["y"], v["z"], G["x"], G["y"], G["z"])
    return r


def test_reflection_factor():
    assert reflection(0.0) == 1.0 and reflection(W.INF) == -1.0 and reflection(1. / 3.) == 0.0
    assert reflection(0.05) == (1. - 3. * 0.05) / (1. + 3. * 0.05)
    for bad in (-0.1, float("nan")):
        with pytest.raises(ValueError):
            reflection(bad)


@pytest.mark.parametrize("open_planes", [True, False])
def test_rates_of_zero_are_the_plain_bounce_back(open_planes):
    """three tracers with the reaction A + B -> C and a full tensor, 20 sub-steps under prescribed fields, with a mineral map: bit for bit"""
    dom, rhoR, v, G, c0 = prescribed_problem(nz=16)
    t = dict(FULL, free_outlet=open_planes, dirichlet_inlet=open_planes)
    a = drive(Tracer3DRef(dom, c0, t), rhoR, v, G, 20)
    b = drive(WallReactionRef(dom, c0, t, rates=np.zeros((3, 3)), minerals=W.minerals_of(dom)), rhoR, v, G, 20)
    assert np.array_equal(a.g, b.g) and np.array_equal(a.C, b.C)
    assert np.all(b.uptake == 0.0) and b.links.sum() > 100 and np.all(b.wall_c.sum(axis=1) > 0)
    c = drive(WallReactionRef(dom, c0, t, rates=0.1), rhoR, v, G, 20)
    assert rel_err(c.C, a.C) > 1e-3


@pytest.mark.parametrize("k,D", SLIT, ids=["k=%g,D=%.3g" % c for c in SLIT])
def test_the_slit_eigenmode_decays_at_d_lambda_squared(k, D):
    dom, conc, tracer, lam, mode = slit_case(k, D)
    assert dom.shape == (4, 3, 18)
    r = WallReactionRef(dom, conc, tracer, rates=k)
    z = np.zeros(dom.shape)
    for _ in range(200):
        r.substep(z, z, z, z, z, z, z)
    m200 = r.mass()[0]
    for _ in range(200):
        r.substep(z, z, z, z, z, z, z)
    m400 = r.mass()[0]
    for y in range(3):
        for zz in range(4):
            assert np.array_equal(r.C[0, zz, y], r.C[0, 0, 0])          # (uniform along the plates)
    rate, prof = slit_deviations(m200, m400, r.C[0, 0, 0, 1:-1], D, lam, mode)
    print("slit k = %g, D = %.4g: lambda %.6f, decay rate off by %.3e, profile off by %.3e" % (k, D, lam, rate, prof))
    assert 0.1 < m400 / m200 < 1.0 - 1e-3
    assert rate < RATE_BOUND and prof < PROFILE_BOUND, (k, D, rate, prof)


def test_the_uptake_is_the_mass_that_left_a_closed_porous_ring():
    """periodic in every direction, no inlet and no outlet, no bulk reaction, a prescribed flow and interface term, three classes with
    one instantaneous: what the tracers lose is what the walls report, step by step and over 60 steps"""
    dom, rhoR, v, G, c0 = prescribed_problem(nz=16)
    t = dict(FULL, reaction_rate=0.0, free_outlet=False, dirichlet_inlet=False)
    rates = np.array([[0.02, W.INF, 0.0], [0.2, 0.01, 0.0], [1.0, 0.5, 0.0]])
    minerals = W.minerals_of(dom)
    assert W.touches_two_classes(dom, minerals) > 20
    r = WallReactionRef(dom, c0, t, rates=rates, minerals=minerals)
    m0 = r.mass()
    taken, worst_step = np.zeros(3), 0.0
    for _ in range(60):
        before = r.mass()
        r.substep(rhoR, v["x"], v["y"], v["z"], G["x"], G["y"], G["z"])
        u = r.uptake.sum(axis=1)
        worst_step = max(worst_step, float(np.max(np.abs(before - r.mass() - u) / m0)))
        taken += u
    res = np.abs(m0 - r.mass() - taken) / m0
    print("mass balance: lost %s of the initial mass, residual %s, worst single step %.3e" % ((m0 - r.mass()) / m0, res, worst_step))
    assert np.all(res < 1e-12) and worst_step < 1e-12
    assert np.all(((m0 - r.mass()) / m0)[:2] > 0.05) and taken[2] == 0.0 and abs((m0 - r.mass())[2]) / m0[2] < 1e-13


# ------------------------------------------------------------------------------------------------ the cases of the GPU comparison
def tracer_difference(a, b, fl, nT):
    return max(max(rel_err(a.C[k][fl], b.C[k][fl]), rel_err(a.g[k][:, fl], b.g[k][:, fl])) for k in range(nT))


_REFS = {}


def good(name):
    """the case's reference, run once for all the tests below: {step: (C, g)}"""
    if name not in _REFS:
        c = W.CASES[name]()
        o, snaps = W.reference(c), {}
        for n in W.STEPS:
            o.run(n - o.steps)
            snaps[n] = (np.array(o.C), np.array(o.g))
        _REFS[name] = (c, snaps)
    return _REFS[name]


class _Snap:
    def __init__(self, Cg):
        self.C, self.g = Cg


@pytest.mark.parametrize("name", sorted(W.CASES))
def test_the_cases_are_what_they_claim_and_well_conditioned(name):
    """fluid cells no multiple of 256, cells that touch two classes, every class at a wall, both tracers taken up; the reference
    started from densities rippled in the last bit stays within a tenth of the GPU tolerance of itself"""
    c, snaps = good(name)
    dom, fl = c["dom"], c["dom"] == 1
    assert int(fl.sum()) % 256 != 0 and W.touches_two_classes(dom, c["minerals"]) >= 3
    assert set(np.unique(c["minerals"][~fl])) == {0, 1, 2}
    two = W.reference(c, rR=P.last_bit(c["rR"], 0.3), rB=P.last_bit(c["rB"], 1.3))
    worst = 0.0
    for n in W.STEPS:
        two.run(n - two.steps)
        worst = max(worst, tracer_difference(two, _Snap(snaps[n]), fl, c["nT"]))
    print("conditioning, %s: the reference against itself from a start rippled in the last bit, worst over the steps %s: %.3e" % (name, W.STEPS, worst))
    assert np.any(two.flow.field("fR") != W.reference(c).run(W.STEPS[-1]).flow.field("fR"))
    assert worst < 0.1 * TOL, worst
    assert all(float(two.tr.uptake[k].sum()) != 0.0 for k in range(c["nT"]))


MISTAKES = {"the rates back at 0": lambda c: dict(rates=np.zeros(W.RATES.shape)),
            "two classes' rates exchanged": lambda c: dict(rates=W.RATES[[1, 0, 2]]),
            "two tracers' rates exchanged": lambda c: dict(rates=W.RATES[:, ::-1]),
            "every solid of class 0": lambda c: dict(minerals=np.zeros_like(c["minerals"]))}


@pytest.mark.parametrize("mistake", sorted(MISTAKES))
@pytest.mark.parametrize("name", sorted(W.CASES))
def test_a_mistake_in_the_rates_is_seen(name, mistake):
    c, snaps = good(name)
    fl = c["dom"] == 1
    bad = W.reference(c, **MISTAKES[mistake](c))
    out = []
    for n in W.STEPS:
        bad.run(n - bad.steps)
        out.append(tracer_difference(bad, _Snap(snaps[n]), fl, c["nT"]) / TOL)
    print("sensitivity, %s, %s: %s x TOL at the steps %s" % (name, mistake, ", ".join("%.3g" % v for v in out), W.STEPS))
    assert all(v >= 1000.0 for v in out), (name, mistake, out)


# ------------------------------------------------------------------------------------------------ ini, command line, refusals
def _ini(d, extra=""):
    from test_tr3d_driver_gpu import write_ini
    write_ini(d, nx=14, ny=12, nz=40, steps=4, relax="MRT", sigma=0.05, theta=60.0)
    if extra:
        with open(os.path.join(str(d), "transportsetup.ini"), "a") as fh:
            fh.write("\n[Reaction]\n" + extra)


def test_the_ini_keys(tmp_path):
    from openlbmpm_amd import config
    _ini(tmp_path)
    p = config.read_transport3d(str(tmp_path))
    assert p["wall_reaction"] is None and p["wall_mineral_file"] is None            # read only when present
    _ini(tmp_path, "WallReactionRate = 0.05, inf\n")
    p = config.read_transport3d(str(tmp_path))
    assert p["wall_reaction"] == [[0.05, W.INF]] and p["wall_mineral_file"] is None and p["reaction_rate"] == 0.0      # (Reaction = 'no')
    _ini(tmp_path, "WallReactionRate = 0.05, inf, 0.2, 0.0\nWallMineralFile = '/data/minerals.npy'\n")
    p = config.read_transport3d(str(tmp_path))
    assert p["wall_reaction"] == [[0.05, W.INF], [0.2, 0.0]] and p["wall_mineral_file"] == "/data/minerals.npy"
    for bad in ("WallReactionRate = 0.05\n", "WallReactionRate = 0.05, -1.0\n", "WallReactionRate = 0.05, nan\n", "WallReactionRate = 0.1, 0.2, 0.3, 0.4\n",
                "WallMineralFile = 'm.npy'\n", "WallReactionRate = " + ", ".join(["0.1"] * 18) + "\nWallMineralFile = 'm.npy'\n"):
        _ini(tmp_path, bad)
        with pytest.raises(config.ConfigError):
            config.read_transport3d(str(tmp_path))


def test_the_2d_tracers_refuse_the_keys(tmp_path):
    from openlbmpm_amd import config
    _ini(tmp_path, "WallReactionRate = 0.05, 0.1\n")
    with pytest.raises(config.ConfigError, match="D2Q5 tracers bounce back unchanged"):
        config.read_transport(str(tmp_path))


def test_the_command_line(tmp_path):
    from openlbmpm_amd.__main__ import main, parser
    a = parser().parse_args(["tr3d", "x", "--wall-reaction", "0.05", "inf", "--wall-minerals", "m.npy"])
    assert a.wall_reaction == [0.05, W.INF] and a.wall_minerals == "m.npy"
    a = parser().parse_args(["tr3d", "x"])
    assert a.wall_reaction is None and a.wall_minerals is None
    for model, words in (("rk3d", "rk3d runs the flow alone"), ("tr", "D2Q5 tracers"), ("rk", "2-D solvers"), ("sc", "2-D solvers")):
        with pytest.raises(SystemExit) as e:
            main([model, str(tmp_path), "--wall-reaction", "0.1"])
        assert words in str(e.value), (model, e.value)
    with pytest.raises(SystemExit):
        main(["rk3d", str(tmp_path), "--wall-minerals", "m.npy"])


def test_the_driver_checks_its_arguments(tmp_path):
    """without a GPU: the constructor reads and checks, nothing runs"""
    from openlbmpm_amd import config
    from openlbmpm_amd.Transport3DRK import Transport3DRK
    _ini(tmp_path)
    sim = Transport3DRK(str(tmp_path), output_dir=str(tmp_path / "o"))
    assert sim.wall_reaction is None and sim.wall_minerals is None
    assert Transport3DRK(str(tmp_path), output_dir=str(tmp_path / "o"), wall_reaction=0.1).wall_reaction == [[0.1, 0.1]]
    assert Transport3DRK(str(tmp_path), output_dir=str(tmp_path / "o"), wall_reaction=(0.1, W.INF)).wall_reaction == [[0.1, W.INF]]
    m = np.zeros((40, 12, 14), dtype=np.uint8)
    sim = Transport3DRK(str(tmp_path), output_dir=str(tmp_path / "o"), wall_reaction=[[0.1, 0.2], [0.3, 0.4]], wall_minerals=m)
    assert sim.wall_reaction == [[0.1, 0.2], [0.3, 0.4]]
    sim.initializeDomainBorder()
    assert sim.solid_minerals().shape == (40, 12, 14) and sim.solid_minerals().dtype == np.uint8
    for kw in (dict(wall_reaction=-0.1), dict(wall_reaction=(0.1, 0.2, 0.3)), dict(wall_reaction=[[0.1, 0.2], [0.3, 0.4]]), dict(wall_minerals=m),
               dict(wall_reaction=float("nan"))):
        with pytest.raises(config.ConfigError):
            Transport3DRK(str(tmp_path), output_dir=str(tmp_path / "o"), **kw)
    for bad in (np.zeros((40, 12, 13), dtype=np.uint8), np.full((40, 12, 14), 9), np.zeros((40, 12, 14))):
        sim = Transport3DRK(str(tmp_path), output_dir=str(tmp_path / "o"), wall_reaction=0.1, wall_minerals=bad)
        sim.initializeDomainBorder()
        with pytest.raises(config.ConfigError):
            sim.solid_minerals()
    _ini(tmp_path, "WallReactionRate = 0.05, inf\n")
    assert Transport3DRK(str(tmp_path), output_dir=str(tmp_path / "o")).wall_reaction == [[0.05, W.INF]]
    assert Transport3DRK(str(tmp_path), output_dir=str(tmp_path / "o"), wall_reaction=0.3).wall_reaction == [[0.3, 0.3]]       # the argument wins


def test_the_python_classes_check_shapes_before_the_library():
    from openlbmpm_amd.integrals import TRACER_WALL_COLUMNS, TracerWallIntegrals
    from openlbmpm_amd.rk3dcsf import wall_rates
    assert wall_rates(0.1, 3).tolist() == [[0.1, 0.1, 0.1]] and wall_rates((0.1, 0.2), 2).tolist() == [[0.1, 0.2]]
    assert wall_rates([[0.1, 0.2], [0.3, W.INF]], 2).shape == (2, 2)
    for bad, n in (((0.1, 0.2), 3), ([[0.1, 0.2]], 3), (np.zeros((9, 2)), 2), (np.zeros((2, 2, 2)), 2)):
        with pytest.raises(ValueError):
            wall_rates(bad, n)
    assert TRACER_WALL_COLUMNS == ("wall_links", "uptake", "wall_c", "nonfinite")
    t = np.zeros((3, 2, 4))
    t[:, :, 0] = 5.0; t[:, 0, 1] = (0.1, 0.2, 0.3); t[:, 1, 2] = 2.0; t[1, 1, 3] = 1.0
    w = TracerWallIntegrals(t, 7, 6)
    assert w.wall_links == 15 and w.uptake(0) == 0.1 + 0.2 + 0.3 and w.uptake(1) == 0.0 and w.nonfinite == 1
    assert w.mean_wall_concentration(1) == 6.0 / 15.0 and np.array_equal(w.column("uptake", 0), [0.1, 0.2, 0.3])
    assert set(w.summary()) == {"uptake0", "wallC0", "uptake1", "wallC1"}
    with pytest.raises(TypeError):
        TracerWallIntegrals(np.zeros((3, 2, 9)), 7, 6)
