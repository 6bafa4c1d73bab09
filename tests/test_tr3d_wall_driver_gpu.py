"""Transport3DRK(..., wall_reaction=, wall_minerals=, integrals_every=N) and `python -m openlbmpm_amd tr3d --wall-reaction ...`: the
/WallReaction and /TracerWallIntegrals groups of ConcentrationResults against the class API, in one process and under two ranks that
share this GPU over gloo; without the option the result files have neither group."""
import os
import sys

import numpy as np
import pytest

from test_tracer_integrals_driver_gpu import SIZE, STEPS, _both, _ini, _results, _run, _torchrun

pytestmark = pytest.mark.gpu

INF = float("inf")
RATES = [[0.05, INF], [0.3, 0.1]]            # [class][tracer]
NEW = ("/WallReaction/", "/TracerWallIntegrals/")


def minerals():
    return np.random.default_rng(3).integers(0, 2, size=(SIZE["nz"], SIZE["ny"], SIZE["nx"])).astype(np.uint8)


def _standalone(d, m):
    """the tables of a stand-alone RK3DCSFSolver with the driver's set-up and set_wall_reaction, stepped to each of STEPS"""
    from openlbmpm_amd import config
    from openlbmpm_amd.RKColorGradientD3Q19 import duct
    from openlbmpm_amd.Transport3DRK import _CSFTracerSlab
    from openlbmpm_amd.geometry import initial_densities_rk3d
    p, t = config.read_rk3d(str(d)), config.read_transport3d(str(d))
    dom = duct(p["nx"], p["ny"], p["nz"])
    nz = dom.shape[0]
    rR, rB = initial_densities_rk3d(dom, 10, p["rho0R"], p["rho0B"])
    s = _CSFTracerSlab(dom, p, t, 0).solver
    s.set_macro(rR, rB)
    planes = np.arange(nz)[:, None, None]
    s.set_concentration(0, np.where((dom == 1) & (planes <= nz - 10), 1.0, 0.0))
    s.set_concentration(1, np.zeros(dom.shape))
    s.set_wall_reaction(RATES, m)
    out, done = {}, 0
    for k in STEPS:
        s.step(k - done); done = k
        out[k] = (s.tracer_integrals().planes, s.tracer_wall_integrals().planes, s.get_concentration(0))
    s.close()
    return out


def test_the_driver_writes_the_rates_and_the_uptake_tables(tmp_path):
    from openlbmpm_amd.Transport3DRK import Transport3DRK
    from openlbmpm_amd.integrals import TRACER_WALL_COLUMNS, column_names
    _ini(tmp_path)
    m = minerals()
    np.save(str(tmp_path / "minerals.npy"), m)
    sim = Transport3DRK(str(tmp_path), output_dir=str(tmp_path / "out"), record_every=6, integrals_every=5, wall_reaction=RATES,
                        wall_minerals=str(tmp_path / "minerals.npy"))
    res = _both(sim.runTransport3DMPMCRK())
    assert res["/WallReaction/Rates"].tolist() == RATES
    g = "/TracerWallIntegrals/"
    assert sorted(k for k in res if k.startswith(g)) == sorted([g + "Steps", g + "Columns"] + [g + "PlanesAtStep%d" % k for k in STEPS])
    assert [int(v) for v in res[g + "Steps"]] == STEPS and column_names(res[g + "Columns"]) == TRACER_WALL_COLUMNS
    assert sim.tracer_wall_integrals.planes.shape == (40, 2, 4) and sim.solver.solver.wall_reaction.tolist() == RATES
    want = _standalone(tmp_path, m)
    for k in STEPS:
        assert np.array_equal(res[g + "PlanesAtStep%d" % k], want[k][1]), k
        assert np.array_equal(res["/TracerIntegrals/PlanesAtStep%d" % k], want[k][0]), k
    assert np.all(want[0][1][:, :, 1:] == 0.0) and want[12][1][:, 0, 1].sum() > 1e-3          # nothing before the first step; then the walls take tracer 0
    assert np.array_equal(res["/TransportMacro/TracerConcType0in2"], want[12][2])
    # without the option: neither group, and other concentrations
    plain = Transport3DRK(str(tmp_path), output_dir=str(tmp_path / "plain"), record_every=6, integrals_every=5)
    ref = _both(plain.runTransport3DMPMCRK())
    assert not any(k.startswith(NEW) for k in ref) and set(ref) == {k for k in res if not k.startswith(NEW)}
    assert not np.array_equal(ref["/TransportMacro/TracerConcType0in2"], res["/TransportMacro/TracerConcType0in2"])
    assert plain.solver.solver.wall_reaction is None
    # the ini's keys give the same files as the arguments
    with open(os.path.join(str(tmp_path), "transportsetup.ini"), "a") as fh:
        fh.write("\n[Reaction]\nWallReactionRate = 0.05, inf, 0.3, 0.1\nWallMineralFile = '%s'\n" % (tmp_path / "minerals.npy"))
    ini = Transport3DRK(str(tmp_path), output_dir=str(tmp_path / "ini"), record_every=6, integrals_every=5)
    got = _both(ini.runTransport3DMPMCRK())
    assert set(got) == set(res)
    for key in res:
        assert np.array_equal(got[key], res[key]), key


def test_two_ranks_write_the_one_process_tables(tmp_path):
    _ini(tmp_path)
    np.save(str(tmp_path / "minerals.npy"), minerals())
    cli = ["-m", "openlbmpm_amd", "tr3d", str(tmp_path), "--integrals-every", "5", "--wall-reaction", "0.05", "inf", "0.3", "0.1",
           "--wall-minerals", str(tmp_path / "minerals.npy"), "--out"]
    _run([sys.executable] + cli + [str(tmp_path / "one")])
    _torchrun(2, cli + [str(tmp_path / "two")], env=dict(LBMPM_DIST_BACKEND="gloo"))
    ref, got = _results(str(tmp_path / "one")), _results(str(tmp_path / "two"))
    assert set(got) == set(ref) and ref["/WallReaction/Rates"].tolist() == RATES
    assert ref["/TracerWallIntegrals/PlanesAtStep5"].shape == (40, 2, 4) and [int(v) for v in ref["/TracerWallIntegrals/Steps"]] == STEPS
    assert ref["/TracerWallIntegrals/PlanesAtStep12"][:, 0, 1].sum() > 1e-3
    for key in ref:
        assert np.array_equal(got[key], ref[key]), key
