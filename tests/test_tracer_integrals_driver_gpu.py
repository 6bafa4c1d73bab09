"""Transport3DRK(..., integrals_every=N) and `python -m openlbmpm_amd tr3d --integrals-every N`: the /Integrals group of
SimulationResultsRK3D and the /TracerIntegrals group of ConcentrationResults, in one process and under two ranks that share this GPU over
gloo; the guard at that cadence."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_rk3d_gpu import _free_port
from test_tr3d_driver_gpu import write_ini

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = [0, 5, 10, 12]
SIZE = dict(nx=14, ny=12, nz=40)
GROUPS = ("/Integrals/", "/TracerIntegrals/")


def _ini(d):
    write_ini(d, steps=12, relax="MRT", sigma=0.05, theta=60.0, **SIZE)


def _both(paths):
    from openlbmpm_amd.results import load_results
    res = dict(load_results(paths[0]))
    res.update(load_results(paths[1]))
    return res


def _standalone_tables(d):
    """(integrals().planes, tracer_integrals().planes) of a stand-alone RK3DCSFSolver with the driver's set-up, stepped to each of STEPS"""
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
    out, done = {}, 0
    for k in STEPS:
        s.step(k - done); done = k
        out[k] = (s.integrals().planes, s.tracer_integrals().planes)
    s.close()
    return out


def test_the_driver_writes_both_groups(tmp_path, caplog):
    import logging
    from openlbmpm_amd.Transport3DRK import Transport3DRK
    from openlbmpm_amd.integrals import COLUMNS, TRACER_COLUMNS, column_names
    _ini(tmp_path)
    with caplog.at_level(logging.INFO, logger="openlbmpm_amd"):
        sim = Transport3DRK(str(tmp_path), output_dir=str(tmp_path / "out"), record_every=6, integrals_every=5)
        res = _both(sim.runTransport3DMPMCRK())
    assert sim.integral_steps == STEPS and sim.integrals.planes.shape == (40, 12) and sim.tracer_integrals.planes.shape == (40, 2, 9)
    for g in GROUPS:
        assert np.array_equal(res[g + "Steps"], np.array(STEPS, dtype=np.int64)) and res[g + "Steps"].dtype == np.int64
        assert sorted(k for k in res if k.startswith(g)) == sorted([g + "Steps", g + "Columns"] + [g + "PlanesAtStep%d" % k for k in STEPS])
    assert column_names(res["/Integrals/Columns"]) == COLUMNS and column_names(res["/TracerIntegrals/Columns"]) == TRACER_COLUMNS
    want = _standalone_tables(tmp_path)
    for k in STEPS:
        flow, tr = res["/Integrals/PlanesAtStep%d" % k], res["/TracerIntegrals/PlanesAtStep%d" % k]
        assert flow.shape == (40, 12) and np.array_equal(flow, want[k][0]), k
        assert tr.shape == (40, 2, 9) and np.array_equal(tr, want[k][1]), k
    assert res["/TracerIntegrals/PlanesAtStep12"][:, 1, 1].sum() > 1e-3       # the inlet feeds tracer 1
    lines = [r.getMessage() for r in caplog.records if "tracers integrals step " in r.getMessage()]
    flow_lines, tracer_lines = [m for m in lines if m.startswith("rk3d+tracers ")], [m for m in lines if m.startswith("tracers ")]
    assert len(flow_lines) == len(tracer_lines) == len(STEPS), lines
    assert all(w in flow_lines[-1] for w in ("saturationR", "massR", "massB", "maxSpeed")), flow_lines
    assert all(w in tracer_lines[-1] for w in ("mass0", "cmin0", "cmax0", "mass1", "cmin1", "cmax1")) and " step 12 " in tracer_lines[-1], tracer_lines
    # the records: the same set with the same values as without the integrals
    plain = Transport3DRK(str(tmp_path), output_dir=str(tmp_path / "plain"), record_every=6)
    ref = _both(plain.runTransport3DMPMCRK())
    assert not any(k.startswith(GROUPS) for k in ref)
    assert set(ref) == {k for k in res if not k.startswith(GROUPS)} and sim.records == plain.records == 3
    for key in ref:
        assert np.array_equal(ref[key], res[key]), key
    assert np.array_equal(sim.solver.get_state()[0], plain.solver.get_state()[0])


def _run(cmd, env=None):
    """one child process under a time limit of its own; the test stops at the first one that fails"""
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, cwd=ROOT, env=dict(os.environ, **(env or {})), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:] + r.stderr[-3000:])
    return r


def _torchrun(ranks, args, env=None):
    return _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
                 "--master-port", str(_free_port())] + args, env)


def _results(directory):
    files = sorted(os.listdir(directory))
    flow = [f for f in files if f.startswith("SimulationResultsRK3D")]
    conc = [f for f in files if f.startswith("ConcentrationResults")]
    assert len(flow) == 1 and len(conc) == 1, files         # ONE file each, whatever the number of ranks
    return _both((os.path.join(directory, flow[0]), os.path.join(directory, conc[0])))


def test_two_ranks_write_the_one_process_tables(tmp_path):
    _ini(tmp_path)
    cli = ["-m", "openlbmpm_amd", "tr3d", str(tmp_path), "--integrals-every", "5", "--out"]
    _run([sys.executable] + cli + [str(tmp_path / "one")])
    _torchrun(2, cli + [str(tmp_path / "two")], env=dict(LBMPM_DIST_BACKEND="gloo"))
    ref, got = _results(str(tmp_path / "one")), _results(str(tmp_path / "two"))
    assert set(got) == set(ref)
    for g in GROUPS:
        assert [int(v) for v in ref[g + "Steps"]] == STEPS and g + "PlanesAtStep12" in got
    assert ref["/TracerIntegrals/PlanesAtStep5"].shape == (40, 2, 9)
    for key in ref:
        assert np.array_equal(got[key], ref[key]), key


def test_a_nan_in_the_initial_concentration_is_met_at_step_0(tmp_path):
    from openlbmpm_amd.RKColorGradientD3Q19 import duct
    from openlbmpm_amd.Transport3DRK import Transport3DRK
    from openlbmpm_amd.results import SimulationDiverged
    _ini(tmp_path)
    dom = duct(SIZE["nx"], SIZE["ny"], SIZE["nz"])
    c0 = np.zeros((2,) + dom.shape)
    c0[0][dom == 1] = 0.5
    y, x = np.argwhere(dom[7] == 1)[11]
    c0[1, 7, y, x] = np.nan
    sim = Transport3DRK(str(tmp_path), output_dir=str(tmp_path / "out"), record_every=6, integrals_every=5, initial_concentration=c0)
    with pytest.raises(SimulationDiverged) as e:
        sim.runTransport3DMPMCRK()
    assert "step 0" in str(e.value) and "plane integrals" in str(e.value) and sim.records == 0
