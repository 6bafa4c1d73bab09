"""RKColorGradient3D(..., steady_every=N, steady_tol=t) and python -m openlbmpm_amd rk3d ... --steady-every N: the /Steady group of the
result file and the early stop, for both 3-D models, in one process and under two ranks that share this GPU over gloo.

The lattice is a 16 x 16 x 32 duct, 3000 steps, a table every 100.  The early stop calibrates itself: its tolerance is the geometric mean
of the least and the largest velocity_change of the monitor-only run, so the crossing k* lies inside that run by construction wherever the
series is not constant.  Checked beforehand with the CPU oracles' velocity fields (oracle/rk3d.py, oracle/rk3dcsf.py; the same set-up):
the series falls from 1 to 4.9e-2 (perturbation model) and from 1.8 to 2.5e-3 (CSF), the crossings are at k* = 300 and k* = 500 -- no need
to lengthen the run.
"""
import os

import numpy as np
import pytest

from test_drivers_gpu import _free_port

pytestmark = pytest.mark.gpu

TOTAL, EVERY = 3000, 100
STEPS = list(range(EVERY, TOTAL + 1, EVERY))           # the steps with a table: step 0 marks


def _write_ini(d, tension):
    from ini_fixtures import write_rk3d, write_rk3d_csf
    (write_rk3d_csf if tension == "CSF" else write_rk3d)(str(d), nx=16, ny=16, nz=32, steps=TOTAL)


def _standalone(d, tension):
    """mark_change() at the second-last multiple and change() at the last of a stand-alone solver with the driver's set-up"""
    from openlbmpm_amd import config
    from openlbmpm_amd.RKColorGradientD3Q19 import PARAM_KEYS, _CSFSlab, duct
    from openlbmpm_amd.geometry import initial_densities_rk3d
    from openlbmpm_amd.rk3d import RK3DSlab
    p = config.read_rk3d(str(d))
    dom = duct(p["nx"], p["ny"], p["nz"])
    rR, rB = initial_densities_rk3d(dom, min(10, p["nz"] // 4), p["rho0R"], p["rho0B"])
    if tension == "CSF":
        s = _CSFSlab(dom, p, 0).solver
        s.set_macro(rR, rB)
        s.step(STEPS[-2])
        s.mark_change()
        s.step(EVERY)
    else:
        s = RK3DSlab(dom, 0, dom.shape[0], {k: p[k] for k in PARAM_KEYS})
        s.set_density(rR, rB)
        s.step_single(STEPS[-2])
        s.phase_field(diagnostics=True)
        s.mark_change()
        s.step_single(EVERY)
        s.phase_field(diagnostics=True)
    g = s.change()
    s.close()
    return g


def _run(d, out, steps=None, **kw):
    from openlbmpm_amd.RKColorGradientD3Q19 import RKColorGradient3D
    from openlbmpm_amd.results import load_results
    sim = RKColorGradient3D(str(d), output_dir=str(out), **kw)
    if steps is not None:
        sim.timeSteps = steps
    return sim, load_results(sim.runRKColorGradient3D())


@pytest.fixture(scope="module", params=["perturbation", "CSF"])
def monitored(request, tmp_path_factory):
    """the monitor-only run through the command line, and what the early-stop tests derive from it"""
    import logging
    from openlbmpm_amd.__main__ import main
    from openlbmpm_amd.results import load_results
    d = tmp_path_factory.mktemp("steady_" + request.param)
    _write_ini(d, request.param)
    out = d / "out"
    lines = []

    class Keep(logging.Handler):
        def emit(self, record):
            lines.append(record.getMessage())
    log, keep = logging.getLogger("openlbmpm_amd"), Keep()
    level = log.level
    log.addHandler(keep); log.setLevel(logging.INFO)
    try:
        assert main(["rk3d", str(d), "--out", str(out), "--steady-every", str(EVERY)]) == 0
    finally:
        log.removeHandler(keep); log.setLevel(level)
    files = os.listdir(out)
    assert len(files) == 1, files
    res = load_results(str(out / files[0]))
    v = res["/Steady/Criteria"][:, 2]
    print("%s velocity_change every %d steps: %s" % (request.param, EVERY, " ".join("%.3e" % x for x in v)))
    assert v.min() < v.max()
    tol = float(np.sqrt(v.min() * v.max()))
    kstar = int(res["/Steady/Criteria"][int(np.argmax(v <= tol)), 0])
    print("%s tol %.6e k* %d" % (request.param, tol, kstar))
    return dict(dir=d, tension=request.param, res=res, lines=lines, tol=tol, kstar=kstar)


def test_the_cli_writes_the_steady_group(monitored):
    from openlbmpm_amd.change import COLUMNS, CRITERIA_COLUMNS, Change
    from openlbmpm_amd.integrals import column_names
    res, d, tension = monitored["res"], monitored["dir"], monitored["tension"]
    assert np.array_equal(res["/Steady/Steps"], np.array(STEPS, dtype=np.int64)) and res["/Steady/Steps"].dtype == np.int64
    assert column_names(res["/Steady/Columns"]) == COLUMNS and column_names(res["/Steady/CriteriaColumns"]) == CRITERIA_COLUMNS
    assert sorted(k for k in res if k.startswith("/Steady/")) == sorted(
        ["/Steady/Steps", "/Steady/Columns", "/Steady/Criteria", "/Steady/CriteriaColumns"] + ["/Steady/PlanesAtStep%d" % k for k in STEPS])
    crit = res["/Steady/Criteria"]
    assert crit.shape == (len(STEPS), 8) and crit.dtype == np.float64
    for row, k in zip(crit, STEPS):
        t = res["/Steady/PlanesAtStep%d" % k]
        assert t.shape == (32, 11) and t.dtype == np.float64, k
        c = Change(t, 16, 16, EVERY)
        assert row.tolist() == [k, EVERY, c.velocity_change(), c.velocity_change("R"), c.velocity_change("B"), c.phase_change(), c.flipped, c.max_du], k
    want = _standalone(d, tension)
    assert want.steps == EVERY and np.array_equal(res["/Steady/PlanesAtStep%d" % STEPS[-1]], want.planes)          # bit for bit
    assert not np.array_equal(res["/Steady/PlanesAtStep%d" % STEPS[0]], want.planes)
    lines = [m for m in monitored["lines"] if " steady step " in m]
    assert len(lines) == len(STEPS) and all(w in lines[-1] for w in ("velocityChange", "phaseChange", "flipped", "maxDu")), lines
    # without the option: no /Steady group, the same records
    plain, ref = _run(d, d / "plain")
    assert plain.steady_step is None and not any(k.startswith("/Steady") for k in ref)
    assert set(ref) == {k for k in res if not k.startswith("/Steady/")}
    for key in ref:
        assert np.array_equal(ref[key], res[key]), key


def test_the_run_ends_where_the_criterion_is_met(monitored):
    d, tol, kstar = monitored["dir"], monitored["tol"], monitored["kstar"]
    assert kstar < TOTAL
    sim, res = _run(d, d / "stop", steady_every=EVERY, steady_tol=tol, steady_phase_tol=1.0)
    assert sim.steady_step == kstar
    assert res["/Steady/Steps"].tolist() == list(range(EVERY, kstar + 1, EVERY))
    for k in res["/Steady/Steps"].tolist():
        assert np.array_equal(res["/Steady/PlanesAtStep%d" % k], monitored["res"]["/Steady/PlanesAtStep%d" % k]), k
    plain, ref = _run(d, d / "short", steps=kstar)
    assert plain.records == sim.records and set(ref) == {k for k in res if not k.startswith("/Steady/")}
    for key in ref:
        assert np.array_equal(ref[key], res[key]), key
    # a tolerance that is never met: the run goes to its end
    full, _ = _run(d, d / "never", steps=3 * EVERY, steady_every=EVERY, steady_tol=1e-300)
    assert full.steady_step is None and full.steady_steps == [EVERY, 2 * EVERY, 3 * EVERY]


def test_two_ranks_stop_at_the_same_step_and_write_the_same_file(monitored):
    import subprocess
    import sys
    from openlbmpm_amd.results import load_results
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d, tol, kstar = monitored["dir"], monitored["tol"], monitored["kstar"]
    script = d / "w.py"
    script.write_text('''
import os, sys
sys.path.insert(0, %r)
import torch, torch.distributed as dist
from openlbmpm_amd.RKColorGradientD3Q19 import RKColorGradient3D
dist.init_process_group("gloo")
torch.cuda.set_device(0)
sim = RKColorGradient3D(%r, output_dir=%r, device=0, steady_every=%d, steady_tol=%r, steady_phase_tol=1.0)
sim.calibrate_partition = False
sim.runRKColorGradient3D()
assert sim.steady_step == %d, sim.steady_step
assert (sim.change is None) == (dist.get_rank() != 0)
dist.destroy_process_group()
''' % (root, str(d), str(d / "out2"), EVERY, tol, kstar))
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(script)], env=dict(os.environ), timeout=600)
    single, ref = _run(d, d / "out1", steady_every=EVERY, steady_tol=tol, steady_phase_tol=1.0)
    assert single.steady_step == kstar
    files = os.listdir(d / "out2")
    assert len(files) == 1 and files[0].startswith("SimulationResultsRK3D."), files      # the other rank writes none
    got = load_results(str(d / "out2" / files[0]))
    assert set(got) == set(ref) and "/Steady/PlanesAtStep%d" % kstar in got
    for key in ref:
        assert np.array_equal(got[key], ref[key]), key
