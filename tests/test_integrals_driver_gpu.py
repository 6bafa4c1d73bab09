"""RKColorGradient3D(..., integrals_every=N): the /Integrals group of the result file, for both 3-D models, in one process and under two
ranks that share this GPU over gloo."""
import os

import numpy as np
import pytest

from test_drivers_gpu import _free_port

pytestmark = pytest.mark.gpu

STEPS = [0, 5, 10, 12]


def _write_ini(d, tension):
    from ini_fixtures import write_rk3d, write_rk3d_csf
    (write_rk3d_csf if tension == "CSF" else write_rk3d)(str(d), steps=12)          # the shipped sizes: 32 x 32 x 96


def _standalone_tables(d, tension):
    """solver.integrals().planes of a stand-alone solver with the driver's set-up, stepped to each of STEPS"""
    from openlbmpm_amd import config
    from openlbmpm_amd.RKColorGradientD3Q19 import PARAM_KEYS, _CSFSlab, duct
    from openlbmpm_amd.geometry import initial_densities_rk3d
    from openlbmpm_amd.rk3d import RK3DSlab
    p = config.read_rk3d(str(d))
    dom = duct(p["nx"], p["ny"], p["nz"])
    rR, rB = initial_densities_rk3d(dom, 10, p["rho0R"], p["rho0B"])
    out, done = {}, 0
    if tension == "CSF":
        s = _CSFSlab(dom, p, 0).solver
        s.set_macro(rR, rB)
        for k in STEPS:
            s.step(k - done); done = k
            out[k] = s.integrals().planes
    else:
        s = RK3DSlab(dom, 0, dom.shape[0], {k: p[k] for k in PARAM_KEYS})
        s.set_density(rR, rB)
        for k in STEPS:
            if k > done:
                s.step_single(k - done); done = k
            s.phase_field(diagnostics=True)
            out[k] = s.integrals().planes
    s.close()
    return out


@pytest.mark.parametrize("tension", ["perturbation", "CSF"])
def test_the_driver_writes_the_integrals_group(tmp_path, tension, caplog):
    import logging
    from openlbmpm_amd.RKColorGradientD3Q19 import RKColorGradient3D
    from openlbmpm_amd.integrals import COLUMNS, column_names
    from openlbmpm_amd.results import load_results
    _write_ini(tmp_path, tension)
    with caplog.at_level(logging.INFO, logger="openlbmpm_amd"):
        sim = RKColorGradient3D(str(tmp_path), output_dir=str(tmp_path / "out"), record_every=6, integrals_every=5)
        res = load_results(sim.runRKColorGradient3D())
    assert sim.integrals.planes.shape == (96, 12) and sim.integral_steps == STEPS
    assert np.array_equal(res["/Integrals/Steps"], np.array(STEPS, dtype=np.int64)) and res["/Integrals/Steps"].dtype == np.int64
    assert column_names(res["/Integrals/Columns"]) == COLUMNS
    want = _standalone_tables(tmp_path, tension)
    for k in STEPS:
        got = res["/Integrals/PlanesAtStep%d" % k]
        assert got.shape == (96, 12) and np.array_equal(got, want[k]), k
    assert sorted(k for k in res if k.startswith("/Integrals/")) == sorted(["/Integrals/Steps", "/Integrals/Columns"] + ["/Integrals/PlanesAtStep%d" % k for k in STEPS])
    lines = [r.getMessage() for r in caplog.records if " integrals step " in r.getMessage()]
    assert len(lines) == len(STEPS) and all(w in lines[-1] for w in ("saturationR", "massR", "massB", "maxSpeed")), lines
    # the records: the same set with the same values as without the integrals
    plain = RKColorGradient3D(str(tmp_path), output_dir=str(tmp_path / "plain"), record_every=6)
    ref = load_results(plain.runRKColorGradient3D())
    assert not any(k.startswith("/Integrals") for k in ref)
    assert set(ref) == {k for k in res if not k.startswith("/Integrals/")} and sim.records == plain.records == 3
    for key in ref:
        assert np.array_equal(ref[key], res[key]), key


@pytest.mark.parametrize("tension", ["perturbation", "CSF"])
def test_two_ranks_write_the_same_integrals_into_rank_0s_file(tmp_path, tension):
    import subprocess
    import sys
    from openlbmpm_amd.RKColorGradientD3Q19 import RKColorGradient3D
    from openlbmpm_amd.results import load_results
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    _write_ini(tmp_path, tension)
    script = tmp_path / "w.py"
    script.write_text('''
import os, sys
sys.path.insert(0, %r)
import torch, torch.distributed as dist
from openlbmpm_amd.RKColorGradientD3Q19 import RKColorGradient3D
dist.init_process_group("gloo")
torch.cuda.set_device(0)
sim = RKColorGradient3D(%r, output_dir=%r, record_every=6, device=0, integrals_every=5)
sim.calibrate_partition = False
sim.runRKColorGradient3D()
assert (sim.integrals is None) == (dist.get_rank() != 0)
dist.destroy_process_group()
''' % (root, str(tmp_path), str(tmp_path / "out2")))
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(script)], env=dict(os.environ), timeout=600)
    single = RKColorGradient3D(str(tmp_path), output_dir=str(tmp_path / "out1"), record_every=6, integrals_every=5)
    ref = load_results(single.runRKColorGradient3D())
    files = os.listdir(tmp_path / "out2")
    assert len(files) == 1 and files[0].startswith("SimulationResultsRK3D."), files      # the other rank writes none
    got = load_results(str(tmp_path / "out2" / files[0]))
    assert set(got) == set(ref) and "/Integrals/PlanesAtStep12" in got
    for key in ref:
        assert np.array_equal(got[key], ref[key]), key
