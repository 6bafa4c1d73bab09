"""The 3-D transport driver (openlbmpm_amd/Transport3DRK.py), its command line `python -m openlbmpm_amd tr3d`, and the reader of its
transportsetup.ini (config.read_transport3d; that test needs no GPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

Z_KEYS = """DiffusionZ = 0.1, 0.14
DiffusionXZ = 0.005, 0.005
DiffusionZX = -0.01, -0.01
DiffusionYZ = 0.015, 0.015
DiffusionZY = 0.02, 0.02
"""


def write_ini(d, z_keys=True, **kw):
    from ini_fixtures import TRANSPORT_INI, write_rk3d_csf
    write_rk3d_csf(str(d), **kw)
    with open(os.path.join(str(d), "transportsetup.ini"), "w") as fh:
        fh.write(TRANSPORT_INI + (Z_KEYS if z_keys else ""))


def test_read_transport3d(tmp_path):
    """a 2-D file describes an isotropic 3-D case (every missing z entry takes the y entry); the z keys are honoured"""
    from openlbmpm_amd import config
    write_ini(tmp_path, z_keys=False)
    p2, p = config.read_transport(str(tmp_path)), config.read_transport3d(str(tmp_path))
    for k, v in p2.items():
        assert p[k] == v, k
    assert p["diffZ"] == p2["diffY"] == [1. / 6., 0.2] and p["dXZ"] == p2["dXY"] == 0.01 and p["dZX"] == p2["dYX"] == 0.02
    assert p["dYZ"] == 0.0 and p["dZY"] == 0.0
    assert np.allclose(p["diffJ3"], [0.0, 0.0], atol=1e-15)         # J0 = 1/3 -> J0' = 0: (1 - J0') / 6 = (1 - J0) / 4
    write_ini(tmp_path, z_keys=True)
    p = config.read_transport3d(str(tmp_path))
    assert p["diffZ"] == [0.1, 0.14] and p["diffY"] == [1. / 6., 0.2]
    assert (p["dXZ"], p["dZX"], p["dYZ"], p["dZY"]) == (0.005, -0.01, 0.015, 0.02) and (p["dXY"], p["dYX"]) == (0.01, 0.02)
    with open(os.path.join(str(tmp_path), "transportsetup.ini")) as fh:
        text = fh.read()
    with open(os.path.join(str(tmp_path), "transportsetup.ini"), "w") as fh:
        fh.write(text.replace("DiffusionJ = 0.3333333333333333, 0.3333333333333333", "DiffusionJ = 0.5, 0.4"))
    p = config.read_transport3d(str(tmp_path))
    for j, j3 in zip(p["diffJ"], p["diffJ3"]):
        assert abs((1. - j3) / 6. - (1. - j) / 4.) < 1e-16
    with pytest.raises(config.ConfigError):
        config.read_transport3d(str(tmp_path / "nowhere"))


PAR = dict(sigma=0.05, theta=60.0, wetting=2, beta=1.0, delta=0.98, tauR=1.0, tauB=0.9, tautype=2, relax="MRT", velocityZR=0.0, velocityZB=-1.0e-4,
           densityBL=1.0, densityRL=1.0e-8)


def by_hand(records, every, steps):
    """the solver API driven by hand: what the driver's records must hold"""
    from openlbmpm_amd import config
    from openlbmpm_amd.RKColorGradientD3Q19 import duct
    from openlbmpm_amd.geometry import initial_densities_rk3d
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    dom = duct(14, 12, 40)
    rR, rB = initial_densities_rk3d(dom, 10, 1.0, 1.0)
    s = RK3DCSFSolver(dom, PAR)
    s.configure_tracers(num_tracers=2, diffusion_x=(1. / 6., 0.12), diffusion_y=(1. / 6., 0.2), diffusion_z=(0.1, 0.14), diffusion_xy=0.01, diffusion_yx=0.02,
                        diffusion_xz=0.005, diffusion_zx=-0.01, diffusion_yz=0.015, diffusion_zy=0.02, beta_interface=0.8, criteria_rho=0.5,
                        inlet_concentration=(1.0, 0.25), dirichlet_inlet=True, free_outlet=True, diffusion_j=(0.0, 0.0))
    s.set_macro(rR, rB)
    zz = np.arange(40)[:, None, None]
    s.set_concentration(0, np.where((dom == 1) & (zz <= 40 - 10), 1.0, 0.0))
    s.set_concentration(1, np.zeros(dom.shape))
    out = {}
    for k in range(records):
        done = k * every
        if done < steps:
            s.step(done - s.steps_done)
            out["/FluidMacro/FluidDensityRin%d" % k] = s.get("rec_rhoR"); out["/FluidVelocity/FluidVelocityZAt%d" % k] = s.get("rec_vz")
            s.step(1)
        else:
            s.step(steps - s.steps_done)
            out["/FluidMacro/FluidDensityRin%d" % k] = s.get("rec_rhoR"); out["/FluidVelocity/FluidVelocityZAt%d" % k] = s.get("rec_vz")
        for i in range(2):
            out["/TransportMacro/TracerConcType%din%d" % (i, k)] = s.get_concentration(i)
    s.close()
    return out


@pytest.mark.gpu
def test_the_tr3d_command_line_writes_both_result_files(tmp_path):
    from openlbmpm_amd.results import load_results
    write_ini(tmp_path, nx=14, ny=12, nz=40, steps=24, relax="MRT", sigma=0.05, theta=60.0)
    out = tmp_path / "results"
    r = subprocess.run([sys.executable, "-m", "openlbmpm_amd", "tr3d", str(tmp_path), "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ConcentrationResults" in r.stdout and "SimulationResultsRK3D" in r.stdout
    from openlbmpm_amd.results import find_result_file
    flow, conc = find_result_file(str(out), "SimulationResultsRK3D"), find_result_file(str(out), "ConcentrationResults")
    assert flow and conc
    res = dict(load_results(flow)); res.update(load_results(conc))
    # [TimeSteps] of the fixture carries no interval: the driver records every steps // 10 = 2 steps, and once more after the last one
    want = by_hand(13, 2, 24)
    assert sum(k.startswith("/TransportMacro/TracerConcType0in") for k in res) == 13
    for key, a in want.items():
        assert np.array_equal(res[key], a), key
    assert np.max(res["/TransportMacro/TracerConcType1in12"]) > 1e-3        # the inlet feeds tracer 1


@pytest.mark.gpu
def test_checkpoint_and_restart_continue_bit_for_bit(tmp_path):
    from openlbmpm_amd.Transport3DRK import Transport3DRK
    from openlbmpm_amd.results import load_results
    write_ini(tmp_path, nx=14, ny=12, nz=40, steps=30, relax="MRT", sigma=0.05, theta=60.0)
    a = Transport3DRK(str(tmp_path), output_dir=str(tmp_path / "a"), record_every=10, checkpoint_every=15)
    fa, ca = a.runTransport3DMPMCRK()
    ra = dict(load_results(fa)); ra.update(load_results(ca))
    assert a.records == 4
    want = by_hand(4, 10, 30)
    for key, v in want.items():
        assert np.array_equal(ra[key], v), key
    b = Transport3DRK(str(tmp_path), output_dir=str(tmp_path / "b"), record_every=10, restart_from=a.checkpoint_path)
    fb, cb = b.runTransport3DMPMCRK()
    rb = dict(load_results(fb)); rb.update(load_results(cb))
    for k in (2, 3):
        for key in ("/FluidMacro/FluidDensityRin%d" % k, "/FluidVelocity/FluidVelocityZAt%d" % k, "/TransportMacro/TracerConcType0in%d" % k,
                    "/TransportMacro/TracerConcType1in%d" % k):
            assert np.array_equal(rb[key], ra[key]), key
    st_a, st_b = a.solver.get_state()[0], b.solver.get_state()[0]
    assert st_a.shape[-1] == 41 + 14 and np.array_equal(st_a, st_b)


@pytest.mark.gpu
def test_a_checkpoint_of_a_restarted_run_continues_bit_for_bit(tmp_path):
    """two generations: the checkpoint a restarted run writes holds the absolute step count, and the run restarted from it performs exactly
    the remaining steps, writes the uninterrupted run's records under their indices and ends in its state"""
    from openlbmpm_amd.Transport3DRK import Transport3DRK
    from openlbmpm_amd.results import load_results, read_planes
    write_ini(tmp_path, nx=14, ny=12, nz=40, steps=40, relax="MRT", sigma=0.05, theta=60.0)
    run = lambda name, **kw: Transport3DRK(str(tmp_path), output_dir=str(tmp_path / name), record_every=10, **kw)

    def results(sim):
        flow, conc = sim.runTransport3DMPMCRK()
        out = dict(load_results(flow)); out.update(load_results(conc))
        return out
    whole = run("whole")
    ref = results(whole)
    assert whole.records == 5 and whole.solver.solver.steps_done == 40
    first = run("first", checkpoint_every=12)
    first.timeSteps = 20                                  # one checkpoint, after 12 steps
    results(first)
    assert [int(v) for v in read_planes(first.checkpoint_path, "/Checkpoint/Info")][:3] == [41 + 14, 12, 0]
    second = run("second", checkpoint_every=12, restart_from=first.checkpoint_path)
    second.timeSteps = 30                                 # steps 13 .. 30, one checkpoint after step 24
    got2 = results(second)
    assert second.solver.solver.steps_done == 18
    info = [int(v) for v in read_planes(second.checkpoint_path, "/Checkpoint/Info")]
    assert info[1] == 24 and info[6] == 3, info           # the absolute step count; records 0, 1, 2 written before it
    last = run("last", restart_from=second.checkpoint_path)
    got = results(last)
    assert last.solver.solver.steps_done == 40 - 24       # exactly the remaining steps
    assert last.records == whole.records == 5
    names = ("/FluidMacro/FluidDensityRin%d", "/FluidVelocity/FluidVelocityZAt%d", "/TransportMacro/TracerConcType0in%d", "/TransportMacro/TracerConcType1in%d")
    assert sorted(k for k in got if k.startswith("/TransportMacro/TracerConcType0in")) == ["/TransportMacro/TracerConcType0in3", "/TransportMacro/TracerConcType0in4"]
    for k, res in ((2, got2), (3, got), (4, got)):
        for name in names:
            assert np.array_equal(res[name % k], ref[name % k]), (name, k)
    (st_a, info_a), (st_b, info_b) = whole.solver.get_state(), last.solver.get_state()
    assert info_a["steps"] == info_b["steps"] == 40 and st_a.shape[-1] == 41 + 14 and np.array_equal(st_a, st_b)
