"""The 3-D transport driver under torchrun (openlbmpm_amd/Transport3DRK.py, `python -m openlbmpm_amd tr3d`): one z-slab per rank (the
ranks share this GPU, gloo carries the set-up and -- by default -- the face messages), rank 0 writes ONE SimulationResultsRK3D and ONE
ConcentrationResults whose every dataset equals the one-GPU driver's bit for bit; a checkpoint written by two ranks restarts on one rank
and on three and continues bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_rk3d_gpu import _free_port
from test_tr3d_driver_gpu import write_ini

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torchrun(ranks, args, env=None):
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
                        "--master-port", str(_free_port())] + args, cwd=ROOT, env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _results(directory):
    from openlbmpm_amd.results import load_results
    files = sorted(os.listdir(directory))
    flow = [f for f in files if f.startswith("SimulationResultsRK3D")]
    conc = [f for f in files if f.startswith("ConcentrationResults")]
    assert len(flow) == 1 and len(conc) == 1, files         # ONE file each, whatever the number of ranks
    res = dict(load_results(os.path.join(directory, flow[0])))
    res.update(load_results(os.path.join(directory, conc[0])))
    return res


@pytest.mark.parametrize("transport", [None, "ipc"])
def test_the_tr3d_command_line_on_two_ranks_writes_the_one_gpu_files(tmp_path, transport):
    write_ini(tmp_path, nx=14, ny=12, nz=40, steps=24, relax="MRT", sigma=0.05, theta=60.0)
    one = subprocess.run([sys.executable, "-m", "openlbmpm_amd", "tr3d", str(tmp_path), "--out", str(tmp_path / "one")], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert one.returncode == 0, one.stdout + one.stderr
    _torchrun(2, ["-m", "openlbmpm_amd", "tr3d", str(tmp_path), "--out", str(tmp_path / "two")] + (["--csf-transport", transport] if transport else []),
              env=dict(LBMPM_DIST_BACKEND="gloo"))
    ref, got = _results(str(tmp_path / "one")), _results(str(tmp_path / "two"))
    assert set(got) == set(ref) and sum(k.startswith("/TransportMacro/TracerConcType0in") for k in ref) == 13
    for key in ref:
        assert np.array_equal(got[key], ref[key]), key
    assert np.max(ref["/TransportMacro/TracerConcType1in12"]) > 1e-3        # the inlet feeds tracer 1: the tracers did move


_WORKER = '''
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from openlbmpm_amd.Transport3DRK import Transport3DRK
dist.init_process_group("gloo")
torch.cuda.set_device(0)
sim = Transport3DRK(%(ini)r, output_dir=%(out)r, record_every=10, device=0, **%(kw)r)
sim.runTransport3DMPMCRK()
d = sim.solver.solver
assert d.world == %(ranks)d and sim.nzl < 40 and d.num_tracers == 2
st = d.gather(sim.solver.get_state()[0])
if dist.get_rank() == 0:
    np.save(os.path.join(%(out)r, "state.npy"), st)
dist.destroy_process_group()
'''


def test_a_checkpoint_of_two_ranks_restarts_on_one_rank_and_on_three(tmp_path):
    from openlbmpm_amd.Transport3DRK import Transport3DRK
    write_ini(tmp_path, nx=14, ny=12, nz=40, steps=30, relax="MRT", sigma=0.05, theta=60.0)
    # the uninterrupted run on one GPU
    a = Transport3DRK(str(tmp_path), output_dir=str(tmp_path / "a"), record_every=10)
    a.runTransport3DMPMCRK()
    ref, state = _results(str(tmp_path / "a")), a.solver.get_state()[0]
    assert state.shape[-1] == 41 + 14

    def ranks(n, out, **kw):
        script = tmp_path / ("w%d.py" % n)
        script.write_text(_WORKER % dict(root=ROOT, ini=str(tmp_path), out=str(tmp_path / out), kw=kw, ranks=n))
        _torchrun(n, [str(script)])
        return _results(str(tmp_path / out))

    two = ranks(2, "two", checkpoint_every=15)
    assert set(two) == set(ref)
    for key in ref:
        assert np.array_equal(two[key], ref[key]), key
    assert np.array_equal(np.load(tmp_path / "two" / "state.npy"), state)
    ck = [f for f in sorted(os.listdir(tmp_path / "two")) if f.startswith("CheckpointRK3D.")]
    assert len(ck) == 1
    ck = str(tmp_path / "two" / ck[0])
    later = [k for k in ref if k.endswith(("in2", "At2", "in3", "At3"))]
    assert len(later) == 2 * (2 + 3 + 2)
    # ... on one rank
    b = Transport3DRK(str(tmp_path), output_dir=str(tmp_path / "b"), record_every=10, restart_from=ck)
    b.runTransport3DMPMCRK()
    rb = _results(str(tmp_path / "b"))
    for key in later:
        assert np.array_equal(rb[key], ref[key]), key
    assert np.array_equal(b.solver.get_state()[0], state)
    # ... and on three
    three = ranks(3, "three", restart_from=ck)
    for key in later:
        assert np.array_equal(three[key], ref[key]), key
    assert np.array_equal(np.load(tmp_path / "three" / "state.npy"), state)
