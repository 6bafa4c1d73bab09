"""D3Q7 tracers on 3-D CSF slabs, one slab per OS process (RK3DCSFDistributed(..., tracers=...)): the tracers' runs ride the population
message through torch.distributed (the default) and over the library's IPC transport (lbmpm_rk3dcsf_step_slab), and the ring stays
bit-equal to the undivided lattice -- concentrations, tracer populations and the flow.  The processes share this GPU
(torch.distributed.run, gloo carries the set-up); every subprocess has a time limit, no process steps two connected contexts, nothing
provokes a hang."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_rk3d_csf_gpu import _slab_case
from test_rk3d_gpu import _free_port
from test_rk3d_tracer_gpu import tracer_case, concentrations

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAR = dict(relax="MRT", theta=55.0, tauB=0.8, velocityZR=0.0, velocityZB=-3.0e-3, sigma=0.06)
FIELDS = ("fR", "phi", "Fz", "rec_rhoB", "rec_vz")
NT = 3
STEPS = 30


def tracers():
    return tracer_case(NT)[0]           # three tracers with the reaction, Dirichlet inlet + free outlet


_SCRIPT = '''
import json, os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np, torch, torch.distributed as dist
from test_rk3d_csf_gpu import _slab_case
from test_rk3d_tracer_gpu import concentrations
from test_rk3d_tracer_transport_gpu import PAR, FIELDS, NT, STEPS, tracers
from openlbmpm_amd.rk3dcsf import RK3DCSFDistributed, RK3DCSFSolver
dev = %(device)s
torch.cuda.set_device(dev)
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
dom, rR, rB = _slab_case()
c0 = concentrations(dom, NT)
seen = {}
for case in %(cases)r:
    d = RK3DCSFDistributed(dom, PAR, device=dev, transport=%(transport)r, tracers=tracers())
    seen[case] = d.transport
    d.set_macro(rR, rB)
    for k in range(NT):
        d.set_concentration(k, c0[k])
    if case == "restart":            # a ring taken down mid-run, a fresh one set up from the undivided lattice's state after 17 steps
        d.step(10); d.sync()          # (the tracers' state is given before a context's first step, so the ring is a new one)
        dist.barrier()
        d.close()
        dist.barrier()
        d = RK3DCSFDistributed(dom, PAR, device=dev, transport=%(transport)r, tracers=tracers())
        a = RK3DCSFSolver(dom, PAR, device=dev, tracers=tracers()); a.set_macro(rR, rB)
        for k in range(NT):
            a.set_concentration(k, c0[k])
        a.step(17)
        d.set_pdf(a.get("fR"), a.get("fB"), force=(a.get("Fx"), a.get("Fy"), a.get("Fz")))
        for k in range(NT):
            d.set_tracer_pdf(k, a.get_tracer_pdf(k))
        a.close()
        d.step(STEPS - 17)
    else:
        d.step(STEPS)
    d.sync()
    got = {f: d.gather(d.get(f)) for f in FIELDS}
    for k in range(NT):
        got["C%%d" %% k] = d.gather(d.get_concentration(k))
        got["g%%d" %% k] = d.gather(d.get_tracer_pdf(k))
    if rank == 0:
        for name, a in got.items():
            np.save(os.path.join(%(out)r, "%%s_%%s.npy" %% (case, name)), a)
    dist.barrier()
    d.close()
    dist.barrier()
if rank == 0:
    json.dump(seen, open(os.path.join(%(out)r, "transport.json"), "w"))
dist.destroy_process_group()
'''


def _run_ranks(tmp_path, world, cases, transport, env=None, one_gpu=True):
    script = tmp_path / "w.py"
    device = "0" if one_gpu else "int(os.environ['LOCAL_RANK'])"
    script.write_text(_SCRIPT % dict(root=ROOT, out=str(tmp_path), cases=list(cases), transport=transport, device=device))
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
                           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(script)],
                          env=dict(os.environ, **(env or {})), timeout=600)
    return json.load(open(tmp_path / "transport.json"))


_REF = {}


def _reference():
    """the undivided lattice after STEPS steps"""
    if not _REF:
        from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
        dom, rR, rB = _slab_case()
        c0 = concentrations(dom, NT)
        a = RK3DCSFSolver(dom, PAR)
        a.configure_tracers(**tracers())
        a.set_macro(rR, rB)
        for k in range(NT):
            a.set_concentration(k, c0[k])
        a.step(STEPS)
        _REF.update({f: a.get(f) for f in FIELDS})
        for k in range(NT):
            _REF["C%d" % k] = a.get_concentration(k)
            _REF["g%d" % k] = a.get_tracer_pdf(k)
            assert np.max(np.abs(_REF["C%d" % k] - c0[k])) > 1e-3          # the tracers did move
        a.close()
    return _REF


def _compare(tmp_path, cases):
    ref = _reference()
    for case in cases:
        for name, want in ref.items():
            got = np.load(tmp_path / ("%s_%s.npy" % (case, name)))
            assert np.array_equal(want, got), (case, name, float(np.max(np.abs(want - got))))


@pytest.mark.parametrize("world,transport,flag_kernels", [(2, "ipc", False), (3, "ipc", False), (2, "ipc", True), (2, None, False), (3, None, False)])
def test_ring_across_processes_equals_the_undivided_lattice(tmp_path, world, transport, flag_kernels):
    """world 2: both faces talk to one peer; world 3: three distinct peers.  transport 'ipc': one lbmpm_rk3dcsf_step_slab per run of steps
    (with LBMPM_IPC_FLAG_KERNELS=1 the flags travel by the one-lane kernels); None: face_pack / face_unpack around torch.distributed.  A
    straight run, and one taken down after 10 steps and set up again through set_pdf + set_tracer_pdf with the undivided lattice's state
    after 17"""
    cases = ["straight", "restart"] if not flag_kernels else ["straight"]
    seen = _run_ranks(tmp_path, world, cases, transport, env=dict(LBMPM_IPC_FLAG_KERNELS="1") if flag_kernels else None)
    for case in cases:
        if transport == "ipc":
            assert seen[case].startswith("ipc"), seen
            if flag_kernels:
                assert "one-lane flag kernels" in seen[case]
        else:
            assert seen[case] == "torch", seen
    _compare(tmp_path, cases)


def test_two_gpu_rccl_ring_equals_the_undivided_lattice(tmp_path):
    """the RCCL transport between two GPUs (RCCL refuses two ranks on one device)"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("RCCL refuses two ranks on one device: needs >= 2 GPUs")
    seen = _run_ranks(tmp_path, 2, ["straight", "restart"], "rccl", one_gpu=False)
    assert all(v == "rccl" for v in seen.values()), seen
    _compare(tmp_path, ["straight", "restart"])
