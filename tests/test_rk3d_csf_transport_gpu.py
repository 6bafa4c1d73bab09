"""3-D CSF slabs stepping over the library's own transports (lbmpm_rk3dcsf_ipc_* / _rccl_connect / _step_slab, include/lbmpm.h): the
three face messages of a step move inside the library, one C call per run of steps, and the ring of slabs stays bit-equal to the
undivided lattice.  Several OS processes share this GPU (torch.distributed.run, gloo carries only the set-up); every subprocess has a
time limit, no process steps two connected contexts, nothing provokes a hang."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_rk3d_csf_gpu import _slab_case
from test_rk3d_gpu import _free_port

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = dict(relax="MRT", theta=55.0, tauB=0.8, velocityZR=0.0, velocityZB=-3.0e-3, sigma=0.06)
CASES = dict(mrt={}, srt=dict(relax="SRT"), convective=dict(outlet="Convective"),
             pressure_inlet=dict(inlet="Dirichlet", densityBH=1.0, densityRH=1e-8), restart={}, release={})
FIELDS = ("fR", "phi", "Fz", "rec_rhoB", "rec_vz")
STEPS = 30


def params(case):
    p = dict(BASE)
    p.update(CASES[case])
    return p


_SCRIPT = '''
import json, os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np, torch, torch.distributed as dist
from test_rk3d_csf_gpu import _slab_case
from test_rk3d_csf_transport_gpu import params, FIELDS, STEPS
from openlbmpm_amd.rk3dcsf import RK3DCSFDistributed, RK3DCSFSolver
from openlbmpm_amd._lib import LbmpmError, ERR_STATE
dev = %(device)s
torch.cuda.set_device(dev)
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
dom, rR, rB = _slab_case()
seen = {}
for case in %(cases)r:
    par = params(case)
    d = RK3DCSFDistributed(dom, par, device=dev, transport=%(transport)r)
    seen[case] = d.transport
    d.set_macro(rR, rB)
    if case == "restart":            # the state replaced across the run (set_pdf) by that of the undivided lattice after 17 steps
        d.step(10); d.sync()
        a = RK3DCSFSolver(dom, par, device=dev); a.set_macro(rR, rB); a.step(17)
        d.set_pdf(a.get("fR"), a.get("fB"), force=(a.get("Fx"), a.get("Fy"), a.get("Fz"))); a.close()
        d.step(STEPS - 17)
    elif case == "release":          # released waits on an idle slab: refused, nothing enqueued; a fresh connect steps again
        d.step(12); d.sync()
        s = d.slab
        s.ipc_release_waits()
        try:
            s.step_slab(1); status = None
        except LbmpmError as e:
            status = e.status
        assert status == ERR_STATE and s.steps_done == 12, (status, s.steps_done)
        dist.barrier()
        s.transport_disconnect()
        dist.barrier()
        blobs = [None] * world
        dist.all_gather_object(blobs, s.ipc_init())
        s.ipc_connect(blobs[(rank - 1) %% world], blobs[(rank + 1) %% world])
        d.step(STEPS - 12)
    else:
        d.step(STEPS)
    d.sync()
    for f in FIELDS:
        g = d.gather(d.get(f))
        if rank == 0:
            np.save(os.path.join(%(out)r, "%%s_%%s.npy" %% (case, f)), g)
    dist.barrier()
    d.close()
    dist.barrier()
if rank == 0:
    json.dump(seen, open(os.path.join(%(out)r, "transport.json"), "w"))
dist.destroy_process_group()
'''


def _run_ranks(tmp_path, world, cases, transport="ipc", env=None, one_gpu=True):
    script = tmp_path / "w.py"
    device = "0" if one_gpu else "int(os.environ['LOCAL_RANK'])"
    script.write_text(_SCRIPT % dict(root=ROOT, out=str(tmp_path), cases=list(cases), transport=transport, device=device))
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
                           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(script)],
                          env=dict(os.environ, **(env or {})), timeout=600)
    return json.load(open(tmp_path / "transport.json"))


_REF = {}


def _reference(case):
    """the undivided lattice after STEPS steps (restart and release: the uninterrupted run of the base case)"""
    key = case if case not in ("restart", "release") else "mrt"
    if key not in _REF:
        from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
        dom, rR, rB = _slab_case()
        a = RK3DCSFSolver(dom, params(key))
        a.set_macro(rR, rB)
        a.step(STEPS)
        _REF[key] = {f: a.get(f) for f in FIELDS}
        a.close()
    return _REF[key]


@pytest.mark.parametrize("world,flag_kernels", [(2, False), (3, False), (2, True), (3, True)])
def test_ipc_ring_across_processes_equals_the_undivided_lattice(tmp_path, world, flag_kernels):
    """world 2: both faces talk to one peer (mapped once); world 3: three distinct peers.  SRT and MRT, the convective outlet, the
    pressure inlet, a restart from set_pdf across the run, the release path -- every field bit for bit; with LBMPM_IPC_FLAG_KERNELS=1
    the flags travel by the one-lane kernels instead of stream value operations"""
    cases = list(CASES) if not flag_kernels else ["mrt", "restart"]
    if world == 3:
        cases = [c for c in cases if c != "release"]
    seen = _run_ranks(tmp_path, world, cases, env=dict(LBMPM_IPC_FLAG_KERNELS="1") if flag_kernels else None)
    for case in cases:
        assert seen[case].startswith("ipc"), seen
        if flag_kernels:
            assert "one-lane flag kernels" in seen[case]
        ref = _reference(case)
        for f in FIELDS:
            got = np.load(tmp_path / ("%s_%s.npy" % (case, f)))
            assert np.array_equal(ref[f], got), (case, f, float(np.max(np.abs(ref[f] - got))))


def _slab(dom, z0, z1, par=None):
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver, _SlabGeometry
    g = _SlabGeometry(dom.shape[0], z0, z1)
    return RK3DCSFSolver(g.cut(dom), par or BASE, slab=g.slab)


def test_refusals_of_connect_and_step():
    """one process, contexts connected by pointer and never stepped: every wrong connect is refused with a status before anything is
    mapped; an undivided context has no transport; a slab without one does not step_slab; release leaves the transport unusable"""
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    from openlbmpm_amd._lib import LbmpmError, ERR_INVALID, ERR_STATE
    dom, rR, rB = _slab_case()
    nz = dom.shape[0]

    def status(fn, *a):
        with pytest.raises(LbmpmError) as e:
            fn(*a)
        return e.value.status

    ring = [_slab(dom, 0, 15), _slab(dom, 15, 30), _slab(dom, 30, nz)]
    before = [s.device_bytes for s in ring]
    ring[1].set_macro(*[np.take(a, np.arange(13, 32), axis=0) for a in (rR, rB)])
    assert status(ring[1].step_slab, 1) == ERR_STATE                         # no transport connected
    assert ring[1].transport == "none"
    blobs = [s.ipc_init() for s in ring]
    assert [s.device_bytes for s in ring] == before                          # (the transport's memory is not the lattice's)
    other_cut = _slab(dom, 0, 20)
    blocked = dom.copy(); blocked[15:17, 5:9, 5:9] = 0                         # another mask beyond the cut at plane 15
    other_mask = _slab(blocked, 0, 15)
    for m in range(3):                                                         # face_copy refuses it for every message, nothing enqueued
        assert other_mask.face_doubles_in(m, 1) != ring[1].face_doubles(m, 0)
        assert status(ring[1].send_to, 0, other_mask, m) == ERR_INVALID
    blocked2 = dom.copy(); blocked2[16:17, 5:9, 5:9] = 0                       # the edge plane's runs match, only the flag stretch differs
    flags_only = _slab(blocked2, 0, 15)
    assert flags_only.face_doubles_in(2, 1) == ring[1].face_doubles(2, 0) and flags_only.face_doubles_in(1, 1) != ring[1].face_doubles(1, 0)
    assert status(ring[1].send_to, 0, flags_only, 0) == ERR_INVALID
    assert status(ring[1].ipc_connect, other_cut.ipc_init(), blobs[2]) == ERR_INVALID      # a slab of another cut
    assert status(ring[1].ipc_connect, other_mask.ipc_init(), blobs[2]) == ERR_INVALID     # other message sizes across the face
    assert status(ring[1].ipc_connect, b"\x17" * 256, blobs[2]) == ERR_INVALID             # not a blob
    assert status(ring[1].ipc_connect, blobs[2], blobs[0]) == ERR_INVALID                  # the neighbours swapped
    assert ring[1].transport == "none"
    whole = RK3DCSFSolver(dom, BASE)
    assert status(whole.ipc_init) == ERR_INVALID                                           # the undivided lattice
    assert status(whole.ipc_connect, blobs[0], blobs[2]) == ERR_INVALID
    assert status(whole.rccl_connect, b"U" * 128, 0, 2) == ERR_INVALID
    # the refused connects left the slab as ipc_init made it: the real neighbours connect (by pointer), the ring stays unstepped
    for k, s in enumerate(ring):
        s.ipc_connect(blobs[k - 1], blobs[(k + 1) % 3])
        assert s.transport.startswith("ipc")
    assert status(ring[1].ipc_connect, blobs[0], blobs[2]) == ERR_STATE     # once
    ring[1].ipc_release_waits()
    assert status(ring[1].step_slab, 1) == ERR_STATE and ring[1].steps_done == 0
    assert status(ring[1].transport_probe, 1) == ERR_STATE
    ring[1].transport_disconnect()
    assert ring[1].transport == "none"
    for s in ring + [other_cut, other_mask, flags_only, whole]:
        s.close()


def test_two_gpu_rccl_ring_equals_the_undivided_lattice(tmp_path):
    """the RCCL transport between two GPUs (RCCL refuses two ranks on one device); set-up over gloo, the messages over the library's
    own communicator"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("RCCL refuses two ranks on one device: needs >= 2 GPUs")
    seen = _run_ranks(tmp_path, 2, ["mrt", "restart"], transport="rccl", one_gpu=False)
    for case in ("mrt", "restart"):
        assert seen[case] == "rccl"
        ref = _reference(case)
        for f in FIELDS:
            assert np.array_equal(ref[f], np.load(tmp_path / ("%s_%s.npy" % (case, f)))), (case, f)
