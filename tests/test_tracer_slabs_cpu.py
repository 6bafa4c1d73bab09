"""RK3DCSFDistributed(..., tracers=...) without a GPU: a host stand-in takes the solver's place under gloo (tests/test_slab_cpu.py).  The
keyword reaches the slab's constructor only when it was given, the undivided concentration is cut into this rank's planes with the images
of the neighbours' (wrapping at the seam of the ring), and own planes gathered on rank 0 restack the undivided array."""
import multiprocessing as mp
import os

import numpy as np
import pytest

dist = pytest.importorskip("torch.distributed")

from test_slab_cpu import _HostSlab, _free_port      # noqa: E402

NZ = 31
TRACERS = dict(num_tracers=2, diffusion_x=0.1, dirichlet_inlet=True)


class _HostTracerSlab(_HostSlab):
    """the stand-in with the tracer calls of RK3DCSFSolver: it keeps what it was given"""
    calls = []

    def __init__(self, a, params, device=0, diagnostics=False, slab=None, **more):
        _HostSlab.__init__(self, a, params, device=device, diagnostics=diagnostics, slab=slab)
        type(self).calls.append(dict(more))
        self.tracers = more.get("tracers")
        self.conc, self.pdf = {}, {}

    def set_concentration(self, t, c):
        assert c.shape[0] == self.nz
        self.conc[t] = np.array(c)

    def set_tracer_pdf(self, t, g):
        assert g.shape[0] == self.nz
        self.pdf[t] = np.array(g)

    def get_concentration(self, t):
        return self.conc[t].copy()

    def get_tracer_pdf(self, t):
        return self.pdf[t].copy()


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from openlbmpm_amd.rk3dcsf import RK3DCSFDistributed
        from openlbmpm_amd._lib import LbmpmError, ERR_UNSUPPORTED
        full = np.random.default_rng(5).standard_normal((NZ, _HostSlab.W))
        ok = []
        # without tracers= the factory is called with the arguments it has always been called with
        d = RK3DCSFDistributed(full, dict(tag="host stand-in"), slab_factory=_HostSlab)
        ok.append(d.num_tracers == 0)
        d.close()
        _HostTracerSlab.calls.clear()
        d = RK3DCSFDistributed(full, dict(tag="host stand-in"), slab_factory=_HostTracerSlab)
        ok.append(_HostTracerSlab.calls == [{}])
        d.close()
        _HostTracerSlab.calls.clear()
        d = RK3DCSFDistributed(full, dict(tag="host stand-in"), slab_factory=_HostTracerSlab, tracers=TRACERS)
        ok.append(_HostTracerSlab.calls == [dict(tracers=TRACERS)] and d.slab.tracers == TRACERS and d.num_tracers == 2)
        z0, z1 = d.cuts[rank], d.cuts[rank + 1]
        ok.append((z0, z1 - z0) == (d.z0, d.nzl))
        planes = np.arange(z0 - 2, z1 + 2) % NZ                  # two images at either end; the first rank's low ones are the planes NZ-2, NZ-1
        ok.append(rank != 0 or list(planes[:2]) == [NZ - 2, NZ - 1])
        ok.append(rank != world - 1 or list(planes[-2:]) == [0, 1])
        for t in range(2):
            c = np.random.default_rng(10 + t).standard_normal((NZ, 4, 3))
            g = np.random.default_rng(20 + t).standard_normal((NZ, 4, 3, 7))
            d.set_concentration(t, c)
            d.set_tracer_pdf(t, g)
            ok.append(np.array_equal(d.slab.conc[t], c[planes]) and np.array_equal(d.slab.pdf[t], g[planes]))
            own_c, own_g = d.get_concentration(t), d.get_tracer_pdf(t)
            ok.append(np.array_equal(own_c, c[z0:z1]) and np.array_equal(own_g, g[z0:z1]))
            wc, wg = d.gather(own_c), d.gather(own_g)
            ok.append((wc is None and wg is None) if rank else (np.array_equal(wc, c) and np.array_equal(wg, g)))
        try:
            d.configure_tracers(num_tracers=1)
            ok.append(False)
        except LbmpmError as e:
            ok.append(e.status == ERR_UNSUPPORTED and "slabs" in str(e) and "tracers=" in str(e))
        # the flow's orchestration is what it was
        d.set_macro(full, full)
        d.step(3)
        ok.append(d.slab.steps_done == 3)
        d.close()
        q.put((rank, ok))
    except Exception as e:                           # (the parent does not wait for its time-out)
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_tracers_reach_the_slab_and_are_cut_and_restacked(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in range(world):
        assert isinstance(results[r], list) and all(results[r]), (r, results[r])


def test_one_function_builds_the_tracer_config():
    """rk3dcsf.tracer_config: the lbmpm_tracer3d_config of configure_tracers(...) and of tracers=dict(...)"""
    from openlbmpm_amd.rk3dcsf import tracer_config
    cfg = tracer_config(num_tracers=3, diffusion_x=(0.1, 0.2, 0.3), reaction_rate=0.05, diffusion_j=0.25, dirichlet_inlet=True)
    assert cfg.num_tracers == 3 and list(cfg.diffusion_x)[:3] == [0.1, 0.2, 0.3] and list(cfg.diffusion_z)[:3] == [0.1, 0.2, 0.3]
    assert cfg.reaction_rate == 0.05 and cfg.dirichlet_inlet == 1 and cfg.free_outlet == 0 and list(cfg.diffusion_j)[:3] == [0.25] * 3
    with pytest.raises(ValueError):
        tracer_config(num_tracers=3, diffusion_x=(0.1, 0.2))
