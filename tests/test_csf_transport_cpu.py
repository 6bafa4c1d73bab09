"""Host logic of the 3-D CSF slabs' in-library transport (openlbmpm_amd/rk3dcsf.py: RK3DCSFDistributed(..., transport=...)), over gloo
without a GPU: the slab is a stand-in that records the library calls and fails where the scenario says so.  Whatever happens on one rank,
every rank ends on the same transport; the slabs form a ring (low neighbour rank - 1, high neighbour rank + 1, modulo the world)."""
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


class _RingSlab:
    """stand-in for RK3DCSFSolver: the face-message sizes of a slab and the transport calls; `fail` names the call that raises on a rank"""
    on_host = True
    fail, world = {}, 0           # set per process before the class is handed over as the slab factory

    def __init__(self, a, params, device=0, diagnostics=False, slab=None):
        self.params, self.slab, self.nz = params, slab, a.shape[0]
        self.rank = dist.get_rank()
        self.kind, self.calls, self.steps_done = "none", [], 0

    def _maybe(self, what):
        self.calls.append(what)
        if self.fail.get(what) in (self.rank, "all"):
            raise RuntimeError("%s fails on rank %d" % (what, self.rank))

    def face_doubles(self, msg, face):
        return (7, 11, 13)[msg] + (1 if self.fail.get("sizes") == self.rank and face == 1 else 0)

    def face_doubles_in(self, msg, face):
        return (7, 11, 13)[msg]

    def ipc_init(self):
        self._maybe("ipc_init")
        return b"blob-of-rank-%d" % self.rank

    def ipc_connect(self, low, high):
        self._maybe("ipc_connect")
        w = self.world
        assert (low, high) == (b"blob-of-rank-%d" % ((self.rank - 1) % w), b"blob-of-rank-%d" % ((self.rank + 1) % w))
        self.kind = "ipc (copy engine + stream value operations)"

    @staticmethod
    def rccl_unique_id(_path=None):
        return b"U" * 128

    def rccl_connect(self, uid, rank, nranks, _path=None):
        self._maybe("rccl_connect")
        assert uid == b"U" * 128 and rank == self.rank and nranks == self.world
        self.kind = "rccl"

    def transport_probe(self, rounds):
        self._maybe("probe")

    def transport_probe_result(self):
        return 3 if self.fail.get("mismatch") in (self.rank, "all") and self.kind.startswith("ipc") else 0

    def transport_disconnect(self):
        self.calls.append("disconnect")
        self.kind = "none"

    def sync(self, deadline_s=None):
        self.calls.append("sync(%s)" % ("deadline" if deadline_s else "no deadline"))
        if self.fail.get("hang") in (self.rank, "all") and self.kind.startswith(tuple(self.fail.get("hang_kinds", ("ipc", "rccl")))):
            raise RuntimeError("lbmpm_rk3dcsf_sync_deadline: the slab's streams were busy for %.1f s" % deadline_s)

    @property
    def transport(self):
        return self.kind

    def set_macro(self, *a):
        self.calls.append("set_macro")

    def step_slab(self, n, timed=False):
        self.calls.append("step_slab(%d)" % n)
        self.steps_done += n

    def stage(self, k):
        self.calls.append("stage")

    def face_pack(self, msg, face, ptr):
        pass

    def face_unpack(self, msg, face, ptr):
        pass

    def close(self):
        pass


def _worker(rank, world, port, q, want, fail, backend_name, construct):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from openlbmpm_amd.rk3dcsf import RK3DCSFDistributed
        _RingSlab.fail, _RingSlab.world = fail, world
        dom = np.ones((8 * world, 3, 4), dtype=np.uint8)
        err = None
        if construct:                   # the public path: the constructor connects (gloo)
            try:
                d = RK3DCSFDistributed(dom, None, slab_factory=_RingSlab, transport=want)
            except RuntimeError as e:
                q.put((rank, "none", str(e), [], []))
                return
            d.set_macro(dom, dom)
            d.step(5)
            d.sync()
        else:                           # the selection alone, with the backend the scenario names ('nccl': auto may go on to rccl)
            d = RK3DCSFDistributed(dom, None, slab_factory=_RingSlab)
            real = dist.get_backend
            dist.get_backend = lambda group=None: backend_name
            try:
                d._connect(want)
            except RuntimeError as e:
                err = str(e)
            finally:
                dist.get_backend = real
        q.put((rank, d.transport, err, d.slab.calls, d.transport_log))
    except Exception as e:              # (the parent does not wait for its time-out)
        q.put((rank, "error", repr(e), [], []))
        raise
    finally:
        dist.destroy_process_group()


def _run(world, want, fail, backend="gloo", construct=False):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, world, port, q, want, fail, backend, construct)) for r in range(world)]
    for p in ps:
        p.start()
    got = sorted(q.get(timeout=120) for _ in ps)
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    return got


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("want,fail,backend,expect", [
    ("auto", {}, "gloo", "ipc"),                                   # everything works: IPC
    ("auto", {"ipc_connect": 1}, "gloo", "torch"),                 # one rank cannot map its neighbours: every rank drops IPC
    ("auto", {"probe": 1}, "gloo", "torch"),                       # one rank cannot even enqueue the probe
    ("auto", {"mismatch": 0}, "nccl", "rccl"),                     # the probe finds wrong data on one rank: on to RCCL (nccl backend)
    ("auto", {"hang": 1, "hang_kinds": ("ipc",)}, "nccl", "rccl"),  # the IPC probe hangs on one rank: its watchdog fires, all go on to RCCL
    ("auto", {"mismatch": "all", "rccl_connect": 1}, "nccl", "torch"),
    ("ipc", {"ipc_init": 0}, "gloo", "raises"),                    # a named transport that fails raises on EVERY rank
    ("rccl", {"hang": 0}, "nccl", "raises"),
    ("rccl", {"sizes": 0}, "nccl", "raises"),                      # ranks that disagree on a message's size never enter ncclCommInitRank
    ("rccl", {}, "nccl", "rccl"),
])
def test_every_rank_of_the_ring_agrees_on_the_transport(world, want, fail, backend, expect):
    got = _run(world, want, fail, backend)
    kinds = [g[1].split(" ")[0] for g in got]
    if expect == "raises":
        assert all(g[2] and "could not be connected on every rank" in g[2] for g in got), got
        assert kinds == ["torch"] * world
    else:
        assert kinds == [expect] * world, got
        assert all(g[2] is None for g in got)
        if fail:
            assert all("disconnect" in g[3] for g in got)       # the dropped candidate was disconnected on every rank
    for g in got:
        log = g[4]
        assert log and all(set(e) == {"transport", "ok", "why"} for e in log)
        assert [e["ok"] for e in log].count(True) == (0 if expect in ("torch", "raises") else 1)
        if expect not in ("torch", "raises"):
            assert log[-1]["ok"] and log[-1]["transport"] == expect
        assert all(c == "sync(deadline)" for c in g[3] if c.startswith("sync"))       # no probe is waited for without a deadline
    if fail.get("sizes") is not None:
        assert all("disagree on the sizes" in g[2] for g in got) and all("rccl_connect" not in g[3] for g in got)


@pytest.mark.parametrize("world", [2, 3])
def test_library_mode_steps_in_one_call_and_syncs_under_the_watchdog(world):
    """transport='auto' through the constructor: step(5) is ONE step_slab(5) (no stage, no face message from Python), sync() has a deadline"""
    got = _run(world, "auto", {}, construct=True)
    for rank, kind, err, calls, log in got:
        assert kind.startswith("ipc") and err is None, (rank, kind, err)
        after = calls[calls.index("set_macro"):]
        assert after == ["set_macro", "step_slab(5)", "sync(deadline)"], calls


def test_a_named_transport_that_fails_raises_from_the_constructor_on_every_rank():
    got = _run(3, "ipc", {"ipc_connect": 2}, construct=True)
    assert [g[1] for g in got] == ["none"] * 3
    assert all("could not be connected on every rank" in g[2] for g in got), got


def test_the_default_touches_no_transport():
    """transport=None (and 'torch'): today's path -- no set-up call of the in-library transport, every step staged from Python"""
    for want in (None, "torch"):
        got = _run(2, want, {}, construct=True)
        for rank, kind, err, calls, log in got:
            assert kind == "torch" and err is None and log == []
            assert not any(c.startswith(("ipc", "rccl", "probe", "step_slab")) for c in calls), calls
            assert calls.count("stage") == 15 and "sync(no deadline)" in calls
