"""z-slab decomposition and neighbour halo exchange (host-side plumbing of the 3-D solver).

Pure torch / Python: no lattice arithmetic here.  The same code path serves
  * one process per GPU over torch.distributed (backend "nccl" = RCCL over xGMI) and
  * CPU tensors over gloo in the tests (tests/test_slab_cpu.py).
torch is imported where it is used: a single-slab run never loads it.
"""


def partition_z(nz_global, world):
    """Contiguous z-ranges, remainder planes to the lowest ranks.  The outermost ranks must
    own at least the boundary plane pair (2 planes)."""
    if world < 1 or nz_global < 2 * world:
        raise ValueError("cannot cut %d planes into %d slabs of >= 2 planes" % (nz_global, world))
    base, rem = divmod(nz_global, world)
    out, z = [], 0
    for r in range(world):
        n = base + (1 if r < rem else 0)
        out.append((z, n))
        z += n
    return out


def partition_z_balanced(fluid_per_plane, world, min_planes=2):
    """Contiguous z-ranges with (nearly) equal numbers of FLUID cells: the time of a slab is
    proportional to its fluid cells, and the all-fluid buffer planes at both ends of a porous
    sample would otherwise make the end ranks ~8 % slower than the rest.
    Every rank derives the same cuts from the same mask; no communication."""
    w = [int(v) for v in fluid_per_plane]
    nz = len(w)
    if world < 1 or nz < min_planes * world:
        raise ValueError("cannot cut %d planes into %d slabs of >= %d planes" % (nz, world, min_planes))
    total, cuts, acc, z = float(sum(w)), [0], 0.0, 0
    for r in range(1, world):
        target = total * r / world
        lo, hi = cuts[-1] + min_planes, nz - min_planes * (world - r)
        while z < hi and (z < lo or acc + w[z] * 0.5 <= target):
            acc += w[z]
            z += 1
        cuts.append(z)
    cuts.append(nz)
    parts = [(cuts[r], cuts[r + 1] - cuts[r]) for r in range(world)]
    # a slab without a fluid cell cannot be created (lbmpm_rk3d_create refuses it), and ONE rank raising while the
    # others enter the first halo exchange would hang the job: fail here, on every rank alike (same mask, same cuts)
    empty = [r for r, (z0, n) in enumerate(parts) if sum(w[z0:z0 + n]) == 0]
    if empty:
        even = partition_z(nz, world)
        if all(sum(w[z0:z0 + n]) > 0 for z0, n in even):
            return even
        raise ValueError("slabs %s of %d would hold no fluid cell; use fewer ranks" % (empty, world))
    return parts


def neighbour_exchange(send_up, send_down, recv_from_below, recv_from_above, rank, world, group=None):
    """Every rank sends `send_up` to rank+1 (which receives it in `recv_from_below`) and
    `send_down` to rank-1 (received in `recv_from_above`).  No wrap-around: the global lattice is
    not periodic in z.  Point-to-point only (ncclSend/ncclRecv pairs grouped in one batch), no
    collective on the data path."""
    import torch
    import torch.distributed as dist
    if send_up.is_cuda and dist.get_backend(group) == "gloo":
        # rehearsal transport (several ranks sharing ONE GPU, where RCCL refuses duplicate
        # devices): stage through host memory; same neighbours, same buffers, same order
        torch.cuda.current_stream(send_up.device).synchronize()
        h = [t.cpu() for t in (send_up, send_down, recv_from_below, recv_from_above)]
        neighbour_exchange(h[0], h[1], h[2], h[3], rank, world, group)
        if rank > 0:
            recv_from_below.copy_(h[2])
        if rank + 1 < world:
            recv_from_above.copy_(h[3])
        return
    ops = []
    if rank + 1 < world:
        ops.append(dist.P2POp(dist.isend, send_up, rank + 1, group))
        ops.append(dist.P2POp(dist.irecv, recv_from_above, rank + 1, group))
    if rank > 0:
        ops.append(dist.P2POp(dist.isend, send_down, rank - 1, group))
        ops.append(dist.P2POp(dist.irecv, recv_from_below, rank - 1, group))
    if not ops:
        return
    for req in dist.batch_isend_irecv(ops):
        req.wait()


def local_exchange(slabs_send_up, slabs_send_down, slabs_recv_below, slabs_recv_above):
    """Same data movement between k 'virtual ranks' living in one process (lists indexed by
    virtual rank): used to prove slab-decomposed == single-domain on one GPU."""
    k = len(slabs_send_up)
    for r in range(k):
        if r + 1 < k:
            slabs_recv_below[r + 1].copy_(slabs_send_up[r])
            slabs_recv_above[r].copy_(slabs_send_down[r + 1])


def gather_planes(local, parts, rank, world, group=None, device=None):
    """Stack the ranks' planes on rank 0 (the reference's record is ONE dense array per field, RKD2Q9.py:938-957): `local` is this
    rank's numpy array [n_r, ...], parts = [(z0, n)] of all ranks.  Returns the [nz, ...] array on rank 0, None elsewhere.
    Point-to-point (send / recv to rank 0), through device memory under NCCL, host memory under gloo."""
    import numpy as np
    if world == 1:
        return np.asarray(local)
    import torch
    import torch.distributed as dist
    on_gpu = dist.get_backend(group) == "nccl"
    dev = torch.device("cuda", device if device is not None else torch.cuda.current_device()) if on_gpu else torch.device("cpu")
    peer = (lambda r: dist.get_global_rank(group, r)) if group is not None else (lambda r: r)
    local = np.ascontiguousarray(local)
    if rank != 0:
        dist.send(torch.from_numpy(local).to(dev), dst=peer(0), group=group)
        return None
    tail = local.shape[1:]
    out = np.empty((sum(n for _, n in parts),) + tail, dtype=local.dtype)
    out[parts[0][0]:parts[0][0] + parts[0][1]] = local
    for r in range(1, world):
        z0, n = parts[r]
        buf = torch.empty((n,) + tail, dtype=torch.from_numpy(local[:0]).dtype, device=dev)
        dist.recv(buf, src=peer(r), group=group)
        out[z0:z0 + n] = buf.cpu().numpy()
    return out


def _torch_librccl():
    """the librccl that ships inside the torch wheel (the one torch.distributed's nccl backend uses), or None: the system's"""
    import os
    try:
        import torch
        p = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        return p if os.path.exists(p) else None
    except ImportError:
        return None


def slab_neighbours(rank, world, ring):
    """(rank below, rank above) of a slab: None at the two ends of a chain, wrapping in a ring (with two ranks both are the same rank)"""
    if ring:
        return (rank - 1) % world, (rank + 1) % world
    return (rank - 1 if rank > 0 else None), (rank + 1 if rank + 1 < world else None)


def slab_pairs(world, ring):
    """[(lower, upper)] ranks on the two sides of every cut: world - 1 cuts in a chain, world in a ring"""
    return [(r, (r + 1) % world) for r in range(world if ring else world - 1)]


def connect_in_library(slab, rank, world, group, want, ring, face_sizes, log, enqueue=None, messages="6", deadline_s=20.0):
    """Connect the in-library transport of `slab` (the SlabTransportCalls of _lib.py) between the ranks of `group`, a chain or a ring of
    slabs; the one set-up of both 3-D models.  want: 'auto' (ipc, then rccl under the nccl backend) | 'ipc' | 'rccl'.  Every rank takes
    the same decision (a transport that works on some ranks only is dropped by all).  Each candidate is probed under a deadline:
    patterned face messages each way between the real neighbours, compared on the receiving GPU; the library's watchdog releases a
    stuck IPC wait and aborts a stuck communicator -- a hang must not stop the job before it has begun.
    face_sizes() -> this rank's dict(up, down, from_below, from_above) of message sizes; enqueue() -> the context manager under which
    the probe is enqueued (None: none needed); messages: how many patterned messages the probe sends each way, for the log.
    Every candidate's verdict is appended to `log` as dict(transport, ok, why).  Returns (kind, reason): the kind that connected and
    None, or None and "<last candidate> did not connect on every rank (<why>)".  A named transport that fails raises RuntimeError
    (on every rank) instead."""
    import contextlib
    import torch.distributed as dist

    def agree(ok):
        """True when every rank says ok (a collective on host objects: works on every backend)"""
        got = [None] * world
        dist.all_gather_object(got, bool(ok), group=group)
        return all(got)

    lo, hi = slab_neighbours(rank, world, ring)
    for kind in (("ipc", "rccl") if want == "auto" and dist.get_backend(group) == "nccl" else (("ipc",) if want in ("auto", "ipc") else ("rccl",))):
        # every rank goes through the same collectives in the same order, whatever fails on it: a rank that skipped one would pair
        # its next collective with its neighbours' current one
        ok, err = True, None
        if kind == "ipc":
            try:
                mine = slab.ipc_init()
            except Exception as e:      # noqa: BLE001
                mine, ok, err = None, False, e
            blobs = [None] * world
            dist.all_gather_object(blobs, mine, group=group)
            if ok and all(b is not None for b in blobs):
                try:
                    slab.ipc_connect(*[None if r is None else blobs[r] for r in (lo, hi)])
                except Exception as e:  # noqa: BLE001
                    ok, err = False, e
            elif ok:
                ok, err = False, "ipc_init failed on rank(s) %s" % [r for r, b in enumerate(blobs) if b is None]
        else:
            box = [None]
            if rank == 0:
                try:
                    box = [slab.rccl_unique_id(_torch_librccl())]
                except Exception as e:  # noqa: BLE001
                    err = e
            dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
            ok = box[0] is not None
            if not ok and err is None:
                err = "rank 0 could not make a unique id"
            # ipc_open compares the neighbours' message sizes; ncclSend / ncclRecv would silently pair messages of different
            # lengths (different cuts or lattices on two ranks): compare them here, before the blocking collective
            sizes = [None] * world
            dist.all_gather_object(sizes, face_sizes(), group=group)
            for r, h in slab_pairs(world, ring):
                if sizes[r]["up"] != sizes[h]["from_below"] or sizes[h]["down"] != sizes[r]["from_above"]:
                    ok, err = False, "ranks %d and %d disagree on the sizes of the face messages across their cut (%s vs %s)" % (r, h, sizes[r], sizes[h])
            if agree(ok):               # ncclCommInitRank is a blocking collective: enter it only if every rank will
                try:
                    slab.rccl_connect(box[0], rank, world, _torch_librccl())
                except Exception as e:  # noqa: BLE001
                    ok, err = False, e
            else:
                ok = False
        connected = agree(ok)
        tested, why = False, "not tried"
        if connected:
            try:
                with (enqueue() if enqueue is not None else contextlib.nullcontext()):
                    slab.transport_probe(6)
                mine, why = True, "ok"
            except Exception as e:      # noqa: BLE001 -- this rank could not even enqueue: it tells the others in the same collective
                mine, why = False, "could not enqueue the probe: %s" % e
            if mine:
                try:
                    slab.sync(deadline_s=deadline_s)
                    bad = slab.transport_probe_result()
                    if bad:
                        mine, why = False, "%d doubles arrived wrong" % bad
                except Exception as e:  # noqa: BLE001 -- the watchdog fired (or the stream failed)
                    mine, why = False, str(e)
            tested = agree(mine)
            if mine and not tested:
                why = "ok here, failed on another rank"
        if connected and tested:
            log.append(dict(transport=kind, ok=True, why="connected; probe of %s patterned messages each way compared equal on every rank" % messages))
            return kind, None
        try:
            slab.transport_disconnect()
        except Exception:               # noqa: BLE001
            pass
        reason = ("connect: %s" % err) if err else ("another rank could not connect" if not connected else "self-test: %s" % why)
        log.append(dict(transport=kind, ok=False, why=str(reason)))
        if want != "auto":
            raise RuntimeError("transport %r could not be connected on every rank: %s" % (kind, reason))
    return None, "%s did not connect on every rank (%s)" % (kind, reason)


class DeviceBuffer:
    """Zero-copy torch view of a raw device allocation owned by liblbmpm_hip.so."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (int(nbytes) // 8,), "typestr": "<f8",
                                         "data": (int(ptr), False), "version": 2}

    def tensor(self, device):
        import torch
        return torch.as_tensor(self, device=device)
