"""What clusters() costs on the bench lattice: the 512^3 porous medium of `bench.py --workload csf3d` under the 3-D CSF model, in the
initial state and after 300 steps, connectivity 6 and 18 -- beside one solver step on the same lattice and beside what the call
replaces (get("rec_phi") over PCIe and a labelling on the CPU: scipy.ndimage.label where scipy is there, once per phase, no periodic
wrap -- a lower bound of that route).  Not part of bench.py; there is no threshold, docs/EXPERIMENTS_r7.md keeps the numbers.

    python tools/clusters_timing.py [--size NX NY NZ] [--steps 300] [--calls 7] [--limit SECONDS]

Every state runs in a child process of its own under a time limit (a child that runs into it is killed and reported, the next one is
not started).  A call is timed twice: by HIP events recorded around it on the default stream, which waits for the solver's stream,
and by the host clock around the synchronous call (it returns the number of clusters, so it ends with a stream synchronisation);
medians over `calls` calls after two warm-up calls.  One JSON line per state.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHES = 7                 # classify, tiles, merge, flatten, scan, rows, sizes (csrc/rk3d_clusters.h)


def one(size, state, steps, calls):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import bench
    t0 = time.perf_counter()
    s, _, _ = bench.build_csf3d(tuple(size), 0, "MRT", "initial")
    out = dict(state=state, size=list(size), fluid_cells=int(s.num_fluid_nodes), build_s=round(time.perf_counter() - t0, 1), launches_per_call=LAUNCHES)
    if state == "stepped":
        s.step(steps)
        out["steps_before"] = steps
    s.sync()
    t0 = time.perf_counter()
    s.step(20); s.sync()
    out["solver_step_ms"] = round((time.perf_counter() - t0) * 1e3 / 20, 3)
    before = s.device_bytes
    for conn in (6, 18):
        ev, wall, n = [], [], 0
        for k in range(2 + calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            n = s.clusters(connectivity=conn).table.shape[0]
            b.record()
            b.synchronize()
            t1 = time.perf_counter()
            if k >= 2:
                ev.append(a.elapsed_time(b)); wall.append((t1 - t0) * 1e3)
        out["conn%d" % conn] = dict(clusters=int(n), events_ms=round(statistics.median(ev), 3), wall_ms=round(statistics.median(wall), 3),
                                   events_min_ms=round(min(ev), 3), events_max_ms=round(max(ev), 3), calls=calls)
    out["device_bytes_per_cell"] = round((s.device_bytes - before) / float(size[0] * size[1] * size[2]), 3)
    c = s.clusters(connectivity=6)
    out["summary"] = {k: (bool(v) if isinstance(v, (bool, np.bool_)) else int(v)) for k, v in c.summary().items()}
    # the route the call replaces
    t0 = time.perf_counter()
    phi = s.get("rec_phi")
    out["get_rec_phi_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    try:
        from scipy import ndimage
        fl = s.is_domain == 1
        t0 = time.perf_counter()
        nr = ndimage.label(fl & (phi > 0))[1]
        nb = ndimage.label(fl & (phi <= 0))[1]
        out["cpu_label_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        out["cpu_labeller"] = "scipy.ndimage.label, faces, once per phase, no periodic wrap (%d + %d components)" % (nr, nb)
    except ImportError:
        out["cpu_label_ms"], out["cpu_labeller"] = None, "scipy is not importable; the union-find of tests/test_clusters_cpu.py is a Python loop over the cell pairs, not run at this size"
    s.close()
    print("CLUSTERS_TIMING " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 512])
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--limit", type=float, default=420.0, help="seconds a state's child process may take")
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.calls < 5:
        ap.error("medians of at least 5 calls")
    if a.one:
        return one(a.size, a.one, a.steps, a.calls)
    for state in ("initial", "stepped"):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", state, "--steps", str(a.steps), "--calls", str(a.calls), "--size"] + [str(v) for v in a.size]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print("CLUSTERS_TIMING " + json.dumps(dict(state=state, error="ran into the limit of %g s" % a.limit)), flush=True)
            return 1
        if rc != 0:              # a child that failed or faulted: nothing more is started on the device
            print("CLUSTERS_TIMING " + json.dumps(dict(state=state, error="exit status %d" % rc)), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
