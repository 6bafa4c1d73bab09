"""What wrap_z=True costs per call: clusters(props=True) and morphology() of RK3DCSFSolver on a lattice that is periodic in z, with the
seam closed and without, the same build on the same state.  Not part of bench.py; there is no threshold, docs/EXPERIMENTS_r7.md keeps
the numbers.

    python tools/wrap_z_timing.py [--size N] [--calls 9] [--states layered random]

The lattice is bench.py's porous medium, taken as periodic.  States: `layered` (red in the quarter of the planes at either end of z, blue
in the half between: red lies across the seam, few clusters) and `random` (every cell R or B by a coin: a cluster per forty cells or so,
the end where the host's share -- the table, the two face planes, one more pass over the rows -- is largest).  Every call returns host
tables, so it ends in a stream synchronisation; host clock, the calls alternate, medians over `calls` rounds after a warm-up round.  One
JSON line per state.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--states", nargs="+", default=["layered", "random"])
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import bench
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    n = a.size
    dom = bench.c5_domain((n, n, n))
    s = RK3DCSFSolver(dom, dict(relax="MRT", inlet="Periodic", outlet="Periodic"))
    fl = dom == 1
    for name in a.states:
        if name == "random":
            red = np.random.default_rng(1).random(dom.shape) < 0.5
        else:
            red = np.broadcast_to(((np.arange(n) + n // 4) % n < n // 2)[:, None, None], dom.shape)
        s.set_macro(np.where(fl & red, 1.0, 0.0), np.where(fl & ~red, 1.0, 0.0))
        calls = dict(clusters_props_ms=lambda: s.clusters(props=True), clusters_props_wrap_ms=lambda: s.clusters(props=True, wrap_z=True),
                     morphology_ms=s.morphology, morphology_wrap_ms=lambda: s.morphology(wrap_z=True))
        opened, closed = calls["clusters_props_ms"](), calls["clusters_props_wrap_ms"]()          # the warm-up round: allocations, code objects
        calls["morphology_ms"](); calls["morphology_wrap_ms"]()
        r = dict(state=name, size=n, fluid_cells=int(s.num_fluid_nodes), open_clusters=int(opened.table.shape[0]), clusters=int(closed.table.shape[0]),
                 winding=int(np.count_nonzero(closed.winding)), across_the_seam=int(np.count_nonzero((closed.winding == 0) & (closed.table[:, 4] >= n))))
        ms = {k: [] for k in calls}
        for _ in range(a.calls):
            for k, call in calls.items():
                t = time.perf_counter()
                call()
                ms[k].append((time.perf_counter() - t) * 1e3)
        for k, v in ms.items():
            r[k] = dict(median=round(float(np.median(v)), 3), min=round(min(v), 3), max=round(max(v), 3))
        print(json.dumps(r), flush=True)
    s.close()


if __name__ == "__main__":
    main()
