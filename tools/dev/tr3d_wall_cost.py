"""What the tracers' wall reaction costs the 3-D CSF step with tracers: the lattice of `bench.py --workload csf3d` with two tracers,
without a wall reaction (the step launches tr3d_step<..., WALL = false>), with one rate per tracer (WALL = true, no class words) and with
three mineral classes on a map (WALL = true, one more word per fluid cell read).

    python tools/dev/tr3d_wall_cost.py [--size 256 256 256] [--steps 60] [--warmup 15] [--runs 3] [--relax MRT|SRT] [--only none|scalar|map]

Prints one JSON line per timed run, the legs in turn, then their medians.  Step times by HIP events on the solver's stream (step_timed).
One context: the tracers' state is given once and the legs follow each other in time (a state cannot be given again after a step); the
rates are small, so the state stays the bench's.  For the times of tr3d_step alone run it under `rocprofv3 --kernel-trace --stats --
python ... --only map --runs 1`: the instances carry their template arguments in their names, the last one is WALL."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import bench  # noqa: E402
from openlbmpm_amd.rk3dcsf import RK3DCSFSolver  # noqa: E402

LEGS = ("none", "scalar", "map")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=(256, 256, 256))
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--relax", default="MRT")
    ap.add_argument("--only", choices=LEGS, default=None)
    a = ap.parse_args()
    size = tuple(a.size)
    dom = bench.c5_domain(size)
    dom[0] = dom[1]; dom[-1] = dom[-2]
    rR, rB = bench.c5_state(dom, 0, size[2], "initial")
    s = RK3DCSFSolver(dom, dict(relax=a.relax, tauB=0.8),
                      tracers=dict(num_tracers=2, diffusion_x=(1. / 6., 0.1), beta_interface=(0.5, 0.0), inlet_concentration=(1.0, 0.5),
                                   dirichlet_inlet=True, free_outlet=True))
    cells = s.num_fluid_nodes
    s.set_macro(rR, rB)
    for k in range(2):
        s.set_concentration(k, np.where(dom == 1, 0.5, 0.0))
    minerals = np.random.default_rng(1).integers(0, 3, size=dom.shape).astype(np.uint8)
    got = {k: [] for k in LEGS}
    for _ in range(a.runs):
        for which in LEGS:
            if a.only and which != a.only:
                continue
            if which == "none":
                s.set_wall_reaction(None)
            elif which == "scalar":
                s.set_wall_reaction((1.0e-3, 2.0e-3))
            else:
                s.set_wall_reaction([[1.0e-3, 2.0e-3], [2.0e-3, 1.0e-3], [0.0, 3.0e-3]], minerals)
            s.step(a.warmup); s.sync()
            ms, _ = s.step_timed(a.steps)
            mlups = cells * a.steps / ms / 1e3
            got[which].append(ms / a.steps)
            print(json.dumps(dict(wall_reaction=which, ms_per_step=round(ms / a.steps, 4), mlups=round(mlups, 1), fluid_nodes=cells,
                                  bulk_cells=s.bulk_cells, device_bytes=s.device_bytes, size=size, relax=a.relax, steps=a.steps)), flush=True)
    print(json.dumps({k: dict(median_ms=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4)) for k, v in got.items() if v}))
    s.close()


if __name__ == "__main__":
    main()
