"""What a body force costs the 3-D CSF step: the lattice of `bench.py --workload csf3d` without one and with one
(lbmpm_rk3dcsf_set_body_force; with it the step launches the BF instances of csf3d_collide and csf3d_collide_deep).

    python tools/dev/csf3d_body_force_cost.py [--size 512 512 512] [--steps 100] [--warmup 20] [--runs 3] [--state initial|mixed]
                                              [--relax MRT|SRT] [--only none|force]

Prints one JSON line per timed run, alternating the two, then their medians.  Step times by HIP events on the solver's stream
(step_timed).  The acceleration is small (1e-6 along z on red, half of it on blue): the state stays the bench's, the kernels do all of
their arithmetic.  For the times of csf3d_collide and csf3d_collide_deep alone run it under
`rocprofv3 --kernel-trace --stats -- python ... --only force --runs 1` (and once with --only none): the instances carry their template
arguments in their names, the last one is BF."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import bench  # noqa: E402
from openlbmpm_amd.rk3dcsf import RK3DCSFSolver  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=(512, 512, 512))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--state", default="initial")
    ap.add_argument("--relax", default="MRT")
    ap.add_argument("--only", choices=["none", "force"], default=None)
    a = ap.parse_args()
    size = tuple(a.size)
    dom = bench.c5_domain(size)
    dom[0] = dom[1]; dom[-1] = dom[-2]
    rR, rB = bench.c5_state(dom, 0, size[2], a.state)
    s = RK3DCSFSolver(dom, dict(relax=a.relax, tauB=0.8))
    cells = s.num_fluid_nodes
    got = {"none": [], "force": []}
    for _ in range(a.runs):
        for which in ("none", "force"):
            if a.only and which != a.only:
                continue
            if which == "force":
                s.set_body_force(red=(0.0, 0.0, -1.0e-6), blue=(0.0, 0.0, -0.5e-6))
            else:
                s.set_body_force(None)
            s.set_macro(rR, rB)
            s.step(a.warmup); s.sync()
            ms, _ = s.step_timed(a.steps)
            mlups = cells * a.steps / ms / 1e3
            got[which].append(mlups)
            print(json.dumps(dict(body_force=which, ms_per_step=round(ms / a.steps, 4), mlups=round(mlups, 1), fluid_nodes=cells,
                                  bulk_cells=s.bulk_cells, size=size, state=a.state, relax=a.relax, steps=a.steps)), flush=True)
    print(json.dumps({k: dict(median_mlups=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1)) for k, v in got.items() if v}))
    s.close()


if __name__ == "__main__":
    main()
