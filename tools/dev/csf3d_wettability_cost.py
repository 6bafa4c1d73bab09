"""What a contact-angle map costs the 3-D CSF step: the lattice of `bench.py --workload csf3d` without a map and with a uniform one
(lbmpm_rk3dcsf_set_contact_angles; the uniform map computes what the scalar computes, bit for bit, through csf3d_gradient<true>).

    python tools/dev/csf3d_wettability_cost.py [--size 512 512 512] [--steps 100] [--warmup 20] [--runs 3] [--state initial|mixed] [--only none|map]

Prints one JSON line per timed run, alternating the two, then their medians.  Step times by HIP events on the solver's stream
(step_timed).  For the time of csf3d_gradient alone run it under `rocprofv3 --kernel-trace --stats -- python ... --only map --runs 1`
(and once with --only none): the two instances carry <true> / <false> in their names."""
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
    ap.add_argument("--only", choices=["none", "map"], default=None)
    a = ap.parse_args()
    size = tuple(a.size)
    dom = bench.c5_domain(size)
    dom[0] = dom[1]; dom[-1] = dom[-2]
    rR, rB = bench.c5_state(dom, 0, size[2], a.state)
    par = dict(relax=a.relax, tauB=0.8)
    s = RK3DCSFSolver(dom, par)
    uniform = np.full(dom.shape, float(s.params["theta"]))
    cells = s.num_fluid_nodes
    walls = int((s.get("kind") == 3).sum())
    got = {"none": [], "map": []}
    for _ in range(a.runs):
        for which in ("none", "map"):
            if a.only and which != a.only:
                continue
            before = s.device_bytes
            s.set_contact_angles(uniform if which == "map" else None)
            map_bytes = s.device_bytes - before
            s.set_macro(rR, rB)
            s.step(a.warmup); s.sync()
            ms, _ = s.step_timed(a.steps)
            mlups = cells * a.steps / ms / 1e3
            got[which].append(mlups)
            print(json.dumps(dict(map=which, ms_per_step=round(ms / a.steps, 4), mlups=round(mlups, 1), fluid_nodes=cells, wall_cells=walls,
                                  map_bytes=max(map_bytes, 0), bulk_cells=s.bulk_cells, size=size, state=a.state, steps=a.steps)), flush=True)
    print(json.dumps({k: dict(median_mlups=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1)) for k, v in got.items() if v}))
    s.close()


if __name__ == "__main__":
    main()
