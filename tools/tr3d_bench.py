"""Times the 3-D CSF colour-gradient step with 0, 1 and 3 D3Q7 tracers (lbmpm_rk3dcsf_tracer_*) on the bench's porous lattice, and the
tracers' kernel tr3d_step alone from a rocprofv3 kernel trace.

    python tools/tr3d_bench.py [--edge 512] [--steps 20] [--relax MRT] [--tracers 0,1,3] [--slabs 1,8] [--trace] [--out DIR]

Every tracer count runs in a child process of its own (a fresh context; with --trace a second child under
`rocprofv3 --kernel-trace --stats`, whose table gives the average duration of tr3d_step).  Prints one JSON line per tracer count:
ms per step by HIP events, and for tr3d_step its time, the bytes it must move per fluid cell -- 7 loads + 7 stores per tracer, rho_R, u
and G read (7), the cell's number and its 6 source-cell numbers (4 bytes each), + the 4 doubles the collision kernels wrote for it -- and that rate as a
fraction of the 6.3 TB/s copy ceiling DESIGN.md uses.
--slabs N (> 1): the lattice cut into N z-slabs, N contexts of this process on this one GPU (rk3dcsf.RK3DCSFCluster(..., tracers=...), as
tests/test_full_size_gpu.py does for the flow): ms per step on the host clock around the enqueued steps, the population message in bytes
per face as the library counts it (lbmpm_rk3dcsf_face_doubles) beside 8 B x (10 + tracers) per fluid cell of the plane + the flag bytes,
and with --trace tr3d_step summed over the slabs.  One GPU: a rehearsal of the decomposition, no multi-GPU scaling figure."""
import argparse
import json
import os
import shutil
import sqlite3
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_CEILING_GBS = 6300.0


TRACERS = lambda ntr: dict(num_tracers=ntr, diffusion_x=1. / 6., diffusion_y=0.12, diffusion_z=0.2, diffusion_xz=0.01, beta_interface=0.8,      # noqa: E731
                           inlet_concentration=1.0, dirichlet_inlet=True, free_outlet=True, reaction_rate=0.01 if ntr == 3 else 0.0)


def one_cluster(edge, steps, relax, ntr, nslabs):
    import time
    import numpy as np
    from openlbmpm_amd.geometry import porous_spheres, initial_densities_rk3d
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster, MSG_PDF
    dom = porous_spheres(edge, edge, edge, porosity=0.65, rmin=6.0, rmax=20.0, seed=20260928, nbuf=10)
    dom[0] = dom[1]; dom[-1] = dom[-2]
    rR, rB = initial_densities_rk3d(dom, 10)
    c = RK3DCSFCluster(dom, dict(relax=relax, tauB=0.8), nslabs=nslabs, tracers=TRACERS(ntr) if ntr else None)
    c.set_macro(rR, rB)
    for k in range(ntr):
        c.set_concentration(k, np.where(dom == 1, 0.5 + 0.1 * k, 0.0))
    c.step(12); c.sync()
    t0 = time.perf_counter()
    c.step(steps); c.sync()
    tot = 1e3 * (time.perf_counter() - t0)
    n = c.num_fluid_nodes
    ok = bool(np.isfinite(c.get("rec_rhoR")).all()) and all(bool(np.isfinite(c.get_concentration(k)).all()) for k in range(ntr))
    faces = []
    for k, s in enumerate(c.slabs):              # the message through every slab's high face
        cells = int((dom[c.cuts[k + 1] - 1] == 1).sum())
        two = cells + int((dom[c.cuts[k + 1] - 2] == 1).sum())
        faces.append(dict(cut=c.cuts[k + 1] % edge, fluid_cells_of_the_plane=cells, bytes=8 * s.face_doubles(MSG_PDF, 1),
                          expected_bytes=8 * ((10 + ntr) * cells + (two + 7) // 8)))
    print("TR3D " + json.dumps(dict(workload="3-D CSF colour gradient %s + %d D3Q7 tracers, %d^3 porous (porosity 0.65), %d z-slabs on one GPU" % (relax, ntr, edge, nslabs),
                                    tracers=ntr, slabs=nslabs, fluid_cells=n, ms_per_step=tot / steps, mlups=n * steps / tot / 1e3, clock="host, around the enqueued steps",
                                    device_gb=sum(s.device_bytes for s in c.slabs) / 1e9, finite=ok, population_message_high_face=faces)))
    c.close()


def one(edge, steps, relax, ntr, nslabs=1):
    if nslabs > 1:
        return one_cluster(edge, steps, relax, ntr, nslabs)
    import numpy as np
    from openlbmpm_amd.geometry import porous_spheres, initial_densities_rk3d
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    dom = porous_spheres(edge, edge, edge, porosity=0.65, rmin=6.0, rmax=20.0, seed=20260928, nbuf=10)
    dom[0] = dom[1]; dom[-1] = dom[-2]
    rR, rB = initial_densities_rk3d(dom, 10)
    s = RK3DCSFSolver(dom, dict(relax=relax, tauB=0.8))
    if ntr:
        s.configure_tracers(**TRACERS(ntr))
    s.set_macro(rR, rB)
    for k in range(ntr):
        s.set_concentration(k, np.where(dom == 1, 0.5 + 0.1 * k, 0.0))
    s.step(12); s.sync()
    tot, _ = s.step_timed(steps)
    n = s.num_fluid_nodes
    ok = bool(np.isfinite(s.get("rec_rhoR")).all()) and all(bool(np.isfinite(s.get_concentration(k)).all()) for k in range(ntr))
    print("TR3D " + json.dumps(dict(workload="3-D CSF colour gradient %s + %d D3Q7 tracers, %d^3 porous (porosity 0.65)" % (relax, ntr, edge), tracers=ntr,
                                    fluid_cells=n, ms_per_step=tot / steps, mlups=n * steps / tot / 1e3, device_gb=s.device_bytes / 1e9, finite=ok)))
    s.close()


def child(args, ntr, trace_dir=None, nslabs=1):
    cmd = [sys.executable, os.path.abspath(__file__), "--one", str(ntr), "--edge", str(args.edge), "--steps", str(args.steps), "--relax", args.relax,
           "--slabs", str(nslabs)]
    if trace_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", trace_dir, "-o", "x", "--"] + cmd
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit("child for %d tracers failed (%d):\n%s" % (ntr, r.returncode, (r.stdout + r.stderr)[-2000:]))
    line = [l for l in r.stdout.splitlines() if l.startswith("TR3D ")][-1]
    return json.loads(line[5:])


def traced_kernels(trace_dir):
    db = None
    for d, _, files in os.walk(trace_dir):
        for f in files:
            if f.endswith("_results.db"):
                db = os.path.join(d, f)
    if db is None:
        return {}
    c = sqlite3.connect(db)
    return {name: dict(calls=calls, avg_us=avg) for name, calls, avg in c.execute("select name, total_calls, average from top_kernels")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--relax", default="MRT", choices=["MRT", "SRT"])
    ap.add_argument("--tracers", default="0,1,3")
    ap.add_argument("--slabs", default="1", help="numbers of z-slabs, e.g. 1,8 (1: the undivided lattice)")
    ap.add_argument("--trace", action="store_true", help="also run every tracer count > 0 under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--one", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one is not None:
        return one(a.edge, a.steps, a.relax, a.one, int(a.slabs))
    for nslabs, ntr in [(int(n), int(v)) for n in a.slabs.split(",") for v in a.tracers.split(",")]:
        out = child(a, ntr, nslabs=nslabs)
        if a.trace and ntr:
            d = tempfile.mkdtemp(prefix="tr3d_trace_")
            try:
                child(a, ntr, d, nslabs=nslabs)
                k = traced_kernels(d)
            finally:
                shutil.rmtree(d, ignore_errors=True)
            step = [v for n, v in k.items() if "tr3d_step<false" in n]      # (the instance of every step but the first; the table is in microseconds)
            if step and nslabs > 1:                 # calls = slabs x steps: the sum over the slabs per step
                out["tr3d_step"] = dict(ms_summed_over_the_slabs=step[0]["avg_us"] * 1e-3 * nslabs, calls=step[0]["calls"])
            elif step:
                us = step[0]["avg_us"]
                per_cell = 8 * (14 * ntr + 7) + 4 * 7
                out["tr3d_step"] = dict(ms=us * 1e-3, calls=step[0]["calls"], bytes_per_cell=per_cell, collision_writes_bytes_per_cell=32,
                                        GBs=per_cell * out["fluid_cells"] / (us * 1e-6) / 1e9)
                out["tr3d_step"]["fraction_of_copy_ceiling"] = out["tr3d_step"]["GBs"] / COPY_CEILING_GBS
                out["traced_kernels_avg_us"] = {n.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]: round(v["avg_us"], 1) for n, v in k.items() if "csf3d" in n or "tr3d" in n}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
