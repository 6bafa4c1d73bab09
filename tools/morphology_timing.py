"""What morphology() costs on the bench lattice: the 512^3 porous medium of bench.py under either 3-D model after `steps` steps, beside
integrals() and clusters() on the same state.  Not part of bench.py; there is no threshold, DESIGN.md keeps the numbers.

    python tools/morphology_timing.py [--size NX NY NZ] [--steps 60] [--calls 7] [--limit SECONDS]

Every model runs in a child process of its own under a time limit (a child that runs into it is killed and reported, the next one is
not started).  A call is timed twice: by HIP events recorded around it on the default stream, which waits for the solver's stream, and
by the host clock around the synchronous call (each ends with a stream synchronisation and the copy of its table); medians over `calls`
calls after two warm-up calls.  The events bracket the whole call -- launches, the copy, the synchronisation, and for morphology() the
allocation of its chunk partials -- not the launches alone.  One JSON line per model.

The kernels' own times come from a trace of one model's child (morphology_*):

    rocprofv3 --kernel-trace --stats -- python tools/morphology_timing.py --one csf|perturbation --steps 10 --calls 5
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(size, model, steps, calls):
    sys.path.insert(0, ROOT)
    import torch
    import bench
    t0 = time.perf_counter()
    if model == "csf":
        s, _, _ = bench.build_csf3d(tuple(size), 0, "MRT", "initial")
        advance = s.step
    else:
        from openlbmpm_amd.rk3d import RK3DSlab
        dom = bench.c5_domain(tuple(size))
        s = RK3DSlab(dom, 0, size[2], dict(relax="MRT"), device=0)
        s.set_density(*bench.c5_state(dom, 0, size[2], "initial"))

        def advance(n):
            s.step_single(n)
            s.phase_field(diagnostics=True)
    out = dict(model=model, size=list(size), fluid_cells=int(s.num_fluid_nodes), build_s=round(time.perf_counter() - t0, 1), steps_before=steps)
    advance(steps)
    s.sync()
    before = s.device_bytes
    for name, call in (("integrals", s.integrals), ("clusters", s.clusters), ("morphology", s.morphology), ("morphology_cut_0.3", lambda: s.morphology(0.3))):
        ev, wall = [], []
        for k in range(2 + calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            got = call()
            b.record()
            b.synchronize()
            t1 = time.perf_counter()
            if k >= 2:
                ev.append(a.elapsed_time(b)); wall.append((t1 - t0) * 1e3)
        out[name] = dict(events_ms=round(statistics.median(ev), 3), wall_ms=round(statistics.median(wall), 3), events_min_ms=round(min(ev), 3),
                         events_max_ms=round(max(ev), 3), calls=calls)
        if name == "clusters":
            before = s.device_bytes
        if name == "morphology":
            out["summary"] = {k: float(v) for k, v in got.summary().items()}
            out["cells"] = {p: got.cells(p) for p in "RBN"}
    out["device_bytes_per_cell"] = round((s.device_bytes - before) / float(size[0] * size[1] * size[2]), 3)
    s.close()
    print("MORPHOLOGY_TIMING " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 512])
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds a model's child process may take")
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.calls < 5:
        ap.error("medians of at least 5 calls")
    if a.one:
        return one(a.size, a.one, a.steps, a.calls)
    for model in ("csf", "perturbation"):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", model, "--steps", str(a.steps), "--calls", str(a.calls), "--size"] + [str(v) for v in a.size]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print("MORPHOLOGY_TIMING " + json.dumps(dict(model=model, error="ran into the limit of %g s" % a.limit)), flush=True)
            return 1
        if rc != 0:              # a child that failed or faulted: nothing more is started on the device
            print("MORPHOLOGY_TIMING " + json.dumps(dict(model=model, error="exit status %d" % rc)), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
