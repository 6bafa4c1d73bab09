"""Times the steady-state monitor beside the plane integrals on the bench's porous lattice, both 3-D models.

    python tools/change_bench.py [nx ny nz]              default 512 512 512

One process, one GPU.  Prints two JSON lines, "c5" (perturbation model, after lbmpm_rk3d_phase_field(ctx, 1)) and "csf3d": the mean, least
and largest of CALLS synchronised integrals(), change(remark=True) and change(remark=False) calls after a warm-up each (host clock around
a call that ends in the stream's synchronisation and the copy of nz * 96 or nz * 88 bytes), and for csf3d the time of four windows of 100
steps by HIP events: one before anything of the monitor exists, one after mark_change() and one after each of two change() calls -- the
step rate around the calls of a run with steady_every = 100 -- beside the same four windows of a solver that never marks ("plain": the
state evolves, so the windows are compared pairwise)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import c5_domain, c5_state  # noqa: E402

CALLS = 10


def timed(fn):
    fn()
    ts = []
    for _ in range(CALLS):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return dict(mean_ms=round(float(np.mean(ts)), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def main():
    size = tuple(int(v) for v in sys.argv[1:4]) if len(sys.argv) >= 4 else (512, 512, 512)
    dom = c5_domain(size)
    rR, rB = c5_state(dom, 0, size[2], "initial")

    from openlbmpm_amd.rk3d import RK3DSlab
    s = RK3DSlab(dom, 0, size[2], dict(relax="MRT"))
    s.set_density(rR, rB)
    s.step_single(20)
    s.phase_field(diagnostics=True)
    s.mark_change()
    s.step_single(10)
    s.phase_field(diagnostics=True)
    print(json.dumps(dict(model="c5", size=size, fluid=s.num_fluid_nodes, integrals=timed(s.integrals), change_remark=timed(lambda: s.change(remark=True)),
                          change_keep=timed(lambda: s.change(remark=False)))), flush=True)
    s.close()

    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    dom[0] = dom[1]; dom[-1] = dom[-2]
    rR, rB = c5_state(dom, 0, size[2], "initial")
    c = RK3DCSFSolver(dom, dict(relax="MRT", tauB=0.8))
    c.set_macro(rR, rB)
    c.step(20)
    plain = [round(c.step_timed(100)[0], 2) for _ in range(4)]        # the same windows of a run that never marks
    c.close()
    c = RK3DCSFSolver(dom, dict(relax="MRT", tauB=0.8))
    c.set_macro(rR, rB)
    c.step(20)
    win = [c.step_timed(100)[0]]
    c.mark_change()
    win.append(c.step_timed(100)[0])
    for _ in range(2):
        g = c.change()
        win.append(c.step_timed(100)[0])
    print(json.dumps(dict(model="csf3d", size=size, fluid=c.num_fluid_nodes, ms_per_100_steps=[round(w, 2) for w in win], ms_per_100_steps_plain=plain, integrals=timed(c.integrals),
                          change_remark=timed(lambda: c.change(remark=True)), change_keep=timed(lambda: c.change(remark=False)),
                          velocity_change_last_window=g.velocity_change())), flush=True)
    c.close()


if __name__ == "__main__":
    main()
