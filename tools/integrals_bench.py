"""Times the plane integrals reduced on the device against the route that existed before them for the same numbers.

    python tools/integrals_bench.py <n> <model>          n: edge of the bench's porous lattice; model: rk3d | csf | tracers

One process, one GPU.  Prints two JSON lines:
  * "integrals": mean of CALLS synchronised integrals() calls after two warm-ups (host clock around a call that ends in the stream's
    synchronisation and the copy of nz * 96 bytes);
  * "fields": the five get() calls (rho_R, rho_B, u) and the numpy reductions that give the same totals -- masses, fluxes, saturation,
    Darcy velocities, the largest speed, the non-finite count.
For the perturbation model both routes need lbmpm_rk3d_phase_field(ctx, 1) first; it is timed on its own ("phase_field_ms").  The time
of one step of the same lattice is printed with the first line (CSF: also its collide launches').
model = tracers: the CSF model with three tracers and the reaction; "tracer_integrals" is the median of TRACER_CALLS synchronised
tracer_integrals() calls after two warm-ups, "tracer_fields" the median of three passes of get_concentration + get_tracer_pdf per tracer
and the numpy sums per plane that give the same table; both lines carry the bytes their route moves."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CALLS = 12


def from_fields(get, dom):
    """the totals by the old route: whole fields to the host, numpy over them"""
    rR, rB, vx, vy, vz = (get(k) for k in ("rhoR", "rhoB", "vx", "vy", "vz"))
    fl = dom == 1
    fin = np.isfinite(rR) & np.isfinite(rB) & np.isfinite(vx) & np.isfinite(vy) & np.isfinite(vz)
    good = fl & fin
    red = good & (rR > rB)                      # phi = (rR - rB) / (rR + rB) > 0
    u2 = vx * vx + vy * vy + vz * vz
    return dict(cells=int(fl.sum()), nonfinite=int((fl & ~fin).sum()), saturationR=float(red.sum() / max(int(good.sum()), 1)),
                massR=float(rR[good].sum()), massB=float(rB[good].sum()), fluxR=float((rR * vz)[good].sum()) / dom.shape[0],
                fluxB=float((rB * vz)[good].sum()) / dom.shape[0], darcyR=float(vz[red].sum()) / dom.size,
                darcyB=float(vz[good & ~red].sum()) / dom.size, maxSpeed=float(np.sqrt(u2[good].max())))


TRACER_CALLS = 15


def tracer_table_from_fields(s, dom, nT):
    """[nz][nT][9] by the route that existed before: dense fields to the host, numpy over the fluid cells of every plane"""
    fl = dom == 1
    out = np.zeros((dom.shape[0], nT, 9))
    for k in range(nT):
        c, g = s.get_concentration(k), s.get_tracer_pdf(k)
        fin = fl & np.isfinite(c) & np.all(np.isfinite(g), axis=-1)
        w = fin.astype(np.float64)
        out[:, k, 0], out[:, k, 8] = fl.sum(axis=(1, 2)), (fl & ~fin).sum(axis=(1, 2))
        cz = np.where(fin, c, 0.0)
        out[:, k, 1] = cz.sum(axis=(1, 2))
        for a in range(3):
            out[:, k, 2 + a] = ((g[..., 1 + 2 * a] - g[..., 2 + 2 * a]) * w).sum(axis=(1, 2))
        out[:, k, 5] = (cz * cz).sum(axis=(1, 2))
        any_good = fin.any(axis=(1, 2))
        out[:, k, 6] = np.where(any_good, np.where(fin, c, np.inf).min(axis=(1, 2)), 0.0)
        out[:, k, 7] = np.where(any_good, np.where(fin, c, -np.inf).max(axis=(1, 2)), 0.0)
    return out


def tracers(n, dom, torch):
    from openlbmpm_amd.geometry import initial_densities_rk3d
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    nT = 3
    dom[0] = dom[1]; dom[-1] = dom[-2]
    rR, rB = initial_densities_rk3d(dom, 10)
    s = RK3DCSFSolver(dom, dict(relax="MRT", theta=60.0, tauB=0.8, velocityZB=-1.0e-3))
    s.configure_tracers(num_tracers=nT, diffusion_x=(1. / 6., 0.1, 0.2), diffusion_z=(0.2, 0.08, 0.1), beta_interface=(1.0, 0.5, 0.0),
                        inlet_concentration=(0.8, 0.4, 0.0), dirichlet_inlet=True, free_outlet=True, reaction_rate=0.03)
    s.set_macro(rR, rB)
    del rR, rB
    zz = np.arange(n, dtype=np.float64)[:, None, None]
    for k in range(nT):
        s.set_concentration(k, (0.5 + 0.3 * np.cos(2 * np.pi * (zz + 3 * k) / n)) * (dom == 1))
    s.step(8); s.sync()
    for _ in range(2):
        t = s.tracer_integrals()
    times = []
    for _ in range(TRACER_CALLS):
        t0 = time.perf_counter()
        t = s.tracer_integrals()
        times.append((time.perf_counter() - t0) * 1e3)
    new_ms = float(np.median(times))
    F, N = s.num_fluid_nodes, dom.size
    what = "csf %d^3 porous (porosity 0.65), MRT, %d tracers with the reaction, after 8 steps" % (n, nT)
    read = F * (7 * nT * 8 + 6 * 4) + N * 4 + F * 4         # populations, the source table once, the mask word of every cell, cidx
    print(json.dumps(dict(route="tracer_integrals", workload=what, gpu=torch.cuda.get_device_name(0), ms=new_ms, ms_min=min(times), ms_max=max(times),
                          calls=TRACER_CALLS, fluid_cells=F, cells=N, device_bytes_read=read, read_tb_per_s=read / new_ms / 1e9, host_bytes=n * nT * 72,
                          device_gb=s.device_bytes / 1e9, mass=[t.mass(k) for k in range(nT)], nonfinite=t.nonfinite)), flush=True)
    old = tracer_table_from_fields(s, dom, nT)          # warm-up
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        old = tracer_table_from_fields(s, dom, nT)
        times.append((time.perf_counter() - t0) * 1e3)
    old_ms = float(np.median(times))
    scale = np.maximum(np.abs(old).max(axis=0), 1e-300)
    print(json.dumps(dict(route="tracer_fields", workload=what, ms=old_ms, ms_min=min(times), ms_max=max(times), calls=3, ratio=old_ms / new_ms,
                          staging_bytes=nT * N * 72, host_bytes=nT * N * 64, counts_equal=bool(np.array_equal(old[..., [0, 6, 7, 8]], t.planes[..., [0, 6, 7, 8]])),
                          worst_relative_difference=float((np.abs(old - t.planes) / scale).max()))), flush=True)
    s.close()


def main():
    n, model = int(sys.argv[1]), sys.argv[2]
    import torch
    assert torch.cuda.is_available(), "integrals_bench.py needs a GPU"
    from openlbmpm_amd.geometry import porous_spheres, initial_densities_rk3d
    dom = porous_spheres(n, n, n, porosity=0.65, rmin=6.0, rmax=20.0, seed=20260928, nbuf=10)
    if model == "tracers":
        return tracers(n, dom, torch)
    extra = {}
    if model == "csf":
        from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
        dom[0] = dom[1]; dom[-1] = dom[-2]
        rR, rB = initial_densities_rk3d(dom, 10)
        s = RK3DCSFSolver(dom, dict(relax="MRT", theta=60.0, tauB=0.8))
        s.set_macro(rR, rB)
        del rR, rB
        s.step(3); s.sync()
        tot, coll = s.step_timed(5)
        extra = dict(step_ms=tot / 5, collide_ms=coll / 5)
        observe, get, sync = (lambda: None), (lambda k: s.get("rec_" + k)), s.sync
    elif model == "rk3d":
        from openlbmpm_amd.rk3d import RK3DSlab
        rR, rB = initial_densities_rk3d(dom, 10)
        s = RK3DSlab(dom, 0, n, dict(relax="MRT", tauB=0.8))
        s.set_density(rR, rB)
        del rR, rB
        s.step_single(3); s.sync()
        tot, _ = s.step_timed(5)
        extra = dict(step_ms=tot / 5)
        observe, get, sync = (lambda: s.phase_field(diagnostics=True)), s.get, s.sync
    else:
        raise SystemExit("model: rk3d | csf | tracers")
    observe(); sync()
    t0 = time.perf_counter(); observe(); sync()
    extra["phase_field_ms"] = (time.perf_counter() - t0) * 1e3 if model == "rk3d" else 0.0
    for _ in range(2):
        g = s.integrals()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        g = s.integrals()
    new_ms = (time.perf_counter() - t0) * 1e3 / CALLS
    what = "%s %d^3 porous (porosity 0.65), MRT, after 8 steps" % (model, n)
    print(json.dumps(dict(route="integrals", workload=what, gpu=torch.cuda.get_device_name(0), ms=new_ms, calls=CALLS, fluid_cells=s.num_fluid_nodes,
                          device_gb=s.device_bytes / 1e9, saturationR=g.saturation_R, massR=g.mass_R, massB=g.mass_B, fluxB=g.flux_B,
                          darcyB=g.darcy_uz_B, maxSpeed=g.max_speed, nonfinite=g.nonfinite, **extra)), flush=True)
    reps = 2 if n <= 256 else 1
    old = from_fields(get, dom)                  # warm-up (the CSF model allocates its staging array here)
    t0 = time.perf_counter()
    for _ in range(reps):
        old = from_fields(get, dom)
    old_ms = (time.perf_counter() - t0) * 1e3 / reps
    print(json.dumps(dict(route="fields", workload=what, ms=old_ms, calls=reps, ratio=old_ms / new_ms, device_gb=s.device_bytes / 1e9, **old)), flush=True)
    s.close()


if __name__ == "__main__":
    main()
