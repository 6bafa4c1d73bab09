"""Non-interactive command line (replaces the reference's interactive, un-importable main.py):

    python -m openlbmpm_amd rk  <ini-dir> [--out DIR] [--steps N] [--device D]
    python -m openlbmpm_amd sc  <ini-dir> [--out DIR] [--steps N] [--device D]
    python -m openlbmpm_amd tr  <ini-dir> ...      colour gradient + tracers (RKtwophasesetup2D.ini + transportsetup.ini)
    python -m openlbmpm_amd tr3d <ini-dir> ...     D3Q19 CSF colour gradient + D3Q7 tracers (RKtwophasesetup3D.ini + transportsetup.ini); under torchrun: z-slabs
    python -m openlbmpm_amd rk3d <ini-dir> ...     D3Q19 colour gradient (RKtwophasesetup3D.ini); under torchrun: z-slabs, one per GPU
        [--csf-transport auto|ipc|rccl]           rk3d with SurfaceTensionType = 'CSF' and tr3d under torchrun: the slabs' face messages over the library's
                                                  own transports (default: through torch.distributed)
        [--integrals-every N]                     rk3d, tr3d: saturation, masses, fluxes, Darcy velocities per plane every N steps (/Integrals of the result
                                                  file); tr3d also the tracers' mass, fluxes and extrema per plane and tracer (/TracerIntegrals of
                                                  ConcentrationResults)
        [--clusters-every N]                      rk3d: the connected clusters of each phase, labelled on the device, every N steps (/Clusters of the
        [--clusters-connectivity 6|18]            result file: label, class, cells, zmin, zmax per cluster); percolation and trapped cells to the log
        [--clusters-props]                        rk3d, with --clusters-every: faces, pairs, squares, cubes, plane sum, mass and momentum per cluster
                                                  (/Clusters/PropsAtStep<step>); ganglia and mobile ganglia to the log
        [--morphology-every N]                    rk3d: cells, class pairs, squares and cubes per plane, counted on the device, every N steps (/Morphology
        [--morphology-phi-cut c]                  of the result file); interfacial area, wetted fraction, Euler characteristics, capillary pressure to the log
        [--wrap-z]                                rk3d with periodic z: --clusters-every / --morphology-every close the seam between plane nz-1 and plane 0
                                                  (a cluster across it is one row, /Clusters/WindingAtStep<step>; percolation = a cluster that winds)
        [--contact-angles FILE]                   rk3d with SurfaceTensionType = 'CSF', tr3d: mixed wettability -- a .npy of contact angles per solid voxel
                                                  (the lattice's shape, or the voxel file's; NaN = the ini's ContactAngle); /Wettability/ContactAngle
        [--body-force GX GY GZ]                   rk3d with SurfaceTensionType = 'CSF', tr3d: an acceleration in lattice units for both colours (gravity,
        [--body-force-blue GX GY GZ]              force-driven flow), the second option: another one for blue; /BodyForce/Acceleration of the result file;
                                                  rk with SurfaceTensionType = 'CSF', tr: the same with GX GY
        [--wall-reaction K [K ...]]               tr3d: first-order reaction of the tracers at solid walls, D dC/dn = k C_wall -- one rate per tracer in lattice
        [--wall-minerals FILE]                    units (inf: C_wall = 0), or classes x tracers with a .npy of class bytes per solid voxel; /WallReaction/Rates
                                                  and, with --integrals-every, /TracerWallIntegrals of ConcentrationResults
        [--steady-every N]                        rk3d: the change of velocity and phase field between multiples of N steps, reduced on the device (/Steady of
        [--steady-tol t] [--steady-phase-tol p]   the result file); with a tolerance the run ends at the first multiple where the change is within it
"""
import argparse
import sys
import time


def _rank_device(device):
    """launched by torchrun: one rank per GPU, the process group of LBMPM_DIST_BACKEND (nccl; gloo: several ranks rehearsing on one GPU)"""
    import os
    if int(os.environ.get("WORLD_SIZE", "1")) <= 1:
        return device
    import torch
    import torch.distributed as dist
    device = int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count()
    torch.cuda.set_device(device)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if os.environ.get("LBMPM_DIST_BACKEND", "nccl") == "nccl":
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", device))
    else:
        dist.init_process_group(backend=os.environ["LBMPM_DIST_BACKEND"])
    return device


def parser():
    ap = argparse.ArgumentParser(prog="python -m openlbmpm_amd")
    # (argparse takes -1e-6 for an option: its pattern of a negative number knows no exponent; --body-force 0 0 -1e-6 is gravity)
    import re
    ap._negative_number_matcher = re.compile(r"^-(\d+\.?\d*|\.\d+)([eE][-+]?\d+)?$")
    ap.add_argument("model", choices=["rk", "sc", "tr", "rk3d", "tr3d"], help="rk = colour gradient (RKtwophasesetup2D.ini); "
                                                       "sc = Shan-Chen / EFS (twophasesetup.ini + efs2D.ini|shanchen2D.ini)")
    ap.add_argument("ini_dir")
    ap.add_argument("--out", default=None, help="result directory (default ~/LBMResults)")
    ap.add_argument("--steps", type=int, default=None, help="override the ini's number of time steps")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--csf-transport", choices=["auto", "ipc", "rccl"], default=None,
                    help="rk3d with SurfaceTensionType = 'CSF', tr3d; under torchrun: move the slabs' face messages over the library's own transport")
    ap.add_argument("--contact-angles", default=None, metavar="FILE",
                    help="rk3d with SurfaceTensionType = 'CSF', tr3d: contact angles in degrees per solid voxel (.npy in the shape of the lattice, or of the "
                         "voxel file; NaN: the ini's ContactAngle) -- every fluid cell next to solid takes the Cassie average over its solid neighbours; "
                         "the angles in force go to /Wettability/ContactAngle of the result file.  The same as [SurfaceTension] ContactAngleFile")
    ap.add_argument("--body-force", type=float, nargs="+", default=None, metavar="G",
                    help="rk3d with SurfaceTensionType = 'CSF', tr3d: GX GY GZ; rk with SurfaceTensionType = 'CSF', tr: GX GY -- an acceleration in lattice "
                         "units on both colours (force density rho_R g + rho_B g): gravity, or the drive of a flow between open ends at equal pressure or "
                         "on a periodic lattice.  rk3d, tr3d: the same as [BodyForce] isBodyForce = 'yes' with bodyForceX / Y / Z (the 2-D ini keeps "
                         "refusing that section: the reference reads it and never uses it); /BodyForce/Acceleration of the result file")
    ap.add_argument("--body-force-blue", type=float, nargs="+", default=None, metavar="G",
                    help="... the blue fluid's acceleration where it differs (--body-force is then the red one's; alone: red has none)")
    ap.add_argument("--wall-reaction", type=float, nargs="+", default=None, metavar="K",
                    help="tr3d: the tracers react at solid walls, D dC/dn = k C_wall (a reactive bounce-back): one rate k >= 0 per tracer in lattice units "
                         "(a velocity; Damkoehler number k H / D; inf: the instantaneous reaction), or classes x tracers values class by class with "
                         "--wall-minerals.  The same as [Reaction] WallReactionRate; /WallReaction/Rates of ConcentrationResults and, with "
                         "--integrals-every, the uptake per plane and tracer in /TracerWallIntegrals")
    ap.add_argument("--wall-minerals", default=None, metavar="FILE",
                    help="tr3d, with --wall-reaction: the mineral class 0 .. 7 of every solid voxel (.npy of integers in the shape of the lattice, or of the "
                         "voxel file).  The same as [Reaction] WallMineralFile")
    ap.add_argument("--integrals-every", type=int, default=0, metavar="N",
                    help="rk3d, tr3d: every N steps the plane integrals (saturation, masses, fluxes, largest speed, non-finite cells), reduced on the device, "
                         "to /Integrals of the result file and the log; tr3d also the tracers' (cells, mass, flux_x, flux_y, flux_z, sum_c2, cmin, cmax, "
                         "nonfinite per plane and tracer) to /TracerIntegrals of ConcentrationResults; 0: off")
    ap.add_argument("--clusters-every", type=int, default=0, metavar="N",
                    help="rk3d: every N steps the connected clusters of each phase (label, class, cells, zmin, zmax per cluster), labelled on the device, "
                         "to /Clusters of the result file; counts, the largest cluster, percolation and trapped cells to the log; 0: off")
    ap.add_argument("--clusters-props", action="store_true",
                    help="rk3d, with --clusters-every: the property table beside every cluster table (faces, pairs, squares, cubes, plane sum, mass and "
                         "momentum per cluster, reduced on the device): /Clusters/PropsAtStep<step>; ganglia and mobile ganglia to the log")
    ap.add_argument("--clusters-connectivity", type=int, choices=[6, 18], default=6, help="rk3d: neighbours of a cell: 6 faces, or the 18 D3Q19 links")
    ap.add_argument("--morphology-every", type=int, default=0, metavar="N",
                    help="rk3d: every N steps the phase morphology (cells, density sums, class pairs, squares and cubes per plane), counted on the device, "
                         "to /Morphology of the result file; interfacial area, wetted fraction, Euler characteristics and capillary pressure to the log; 0: off")
    ap.add_argument("--morphology-phi-cut", type=float, default=0.0, metavar="c", help="rk3d: cells with |phi| within c of 0 belong to neither phase")
    ap.add_argument("--wrap-z", action="store_true",
                    help="rk3d with periodic z (BoundaryTypeInlet = BoundaryTypeOutlet = 'Periodic'), with --clusters-every / --morphology-every: close the "
                         "seam between plane nz-1 and plane 0 -- a cluster across it is one row (zmax may exceed nz-1), /Clusters/WindingAtStep<step> says "
                         "by how many periods a cluster is connected to its own image (0: a ganglion), the morphology counts across the seam; "
                         "/Clusters/WrapZ and /Morphology/WrapZ = 1")
    ap.add_argument("--steady-every", type=int, default=0, metavar="N",
                    help="rk3d: at every multiple of N steps the change of the velocity and the phase field since the multiple before (per plane: squared "
                         "changes by phase, cells that changed colour, largest changes), reduced on the device against a snapshot kept there, to /Steady "
                         "of the result file and the log; 0: off")
    ap.add_argument("--steady-tol", type=float, default=0.0, metavar="t",
                    help="rk3d, with --steady-every: end the run at the first multiple where the relative L2 change of the velocity is <= t (and that of the "
                         "phase field <= --steady-phase-tol); 0: monitor only")
    ap.add_argument("--steady-phase-tol", type=float, default=None, metavar="p", help="rk3d: the bound on the rms change of phi (default: --steady-tol)")
    return ap


def _body_force(a):
    """--body-force / --body-force-blue as the drivers' body_force=, or None: three components for the 3-D models, two for rk and tr"""
    if a.body_force is None and a.body_force_blue is None:
        return None
    n = 3 if a.model in ("rk3d", "tr3d") else 2
    for opt, v in (("--body-force", a.body_force), ("--body-force-blue", a.body_force_blue)):
        if v is not None and len(v) != n:
            raise SystemExit("%s of %s takes %s, not %d values" % (opt, a.model, "GX GY GZ" if n == 3 else "GX GY", len(v)))
    if a.body_force_blue is None:
        return tuple(a.body_force)
    return dict(red=tuple(a.body_force or (0.0,) * n), blue=tuple(a.body_force_blue))


def main(argv=None):
    a = parser().parse_args(argv)
    t0 = time.time()
    if a.model == "sc" and _body_force(a) is not None:
        raise SystemExit("--body-force belongs to the colour-gradient CSF models (rk, tr, rk3d, tr3d): the Shan-Chen solvers have no body force")
    if a.model != "tr3d" and (a.wall_reaction is not None or a.wall_minerals is not None):
        raise SystemExit({"rk3d": "--wall-reaction belongs to tr3d: rk3d runs the flow alone, there is no tracer to react",
                          "tr": "--wall-reaction belongs to tr3d: the D2Q5 tracers of tr bounce back from solids unchanged"}
                         .get(a.model, "--wall-reaction belongs to tr3d: the 2-D solvers carry no tracers that could react at a wall"))
    if a.model == "rk":
        from .RKD2Q9 import RKColorGradientLBM
        sim = RKColorGradientLBM(a.ini_dir, output_dir=a.out, device=a.device, body_force=_body_force(a))
        if a.steps is not None:
            sim.timeSteps = a.steps
        path = sim.runRKColorGradient2D()
        steps, nodes = sim.timeSteps, sim.voidSpace
    elif a.model == "rk3d":
        from .RKColorGradientD3Q19 import RKColorGradient3D
        device = _rank_device(a.device)
        sim = RKColorGradient3D(a.ini_dir, output_dir=a.out, device=device, csf_transport=a.csf_transport, integrals_every=a.integrals_every,
                                clusters_every=a.clusters_every, clusters_connectivity=a.clusters_connectivity, clusters_props=a.clusters_props,
                                morphology_every=a.morphology_every, morphology_phi_cut=a.morphology_phi_cut, steady_every=a.steady_every,
                                steady_tol=a.steady_tol, steady_phase_tol=a.steady_phase_tol, contact_angle_solids=a.contact_angles,
                                body_force=_body_force(a), analyses_wrap_z=a.wrap_z)
        if a.steps is not None:
            sim.timeSteps = a.steps
        path = sim.runRKColorGradient3D()
        steps, nodes = sim.timeSteps if sim.steady_step is None else sim.steady_step, sim.voidSpace
        if sim.steady_step is not None:
            print("steady at step %d" % sim.steady_step)
    elif a.model == "tr3d":
        from .Transport3DRK import Transport3DRK
        sim = Transport3DRK(a.ini_dir, output_dir=a.out, device=_rank_device(a.device), csf_transport=a.csf_transport,
                            integrals_every=a.integrals_every, contact_angle_solids=a.contact_angles, body_force=_body_force(a),
                            wall_reaction=a.wall_reaction, wall_minerals=a.wall_minerals)
        if a.steps is not None:
            sim.timeSteps = a.steps
        path = " and ".join(str(f) for f in sim.runTransport3DMPMCRK())        # (under torchrun rank 0 writes both files)
        steps, nodes = sim.timeSteps, sim.voidSpace
    elif a.model == "tr":
        from .Transport2DRK import Transport2DRK
        sim = Transport2DRK(a.ini_dir, output_dir=a.out, device=a.device, body_force=_body_force(a))
        if a.steps is not None:
            sim.timeSteps = a.steps
        path = " and ".join(sim.runTransport2DMPMCRKNew())
        steps, nodes = sim.timeSteps, sim.voidSpace
    else:
        from .ShanChenD2Q9 import ShanChenD2Q9
        sim = ShanChenD2Q9(a.ini_dir, output_dir=a.out, device=a.device)
        if a.steps is not None:
            sim.numTimeStep = a.steps
        path = sim.runTypeSCmodel()
        steps, nodes = sim.numTimeStep + 1, int(sim.isDomain.sum())
    dt = time.time() - t0
    print("%d steps on %d fluid nodes in %.2f s (%.1f MLUPS incl. output); results in %s"
          % (steps, nodes, dt, steps * nodes / dt / 1e6, path))
    return 0


if __name__ == "__main__":
    sys.exit(main())
