"""3-D colour-gradient driver: class RKColorGradient3D(pathIniFile).runRKColorGradient3D() -- the
entry the reference's main.py:22,80-81 calls but whose module is missing from its tree.  Own
design by analogy with the 2-D driver (RKD2Q9.py): reads IniFiles/RKtwophasesetup3D.ini, builds a
duct (solid side walls, open z planes) or takes a voxel array, starts red below the top buffer
planes and blue in them (RKD2Q9.py:511-531 carried to 3-D), records densities and velocity
(RKD2Q9.py:938-957; the populations too with record_pdf=True).

[CyclesSetup] IsCycle = 'yes' (RKtwophasesetup3D.ini:57-59) follows the 2-D rules (RKD2Q9.py:491-559) with z in the place of y:
  * no image: the record LastStep of <initial_dir>/SimulationResultsRK3D (densities + velocity), the top 20 planes refilled with
    blue, populations = equilibria of those fields (RKD2Q9.py:492-508),
  * image: <initial_dir>/cycleInitialRK3D -- /FluidMacro/FluidDensityR|B, /FluidPDF/FluidPDFR|B [nz][ny][nx][19],
    /FluidVelocity/FluidVelocityX|Y|Z -- taken over with the colours swapped in the top buffer planes (RKD2Q9.py:532-556);
    write_cycle_initial() writes that file from a finished run.
Beyond the reference: checkpoint() / restart_from= keep the solver's stored state (lbmpm_rk3d_get_state / set_state): a run
continued from a checkpoint equals the uninterrupted one bit for bit, on any number of ranks.

[SurfaceTension] SurfaceTensionType = 'CSF' (the section of RKtwophasesetup2D.ini added to the 3-D file): the 2-D CSF loop carried to
D3Q19 (openlbmpm_amd/rk3dcsf.py, lbmpm_rk3dcsf_*) instead of the perturbation loop -- surface tension, contact angle (wetting rule 2),
DeltaValue, TauType from the ini; one GPU or one z-slab per rank (rk3dcsf.RK3DCSFDistributed: three face messages per step, through
torch.distributed from Python after every stage, or -- csf_transport = 'auto' | 'ipc' | 'rccl' -- over the library's own transports, one C
call per run of steps); records hold what the reference records (the lattice after the next step's boundary
planes, RKD2Q9.py:1382-1393); IsCycle and checkpoints as above (a checkpoint keeps the streamed populations and the last force).

One process per GPU: when torch.distributed is initialised with world size > 1 the lattice is cut
into z-slabs (openlbmpm_amd/rk3d.py: RK3DDistributed, halos over xGMI) and rank 0 writes ONE result file with the
whole lattice's arrays, gathered at the record cadence (gather_records = False: every rank its own planes in its own file);
otherwise a single slab on `device`.

integrals_every = N > 0: every N steps (step 0 and the last step included) the plane integrals of the recorded state
(openlbmpm_amd/integrals.py; reduced on the device, a few kB per call) go to /Integrals/PlanesAtStep<step> [nz][12] of the result file
(rank 0's in a distributed run: the whole lattice's table), /Integrals/Steps and /Integrals/Columns (the names as zero-padded bytes,
integrals.column_names reads them) at the end; saturation, masses and the largest speed go to the log, and cells that are not finite are
met with the nan_guard rule at that cadence.

clusters_every = N > 0: at the same kind of cadence the connected clusters of each phase, labelled on the device (openlbmpm_amd/clusters.py;
clusters_connectivity 6 or 18): /Clusters/TableAtStep<step> [n][5] int64 (label, class, cells, zmin, zmax; the whole lattice's, joined on
rank 0 in a distributed run), /Clusters/Steps and /Clusters/Columns at the end; counts, the largest cluster, percolation and the trapped
cells of each phase go to the log.  clusters_props = True (only meaningful with clusters_every): the property table beside it, reduced on
the device too: /Clusters/PropsAtStep<step> [n][14] int64 (label, class, cells, then faces towards the other phase and the solid, pairs,
squares, cubes, the plane sum, mass and momentum in fixed point, clipped cells) and /Clusters/PropColumns; the ganglia of each phase and
the mobile ones among them join the log line.

morphology_every = N > 0: at the same kind of cadence the phase morphology, counted on the device (openlbmpm_amd/morphology.py;
morphology_phi_cut: the band around phi = 0 that belongs to neither phase): /Morphology/PlanesAtStep<step> [nz][28] (cells, density
sums, class pairs, squares and cubes per plane; the whole lattice's table on rank 0 in a distributed run), /Morphology/Steps and
/Morphology/Columns at the end; the interfacial area, the wetted fraction, the Euler characteristics and the capillary pressure go to
the log.

steady_every = N > 0: the steady-state monitor (openlbmpm_amd/change.py; reduced on the device against a snapshot kept there, 32 bytes per
lattice cell).  At every multiple of N the run reaches (step 0, the first one after a restart_from and the last step, where it is one,
included; only multiples: rows over unequal intervals would not be comparable) the first visit marks and every later one takes the
change since the visit before and marks again: /Steady/PlanesAtStep<step> [nz][11] (rank 0's in a distributed run: the whole lattice's
table), and at the end /Steady/Steps (the steps with a table, not the marking one), /Steady/Columns, /Steady/Criteria [rows][8] (step,
steps_between, velocity_change, velocity_change_R, velocity_change_B, phase_change, flipped, max_du) and /Steady/CriteriaColumns; the
summary goes to the log.  steady_tol > 0 (needs steady_every): the run ends at the first visit where Change.is_steady(steady_tol,
steady_phase_tol) holds -- its last record, tables and sync are taken at that step, which self.steady_step then names (None: never met;
distributed: rank 0 decides and every rank hears of it before the next step is issued).  A checkpoint does not hold the snapshot.

contact_angle_solids = array or path of a .npy file (also [SurfaceTension] ContactAngleFile = '...' of the ini, --contact-angles FILE of the
command line; 3-D CSF only, ConfigError on the perturbation model, whose wetting is SolidRhoR / SolidRhoB): mixed wettability.  Contact
angles in degrees per SOLID voxel, in the shape of the lattice -- with a voxel file ([ImageSetup], framed by geometry.voxel_domain) in the
shape of that file, framed the same way.  Solids it does not cover -- NaN entries, the forced side walls, the buffer planes -- take the
ini's ContactAngle.  geometry.wall_contact_angles turns it into the angle of every fluid cell next to solid (Cassie average over the
cell's solid neighbours), set_contact_angles hands that to the solver (under torchrun every rank cuts its planes), and the result file
gets /Wettability/ContactAngle once: the angles in force, get("theta") of the whole lattice (rank 0 writes).  A checkpoint does not hold
the map: restart_from= applies it again from the same argument.

body_force = (gx, gy, gz) for both colours | dict(red=(gx, gy, gz), blue=(gx, gy, gz)) (also [BodyForce] isBodyForce = 'yes' with
bodyForceX / Y / Z and the optional bodyForce{X,Y,Z}R / ...B of the ini, --body-force GX GY GZ [--body-force-blue GX GY GZ] of the command
line; 3-D CSF only, ConfigError on the perturbation model, whose solver has no force term): an acceleration per colour in lattice units --
gravity, or the drive of a force-driven flow, between open planes at equal pressure or with periodic z (set_body_force; the model:
include/lbmpm.h).  The
result file gets /BodyForce/Acceleration [2][3] once: red, blue as the solver holds them.  A checkpoint does not hold the force:
restart_from= applies it again from the same argument.

[BoundaryCondition] BoundaryTypeInlet = 'Periodic' with BoundaryTypeOutlet = 'Periodic' (3-D CSF only; one without the other and the
perturbation model are a ConfigError): periodic z -- no inlet, no outlet, every plane wraps like x and y, so a body force is the only
drive and the saturation is conserved (the relative-permeability set-up; README).  The mask is taken as given: duct() keeps its four side
walls, a voxel file gets its side walls and NO buffer planes (num_buffering_layers is not applied), the planes at the ends need not
repeat.  NeumannType, velocityZ*, density* are not used.  The result file gets /BoundaryCondition/PeriodicZ = 1; IsCycle, checkpoints
and restart_from= work unchanged.  clusters_every / morphology_every tables by default do not wrap z: plane nz-1 and plane 0 are ends of
the lattice to them, a ganglion across the seam is two rows, and what Clusters defines through open planes (percolation, trapped cells)
has no meaning.

analyses_wrap_z = True (--wrap-z of the command line; periodic z only, ConfigError otherwise): the clusters and morphology tasks close
the seam (wrap_z=True of clusters() / morphology(); openlbmpm_amd/clusters.py: close_seam).  A cluster across the seam is one row whose
zmax exceeds nz-1 (its planes zmin .. zmax counted on without a break, 0 <= zmin < nz; sum_z of the property table likewise), every row
has a winding in /Clusters/WindingAtStep<step> [n] int64 -- 0: a ganglion; w > 0: the cluster is connected to its own image w periods
further along z, it conducts round the ring and has zmin = 0, zmax = nz-1 -- and the logged percolation, trapped cells and ganglia are
defined through the winding (with winding_R / winding_B, the largest of each phase).  The morphology table counts what reaches from plane
nz-1 up into plane 0.  /Clusters/WrapZ = 1 and /Morphology/WrapZ = 1 mark the groups; without the flag neither they nor a Winding dataset
exist and the file is what it was.  Windings along x and y are not computed.
"""
import os

import numpy as np

from . import config
from .change import CRITERIA_COLUMNS, column_bytes as change_column_bytes, criteria_column_bytes
from .clusters import column_bytes as cluster_column_bytes, prop_column_bytes
from .geometry import initial_densities_rk3d, voxel_domain, wall_contact_angles
from .integrals import column_bytes, fresh
from .morphology import column_bytes as morphology_column_bytes
from .results import RecordGuard, ResultFile, find_result_file, read_planes
from .rk3d import RK3DSlab, RK3DDistributed
from . import runloop
from .runloop import PeriodicTask

PARAM_KEYS = ("AkR", "AkB", "beta", "tauR", "tauB", "SolidRhoR", "SolidRhoB", "velocityZR", "velocityZB",
              "densityRL", "densityBL", "relax", "inlet", "densityRH", "densityBH", "outlet")
GROUPS = (("FluidMacro", "MacroData"), ("FluidPDF", "MicroData"), ("FluidVelocity", "MacroVelocity"))
ANALYSES =("integrals", "clusters", "morphology", "mark_change", "change")


class _SolverHandle:
    """What a driver's run talks to, whichever solver the ini chose:
      step(n), observe() (refreshes what a record or an analysis reads; nothing for CSF), the calls of ANALYSES,
      slab   the calls of a slab of the perturbation model: set_density / set_macro / set_pdf, get, get_pdf, get_state / set_state, sync
      sim    what the driver keeps as self.solver after the run;  solver: the CSF solver (contact angles, body force)
      rank, z0 / nzl (this rank's planes), gather (a rank's planes -> the whole lattice's on the writing rank, None on the others),
      suffix of the result file's name, whole_arrays (set_* take the undivided arrays and cut this rank's planes out themselves)"""
    whole_arrays = False

    def _place(self, s, nz, distributed, gather_records):
        self.rank, self.z0, self.nzl, self.gather, self.suffix = 0, 0, nz, (lambda a: a), ""
        if distributed:
            import torch.distributed as dist
            self.rank, self.z0, self.nzl = dist.get_rank(), s.z0, s.nzl
            if gather_records:
                self.gather = s.gather
            else:
                self.suffix = "_rank%d" % self.rank          # every rank its own planes in its own file


class _PerturbationSlab(_SolverHandle):
    """RK3DSlab, or RK3DDistributed (one slab per rank), behind the handle's calls"""

    def __init__(self, sim, nz, gather_records=True):
        many = isinstance(sim, RK3DDistributed)
        self.sim, self.slab, self.close = sim, (sim.slab if many else sim), sim.close
        self._place(sim, nz, many, gather_records)
        if many:
            self.step, self.observe = sim.step, sim.observe
            checked = lambda call: call
        else:
            # a single slab's diagnostics are stale after a step: an analysis that finds them so observes and asks again
            observe = lambda: sim.phase_field(diagnostics=True)
            self.step, self.observe = sim.step_single, observe
            checked = lambda call: (lambda *a, **kw: fresh(lambda: call(*a, **kw), observe))
        for name in ANALYSES:
            setattr(self, name, checked(getattr(sim, name)))


class _CSFSlab(_SolverHandle):
    """RK3DCSFSolver (under torchrun RK3DCSFDistributed, one slab per rank) behind the handle's calls; it is its own `slab` and `sim`"""

    def __init__(self, dom, par, device, bulk_epsilon=0.0, distributed=False, transport=None, tracers=None, gather_records=True):
        from .rk3dcsf import RK3DCSFSolver, RK3DCSFDistributed
        q = dict(sigma=par["sigma"], theta=par["theta"], wetting=par["wetting"], beta=par["beta"], delta=par["delta"], tauR=par["tauR"], tauB=par["tauB"],
                 tautype=par["tautype"], relax=par["relax"], inlet=par["inlet"], outlet=par["outlet"], velocityZR=par["velocityZR"],
                 velocityZB=par["velocityZB"], densityBH=par["densityBH"], densityRH=par["densityRH"], densityBL=par["densityBL"], densityRL=par["densityRL"],
                 bulk_epsilon=float(bulk_epsilon))
        # distributed: one slab per rank; set_* take the undivided arrays (a slab cuts its planes and the images of its neighbours' out of
        # them), get* return the rank's own planes
        # tracers (Transport3DRK): the keyword arguments of RK3DCSFSolver.configure_tracers, given at construction -- on slabs they are
        # part of the population message, which is sized before the transport connects
        more = {} if tracers is None else dict(tracers=tracers)
        self.solver = RK3DCSFDistributed(dom, q, device=device, transport=transport, **more) if distributed else RK3DCSFSolver(dom, q, device=device, **more)
        self.step = self.step_single = self.solver.step
        self.sync, self.close = self.solver.sync, self.solver.close
        self.base_steps = 0          # the steps a restored checkpoint had behind it (set_pdf starts the solver's own counter again)
        self.whole_arrays = bool(distributed)        # the slabs carry images of their neighbours' planes and cut them out of the undivided arrays
        self._place(self.solver, np.shape(dom)[0], distributed, gather_records)
        for name in ANALYSES:                        # (never stale: the CSF loop keeps what they read)
            setattr(self, name, getattr(self.solver, name))

    slab = sim = property(lambda self: self)

    def observe(self):
        pass

    num_fluid_nodes = property(lambda self: self.solver.num_fluid_nodes)
    dominant_kernel = property(lambda self: self.solver.dominant_kernel)

    def set_density(self, rR, rB):
        self.solver.set_macro(rR, rB)

    def set_macro(self, rR, rB, vx, vy, vz):
        self.solver.set_macro(rR, rB, vx, vy, vz)

    def set_pdf(self, fR, fB, post_collision=True):
        self.solver.set_pdf(fR, fB)          # the recorded arrays are the loop's arrays at its top: streamed populations

    def get(self, name):
        return self.solver.get("rec_" + name)

    def get_pdf(self):
        return self.solver.get("rec_fR"), self.solver.get("rec_fB")

    def get_state(self):
        s = self.solver
        st = np.concatenate([s.get("fR"), s.get("fB")] + [s.get(c)[..., None] for c in ("Fx", "Fy", "Fz")], axis=-1)
        return st, dict(doubles_per_cell=41, steps=self.base_steps + s.steps_done, post_collision=False)

    def set_state(self, st, steps, post_collision):
        st = np.asarray(st)
        if st.shape[-1] != 41:
            raise config.ConfigError("restart_from: this checkpoint is not one of the 3-D CSF model (41 doubles per cell: f_R, f_B, F)")
        self.solver.set_pdf(st[..., :19], st[..., 19:38], force=tuple(np.ascontiguousarray(st[..., 38 + a]) for a in range(3)))
        self.base_steps = int(steps)


def duct(nx, ny, nz):
    """[nz][ny][nx] mask: solid walls on the four sides, open inlet / outlet planes in z"""
    dom = np.ones((nz, ny, nx), dtype=np.uint8)
    dom[:, 0, :] = dom[:, -1, :] = 0
    dom[:, :, 0] = dom[:, :, -1] = 0
    return dom


class RKColorGradient3D:
    def __init__(self, pathIniFile, output_dir=None, domain=None, device=0, record_every=None, num_buffering_layers=10,
                 structure_path=None, initial_dir=None, record_pdf=False, restart_from=None, checkpoint_every=0, csf_bulk_epsilon=0.0,
                 csf_transport=None, integrals_every=0, clusters_every=0, clusters_connectivity=6, morphology_every=0,
                 morphology_phi_cut=0.0, clusters_props=False, steady_every=0, steady_tol=0.0, steady_phase_tol=None, contact_angle_solids=None,
                 body_force=None, analyses_wrap_z=False):
        self.pathIni = pathIniFile
        self.par = config.read_rk3d(pathIniFile)
        # periodic z (3-D CSF only; BoundaryTypeInlet = BoundaryTypeOutlet = 'Periodic'): no open planes -- the mask is taken as given
        self.periodic_z = bool(self.par.get("periodic_z"))
        # an acceleration per colour (3-D CSF only): (gx, gy, gz) for both, or dict(red=, blue=); None: the ini's [BodyForce], if any
        self.body_force = self._body_force_arg(body_force if body_force is not None else self.par.get("body_force"))
        if self.body_force is not None and self.par["tension_type"] != "CSF":
            raise config.ConfigError("body_force belongs to SurfaceTensionType = 'CSF': the perturbation model's solver has no force term")
        # mixed wettability (3-D CSF only): contact angles per solid voxel, an array or the path of a .npy file; None: the ini's ContactAngleFile, if any
        self.contact_angle_solids = contact_angle_solids if contact_angle_solids is not None else self.par.get("contact_angle_file")
        if self.contact_angle_solids is not None and self.par["tension_type"] != "CSF":
            raise config.ConfigError("contact_angle_solids belongs to SurfaceTensionType = 'CSF': the perturbation model's wetting is SolidRhoR / SolidRhoB")
        self.output_dir = output_dir or os.path.expanduser("~/LBMResults3D")       # main.py:28
        self.initial_dir = initial_dir or os.path.expanduser("~/LBMInitial")       # RKD2Q9.py:492
        self.device, self._domain, self.nbuf = device, domain, int(num_buffering_layers)
        self.structure_path = structure_path
        self.timeSteps = self.par["steps"]
        self.timeInterval = record_every or self.par["interval"] or max(1, self.timeSteps // 10)
        self.record_pdf = bool(record_pdf)          # /FluidPDF/FluidPDFRat<k>, ...Bat<k> [nz][ny][nx][19] with every record (38 doubles per cell)
        self.restart_from, self.checkpoint_every = restart_from, int(checkpoint_every)
        self.csf_bulk_epsilon = float(csf_bulk_epsilon)      # 3-D CSF only, opt-in (include/lbmpm.h: lbmpm_rk3dcsf_config.bulk_epsilon; 0 = exact)
        # 3-D CSF under torchrun only, opt-in: None = the face messages through torch.distributed; 'auto' | 'ipc' | 'rccl' = over a transport
        # inside the library, one C call per run of steps (rk3dcsf.RK3DCSFDistributed)
        self.csf_transport = csf_transport
        self.integrals_every = int(integrals_every)      # 0: no /Integrals group, no extra stop of the step loop
        # 0: no /Clusters group, no extra stop of the step loop; connectivity 6 (faces) or 18 (the D3Q19 links)
        self.clusters_every, self.clusters_connectivity = int(clusters_every), int(clusters_connectivity)
        self.clusters_props = bool(clusters_props)       # with clusters_every: the property table beside every cluster table
        # 0: no /Morphology group, no extra stop of the step loop
        self.morphology_every, self.morphology_phi_cut = int(morphology_every), float(morphology_phi_cut)
        # 0: no /Steady group, no extra stop of the step loop, nothing kept on the device; steady_tol 0: monitor only
        self.steady_every, self.steady_tol = int(steady_every), float(steady_tol)
        self.steady_phase_tol = None if steady_phase_tol is None else float(steady_phase_tol)
        if self.steady_tol > 0 and self.steady_every <= 0:
            raise config.ConfigError("steady_tol = %g needs steady_every > 0: the cadence at which the criterion is looked at" % self.steady_tol)
        self.steady_step = None         # the step at which the criterion was met
        # periodic z only, opt-in: the clusters and morphology tasks close the seam between plane nz-1 and plane 0 (wrap_z=True)
        self.analyses_wrap_z = bool(analyses_wrap_z)
        if self.analyses_wrap_z and not self.periodic_z:
            raise config.ConfigError("analyses_wrap_z closes the seam of a run that is periodic in z: BoundaryTypeInlet = BoundaryTypeOutlet = 'Periodic'")
        self.gather_records = True
        self.records = 0
        self.physicalVX = self.physicalVY = self.physicalVZ = None
        self.fluidPDFR = self.fluidPDFB = None

    def initializeDomainBorder(self):
        p = self.par
        if self._domain is not None:
            self.isDomain = np.ascontiguousarray(self._domain, dtype=np.uint8)
            if self.isDomain.ndim != 3:
                raise TypeError("domain must be a [nz][ny][nx] array")
        elif p["image"]:
            # the reference ships no 3-D image reader; a NumPy voxel file next to where its 2-D drivers look
            # for structure.png (non-zero = pore), framed like the 2-D images are
            path = self.structure_path or os.path.expanduser("~/StructureImage/structure3D.npy")
            if not os.path.isfile(path):
                raise config.ConfigError("[ImageSetup] Existance = 'yes': voxel file %s not found (or pass `domain=`)" % path)
            self._voxels = np.load(path)
            self.isDomain = voxel_domain(self._voxels, self._image_buffer)
        else:
            self.isDomain = duct(p["nx"], p["ny"], p["nz"])
        self.zDomain, self.yDomain, self.xDomain = self.isDomain.shape
        self.voidSpace = int(np.count_nonzero(self.isDomain))

    @property
    def _is_image(self):
        return self._domain is not None or self.par["image"]

    @property
    def _image_buffer(self):
        """the all-fluid planes a voxel file gets below and above: num_buffering_layers between open planes, none with periodic z
        (the sample is its own neighbour there; the side walls stay, as duct() keeps its four)"""
        return 0 if self.periodic_z else self.nbuf

    def solid_contact_angles(self):
        """contact_angle_solids on the lattice [nz][ny][nx] (NaN: the ini's ContactAngle), or None; after initializeDomainBorder"""
        a = self.contact_angle_solids
        if a is None:
            return None
        if isinstance(a, (str, os.PathLike)):
            if not os.path.isfile(a):
                raise config.ConfigError("contact angles: file %s not found" % a)
            a = np.load(a)
        a = np.array(a, dtype=np.float64)
        voxels = getattr(self, "_voxels", None) if self._domain is None else None
        if voxels is not None:
            # framed like the voxel file (geometry.voxel_domain): buffer planes below and above; what the file calls pore is not covered --
            # the side walls forced solid there take the ini's angle
            if a.shape != np.shape(voxels):
                raise config.ConfigError("contact angles have shape %s, the voxel file %s" % (a.shape, np.shape(voxels)))
            a[np.asarray(voxels) != 0] = np.nan
            buf = np.full((self._image_buffer,) + a.shape[1:], np.nan)
            a = np.concatenate([buf, a, buf], axis=0)
        if a.shape != self.isDomain.shape:
            raise config.ConfigError("contact angles have shape %s, the lattice %s" % (a.shape, self.isDomain.shape))
        return a

    @staticmethod
    def _body_force_arg(bf):
        """body_force= as the keyword arguments of set_body_force, or None"""
        if bf is None:
            return None
        kw = dict(bf) if isinstance(bf, dict) else dict(g=bf)
        if set(kw) - {"g", "red", "blue"}:
            raise config.ConfigError("body_force = (gx, gy, gz) or dict(red=(gx, gy, gz), blue=(gx, gy, gz)), not %r" % (bf,))
        try:
            from .rk3dcsf import body_force_pair
            body_force_pair(kw.get("g"), kw.get("red"), kw.get("blue"))
        except (ValueError, TypeError) as e:
            raise config.ConfigError("body_force: %s" % e)
        return kw

    def _apply_body_force(self, solver, out):
        """body_force into the solver (every rank makes the same call) and the accelerations in force into /BodyForce/Acceleration"""
        kw = dict(self.body_force)
        solver.set_body_force(kw.pop("g", None), **kw)
        if out is not None:
            out.write("BodyForce", "Acceleration", np.array(solver.body_force, dtype=np.float64))

    def _apply_contact_angles(self, solver, out):
        """the wall angles of contact_angle_solids into the solver (the undivided array: a distributed solver cuts its planes), and the
        angles in force into /Wettability/ContactAngle (collective: rank 0, or everyone ungathered, writes)"""
        solids = self.solid_contact_angles()
        if solids is None:
            return
        try:
            self.wallContactAngle = wall_contact_angles(self.isDomain, solids, self.par["theta"])
        except ValueError as e:
            raise config.ConfigError("contact angles: %s" % e)
        solver.set_contact_angles(self.wallContactAngle)
        a = self._gather(solver.get("theta"))
        if out is not None and a is not None:
            out.write("Wettability", "ContactAngle", a)

    def initializeDomainCondition(self, z0=0, nzl=None):
        """initial fields of the planes [z0, z0 + nzl) (a rank's slab; default: the whole lattice)"""
        p = self.par
        nzl = self.zDomain if nzl is None else nzl
        if p["cycle"]:
            self._initial_state_from_files(z0, nzl)
            return
        rR, rB = initial_densities_rk3d(self.isDomain, min(self.nbuf, self.zDomain // 4), p["rho0R"], p["rho0B"])
        self.fluidsRhoR, self.fluidsRhoB = rR[z0:z0 + nzl], rB[z0:z0 + nzl]

    def _initial_state_from_files(self, z0, nzl):
        """[CyclesSetup] IsCycle = 'yes': RKD2Q9.py:491-559 with planes in the place of rows"""
        p = self.par
        dom = self.isDomain[z0:z0 + nzl]

        def find(stem):
            f = find_result_file(self.initial_dir, stem)
            if f is None:
                raise config.ConfigError("IsCycle = 'yes': no %s.h5/.npz in %s" % (stem, self.initial_dir))
            return f

        def need(path, key, tail=()):
            try:
                a = np.array(read_planes(path, key, z0, nzl), dtype=np.float64)
            except KeyError:
                raise config.ConfigError("IsCycle = 'yes': dataset %s missing in %s" % (key, path))
            if a.shape != dom.shape + tuple(tail):
                raise config.ConfigError("IsCycle = 'yes': %s has shape %s, the planes %d..%d of the domain are %s" % (key, a.shape, z0, z0 + nzl - 1, dom.shape + tuple(tail)))
            return a

        zz = np.arange(z0, z0 + nzl)
        if not self._is_image:
            # last record of the previous run; the top 20 planes refilled with blue; f = f_eq(rho, u) (:492-508)
            path, k = find("SimulationResultsRK3D"), p["last_step"]
            self.fluidsRhoR = need(path, "/FluidMacro/FluidDensityRin%d" % k)
            self.fluidsRhoB = need(path, "/FluidMacro/FluidDensityBin%d" % k)
            self.physicalVX, self.physicalVY, self.physicalVZ = (need(path, "/FluidVelocity/FluidVelocity%sAt%d" % (ax, k)) for ax in "XYZ")
            top = zz >= self.zDomain - 20
            self.fluidsRhoR[top] = 0.0
            self.fluidsRhoB[top] = p["rho0B"]
            for a in (self.fluidsRhoR, self.fluidsRhoB, self.physicalVX, self.physicalVY, self.physicalVZ):
                a[dom != 1] = 0.0
        else:
            # cycleInitialRK3D: populations taken over, colours swapped in the top buffer planes (:532-556)
            path = find("cycleInitialRK3D")
            rR, rB = need(path, "/FluidMacro/FluidDensityR"), need(path, "/FluidMacro/FluidDensityB")
            fR, fB = need(path, "/FluidPDF/FluidPDFR", (19,)), need(path, "/FluidPDF/FluidPDFB", (19,))
            top = zz >= self.zDomain - self.nbuf
            self.fluidsRhoR, self.fluidsRhoB = np.where(top[:, None, None], rB, rR), np.where(top[:, None, None], rR, rB)
            self.fluidPDFR, self.fluidPDFB = np.where(top[:, None, None, None], fB, fR), np.where(top[:, None, None, None], fR, fB)
            self.physicalVX, self.physicalVY, self.physicalVZ = (need(path, "/FluidVelocity/FluidVelocity%s" % ax) for ax in "XYZ")

    def _upload_initial_state(self, slab):
        if self.fluidPDFR is not None:
            slab.set_pdf(self.fluidPDFR, self.fluidPDFB, post_collision=True)       # what the reference's arrays hold when recorded
        elif self.physicalVX is not None:
            slab.set_macro(self.fluidsRhoR, self.fluidsRhoB, self.physicalVX, self.physicalVY, self.physicalVZ)
        else:
            slab.set_density(self.fluidsRhoR, self.fluidsRhoB)

    def _distributed(self):
        try:
            import torch.distributed as dist
            return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        except ImportError:
            return False

    # ---- exact checkpoints (lbmpm_rk3d_get_state / set_state)
    def _load_checkpoint(self, slab, z0, nzl):
        path = self.restart_from
        info = [int(v) for v in read_planes(path, "/Checkpoint/Info")]
        S, steps, post, nz, ny, nx, records = info[:7]
        if (nz, ny, nx) != self.isDomain.shape:
            raise config.ConfigError("restart_from: the checkpoint holds a %s lattice, the domain is %s" % ((nz, ny, nx), self.isDomain.shape))
        slab.set_state(read_planes(path, "/Checkpoint/State", z0, nzl), steps, bool(post))
        return steps, records

    def checkpoint(self, path=None):
        """the solver's stored state + step and record counters -> <output_dir>/CheckpointRK3D (collective in a distributed run: rank 0
        writes the stacked state).  restart_from=<that file> continues bit for bit."""
        slab = self._slab
        st, info = slab.get_state()
        st = self._gather(st)
        if st is None:
            return None
        directory, name = (os.path.dirname(path), os.path.splitext(os.path.basename(path))[0]) if path else (self.output_dir, "CheckpointRK3D")
        out = ResultFile(directory, name, (("Checkpoint", "ExactState"),))
        out.write("Checkpoint", "State", st)
        out.write("Checkpoint", "Info", np.array([info["doubles_per_cell"], info["steps"], int(info["post_collision"]), self.zDomain, self.yDomain,
                                                    self.xDomain, self.records], dtype=np.int64))
        return out.path

    def write_cycle_initial(self, directory=None):
        """the current state as <directory>/cycleInitialRK3D (the file the image branch of IsCycle = 'yes' starts from)"""
        slab = self._slab
        self._observe()
        fields = dict(R=slab.get("rhoR"), B=slab.get("rhoB"), X=slab.get("vx"), Y=slab.get("vy"), Z=slab.get("vz"))
        fR, fB = slab.get_pdf()
        got = {k: self._gather(a) for k, a in dict(fields, PR=fR, PB=fB).items()}
        if got["R"] is None:
            return None
        out = ResultFile(directory or self.initial_dir, "cycleInitialRK3D", GROUPS)
        out.write("FluidMacro", "FluidDensityR", got["R"]); out.write("FluidMacro", "FluidDensityB", got["B"])
        out.write("FluidPDF", "FluidPDFR", got["PR"]); out.write("FluidPDF", "FluidPDFB", got["PB"])
        for ax in "XYZ":
            out.write("FluidVelocity", "FluidVelocity" + ax, got[ax])
        return out.path

    # ---- the pieces of a run (Transport3DRK runs on the same ones)
    def _open_solver(self):
        """the handle of the solver the ini chooses, on this process's share of the lattice"""
        p = self.par
        if p["tension_type"] == "CSF":
            return _CSFSlab(self.isDomain, p, self.device, self.csf_bulk_epsilon, distributed=self._distributed(), transport=self.csf_transport,
                            gather_records=self.gather_records)
        par = {k: p[k] for k in PARAM_KEYS}
        if not self._distributed():
            return _PerturbationSlab(RK3DSlab(self.isDomain, 0, self.zDomain, par, self.device), self.zDomain)
        sim = RK3DDistributed(self.isDomain, par, device=self.device)
        if getattr(self, "calibrate_partition", self.timeSteps >= 1000):
            # long runs: one measured re-cut of the slabs (rk3d.RK3DDistributed.calibrated_plane_cost) from the plain initial
            # state -- the rank that holds the colour interface otherwise runs ~10 % behind the others
            rR, rB = initial_densities_rk3d(self.isDomain, min(self.nbuf, self.zDomain // 4), p["rho0R"], p["rho0B"])
            sim.set_density(rR, rB)
            cost = sim.calibrated_plane_cost(8)
            sim.close()
            sim = RK3DDistributed(self.isDomain, par, device=self.device, plane_cost=cost)
        return _PerturbationSlab(sim, self.zDomain, self.gather_records)

    def _start(self, h):
        """the handle becomes this run's solver and takes the initial state or the checkpoint's; -> the steps behind it"""
        self._slab, self._observe, self._gather, self.z0, self.nzl = h.slab, h.observe, h.gather, h.z0, h.nzl
        z0, nzl = (0, self.zDomain) if h.whole_arrays else (h.z0, h.nzl)
        if self.restart_from:
            done, self.records = self._load_checkpoint(h.slab, z0, nzl)
            return done
        self.initializeDomainCondition(z0, nzl)
        self._upload_initial_state(h.slab)
        return 0

    def _integrals_task(self, h, **kw):
        def report(step, t):
            self._guard.integrals(step, None if t is None else t.nonfinite, None if t is None else t.summary())
        return PeriodicTask(self, self.integrals_every, ("Integrals", "PlaneIntegrals"), h.rank == 0, h.integrals, "integrals", "integral_steps",
                            report=report, closing=lambda: [("Columns", column_bytes())], **kw)

    def _tasks(self, h):
        """The periodic analyses of a run, in the order a stop visits them: the one place that names them.  Another analysis is a
        constructor argument for its cadence and an entry here.  (Their tables are gathered: the whole lattice's on rank 0, whether the
        records are gathered or not.)"""
        def log(name):
            def report(step, t):
                if t is not None:
                    self._guard.log.info("rk3d %s step %d: %s", name, step, " ".join("%s=%s" % kv for kv in t.summary().items()))
            return report

        def steady(step, t):
            """true when the criterion is met -- rank 0's verdict, which every rank hears of here (one all-reduce of a flag) before
            anybody issues the next step"""
            met = False
            if t is not None:
                self.steady_criteria.append(t.criteria(step))
                log("steady")(step, t)
                met = self.steady_tol > 0 and t.is_steady(self.steady_tol, self.steady_phase_tol)
            if self.steady_tol > 0 and self._guard.anyone(met):
                if self.steady_step is None:
                    self.steady_step = int(step)
                return True
            return False
        self.steady_criteria, self.steady_step = [], None
        here, ckw = h.rank == 0, (dict(props=True) if self.clusters_props else {})
        wrap = dict(wrap_z=True) if self.analyses_wrap_z else {}          # (absent by default: the perturbation model's handle is called as ever)
        marked = lambda: [("WrapZ", np.array([1], dtype=np.int64))] if self.analyses_wrap_z else []
        return [
            self._integrals_task(h),
            PeriodicTask(self, self.clusters_every, ("Clusters", "PhaseClusters"), here, lambda: h.clusters(connectivity=self.clusters_connectivity, **ckw, **wrap),
                         "clusters", "cluster_steps", datasets=(("TableAtStep%d", "table"), ("PropsAtStep%d", "props"), ("WindingAtStep%d", "winding")),
                         report=log("clusters"),
                         closing=lambda: [("Columns", cluster_column_bytes())] + ([("PropColumns", prop_column_bytes())] if self.clusters_props else []) + marked()),
            PeriodicTask(self, self.morphology_every, ("Morphology", "PhaseMorphology"), here, lambda: h.morphology(self.morphology_phi_cut, **wrap),
                         "morphology", "morphology_steps", report=log("morphology"), closing=lambda: [("Columns", morphology_column_bytes())] + marked()),
            # the steady-state monitor: only multiples of its cadence, the first visit marks, its verdict ends the run before that step's record
            PeriodicTask(self, self.steady_every, ("Steady", "SteadyState"), here, h.change, "change", "steady_steps", report=steady, mark=h.mark_change,
                         before_record=True, only_multiples=True,
                         closing=lambda: [("Columns", change_column_bytes()),
                                          ("Criteria", np.array(self.steady_criteria, dtype=np.float64).reshape(-1, len(CRITERIA_COLUMNS))),
                                          ("CriteriaColumns", criteria_column_bytes())])]

    def _open_flow_file(self, h, tasks, writes):
        """SimulationResultsRK3D with the tasks' groups (None on a rank that writes none); contact angles and body force go into the solver
        (after a restart_from too: a checkpoint holds neither) and, once, into the file"""
        more = runloop.groups(tasks) + ((("Wettability", "ContactAngles"),) if self.contact_angle_solids is not None else ()) + \
            ((("BodyForce", "Acceleration"),) if self.body_force is not None else ()) + \
            ((("BoundaryCondition", "OpenPlanes"),) if self.periodic_z else ())
        out = ResultFile(self.output_dir, "SimulationResultsRK3D" + h.suffix, GROUPS + more) if writes else None
        runloop.attach(tasks, out)
        if self.periodic_z and out is not None:
            out.write("BoundaryCondition", "PeriodicZ", np.array([1], dtype=np.int64))     # (only a periodic run has the group)
        if self.contact_angle_solids is not None:
            self._apply_contact_angles(h.solver, out)
        if self.body_force is not None:
            self._apply_body_force(h.solver, out)
        self.result_path = out.path if out else None
        return out

    def _synced_checkpoint(self):
        self._slab.sync()
        self.checkpoint_path = self.checkpoint()

    def runRKColorGradient3D(self, progress=None):
        self.initializeDomainBorder()
        h = self._open_solver()
        done = self._start(h)
        tasks = self._tasks(h)
        out = self._open_flow_file(h, tasks, h.rank == 0 or not (self._distributed() and self.gather_records))
        # distributed: every rank checks its own slab, the verdict is collective (all ranks raise together, none is left in an exchange)
        self._guard = RecordGuard("rk3d", h.slab.num_fluid_nodes, getattr(self, "nan_guard", "raise"), collective=self._distributed(), device=self.device)

        def record(done, tail):
            h.observe()
            self._step_now = done
            self._record(h.slab, out)
            return done
        runloop.run(tasks, done, self.timeSteps, self.timeInterval, self.checkpoint_every, record, h.step, self._synced_checkpoint, progress)
        h.slab.sync()
        self.solver = h.sim
        return self.result_path

    def _record(self, slab, out):
        k = self.records
        self.fluidsRhoR, self.fluidsRhoB = slab.get("rhoR"), slab.get("rhoB")
        self.physicalVX, self.physicalVY, self.physicalVZ = slab.get("vx"), slab.get("vy"), slab.get("vz")
        guard = getattr(self, "_guard", None)
        if guard:
            guard(k, getattr(self, "_step_now", 0), dict(rhoR=self.fluidsRhoR, rhoB=self.fluidsRhoB, vx=self.physicalVX, vy=self.physicalVY, vz=self.physicalVZ),
                  dict(massR=float(self.fluidsRhoR.sum()), massB=float(self.fluidsRhoB.sum())))
        items = [("FluidMacro", "FluidDensityRin%g" % k, self.fluidsRhoR), ("FluidMacro", "FluidDensityBin%g" % k, self.fluidsRhoB)]
        items += [("FluidVelocity", "FluidVelocity%sAt%g" % (axis, k), a) for axis, a in (("X", self.physicalVX), ("Y", self.physicalVY), ("Z", self.physicalVZ))]
        if self.record_pdf:
            self.fluidPDFR, self.fluidPDFB = slab.get_pdf()
            items += [("FluidPDF", "FluidPDFBat%g" % k, self.fluidPDFB), ("FluidPDF", "FluidPDFRat%g" % k, self.fluidPDFR)]
        for group, name, a in items:
            a = self._gather(a)         # (collective: every rank passes through, rank 0 -- or everyone, ungathered -- writes)
            if out is not None and a is not None:
                out.write(group, name, a)
        self.records += 1
