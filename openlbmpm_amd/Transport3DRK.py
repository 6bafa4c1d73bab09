"""Tracers carried by the 3-D colour-gradient CSF flow: class Transport3DRK(pathIniFile).runTransport3DMPMCRK().

The reference couples tracers to its 2-D CSF loop only (RKCG2D/Transport2DRK.py; openlbmpm_amd/Transport2DRK.py is its counterpart
here).  This is the same coupling on the D3Q19 CSF flow of RKColorGradientD3Q19.py with D3Q7 tracers (include/lbmpm.h,
lbmpm_rk3dcsf_tracer_*): IniFiles/RKtwophasesetup3D.ini with [SurfaceTension] SurfaceTensionType = 'CSF' for the flow,
transportsetup.ini (config.read_transport3d: the 2-D file's keys plus the z entries) for the tracers.  One GPU, or one z-slab per rank
under torchrun like the flow's driver (rk3dcsf.RK3DCSFDistributed; csf_transport honoured): the tracers' populations that cross a cut
ride the flow's population message, rank 0 writes ONE SimulationResultsRK3D.h5 and ONE ConcentrationResults.h5 with the stacked planes,
the records' verdicts are collective, and a checkpoint (the undivided state, stacked on rank 0) restarts on any number of ranks.

Kept from the 2-D driver: the initial concentration rules with planes in the place of rows (tracer 0 = 1 below the top buffer planes
for generated geometries, every tracer = 1 in the 10 top planes for voxel geometries; or initial_concentration=[nT][nz][ny][nx]),
g_i = w_i C, one tracer sub-step inside every flow step after the wetting-corrected colour gradient, the record cadence, and
`/TransportMacro/TracerConcType<k>in<record>` of ConcentrationResults.h5 beside the flow's SimulationResultsRK3D.h5.  As there, a
record holds two views: the flow arrays at the START of step iStep, the concentrations AFTER the tracer update of that step; the
record the 3-D driver writes after the last step holds the concentrations as they stand.  The inlet concentrations are the file's.
checkpoint() / restart_from= carry the tracers' populations behind the flow's (41 + 7 per tracer doubles per cell): bit for bit.
contact_angle_solids= / [SurfaceTension] ContactAngleFile: mixed wettability exactly as in the flow's driver (RKColorGradientD3Q19.py),
/Wettability/ContactAngle in SimulationResultsRK3D.h5; a checkpoint does not hold the map, restart_from= applies it again.
body_force= / [BodyForce] isBodyForce = 'yes': an acceleration per colour exactly as in the flow's driver; the tracers are advected by the
velocity that holds half of it.  /BodyForce/Acceleration in SimulationResultsRK3D.h5; restart_from= applies it again.

integrals_every = N > 0: every N steps (step 0 and the last step included; the step loop's runs are cut there as at the record and
checkpoint cadences) two tables, both reduced on the device and the same bit for bit on any number of ranks: the flow's plane integrals
go to /Integrals/PlanesAtStep<step> [nz][12], /Integrals/Steps and /Integrals/Columns of SimulationResultsRK3D.h5 exactly as the flow's
driver writes them, the tracers' (integrals.TracerIntegrals: cells, mass, flux_x, flux_y, flux_z, sum_c2, cmin, cmax, nonfinite per plane
and tracer -- mass balances, the breakthrough -flux_z at the outlet, the plume's moments along z) to /TracerIntegrals/PlanesAtStep<step>
[nz][nT][9], /TracerIntegrals/Steps and /TracerIntegrals/Columns of ConcentrationResults.h5.  Both counts of non-finite cells meet the
nan_guard rule at that cadence (collective under torchrun; rank 0 writes), masses and extrema go to the log.  N = 0 writes no group and
adds no stop; the records and checkpoints of a run do not depend on N.  The flow driver's other cadences (clusters_every,
morphology_every, steady_every, and analyses_wrap_z with them) are accepted by the constructor and not acted on: this driver runs the two
integrals tasks only.

wall_reaction= / [Reaction] WallReactionRate: the tracers' first-order reaction at solid walls (RK3DCSFSolver.set_wall_reaction;
include/lbmpm.h) -- rates k >= 0 in lattice units, a number, one per tracer, or [classes][nT] with wall_minerals= / [Reaction]
WallMineralFile, the class byte of every solid voxel (an array or a .npy in the lattice's shape, or the voxel file's).  Independent of
[SystemType] Reaction.  ConcentrationResults.h5 gets /WallReaction/Rates [classes][nT] once, and with integrals_every the uptake table
(integrals.TracerWallIntegrals: wall_links, uptake, wall_c, nonfinite per plane and tracer) as /TracerWallIntegrals/PlanesAtStep<step>
[nz][nT][4], /Steps and /Columns, one more task at the tracers' cadence.  A checkpoint does not hold the rates: restart_from= applies
them again.  Without the option the files are what they were.
"""
import numpy as np

from . import config, runloop
from .RKColorGradientD3Q19 import RKColorGradient3D, _CSFSlab
from .integrals import tracer_column_bytes, tracer_wall_column_bytes
from .results import RecordGuard, ResultFile
from .runloop import PeriodicTask


class _CSFTracerSlab(_CSFSlab):
    def __init__(self, dom, par, t, device, bulk_epsilon=0.0, distributed=False, transport=None):
        n = t["num_tracers"]
        self.num_tracers = n
        tracers = dict(num_tracers=n, diffusion_x=tuple(t["diffX"]), diffusion_y=tuple(t["diffY"]), diffusion_z=tuple(t["diffZ"]),
                       diffusion_xy=t["dXY"], diffusion_yx=t["dYX"], diffusion_xz=t["dXZ"], diffusion_zx=t["dZX"],
                       diffusion_yz=t["dYZ"], diffusion_zy=t["dZY"], beta_interface=t["beta"], criteria_rho=0.5,
                       inlet_concentration=tuple(t["inlet_conc"]), dirichlet_inlet=t["inlet_type"] == "Dirichlet",
                       free_outlet=t["outlet_type"] == "Freeflow", reaction_rate=t["reaction_rate"], diffusion_j=tuple(t["diffJ3"]))
        _CSFSlab.__init__(self, dom, par, device, bulk_epsilon, distributed=distributed, transport=transport, tracers=tracers)
        self.tracer_integrals = self.solver.tracer_integrals
        self.tracer_wall_integrals = self.solver.tracer_wall_integrals

    def get_state(self):
        st, info = _CSFSlab.get_state(self)
        st = np.concatenate([st] + [self.solver.get_tracer_pdf(k) for k in range(self.num_tracers)], axis=-1)
        return st, dict(info, doubles_per_cell=st.shape[-1])

    def set_state(self, st, steps, post_collision):
        st = np.asarray(st)
        if st.shape[-1] != 41 + 7 * self.num_tracers:
            raise config.ConfigError("restart_from: this checkpoint holds %d doubles per cell, the 3-D CSF model with %d tracers keeps %d (f_R, f_B, F, g)"
                                     % (st.shape[-1], self.num_tracers, 41 + 7 * self.num_tracers))
        _CSFSlab.set_state(self, st[..., :41], steps, post_collision)
        for k in range(self.num_tracers):
            self.solver.set_tracer_pdf(k, np.ascontiguousarray(st[..., 41 + 7 * k:48 + 7 * k]))


class Transport3DRK(RKColorGradient3D):
    def __init__(self, pathIniFile, initial_concentration=None, wall_reaction=None, wall_minerals=None, **kw):
        RKColorGradient3D.__init__(self, pathIniFile, **kw)
        self.tr = config.read_transport3d(pathIniFile, periodic_z=self.periodic_z)      # (periodic z: no Dirichlet inlet, no Freeflow outlet)
        self.numTracers = self.tr["num_tracers"]
        self._initial_concentration = initial_concentration
        # the reaction at solid walls: rates [classes][nT] (a number, [nT] or [classes][nT]) and the solid voxels' classes, an array or the
        # path of a .npy file; None: the ini's [Reaction] WallReactionRate / WallMineralFile, if any
        self.wall_reaction = self._wall_reaction_arg(wall_reaction) if wall_reaction is not None else self.tr["wall_reaction"]
        self.wall_minerals = wall_minerals if wall_minerals is not None else (self.tr["wall_mineral_file"] if wall_reaction is None else None)
        if self.wall_minerals is not None and self.wall_reaction is None:
            raise config.ConfigError("wall_minerals without wall_reaction: the classes belong to the rates")
        if self.wall_reaction is not None and len(self.wall_reaction) > 1 and self.wall_minerals is None:
            raise config.ConfigError("wall_reaction gives %d classes: wall_minerals says which solid voxel is of which" % len(self.wall_reaction))
        if self.wall_reaction is not None and self.par["tension_type"] != "CSF":
            raise config.ConfigError("wall_reaction belongs to the D3Q7 tracers of SurfaceTensionType = 'CSF': the perturbation model carries no tracers")

    def _wall_reaction_arg(self, rates):
        a = np.asarray(rates, dtype=np.float64)
        if a.ndim > 2 or (a.ndim == 2 and a.shape[1] != self.numTracers):
            raise config.ConfigError("wall_reaction: a number, %d numbers (one per tracer) or [classes][%d], not shape %s" % (self.numTracers, self.numTracers, a.shape))
        flat = np.full(self.numTracers, float(a)) if a.ndim == 0 else a.reshape(-1)
        return config.wall_reaction_rates(flat.tolist(), self.numTracers)

    def solid_minerals(self):
        """wall_minerals on the lattice [nz][ny][nx] as class bytes (class 0 where the file does not reach: buffer planes, forced side
        walls), or None; after initializeDomainBorder"""
        import os
        m = self.wall_minerals
        if m is None:
            return None
        if isinstance(m, (str, os.PathLike)):
            if not os.path.isfile(m):
                raise config.ConfigError("wall minerals: file %s not found" % m)
            m = np.load(m)
        m = np.asarray(m)
        if m.dtype.kind not in "ui" or m.size and (m.min() < 0 or m.max() > 7):
            raise config.ConfigError("wall minerals: one class 0 .. 7 per voxel (an integer array)")
        m = m.astype(np.uint8)
        voxels = getattr(self, "_voxels", None) if self._domain is None else None
        if voxels is not None:         # framed like the voxel file (geometry.voxel_domain): buffer planes below and above
            if m.shape != np.shape(voxels):
                raise config.ConfigError("wall minerals have shape %s, the voxel file %s" % (m.shape, np.shape(voxels)))
            buf = np.zeros((self._image_buffer,) + m.shape[1:], dtype=np.uint8)
            m = np.concatenate([buf, m, buf], axis=0)
        if m.shape != self.isDomain.shape:
            raise config.ConfigError("wall minerals have shape %s, the lattice %s" % (m.shape, self.isDomain.shape))
        return np.ascontiguousarray(m)

    def _apply_wall_reaction(self, solver, out):
        """wall_reaction into the solver (every rank makes the same call with the undivided map) and the rates in force into
        /WallReaction/Rates"""
        from ._lib import LbmpmError
        try:
            solver.set_wall_reaction(np.array(self.wall_reaction, dtype=np.float64), self.solid_minerals())
        except (ValueError, LbmpmError) as e:
            raise config.ConfigError("wall_reaction: %s" % e)
        if out is not None:
            out.write("WallReaction", "Rates", np.array(solver.wall_reaction, dtype=np.float64))

    def initializeTransportDomain(self):
        fluid = self.isDomain == 1
        nz = self.zDomain
        if self._initial_concentration is not None:
            conc = np.array(self._initial_concentration, dtype=np.float64)
            if conc.shape != (self.numTracers,) + self.isDomain.shape:
                raise config.ConfigError("initial_concentration has shape %s, %d tracers on the domain are %s" % (conc.shape, self.numTracers, (self.numTracers,) + self.isDomain.shape))
            conc = conc * fluid
        else:
            planes = np.arange(nz)[:, None, None]
            conc = np.zeros((self.numTracers,) + self.isDomain.shape)
            if self._is_image:
                conc[:, fluid & (planes >= nz - 10)] = 1.0
            else:
                conc[0, fluid & (planes <= nz - self.nbuf)] = 1.0
        self.tracerConc = conc

    def _open_solver(self):
        # distributed: one slab per rank; set_* take the undivided arrays, get* return the rank's own planes, rank 0 writes what it gathers
        return _CSFTracerSlab(self.isDomain, self.par, self.tr, self.device, self.csf_bulk_epsilon, distributed=self._distributed(), transport=self.csf_transport)

    def _start(self, h):
        done = RKColorGradient3D._start(self, h)
        if not self.restart_from:
            self.initializeTransportDomain()
            for k in range(self.numTracers):
                h.solver.set_concentration(k, self.tracerConc[k])
        return done

    def _tasks(self, h):
        """Both tables at one cadence, looked at before a stop's record (which steps): the flow's as the flow's driver writes them,
        the tracers' into ConcentrationResults and past the tracers' guard.  clusters_every, morphology_every and steady_every are not
        among them."""
        def report(step, t):
            self._tracer_guard.integrals(step, None if t is None else t.nonfinite, None if t is None else t.summary())
        def report_wall(step, t):
            self._tracer_guard.integrals(step, None if t is None else t.nonfinite, None if t is None else t.summary())
        tasks = [self._integrals_task(h, before_record=True),
                 PeriodicTask(self, self.integrals_every, ("TracerIntegrals", "PlaneIntegrals"), h.rank == 0, h.tracer_integrals, "tracer_integrals", file="conc",
                              report=report, closing=lambda: [("Columns", tracer_column_bytes())], before_record=True, joined=True)]
        if self.wall_reaction is not None:       # (only a run with a wall reaction has the task and its group)
            tasks.append(PeriodicTask(self, self.integrals_every, ("TracerWallIntegrals", "WallUptake"), h.rank == 0, h.tracer_wall_integrals,
                                      "tracer_wall_integrals", file="conc", report=report_wall,
                                      closing=lambda: [("Columns", tracer_wall_column_bytes())], before_record=True, joined=True))
        return tasks

    def runTransport3DMPMCRK(self, progress=None):
        if self.par["tension_type"] != "CSF":
            raise config.ConfigError("the tracers are coupled to the CSF colour-gradient flow: [SurfaceTension] SurfaceTensionType = 'CSF'")
        self.initializeDomainBorder()
        h = self._open_solver()
        done = self._start(h)
        tasks = self._tasks(h)
        flow = self._open_flow_file(h, tasks, h.rank == 0)
        more = (("WallReaction", "SurfaceRates"),) if self.wall_reaction is not None else ()
        conc = ResultFile(self.output_dir, "ConcentrationResults", (("TransportMacro", "MacroData"),) + runloop.groups(tasks, "conc") + more) if h.rank == 0 else None
        runloop.attach(tasks, conc, "conc")
        if self.wall_reaction is not None:       # (after a restart_from too: a checkpoint does not hold the rates)
            self._apply_wall_reaction(h.solver, conc)
        self.concentration_path = conc.path if conc else None
        # distributed: every rank checks its own planes, the verdict is collective (all ranks raise together, none is left in an exchange)
        guard = dict(nan_guard=getattr(self, "nan_guard", "raise"), collective=self._distributed(), device=self.device)
        self._guard = RecordGuard("rk3d+tracers", h.num_fluid_nodes, **guard)
        self._tracer_guard = RecordGuard("tracers", h.num_fluid_nodes, **guard)
        n = self.numTracers

        def record(done, tail):
            """the flow at the start of step done + 1 and the concentrations after the tracer update of that step, under one record
            number; in the tail: both as they stand"""
            self._step_now, k = done, self.records
            self._record(h, flow)
            if not tail:
                h.step(1)
                done += 1
            self.tracerConc = np.array([h.solver.get_concentration(i) for i in range(n)])      # (distributed: this rank's planes)
            for i in range(n):
                whole = self._gather(self.tracerConc[i])
                if conc is not None and whole is not None:
                    conc.write("TransportMacro", "TracerConcType%gin%g" % (i, k), whole)
            self._tracer_guard(k, done, {"tracer%d" % i: self.tracerConc[i] for i in range(n)}, {"tracer%d" % i: float(self.tracerConc[i].sum()) for i in range(n)})
            return done
        runloop.run(tasks, done, self.timeSteps, self.timeInterval, self.checkpoint_every, record, h.step, self._synced_checkpoint, progress)
        h.sync()
        self.solver = h
        return self.result_path, self.concentration_path
