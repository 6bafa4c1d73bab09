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
"""
import numpy as np

from . import config, runloop
from .RKColorGradientD3Q19 import RKColorGradient3D, _CSFSlab
from .integrals import tracer_column_bytes
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
    def __init__(self, pathIniFile, initial_concentration=None, **kw):
        RKColorGradient3D.__init__(self, pathIniFile, **kw)
        self.tr = config.read_transport3d(pathIniFile, periodic_z=self.periodic_z)      # (periodic z: no Dirichlet inlet, no Freeflow outlet)
        self.numTracers = self.tr["num_tracers"]
        self._initial_concentration = initial_concentration

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
        return [self._integrals_task(h, before_record=True),
                PeriodicTask(self, self.integrals_every, ("TracerIntegrals", "PlaneIntegrals"), h.rank == 0, h.tracer_integrals, "tracer_integrals", file="conc",
                             report=report, closing=lambda: [("Columns", tracer_column_bytes())], before_record=True, joined=True)]

    def runTransport3DMPMCRK(self, progress=None):
        if self.par["tension_type"] != "CSF":
            raise config.ConfigError("the tracers are coupled to the CSF colour-gradient flow: [SurfaceTension] SurfaceTensionType = 'CSF'")
        self.initializeDomainBorder()
        h = self._open_solver()
        done = self._start(h)
        tasks = self._tasks(h)
        flow = self._open_flow_file(h, tasks, h.rank == 0)
        conc = ResultFile(self.output_dir, "ConcentrationResults", (("TransportMacro", "MacroData"),) + runloop.groups(tasks, "conc")) if h.rank == 0 else None
        runloop.attach(tasks, conc, "conc")
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
