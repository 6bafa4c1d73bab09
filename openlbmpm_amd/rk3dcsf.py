"""Colour-gradient D3Q19 solver with continuum-surface-force tension -- Python face of lbmpm_rk3dcsf_* (include/lbmpm.h).

[SurfaceTension] SurfaceTensionType = 'CSF' in three dimensions: the reference's 2-D CSF loop (RKColorGradientLBM.runRKColorGradient2DCSF,
RKCG2D/RKD2Q9.py:1295-1490) carried to D3Q19 with z as the flow axis.  All arithmetic happens in liblbmpm_hip.so.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import F64P, U8P, RK3DCSFConfig, SlabTransportCalls, check
from .analysis import GatheredAnalysis, SlabAnalysisCalls, StackedAnalysis
from .slab import connect_in_library

FIELDS = dict(fR=0, fB=1, rhoR=2, rhoB=3, vx=4, vy=5, vz=6, phi=7, Gx=8, Gy=9, Gz=10, Fx=11, Fy=12, Fz=13, K=14, nsx=15, nsy=16, nsz=17,
              kind=18, theta=19, rec_fR=30, rec_fB=31, rec_rhoR=32, rec_rhoB=33, rec_vx=34, rec_vy=35, rec_vz=36, rec_phi=37)
_PDF_FIELDS = {"fR", "fB", "rec_fR", "rec_fB"}

# the 2-D ini's parameters (IniFiles/RKtwophasesetup2D.ini) under the 3-D ini's key names for the flow axis (RKtwophasesetup3D.ini:27-38)
DEFAULT_PARAMS = dict(sigma=0.1, theta=60.0, wetting=2, beta=0.7, delta=0.98, tauR=1.0, tauB=1.0, tautype=2, relax="MRT",
                      inlet="Neumann", outlet="Dirichlet", velocityZR=-1.0e-4, velocityZB=0.0, densityBH=5e-8, densityRH=1.00536,
                      densityBL=1.0, densityRL=5e-8, rates=None, variant=0, bulk_epsilon=0.0)


_INLETS = dict(Neumann=0, Dirichlet=1, Periodic=2)          # LBMPM_INLET_VELOCITY | _PRESSURE | _PERIODIC
_OUTLETS = dict(Dirichlet=0, Convective=1, Periodic=2)      # LBMPM_OUTLET_PRESSURE | _CONVECTIVE | _NONE


def periodic_pair(inlet, outlet):
    """periodic z: inlet 'Periodic' with outlet 'Periodic' -- no open planes, all nz planes wrap like x and y, the mask is taken as given
    and the velocity / density parameters of the open planes are not read.  True for the pair, False for neither; ValueError for one
    without the other"""
    if (inlet == "Periodic") != (outlet == "Periodic"):
        raise ValueError("periodic z is BoundaryTypeInlet 'Periodic' together with BoundaryTypeOutlet 'Periodic', not inlet=%r with outlet=%r"
                         % (inlet, outlet))
    return inlet == "Periodic"


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def tracer_config(num_tracers=1, diffusion_x=1. / 6., diffusion_y=None, diffusion_z=None, diffusion_xy=0., diffusion_yx=0.,
                  diffusion_xz=0., diffusion_zx=0., diffusion_yz=0., diffusion_zy=0., beta_interface=0., criteria_rho=0.5,
                  inlet_concentration=0., dirichlet_inlet=False, free_outlet=False, reaction_rate=0., diffusion_j=0.):
    """the lbmpm_tracer3d_config of RK3DCSFSolver.configure_tracers(...) and of RK3DCSFSolver(..., tracers=dict(...)).  Per-tracer entries
    are a number or a sequence of num_tracers numbers; diffusion_y, diffusion_z default to diffusion_x"""
    from ._lib import Tracer3DConfig
    nT = int(num_tracers)
    cfg = Tracer3DConfig()
    cfg.num_tracers = nT

    def per(v, what):
        a = np.broadcast_to(np.asarray(v, dtype=np.float64), (max(min(nT, 4), 1),)) if np.ndim(v) == 0 else np.asarray(v, dtype=np.float64)
        if a.shape[0] < min(nT, 4):
            raise ValueError("%s: %d entries for %d tracers" % (what, a.shape[0], nT))
        return a
    dy = diffusion_x if diffusion_y is None else diffusion_y
    dz = diffusion_x if diffusion_z is None else diffusion_z
    for name, v in (("diffusion_x", diffusion_x), ("diffusion_y", dy), ("diffusion_z", dz), ("beta_interface", beta_interface),
                    ("inlet_concentration", inlet_concentration), ("diffusion_j", diffusion_j)):
        a = per(v, name)
        for t in range(min(nT, 4)):
            getattr(cfg, name)[t] = float(a[t])
    cfg.diffusion_xy, cfg.diffusion_yx, cfg.diffusion_xz = float(diffusion_xy), float(diffusion_yx), float(diffusion_xz)
    cfg.diffusion_zx, cfg.diffusion_yz, cfg.diffusion_zy = float(diffusion_zx), float(diffusion_yz), float(diffusion_zy)
    cfg.criteria_rho = float(criteria_rho)
    cfg.dirichlet_inlet, cfg.free_outlet = int(bool(dirichlet_inlet)), int(bool(free_outlet))
    cfg.reaction_rate = float(reaction_rate)
    return cfg


def body_force_pair(g=None, red=None, blue=None):
    """the arguments of set_body_force as ((gx, gy, gz) of red, ... of blue): g for both colours, red / blue in its place for one;
    a colour nobody names is zero.  ValueError: not three numbers"""
    def three(v, what):
        if v is None:
            return (0.0, 0.0, 0.0)
        a = np.asarray(v, dtype=np.float64)
        if a.shape != (3,):
            raise ValueError("body force %s = (gx, gy, gz), not %r" % (what, v))
        return tuple(float(x) for x in a)
    return three(g if red is None else red, "red"), three(g if blue is None else blue, "blue")


def wall_rates(rates, num_tracers):
    """the rates of set_wall_reaction as a float64 array [classes][nT]: a scalar (every tracer, one class), [nT] (one class) or
    [classes][nT], 1 .. 8 classes.  ValueError: another shape.  (The values are the library's to check: k >= 0, inf allowed.)"""
    nT = int(num_tracers)
    a = np.asarray(rates, dtype=np.float64)
    if a.ndim == 0:
        a = np.full((1, nT), float(a))
    elif a.ndim == 1:
        a = a.reshape(1, -1)
    if a.ndim != 2 or a.shape[1] != nT or not 1 <= a.shape[0] <= 8:
        raise ValueError("wall reaction rates: a number, [%d] numbers (one per tracer) or [classes][%d] with 1 .. 8 classes, not shape %s"
                         % (nT, nT, np.shape(rates)))
    return np.ascontiguousarray(a)


def _undivided_minerals(minerals, shape):
    if minerals is None:
        return None
    m = np.asarray(minerals)
    if m.shape != tuple(shape):
        raise ValueError("minerals must have the shape of the lattice %s, not %s" % (tuple(shape), m.shape))
    if m.dtype.kind not in "ui" or m.min() < 0 or m.max() > 255:
        raise ValueError("minerals: one class byte (0 .. 7) per cell")
    return np.ascontiguousarray(m, dtype=np.uint8)


def _wall_valid(dom, rates, minerals):
    """what lbmpm_rk3dcsf_tracer_set_wall_reaction checks, ahead of the calls: RK3DCSFCluster changes no slab when another would refuse"""
    if not bool(np.all(rates >= 0.0)):
        raise _lib.LbmpmError("set_wall_reaction: a rate that is negative or NaN", _lib.ERR_INVALID)
    if minerals is None and rates.shape[0] != 1:
        raise _lib.LbmpmError("set_wall_reaction: %d classes without a mineral map" % rates.shape[0], _lib.ERR_INVALID)
    if minerals is not None:
        bad = (np.asarray(dom) != 1) & (minerals >= rates.shape[0])
        if bad.any():
            z, y, x = [int(i[0]) for i in np.nonzero(bad)]
            raise _lib.LbmpmError("set_wall_reaction: mineral class %d at the solid cell (z, y, x) = (%d, %d, %d), %d classes were given"
                                  % (int(minerals[z, y, x]), z, y, x, rates.shape[0]), _lib.ERR_INVALID)


class RK3DCSFSolver(SlabTransportCalls, SlabAnalysisCalls):
    _C_PREFIX, _NO_TRANSPORT = "lbmpm_rk3dcsf", "none"

    def __init__(self, is_domain, params=None, device=0, diagnostics=False, slab=None, tracers=None):
        """slab = (z0, global_nz): this lattice is a slab of an undivided lattice of global_nz planes -- its planes 2 .. nz-3 are the planes
        z0 .. of that lattice, its two planes at either end images of the neighbouring slabs' edge planes (cut from the undivided lattice,
        wrapping around its ends, like the rest).
        params: DEFAULT_PARAMS' keys.  inlet="Periodic" with outlet="Periodic" (both or neither, else ValueError) is periodic z: no open
        planes, every plane wraps like x and y, the mask is taken as given (nz >= 4) and velocityZ*, density* are not read; self.periodic_z
        says so.  Tracers then take neither dirichlet_inlet nor free_outlet (LbmpmError, LBMPM_ERR_INVALID).  clusters() / morphology()
        by default still take plane nz-1 and plane 0 as ends of the lattice; wrap_z=True closes the seam (analysis.py, clusters.close_seam).
        tracers = dict(<the keyword arguments of configure_tracers>): the D3Q7 tracers, configured at construction.  On a slab this is the
        only way to them (lbmpm_rk3dcsf_tracer_configure_slab): their populations travel inside the population message, so every slab of
        the ring is given the same dict, before a transport is connected."""
        L = _lib.lib()
        p = dict(DEFAULT_PARAMS)
        p.update(params or {})
        unknown = set(p) - set(DEFAULT_PARAMS)
        if unknown:
            raise KeyError("unknown RK3DCSF parameters: %s" % sorted(unknown))
        self.params = p
        dom = np.ascontiguousarray(is_domain, dtype=np.uint8)
        if dom.ndim != 3:
            raise TypeError("is_domain must be a 3-D array [nz, ny, nx]")
        self.nz, self.ny, self.nx = dom.shape
        self.shape = dom.shape
        self.is_domain = dom
        cfg = RK3DCSFConfig()
        cfg.nx, cfg.ny, cfg.nz = self.nx, self.ny, self.nz
        cfg.surface_tension, cfg.contact_angle_deg = p["sigma"], p["theta"]
        cfg.beta, cfg.delta, cfg.tau_r, cfg.tau_b = p["beta"], p["delta"], p["tauR"], p["tauB"]
        cfg.inlet_velocity_z = p["velocityZB"] + p["velocityZR"]
        cfg.inlet_rho_r, cfg.inlet_rho_b = p["densityRH"], p["densityBH"]
        cfg.outlet_rho_total = p["densityBL"] + p["densityRL"]
        cfg.wetting_type, cfg.tau_type = int(p["wetting"]), int(p["tautype"])
        if p["relax"] not in ("SRT", "MRT"):
            raise ValueError("RelaxationType must be 'SRT' or 'MRT'")
        cfg.relaxation = 1 if p["relax"] == "MRT" else 0
        self.periodic_z = periodic_pair(p["inlet"], p["outlet"])
        if p["inlet"] not in _INLETS:
            raise ValueError("BoundaryTypeInlet must be 'Neumann' or 'Dirichlet' (or 'Periodic', with BoundaryTypeOutlet 'Periodic')")
        if p["outlet"] not in _OUTLETS:
            raise ValueError("BoundaryTypeOutlet must be 'Dirichlet' or 'Convective' (or 'Periodic', with BoundaryTypeInlet 'Periodic')")
        cfg.inlet_type, cfg.outlet_type = _INLETS[p["inlet"]], _OUTLETS[p["outlet"]]
        cfg.device = int(device)
        cfg.variant = int(p["variant"])        # 1: no bulk skip (cross-check)
        cfg.bulk_epsilon = float(p["bulk_epsilon"])      # 0: exact (2^-51); opt-in: cut a colour's tail below this fraction of the density
        self.ghost = (GHOST, GHOST) if slab else (0, 0)
        cfg.ghost_lo, cfg.ghost_hi = self.ghost
        self.global_nz = int(slab[1]) if slab else self.nz
        if slab:
            cfg.slab_z0, cfg.global_nz = int(slab[0]), int(slab[1])
        if p["rates"] is not None:
            if len(p["rates"]) != 6:
                raise ValueError("rates = (s_e, s_eps, s_q, s_pi, s_m, rate of the conserved moments)")
            for i, r in enumerate(p["rates"]):
                cfg.mrt_rates[i] = float(r)
        self._h = C.c_void_p()
        check(L.lbmpm_rk3dcsf_create(C.byref(cfg), dom.ctypes.data_as(U8P), C.byref(self._h)), "lbmpm_rk3dcsf_create")
        self._L = L
        if diagnostics:
            self.enable_diagnostics(True)
        if tracers is not None:
            cfg = tracer_config(**tracers)
            if slab:
                check(L.lbmpm_rk3dcsf_tracer_configure_slab(self._h, C.byref(cfg)), "lbmpm_rk3dcsf_tracer_configure_slab")
            else:
                check(L.lbmpm_rk3dcsf_tracer_configure(self._h, C.byref(cfg)), "lbmpm_rk3dcsf_tracer_configure")
            self.num_tracers = int(cfg.num_tracers)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.lbmpm_rk3dcsf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ptr(self, a, shape, what):
        if a is None:
            return None
        a = _f64(a)
        if a.shape != shape:
            raise TypeError("%s must have shape %s" % (what, shape))
        self._keep.append(a)
        return a.ctypes.data_as(F64P)

    def set_macro(self, rhoR, rhoB, vx=None, vy=None, vz=None):
        self._keep = []
        ptr = [self._ptr(a, self.shape, "macroscopic arrays") for a in (rhoR, rhoB, vx, vy, vz)]
        check(self._L.lbmpm_rk3dcsf_set_macro(self._h, *ptr), "lbmpm_rk3dcsf_set_macro")
        self._keep = []

    def set_pdf(self, fR, fB, force=None):
        """streamed populations [nz][ny][nx][19] per colour + the force of the last step (Fx, Fy, Fz): the restart"""
        self._keep = []
        ptr = [self._ptr(a, self.shape + (19,), "populations") for a in (fR, fB)]
        ptr += [self._ptr(a, self.shape, "force") for a in (force or (None, None, None))]
        check(self._L.lbmpm_rk3dcsf_set_pdf(self._h, *ptr), "lbmpm_rk3dcsf_set_pdf")
        self._keep = []

    def set_contact_angles(self, theta):
        """mixed wettability: theta [nz][ny][nx] in degrees (a slab: with its ghost planes, like set_macro), read at the fluid cells next
        to solid (get("kind") == 3) and ignored elsewhere, where it may be NaN -- what geometry.wall_contact_angles returns.  It takes
        the place of params["theta"] in the wetting rule from the next step on; None: back to params["theta"].  Whenever the solver is
        idle, repeatedly; the state, the step counter and the snapshot of change() stay, and set_macro / set_pdf keep the map.
        get("theta") returns the angles in force.  ValueError: a wrong shape; LbmpmError (LBMPM_ERR_INVALID): an angle at such a cell
        that is not finite or not within [0, 180], or params["wetting"] == 0"""
        if theta is None:
            check(self._L.lbmpm_rk3dcsf_set_contact_angles(self._h, None), "lbmpm_rk3dcsf_set_contact_angles")
            return
        a = _f64(theta)
        if a.shape != self.shape:
            raise ValueError("contact angles must have shape %s, not %s" % (self.shape, a.shape))
        check(self._L.lbmpm_rk3dcsf_set_contact_angles(self._h, a.ctypes.data_as(F64P)), "lbmpm_rk3dcsf_set_contact_angles")

    def set_body_force(self, g=None, *, red=None, blue=None):
        """an acceleration per colour in lattice units (gravity, force-driven flow): g = (gx, gy, gz) for both colours, red= / blue= in
        its place for one; all None (or all zeros): no body force, the step runs the kernels it ran before.  The force density of a cell
        is rho_R g_R + rho_B g_B; half of it enters u, the Guo source takes it beside the CSF force (include/lbmpm.h).  get("Fx" ...) and
        the force= of set_pdf stay the CSF force alone.  Whenever the solver is idle, repeatedly; the state, the step counter, the
        contact angles and the snapshot of change() stay, and set_macro / set_pdf keep it.  ValueError: not three numbers; LbmpmError:
        a value that is not finite (LBMPM_ERR_INVALID), a call between the stages of a step (LBMPM_ERR_STATE)"""
        if g is None and red is None and blue is None:
            check(self._L.lbmpm_rk3dcsf_set_body_force(self._h, None, None), "lbmpm_rk3dcsf_set_body_force")
            return
        gr, gb = body_force_pair(g, red, blue)
        check(self._L.lbmpm_rk3dcsf_set_body_force(self._h, (C.c_double * 3)(*gr), (C.c_double * 3)(*gb)), "lbmpm_rk3dcsf_set_body_force")

    @property
    def body_force(self):
        """((gx, gy, gz) of red, (gx, gy, gz) of blue) in force; zeros without a body force"""
        gr, gb = (C.c_double * 3)(), (C.c_double * 3)()
        check(self._L.lbmpm_rk3dcsf_get_body_force(self._h, gr, gb), "lbmpm_rk3dcsf_get_body_force")
        return tuple(gr), tuple(gb)

    def enable_diagnostics(self, on=True):
        check(self._L.lbmpm_rk3dcsf_enable_diagnostics(self._h, 1 if on else 0), "enable_diagnostics")

    def step(self, nsteps=1):
        check(self._L.lbmpm_rk3dcsf_step(self._h, int(nsteps)), "lbmpm_rk3dcsf_step")

    def stage(self, k):
        """a third of a step (0 phase field, 1 gradient, 2 collision); the face messages go in between (include/lbmpm.h)"""
        check(self._L.lbmpm_rk3dcsf_stage(self._h, int(k)), "lbmpm_rk3dcsf_stage")

    def face_doubles(self, msg, face):
        return int(self._L.lbmpm_rk3dcsf_face_doubles(self._h, int(msg), int(face)))

    def face_doubles_in(self, msg, face):
        return int(self._L.lbmpm_rk3dcsf_face_doubles_in(self._h, int(msg), int(face)))

    def face_pack(self, msg, face, device_ptr):
        check(self._L.lbmpm_rk3dcsf_face_pack(self._h, int(msg), int(face), C.c_void_p(int(device_ptr))), "lbmpm_rk3dcsf_face_pack")

    def face_unpack(self, msg, face, device_ptr):
        check(self._L.lbmpm_rk3dcsf_face_unpack(self._h, int(msg), int(face), C.c_void_p(int(device_ptr))), "lbmpm_rk3dcsf_face_unpack")

    def send_to(self, face, other, msg):
        """same process: this slab's message through `face` into the ghost planes of the slab on the other side"""
        check(self._L.lbmpm_rk3dcsf_face_copy(self._h, int(face), other._h, int(msg)), "lbmpm_rk3dcsf_face_copy")

    def step_timed(self, nsteps):
        """(ms_total, ms of the csf3d_collide launches) by HIP events on the solver's stream"""
        a, b = C.c_double(0), C.c_double(0)
        check(self._L.lbmpm_rk3dcsf_step_timed(self._h, int(nsteps), C.byref(a), C.byref(b)), "lbmpm_rk3dcsf_step_timed")
        return a.value, b.value

    # ---- a slab's face messages over a transport inside the library (the slabs form a ring): ipc_init .. sync(deadline_s) are
    # _lib.SlabTransportCalls; `transport` says 'none' while the slab steps by stage() and the caller moves the messages
    def step_slab(self, nsteps=1, timed=False):
        """nsteps whole steps of a connected slab behind one C call: stages and face messages enqueued, the host not blocked"""
        check(self._L.lbmpm_rk3dcsf_step_slab(self._h, int(nsteps), int(bool(timed))), "lbmpm_rk3dcsf_step_slab")

    def slab_timing(self):
        """average ms per stage and per message over the timed steps of the last step_slab(..., timed=True)"""
        out = (C.c_double * 7)()
        check(self._L.lbmpm_rk3dcsf_slab_timing(self._h, out), "lbmpm_rk3dcsf_slab_timing")
        return dict(stage_ms=list(out[0:3]), message_ms=list(out[3:6]), messages=["phi", "normal", "populations"], steps=int(out[6]))

    # ---- D3Q7 tracers advected by the flow (lbmpm_rk3dcsf_tracer_*)
    def configure_tracers(self, *args, **kwargs):
        """Before the first step, on the undivided lattice (a slab takes them at construction: tracers=); the keyword arguments of
        tracer_config().  diffusion_j is the rest weight J0' of the reaction source on the D3Q7 lattice ((3 J0 - 1) / 2 of the 2-D file's J0:
        config.read_transport3d maps it).  The tracer sub-step runs after the flow's collision with rho_R, u and G of that flow step."""
        cfg = tracer_config(*args, **kwargs)
        check(self._L.lbmpm_rk3dcsf_tracer_configure(self._h, C.byref(cfg)), "lbmpm_rk3dcsf_tracer_configure")
        self.num_tracers = int(cfg.num_tracers)

    def set_concentration(self, t, conc):
        """dense [nz][ny][nx] (a slab: with its ghost planes, like set_macro); g_i = C w_i; before the first step"""
        self._keep = []
        ptr = self._ptr(conc, self.shape, "concentration")
        check(self._L.lbmpm_rk3dcsf_tracer_set_concentration(self._h, int(t), ptr), "lbmpm_rk3dcsf_tracer_set_concentration")
        self._keep = []

    def get_concentration(self, t):
        """the concentration the reference records after the last completed step, [nz][ny][nx] (zeros off the fluid)"""
        out = np.empty(self.shape, dtype=np.float64)
        check(self._L.lbmpm_rk3dcsf_tracer_get_concentration(self._h, int(t), out.ctypes.data_as(F64P)), "lbmpm_rk3dcsf_tracer_get_concentration")
        return out

    def get_tracer_pdf(self, t):
        """the populations behind get_concentration, [nz][ny][nx][7] in the order rest, +x, -x, +y, -y, +z, -z"""
        out = np.empty(self.shape + (7,), dtype=np.float64)
        check(self._L.lbmpm_rk3dcsf_tracer_get_pdf(self._h, int(t), out.ctypes.data_as(F64P)), "lbmpm_rk3dcsf_tracer_get_pdf")
        return out

    def set_tracer_pdf(self, t, g):
        """the restart: populations as get_tracer_pdf returns them, together with set_pdf of the flow"""
        self._keep = []
        ptr = self._ptr(g, self.shape + (7,), "tracer populations")
        check(self._L.lbmpm_rk3dcsf_tracer_set_pdf(self._h, int(t), ptr), "lbmpm_rk3dcsf_tracer_set_pdf")
        self._keep = []

    def set_wall_reaction(self, rates, minerals=None):
        """first-order reaction of the tracers at solid walls, D dC/dn = k C_wall: a population that bounces off a solid comes back times
        r = (1 - 3 k) / (1 + 3 k) (include/lbmpm.h).  rates: k >= 0 in lattice units (a velocity; Damkoehler number k H / D; inf: C_wall
        = 0) -- a number for every tracer, [nT] numbers, or [classes][nT] with minerals [nz][ny][nx] (a slab: with its ghost planes), the
        class byte 0 .. classes-1 of every solid cell (ignored at fluid cells).  None: off.  Needs configured tracers; whenever the
        solver is idle, repeatedly; the state, the step counter, the contact angles, the body force and the snapshot of change() stay,
        set_concentration / set_tracer_pdf keep it, and the observers see the new rate's pull at once.  k = 0 leaves the fields bit-equal
        to a run without the call.  ValueError: a wrong shape; LbmpmError: no tracers (LBMPM_ERR_STATE); a negative or NaN rate, a class
        at a solid cell that is not below `classes` (LBMPM_ERR_INVALID) -- nothing changed"""
        name = "lbmpm_rk3dcsf_tracer_set_wall_reaction"
        if rates is None:
            if minerals is not None:
                raise ValueError("set_wall_reaction: a mineral map without rates")
            check(self._L.lbmpm_rk3dcsf_tracer_set_wall_reaction(self._h, 0, None, None), name)
            return
        if not getattr(self, "num_tracers", 0):
            raise _lib.LbmpmError("set_wall_reaction before configure_tracers", _lib.ERR_STATE)
        a = wall_rates(rates, self.num_tracers)
        m = _undivided_minerals(minerals, self.shape)
        check(self._L.lbmpm_rk3dcsf_tracer_set_wall_reaction(self._h, a.shape[0], a.ctypes.data_as(F64P), None if m is None else m.ctypes.data_as(U8P)), name)

    @property
    def wall_reaction(self):
        """the rates in force, [classes][nT]; None without a wall reaction"""
        n = C.c_int(0)
        out = np.zeros((8, max(1, getattr(self, "num_tracers", 0))), dtype=np.float64)
        check(self._L.lbmpm_rk3dcsf_tracer_get_wall_reaction(self._h, C.byref(n), out.ctypes.data_as(F64P)), "lbmpm_rk3dcsf_tracer_get_wall_reaction")
        return out[:n.value].copy() if n.value else None

    def tracer_wall_integrals(self):
        """integrals.TracerWallIntegrals of the own planes, [planes][nT][4]: wall links, uptake, summed wall concentration and the
        non-finite count per plane and tracer (lbmpm_rk3dcsf_tracer_wall_integrals), reduced on the device from the stored populations;
        valid with or without a wall reaction (without: an uptake of exactly 0)"""
        from .integrals import TracerWallIntegrals, tracer_wall_table
        n = max(1, getattr(self, "num_tracers", 0))          # (without tracers the library refuses before it writes)
        return TracerWallIntegrals(tracer_wall_table(self._L, self._h, self.own_planes, n), self.nx, self.ny)

    def get(self, name):
        out = np.empty(self.shape + ((19,) if name in _PDF_FIELDS else ()), dtype=np.float64)
        check(self._L.lbmpm_rk3dcsf_get_field(self._h, FIELDS[name], out.ctypes.data_as(F64P)), "get_field(%s)" % name)
        return out

    # ---- integrals() .. morphology(): analysis.SlabAnalysisCalls, here over what get("rec_*") hands out for the own planes (a slab:
    # without its ghost planes), taken from the populations in registers -- no per-cell staging, nothing to call beforehand
    own_planes = property(lambda self: self.nz - self.ghost[0] - self.ghost[1])
    lattice_nz = property(lambda self: self.global_nz)

    def tracer_integrals(self):
        """integrals.TracerIntegrals of the own planes, [planes][nT][9]: cells, mass, the first moments g(+a) - g(-a) per axis, sum C^2,
        the extrema of C and the non-finite count per plane and tracer, over the populations get_tracer_pdf hands out -- reduced on the
        device for all tracers at once (lbmpm_rk3dcsf_tracer_integrals), no dense field staged or copied"""
        from .integrals import TracerIntegrals, tracer_table
        n = max(1, getattr(self, "num_tracers", 0))          # (without tracers the library refuses before it writes)
        return TracerIntegrals(tracer_table(self._L, self._h, self.own_planes, n), self.nx, self.ny)

    @property
    def num_fluid_nodes(self):
        return int(self._L.lbmpm_rk3dcsf_num_fluid_nodes(self._h))

    @property
    def num_wetting_solids(self):
        return int(self._L.lbmpm_rk3dcsf_num_wetting_solids(self._h))

    @property
    def bulk_cells(self):
        """fluid cells whose block of 256 skipped the phase-field pull, the gradient and the curvature in the last step"""
        return int(self._L.lbmpm_rk3dcsf_bulk_cells(self._h))

    @property
    def steps_done(self):
        return int(self._L.lbmpm_rk3dcsf_steps_done(self._h))

    @property
    def device_bytes(self):
        return int(self._L.lbmpm_rk3dcsf_device_bytes(self._h))

    @property
    def dominant_kernel(self):
        return self._L.lbmpm_rk3dcsf_dominant_kernel(self._h).decode()


MSG_PDF, MSG_PHI, MSG_NORMAL = 0, 1, 2        # LBMPM_CSF_MSG_*
_AFTER_STAGE = (MSG_PHI, MSG_NORMAL, MSG_PDF)  # the message that follows stage 0, 1, 2
GHOST = 2


def slab_cuts(nz, nslabs, weights=None):
    """z0 of every slab + nz: equal shares of the planes (or of `weights`, one number per plane), at least 4 planes each"""
    nslabs = int(nslabs)
    if nslabs < 1 or nz < 4 * nslabs:
        raise ValueError("%d planes do not make %d slabs of at least 4" % (nz, nslabs))
    w = np.ones(nz) if weights is None else np.asarray(weights, dtype=np.float64)
    acc = np.concatenate([[0.0], np.cumsum(w)])
    cuts = [0]
    for k in range(1, nslabs):
        z = int(np.searchsorted(acc, acc[-1] * k / nslabs))
        cuts.append(min(max(z, cuts[-1] + 4), nz - 4 * (nslabs - k)))
    return cuts + [nz]


class _SlabGeometry:
    """the planes [z0, z1) of a lattice [nz][ny][nx] with the two ghost planes a slab of the CSF model carries at either end (the slabs
    form a ring: the loop wraps z, so the first slab's low neighbour is the last slab)"""

    def __init__(self, nz, z0, z1):
        self.nz, self.z0, self.z1 = int(nz), int(z0), int(z1)
        self.whole = self.z0 == 0 and self.z1 == self.nz
        self.ghost = (0, 0) if self.whole else (GHOST, GHOST)
        self.planes = np.arange(self.z0 - self.ghost[0], self.z1 + self.ghost[1]) % self.nz
        self.slab = None if self.whole else (self.z0, self.nz)

    def cut(self, a):
        return None if a is None else np.ascontiguousarray(np.take(a, self.planes, axis=0))

    def own(self, a):
        return a[self.ghost[0]:a.shape[0] - self.ghost[1]]


def _undivided_angles(theta, shape):
    if theta is None:
        return None
    a = _f64(theta)
    if a.shape != tuple(shape):
        raise ValueError("contact angles must have the shape of the undivided lattice %s, not %s" % (tuple(shape), a.shape))
    return a


def _angles_valid(slab, a):
    """what lbmpm_rk3dcsf_set_contact_angles checks, ahead of the call: RK3DCSFCluster changes no slab when another would refuse"""
    wall = slab.get("kind") == 3
    if slab.ghost[0]:
        wall[0] = False
    if slab.ghost[1]:
        wall[-1] = False
    v = a[wall]
    if not bool(np.all(np.isfinite(v) & (v >= 0.0) & (v <= 180.0))):
        z, y, x = [int(i[0]) for i in np.nonzero(wall & ~(np.isfinite(a) & (a >= 0.0) & (a <= 180.0)))]
        raise _lib.LbmpmError("contact angle %r at the cell (z, y, x) = (%d, %d, %d) of a slab, a fluid cell next to solid: finite and "
                              "within [0, 180] degrees" % (float(a[z, y, x]), z, y, x), _lib.ERR_INVALID)


def _periodic_params(params):
    """periodic_pair of the inlet / outlet a params dict (or None) asks for"""
    p = params or {}
    return periodic_pair(p.get("inlet", DEFAULT_PARAMS["inlet"]), p.get("outlet", DEFAULT_PARAMS["outlet"]))


_TRACERS_AT_CONSTRUCTION = ("tracers on z-slabs are part of the slabs' population message, which is sized when the ring is set up: "
                            "give them to %s at construction (tracers=dict(...)), not afterwards")


class _SlabSetup:
    """What RK3DCSFCluster and RK3DCSFDistributed share: how a set-up call with undivided arrays reaches the slabs, and how the slabs'
    arrays come back.  self.slabs is the slabs this object holds, self._pairs() the (slab, _SlabGeometry) pairs -- all of them in a
    cluster, this rank's one under torch.distributed.  A setter takes the undivided array [nz][ny][nx] and gives every slab its planes and the images of its
    neighbours'; a getter returns the own planes of the pairs, stacked along z (Distributed: this rank's own planes, gather() stacks
    them on rank 0).  Distributed: the same call with the same arrays on every rank, and the setters after sync() -- the slab must be idle."""

    def set_macro(self, rhoR, rhoB, vx=None, vy=None, vz=None):
        """the undivided arrays [nz][ny][nx]; every slab takes its planes"""
        for s, g in self._pairs():
            s.set_macro(*[g.cut(None if a is None else np.asarray(a, dtype=np.float64)) for a in (rhoR, rhoB, vx, vy, vz)])

    def set_pdf(self, fR, fB, force=None):
        for s, g in self._pairs():
            s.set_pdf(g.cut(np.asarray(fR)), g.cut(np.asarray(fB)), None if force is None else tuple(g.cut(np.asarray(c)) for c in force))

    def set_contact_angles(self, theta):
        """the undivided array [nz][ny][nx], the same on every rank (RK3DCSFSolver.set_contact_angles; None: the scalar angle again);
        every slab takes its planes and the images of its neighbours'.  Distributed: call it after sync(), the slab must be idle"""
        theta = _undivided_angles(theta, self.shape)
        for s, g in self._pairs():
            s.set_contact_angles(g.cut(theta))

    def set_body_force(self, g=None, *, red=None, blue=None):
        """RK3DCSFSolver.set_body_force on every slab, the same call on every rank (the force is local to a cell: no message changes)"""
        for s in self.slabs:
            s.set_body_force(g, red=red, blue=blue)

    def configure_tracers(self, *args, **kwargs):
        """refused: on slabs the tracers change the size of the population message, so they are given at construction (tracers=)"""
        raise _lib.LbmpmError(_TRACERS_AT_CONSTRUCTION % type(self).__name__, _lib.ERR_UNSUPPORTED)

    def set_concentration(self, t, conc):
        """the undivided array [nz][ny][nx]; every slab takes its planes (and the images of its neighbours')"""
        for s, g in self._pairs():
            s.set_concentration(t, g.cut(np.asarray(conc, dtype=np.float64)))

    def set_tracer_pdf(self, t, pdf):
        for s, g in self._pairs():
            s.set_tracer_pdf(t, g.cut(np.asarray(pdf, dtype=np.float64)))

    def set_wall_reaction(self, rates, minerals=None):
        """RK3DCSFSolver.set_wall_reaction, the same call on every rank, with the undivided `minerals` [nz][ny][nx]; every slab takes
        its planes and the images of its neighbours'.  Distributed: call it after sync(), the slab must be idle"""
        m = _undivided_minerals(minerals, self.shape)
        for s, g in self._pairs():
            s.set_wall_reaction(rates, g.cut(m))

    def _own(self, of):
        return np.concatenate([g.own(of(s)) for s, g in self._pairs()], axis=0)

    def get(self, name):
        """the own planes of the slabs held (Distributed: this rank's)"""
        return self._own(lambda s: s.get(name))

    def get_concentration(self, t):
        """the own planes of the slabs held (Distributed: this rank's; gather() stacks them on rank 0)"""
        return self._own(lambda s: s.get_concentration(t))

    def get_tracer_pdf(self, t):
        return self._own(lambda s: s.get_tracer_pdf(t))

    # (the same on every slab)
    body_force = property(lambda self: self.slabs[0].body_force)
    wall_reaction = property(lambda self: self.slabs[0].wall_reaction)
    steps_done = property(lambda self: self.slabs[0].steps_done)
    dominant_kernel = property(lambda self: self.slabs[0].dominant_kernel)
    num_fluid_nodes = property(lambda self: sum(int((g.own(s.is_domain) == 1).sum()) for s, g in self._pairs()))


class RK3DCSFCluster(_SlabSetup, StackedAnalysis):
    """The 3-D CSF model cut into slabs along z, every slab a context of its own (devices[k]; all on one GPU: a rehearsal of the
    decomposition, bit-equal to the undivided lattice).  One time step = three stages with a face message after each: phi (two planes),
    n (one plane), the populations crossing the face (lbmpm_rk3dcsf_stage / _face_copy).
    integrals() .. morphology(): analysis.StackedAnalysis; nothing can be stale, so nothing is refreshed."""

    def __init__(self, is_domain, params=None, nslabs=2, devices=None, cuts=None, diagnostics=False, tracers=None):
        """tracers = dict(<the keyword arguments of RK3DCSFSolver.configure_tracers>): D3Q7 tracers on every slab"""
        dom = np.ascontiguousarray(is_domain, dtype=np.uint8)
        self.shape = dom.shape
        self.nz, self.ny, self.nx = dom.shape
        self.periodic_z = _periodic_params(params)       # (periodic z: a cut may fall anywhere, the ring's seam is one more face)
        self.cuts = list(cuts) if cuts is not None else slab_cuts(self.nz, nslabs)
        n = len(self.cuts) - 1
        devices = list(devices) if devices is not None else [0] * n
        self.geo = [_SlabGeometry(self.nz, self.cuts[k], self.cuts[k + 1]) for k in range(n)]
        self.slabs = [RK3DCSFSolver(g.cut(dom), params, device=devices[k], diagnostics=diagnostics, slab=g.slab, tracers=tracers) for k, g in enumerate(self.geo)]
        self.params = self.slabs[0].params
        self.num_tracers = getattr(self.slabs[0], "num_tracers", 0)

    def close(self):
        for s in self.slabs:
            s.close()

    def _pairs(self):
        return list(zip(self.slabs, self.geo))

    def set_contact_angles(self, theta):
        """_SlabSetup.set_contact_angles.  Checked on every slab before any is changed"""
        theta = _undivided_angles(theta, self.shape)
        if theta is not None:
            for s, g in self._pairs():
                _angles_valid(s, g.cut(theta))
        super().set_contact_angles(theta)

    def set_body_force(self, g=None, *, red=None, blue=None):
        """_SlabSetup.set_body_force.  Checked before any slab is changed"""
        if not (g is None and red is None and blue is None):
            if not np.all(np.isfinite(body_force_pair(g, red, blue))):
                raise _lib.LbmpmError("set_body_force: an acceleration that is not finite", _lib.ERR_INVALID)
        super().set_body_force(g, red=red, blue=blue)

    def set_wall_reaction(self, rates, minerals=None):
        """_SlabSetup.set_wall_reaction.  Checked on every slab before any is changed"""
        if rates is not None:
            if not self.num_tracers:
                raise _lib.LbmpmError("set_wall_reaction before configure_tracers", _lib.ERR_STATE)
            a, m = wall_rates(rates, self.num_tracers), _undivided_minerals(minerals, self.shape)
            for s, g in self._pairs():
                _wall_valid(s.is_domain, a, g.cut(m))
        super().set_wall_reaction(rates, minerals)

    def tracer_wall_integrals(self):
        """the slabs' wall tables in plane order: bit-equal to the undivided lattice's"""
        from .integrals import TracerWallIntegrals
        return TracerWallIntegrals(np.concatenate([s.tracer_wall_integrals().planes for s in self.slabs], axis=0), self.nx, self.ny)

    def _exchange(self, msg):
        n = len(self.slabs)
        for k in range(n):                         # a ring: the last slab's high face is the first slab's low face
            up = self.slabs[(k + 1) % n]
            self.slabs[k].send_to(1, up, msg)
            up.send_to(0, self.slabs[k], msg)

    def step(self, nsteps=1):
        if len(self.slabs) == 1:
            return self.slabs[0].step(nsteps)
        for _ in range(int(nsteps)):
            for stage in range(3):
                for s in self.slabs:
                    s.stage(stage)
                self._exchange(_AFTER_STAGE[stage])

    def sync(self):
        for s in self.slabs:
            s.sync()

    def tracer_integrals(self):
        """the slabs' tracer tables in plane order: bit-equal to the undivided lattice's"""
        from .integrals import TracerIntegrals
        return TracerIntegrals(np.concatenate([s.tracer_integrals().planes for s in self.slabs], axis=0), self.nx, self.ny)

    is_fluid_total = property(lambda self: self.num_fluid_nodes)

    @property
    def bulk_cells(self):
        return sum(s.bulk_cells for s in self.slabs)


class RK3DCSFDistributed(_SlabSetup, GatheredAnalysis):
    """One slab of the 3-D CSF model per rank of torch.distributed (launch: one process per GPU).  The face messages travel as device
    tensors under the nccl (= RCCL) backend and through host memory under gloo; three per step and face (phi, n, populations: 2 + 3 +
    10 doubles per cell of a plane, + 1 per tracer), batched per stage.  Opt-in (transport='ipc' | 'rccl' | 'auto'): the messages travel over a transport
    inside the library instead, and a call to step() is one lbmpm_rk3dcsf_step_slab -- no Python and no host synchronisation between the
    stages; torch.distributed then only carries the set-up (blobs, unique id, agreement).
    integrals() .. morphology(): analysis.GatheredAnalysis over the default group; nothing can be stale, so nothing is refreshed."""

    def __init__(self, is_domain, params=None, device=0, cuts=None, diagnostics=False, slab_factory=None, transport=None, tracers=None):
        """tracers = dict(<the keyword arguments of RK3DCSFSolver.configure_tracers>), the same on every rank: D3Q7 tracers, one more
        double per tracer and fluid cell of a plane in the population message (configured before the transport connects).
        slab_factory: tests/test_slab_cpu.py puts a host stand-in with the library's stage / face calls in the solver's place (attribute
        on_host: its buffers are host tensors) to run this class's orchestration under gloo without a GPU.
        transport: None or 'torch' (default) -- the messages through torch.distributed, from Python, after every stage; 'ipc' | 'rccl' --
        that in-library transport, which must connect and pass its probe on every rank, else RuntimeError on every rank; 'auto' -- ipc
        (then rccl under the nccl backend) where every rank connects and passes the probe, else 'torch'.  What set-up tried: transport_log."""
        import os
        import torch
        import torch.distributed as dist
        self._torch, self._dist = torch, dist
        self.rank, self.world = dist.get_rank(), dist.get_world_size()
        dom = np.ascontiguousarray(is_domain, dtype=np.uint8)
        self.shape = dom.shape
        self.nz = dom.shape[0]
        self.group = None
        self.periodic_z = _periodic_params(params)
        # (default: equal shares of the fluid cells -- the same cuts on every rank, they hold the same mask)
        self.cuts = list(cuts) if cuts is not None else slab_cuts(self.nz, self.world, weights=(dom.reshape(self.nz, -1) == 1).sum(axis=1) + 1.0e-3)
        if len(self.cuts) != self.world + 1:
            raise ValueError("one slab per rank: %d cuts for %d ranks" % (len(self.cuts) - 1, self.world))
        self.geo = _SlabGeometry(self.nz, self.cuts[self.rank], self.cuts[self.rank + 1])
        self.z0, self.nzl = self.geo.z0, self.geo.z1 - self.geo.z0
        more = {} if tracers is None else dict(tracers=tracers)
        self.slab = (slab_factory or RK3DCSFSolver)(self.geo.cut(dom), params, device=device, diagnostics=diagnostics, slab=self.geo.slab, **more)
        self.params = self.slab.params
        self.num_tracers = 0 if tracers is None else int(dict(tracers).get("num_tracers", 1))
        self._on_device = dist.get_backend() == "nccl"
        dev = self._dev = torch.device("cpu") if getattr(slab_factory, "on_host", False) else torch.device("cuda", int(device))
        self._t_stage, self._t_msg, self._t_count = [0.0] * 3, [0.0] * 3, [0] * 3
        self._buf = {}
        for face in (0, 1):
            if self.geo.ghost[face]:
                for msg in (MSG_PDF, MSG_PHI, MSG_NORMAL):
                    n, m = self.slab.face_doubles(msg, face), self.slab.face_doubles_in(msg, face)
                    self._buf[(msg, face)] = (torch.empty(n, dtype=torch.float64, device=dev), torch.empty(m, dtype=torch.float64, device=dev))
        # every rank cuts its slab out of the same undivided lattice
        import zlib
        mine = torch.tensor([zlib.crc32(dom.tobytes())] + list(dom.shape) + self.cuts + [self.num_tracers], dtype=torch.int64)
        every = [torch.zeros_like(mine) for _ in range(self.world)]
        if self._on_device:
            every = [t.to(dev) for t in every]
            mine = mine.to(dev)
        dist.all_gather(every, mine)
        for r in range(self.world):
            if not bool((every[r] == mine).all()):
                raise ValueError("rank %d holds another lattice, other cuts or another number of tracers than rank %d" % (r, self.rank))
        want = "torch" if transport is None else transport
        if want not in ("torch", "auto", "ipc", "rccl"):
            raise ValueError("transport must be None, 'torch', 'auto', 'ipc' or 'rccl'")
        self._library = False
        # what set-up tried, in order: [{"transport": kind, "ok": bool, "why": text}]
        self.transport_log = []
        self.deadline_s = float(os.environ.get("LBMPM_SLAB_DEADLINE_S", "120"))      # the watchdog of sync() in library mode
        if self.world > 1 and want != "torch":
            self._connect(want)

    slabs = property(lambda self: [self.slab])

    def _pairs(self):
        return [(self.slab, self.geo)]

    def tracer_wall_integrals(self):
        """collective: rank 0 returns the integrals.TracerWallIntegrals of the whole lattice ([nz][nT][4]), the others None"""
        from .integrals import TracerWallIntegrals
        t = self.gather(self.slab.tracer_wall_integrals().planes)
        return None if t is None else TracerWallIntegrals(t, self.shape[2], self.shape[1])

    def _face_sizes(self):
        """doubles of the three messages (LBMPM_CSF_MSG_* order) this slab sends / expects through either face"""
        s = self.slab
        return dict(down=[s.face_doubles(m, 0) for m in range(3)], up=[s.face_doubles(m, 1) for m in range(3)],
                    from_below=[s.face_doubles_in(m, 0) for m in range(3)], from_above=[s.face_doubles_in(m, 1) for m in range(3)])

    def _connect(self, want):
        """Connect the in-library transport around the ring of slabs -- the low neighbour is rank - 1, the high one rank + 1 (mod world;
        with two ranks the same) -- by slab.connect_in_library: every rank takes the same decision, every candidate is probed under a
        deadline and leaves its verdict in self.transport_log"""
        if self._dev.type == "cuda":
            self._torch.cuda.set_device(self._dev)       # (collectives of the nccl backend run on the current device)
        self._library = connect_in_library(self.slab, self.rank, self.world, None, want, True, self._face_sizes, self.transport_log,
                                           messages="6 x 3")[0] is not None

    @property
    def transport(self):
        """'torch' (the messages through torch.distributed from Python) or the in-library transport the slab steps with"""
        return self.slab.transport if self._library else "torch"

    def close(self):
        self.slab.close()

    def _exchange(self, msg):
        torch, dist = self._torch, self._dist
        if self.world == 1:
            return
        lo_peer, hi_peer = (self.rank - 1) % self.world, (self.rank + 1) % self.world
        import time
        t0 = time.perf_counter()
        for face in (0, 1):
            self.slab.face_pack(msg, face, self._buf[(msg, face)][0].data_ptr())
        self.slab.sync()
        t1 = time.perf_counter()
        staged = []
        if self._on_device:
            # (no tags under NCCL: between two ranks the messages pair up in the order posted -- with two ranks both faces join the same
            # pair, so every rank sends low, high and receives high, low: the peer's low-face message is what arrives through my high face)
            ops = [dist.P2POp(dist.isend, self._buf[(msg, 0)][0], lo_peer), dist.P2POp(dist.isend, self._buf[(msg, 1)][0], hi_peer),
                   dist.P2POp(dist.irecv, self._buf[(msg, 1)][1], hi_peer), dist.P2POp(dist.irecv, self._buf[(msg, 0)][1], lo_peer)]
            reqs = dist.batch_isend_irecv(ops)
        else:
            reqs = []
            for face, peer in ((0, lo_peer), (1, hi_peer)):
                out, inn = self._buf[(msg, face)]
                o = out.cpu()
                i = torch.empty(inn.shape, dtype=inn.dtype)
                staged.append((inn, i))
                # tag = the face of the RECEIVER the message enters through
                reqs += [dist.isend(o, peer, tag=1 - face), dist.irecv(i, peer, tag=face)]
        for w in reqs:
            w.wait()
        for inn, i in staged:
            inn.copy_(i)
        if self._dev.type == "cuda":
            # the messages are in the buffers before the library's stream takes them; torch's stream only -- the bulk's collision keeps
            # running on the library's second stream while phi and n travel
            torch.cuda.current_stream(self._dev).synchronize()
        for face in (0, 1):
            self.slab.face_unpack(msg, face, self._buf[(msg, face)][1].data_ptr())
        t2 = time.perf_counter()
        # host clock: [stage's launches on the first stream + pack] until they have run | the message (both faces) until it is unpacked
        k = _AFTER_STAGE.index(msg)
        self._t_stage[k] += t1 - t0
        self._t_msg[k] += t2 - t1
        self._t_count[k] += 1

    def timing(self, reset=True):
        """per step and stage, on this rank's host clock (ms): 'wait_stage' = from the stage's call to the moment its launches on the first
        stream and the pack have run (the bulk's collision on the second stream is not waited for before stage 2), 'message' = from there
        until both faces' messages are unpacked; names of the stages' messages: phi, normal, populations"""
        n = [max(1, c) for c in self._t_count]
        out = dict(steps=int(self._t_count[2]), wait_stage_ms=[round(1e3 * t / c, 4) for t, c in zip(self._t_stage, n)],
                   message_ms=[round(1e3 * t / c, 4) for t, c in zip(self._t_msg, n)], messages=["phi", "normal", "populations"],
                   bytes_per_face=[8 * self.slab.face_doubles(m, 1) for m in _AFTER_STAGE], planes=[self.z0, self.z0 + self.nzl])
        if reset:
            self._t_stage, self._t_msg, self._t_count = [0.0] * 3, [0.0] * 3, [0] * 3
        return out

    def step(self, nsteps=1):
        if self.world == 1:
            return self.slab.step(nsteps)
        if self._library:
            return self.slab.step_slab(nsteps)             # enqueued: sync() waits for it
        for _ in range(int(nsteps)):
            for stage in range(3):
                self.slab.stage(stage)
                self._exchange(_AFTER_STAGE[stage])       # (its clock starts right after the stage's launches are queued)

    def sync(self):
        """in library mode under the watchdog (LBMPM_SLAB_DEADLINE_S seconds without a step coming through): a neighbour that stopped
        answering raises LbmpmError (status LBMPM_ERR_TIMEOUT) instead of hanging this rank"""
        if self._library:
            self.slab.sync(deadline_s=self.deadline_s)
        else:
            self.slab.sync()

    def tracer_integrals(self):
        """collective: rank 0 returns the integrals.TracerIntegrals of the whole lattice ([nz][nT][9]: axis 0 is z, so gather() stacks the
        ranks' tables), the others None"""
        from .integrals import TracerIntegrals
        t = self.gather(self.slab.tracer_integrals().planes)
        return None if t is None else TracerIntegrals(t, self.shape[2], self.shape[1])

    def gather(self, a):
        """rank 0: the ranks' planes stacked along z (None elsewhere); slab.gather_planes"""
        from .slab import gather_planes
        parts = [(self.cuts[r], self.cuts[r + 1] - self.cuts[r]) for r in range(self.world)]
        return gather_planes(a, parts, self.rank, self.world, device=self.device_index)

    device_index = property(lambda self: self._dev.index)
    ny = property(lambda self: self.shape[1])
    nx = property(lambda self: self.shape[2])
