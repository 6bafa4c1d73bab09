"""Two points A and B of every fused solver's parameter space, off the values of the shipped ini files, and what the tests around them
share: the small lattices, the oracle runs, the list of compared fields.

The shape tests (test_ragged_sizes_gpu.py and friends) sit on the ini files' values.  There beta = 1, solid phi = 1, AkR = AkB, the 3-D
CSF rates are pairwise equal, one colour's inlet velocity is 0: a kernel that hard-codes such a value, drops the factor, or swaps two fields
passes them all.  At A and B every numeric parameter differs from its default, A differs from B, and the two members of every colour
pair differ from each other.  tests/test_param_points_cpu.py proves on the oracles that each value matters by at least 1000 x the GPU
tolerance (and that the oracles are well conditioned there); tests/test_param_points_gpu.py holds every kernel instance to the oracle
at both points.

A table (one per solver):
  defaults     the numeric keys of the solver's DEFAULT_PARAMS (checked against it by the CPU module)
  A, B         the two points
  pairs        colour pairs (R member, B member)
  degenerate   pairs the MODEL reads only through their sum or mean, with the reference line that shows it: (R, B, why)
  live         {parameter: instance}  the instance in which the parameter is read, where that is not `base`
  base         the instance (relaxation, boundary kinds, ...) of the sensitivity runs
  instances    the instances the GPU module compares (a pairwise cover of the instance axes within what the solver accepts)
  fields       {ctypes config field: the parameters it is made of}, for the completeness check
The table of the 2-D tracers (rk2d-tr) holds beside the flow rows of rk2d-csf:
  tracer       the tracer rows -- defaults, A, B, fields, the keys of transportsetup.ini -- of RK2DSolver.configure_tracers; a row moves
               as "tr_" + keyword through params()
  axes         the instance axes that are no flow parameter: tracer set, ends, lattice
  sensed       the fields a sensitivity run measures (the concentrations)
"""
import numpy as np

from helpers import rel_err

TOL_2D, TOL_3D = 1e-9, 1e-10
STEPS = 10                       # compared after step 1 and after step STEPS
CRISP = 2.0 ** -51               # the library's "one colour alone" rule of the 3-D CSF model (tests/test_rk3d_csf_gpu.py)

# ------------------------------------------------------------------------------------------------ tables
_CSF_DEGENERATE_2D = [("vyR", "vyB", "the CSF loop has one inlet velocity, specificVY = velocityYB + velocityYR (RKD2Q9.py:1300, constantTotalVelocityInlet)"),
                      ("rhoRL", "rhoBL", "the CSF loop's outlet holds the total density, totalPressure = densityRhoBL + densityRhoRL (RKD2Q9.py:1344, "
                                         "calConstPressureLowerGPUTotal)")]

RK2D_CSF = dict(
    name="rk2d-csf", tol=TOL_2D,
    defaults=dict(sigma=0.1, theta=60.0, beta=0.7, delta=0.98, tauR=1.0, tauB=1.0, vyR=-1.0e-4, vyB=0.0, rhoBH=5e-8, rhoRH=1.00536, rhoBL=1.0,
                  rhoRL=5e-8),
    A=dict(sigma=0.07, theta=72.0, beta=0.65, delta=0.9, tauR=0.85, tauB=1.15, vyR=-3.0e-4, vyB=-2.0e-4, rhoRH=1.02, rhoBH=0.03, rhoBL=0.97,
           rhoRL=0.02),
    B=dict(sigma=0.13, theta=48.0, beta=0.6, delta=0.95, tauR=1.2, tauB=0.8, vyR=-5.0e-4, vyB=1.0e-4, rhoRH=0.99, rhoBH=0.04, rhoBL=1.01,
           rhoRL=0.01),
    pairs=[("tauR", "tauB"), ("vyR", "vyB"), ("rhoRH", "rhoBH"), ("rhoRL", "rhoBL")],
    degenerate=_CSF_DEGENERATE_2D,
    base=dict(relax="MRT", wetting=2, tautype=2, inlet="Neumann", outlet="Dirichlet"),
    live=dict(rhoRH=dict(inlet="Dirichlet"), rhoBH=dict(inlet="Dirichlet")),
    categorical=dict(relax=("SRT", "MRT"), wetting=(1, 2), tautype=(1, 2), inlet=("Neumann", "Dirichlet"), outlet=("Dirichlet", "Convective")),
    fields=dict(surface_tension=["sigma"], contact_angle_deg=["theta"], wetting_type=["wetting"], beta=["beta"], delta=["delta"], tau_r=["tauR"],
                tau_b=["tauB"], tau_type=["tautype"], relaxation=["relax"], inlet_type=["inlet"], outlet_type=["outlet"],
                inlet_velocity_y=["vyR", "vyB"], inlet_rho_r=["rhoRH"], inlet_rho_b=["rhoBH"], outlet_rho_total=["rhoRL", "rhoBL"]),
)

_AK_DEGENERATE = "the perturbation term carries (AkR + AkB) * 0.5 (AcceleratedRKGPU2D.py:1235, calRKCollision23GPUNew)"

RK2D_PERT = dict(
    name="rk2d-pert", tol=TOL_2D,
    defaults=dict(beta=0.7, tauR=1.0, tauB=1.0, vyR=-1.0e-4, vyB=0.0, rhoBL=1.0, rhoRL=5e-8, rhoBH=5e-8, rhoRH=1.00536),
    # AkR, AkB, solidPhi have no default in RK2DSolver (perturbation=dict(...)); the reference ini's are 7e-3, 7e-3 and 1
    extra_defaults=dict(AkR=7.0e-3, AkB=7.0e-3, solidPhi=1.0),
    A=dict(beta=0.9, tauR=0.85, tauB=1.15, vyR=3.0e-4, vyB=-4.0e-4, rhoBL=0.97, rhoRL=0.04, rhoRH=0.98, rhoBH=0.05, AkR=6.0e-3, AkB=9.0e-3,
           solidPhi=0.7),
    B=dict(beta=0.8, tauR=1.2, tauB=0.8, vyR=-2.0e-4, vyB=-6.0e-4, rhoBL=1.02, rhoRL=0.02, rhoRH=1.01, rhoBH=0.02, AkR=8.0e-3, AkB=5.0e-3,
           solidPhi=0.4),
    # (rhoRH + rhoBH is not the lattice's 1.05: with the pressure inlet at the density that is there, nothing moves in step 1 and the
    # velocity of that step is round-off without a scale)
    pairs=[("tauR", "tauB"), ("vyR", "vyB"), ("rhoRL", "rhoBL"), ("rhoRH", "rhoBH"), ("AkR", "AkB")],
    degenerate=[("AkR", "AkB", _AK_DEGENERATE)],
    base=dict(relax="MRT", inlet="Neumann", outlet="Dirichlet"),
    # the oracle of the perturbation loop (oracle/rk_pert_oracle.c) states the velocity inlet and the pressure outlet.  The other boundary
    # pairs are held to oracle/rk3d_oracle.c on a y-uniform lattice with the projection-exact recolouring weights, which IS the 2-D loop
    # (tests/test_rk3d_reduction.py) -- with SRT: the D3Q19 moment basis does not project onto the D2Q9 one
    live=dict(rhoRH=dict(relax="SRT", inlet="Dirichlet"), rhoBH=dict(relax="SRT", inlet="Dirichlet")),
    categorical=dict(relax=("SRT", "MRT"), inlet=("Neumann", "Dirichlet"), outlet=("Dirichlet", "Convective")),
    # keys of RK2DSolver's DEFAULT_PARAMS the perturbation step does not read (the GPU module proves it: bit-equal runs): its relaxation
    # time is harmonic in phi without a delta window (A:1144-1145), it has no tension coefficient, no contact angle and no wetting rule
    unread=("sigma", "theta", "delta", "wetting", "tautype"),
    fields=dict(ak_r=["AkR"], ak_b=["AkB"], solid_phi=["solidPhi"], inlet_velocity_y_r=["vyR"], inlet_velocity_y_b=["vyB"], outlet_rho_r=["rhoRL"],
                outlet_rho_b=["rhoBL"]),
)

_SC_FIELDS = dict(model=["inter"], relaxation=["relax"], tau=["tau0", "tau1"], g_fluid=["G"], g_solid=["Gs0", "Gs1"], outlet_type=["outlet"],
                  inlet_velocity_y=["vy0", "vy1"], force_scheme=["scheme"], inlet_method=["method"])
_SC_DEFAULTS = dict(tau0=1.0, tau1=1.0, G=0.20, Gs0=-0.14, Gs1=0.14, vy0=0.0, vy1=-5.03e-4)
_SC_PAIRS = [("tau0", "tau1"), ("Gs0", "Gs1"), ("vy0", "vy1")]

SC2D_EFS = dict(
    name="sc2d-efs", tol=TOL_2D, defaults=_SC_DEFAULTS,
    A=dict(tau0=0.9, tau1=1.15, G=0.17, Gs0=-0.11, Gs1=0.16, vy0=-2.0e-4, vy1=-7.0e-4),
    B=dict(tau0=1.2, tau1=0.85, G=0.23, Gs0=-0.17, Gs1=0.10, vy0=3.0e-4, vy1=-3.0e-4),
    pairs=_SC_PAIRS, degenerate=[],
    base=dict(inter="EFS", relax="SRT", scheme=4, method="ZouHe", outlet="Dirichlet"), live={},
    categorical=dict(inter=("EFS", "ShanChen"), relax=("SRT", "MRT"), scheme=(4, 8, 10), method=("ZouHe", "Chang"),
                     outlet=("Dirichlet", "Convective", "Freeflow")),
    fields=_SC_FIELDS,
)

SC2D_ORIGINAL = dict(
    name="sc2d-original", tol=TOL_2D, defaults=_SC_DEFAULTS,
    # (the original Shan-Chen loop separates the fluids at G ~ 2.6, Gs ~ +-0.2: tests/test_ragged_sizes_gpu.py SC_ORIGINAL)
    A=dict(tau0=0.9, tau1=1.15, G=2.3, Gs0=-0.25, Gs1=0.15, vy0=-2.0e-4, vy1=-7.0e-4),
    B=dict(tau0=1.2, tau1=0.85, G=2.8, Gs0=-0.15, Gs1=0.24, vy0=3.0e-4, vy1=-3.0e-4),
    pairs=_SC_PAIRS, degenerate=[],
    base=dict(inter="ShanChen", relax="SRT", scheme=4, method="ZouHe", outlet="Dirichlet"), live={},
    categorical=SC2D_EFS["categorical"], fields=_SC_FIELDS,
)

RK3D = dict(
    name="rk3d", tol=TOL_3D,
    defaults=dict(AkR=7.0e-3, AkB=7.0e-3, beta=1.0, tauR=1.0, tauB=1.0, SolidRhoR=0.7, SolidRhoB=0.0, velocityZR=0.0, velocityZB=-1.0e-4,
                  densityRL=1.0e-8, densityBL=1.0, recolor_axis=0.0, recolor_diag=0.0, densityRH=1.0e-8, densityBH=1.0),
    A=dict(AkR=6.0e-3, AkB=9.0e-3, beta=0.9, tauR=0.9, tauB=1.1, SolidRhoR=0.6, SolidRhoB=0.1, velocityZR=5.0e-4, velocityZB=-3.0e-4,
           densityRL=0.05, densityBL=0.97, recolor_axis=0.06, recolor_diag=0.021, densityRH=0.04, densityBH=1.02),
    B=dict(AkR=8.0e-3, AkB=5.0e-3, beta=0.8, tauR=1.15, tauB=0.85, SolidRhoR=0.5, SolidRhoB=0.2, velocityZR=-2.0e-4, velocityZB=-6.0e-4,
           densityRL=0.03, densityBL=1.01, recolor_axis=0.05, recolor_diag=0.018, densityRH=0.07, densityBH=0.98),
    pairs=[("AkR", "AkB"), ("tauR", "tauB"), ("SolidRhoR", "SolidRhoB"), ("velocityZR", "velocityZB"), ("densityRL", "densityBL"),
           ("densityRH", "densityBH")],
    degenerate=[("AkR", "AkB", _AK_DEGENERATE + ", carried to D3Q19")],
    base=dict(relax="MRT", inlet="Neumann", outlet="Dirichlet"),
    live=dict(densityRH=dict(inlet="Dirichlet"), densityBH=dict(inlet="Dirichlet")),
    categorical=dict(relax=("SRT", "MRT"), inlet=("Neumann", "Dirichlet"), outlet=("Dirichlet", "Convective")),
    fields=dict(ak_r=["AkR"], ak_b=["AkB"], beta=["beta"], tau_r=["tauR"], tau_b=["tauB"], solid_phi=["SolidRhoR", "SolidRhoB"],
                inlet_vz_r=["velocityZR"], inlet_vz_b=["velocityZB"], outlet_rho_r=["densityRL"], outlet_rho_b=["densityBL"], relaxation=["relax"],
                inlet_type=["inlet"], recolor_axis=["recolor_axis"], recolor_diag=["recolor_diag"], inlet_rho_r=["densityRH"],
                inlet_rho_b=["densityBH"], outlet_type=["outlet"]),
)

RK3D_CSF = dict(
    name="rk3dcsf", tol=TOL_3D,
    defaults=dict(sigma=0.1, theta=60.0, beta=0.7, delta=0.98, tauR=1.0, tauB=1.0, velocityZR=-1.0e-4, velocityZB=0.0, densityBH=5e-8,
                  densityRH=1.00536, densityBL=1.0, densityRL=5e-8, rates=(1.19, 1.4, 1.2, 1.4, 1.2, 0.0)),
    # rates = (s_e, s_eps, s_q, s_pi, s_m, the conserved moments' rate): six pairwise distinct values
    A=dict(sigma=0.07, theta=50.0, beta=0.65, delta=0.9, tauR=0.9, tauB=0.75, velocityZR=-3.0e-4, velocityZB=-2.0e-4, densityRH=1.02,
           densityBH=0.03, densityBL=0.97, densityRL=0.02, rates=(1.1, 1.5, 1.25, 1.35, 1.7, 0.0)),
    B=dict(sigma=0.13, theta=70.0, beta=0.6, delta=0.95, tauR=1.1, tauB=0.85, velocityZR=-5.0e-4, velocityZB=1.0e-4, densityRH=0.99,
           densityBH=0.04, densityBL=1.01, densityRL=0.01, rates=(1.3, 1.2, 1.6, 1.45, 1.05, 0.0)),
    pairs=[("tauR", "tauB"), ("velocityZR", "velocityZB"), ("densityRH", "densityBH"), ("densityRL", "densityBL")],
    degenerate=[("velocityZR", "velocityZB", _CSF_DEGENERATE_2D[0][2] + ", z for y"), ("densityRL", "densityBL", _CSF_DEGENERATE_2D[1][2] + ", z for y")],
    base=dict(relax="MRT", tautype=2, wetting=2, inlet="Neumann", outlet="Dirichlet", variant=0),
    live=dict(densityRH=dict(inlet="Dirichlet"), densityBH=dict(inlet="Dirichlet")),
    categorical=dict(relax=("SRT", "MRT"), variant=(0, 1), inlet=("Neumann", "Dirichlet"), outlet=("Dirichlet", "Convective"), tautype=(1, 2),
                     wetting=(0, 2)),
    fields=dict(surface_tension=["sigma"], contact_angle_deg=["theta"], beta=["beta"], delta=["delta"], tau_r=["tauR"], tau_b=["tauB"],
                inlet_velocity_z=["velocityZR", "velocityZB"], inlet_rho_r=["densityRH"], inlet_rho_b=["densityBH"],
                outlet_rho_total=["densityRL", "densityBL"], wetting_type=["wetting"], tau_type=["tautype"], relaxation=["relax"],
                inlet_type=["inlet"], outlet_type=["outlet"], mrt_rates=["rates"]),
)
RATE_NAMES = ("s_e", "s_eps", "s_q", "s_pi", "s_m", "conserved")
RATE_SWAPS = ((0, 1), (1, 3), (2, 4))          # s_e <-> s_eps, s_eps <-> s_pi, s_q <-> s_m

# The 2-D CSF step with D2Q5 tracers fused into it (launch_fused_tracer, csrc/rk2d.hip): its own instantiations of the fused tile.  The
# flow rows are those of RK2D_CSF.  The tracer rows: one per keyword of RK2DSolver.configure_tracers / field of lbmpm_tracer_config; a
# per-tracer list holds four pairwise distinct values (the first n are used), dXY != dYX, crit lies strictly between the densities the
# lattices hold (0 and ~1), away from 0.5.  No two tracer parameters are read through a combination (oracle/tr_oracle.c: S_T holds each
# diffusion entry in its own slot, beta and the inlet value enter once each, the reaction source spreads k C_0 C_1 with J_0 = diffJ on
# the rest population and (1 - diffJ) / 4 on the others), so the table declares no tracer degeneracy.
TRACER = dict(
    defaults=dict(diffX=1. / 6., diffY=1. / 6., beta=1.0, inlet_conc=1.0, diffJ=1. / 3., dXY=0.0, dYX=0.0, crit=0.5, reaction_rate=0.0),
    per_tracer=("diffX", "diffY", "beta", "inlet_conc", "diffJ"),
    A=dict(diffX=(0.12, 0.2, 0.15, 0.09), diffY=(0.21, 0.1, 0.14, 0.18), beta=(0.8, 0.55, 0.35, 0.65), inlet_conc=(0.9, 0.3, 0.6, 0.45),
           diffJ=(0.3, 0.4, 0.25, 0.36), dXY=0.015, dYX=0.03, crit=0.35, reaction_rate=0.05),
    B=dict(diffX=(0.1, 0.18, 0.13, 0.22), diffY=(0.19, 0.08, 0.16, 0.12), beta=(0.7, 0.45, 0.9, 0.25), inlet_conc=(0.8, 0.2, 0.5, 0.7),
           diffJ=(0.28, 0.38, 0.45, 0.22), dXY=-0.02, dYX=0.01, crit=0.65, reaction_rate=0.08),
    # the reaction couples exactly three tracers (lbmpm_rk2d_tracer_configure refuses a rate with another number): diffJ and the rate are
    # read with the tracer set 3 only, the fourth value of a list with the tracer set 4 only; inlet_conc with dirichlet_inlet only
    fields=dict(num_tracers=["tracers"], diffusion_x=["diffX", "tracers"], diffusion_y=["diffY", "tracers"], diffusion_xy=["dXY"], diffusion_yx=["dYX"],
                beta_interface=["beta", "tracers"], criteria_rho=["crit"], inlet_concentration=["inlet_conc", "tracers"], dirichlet_inlet=["ends"],
                free_outlet=["ends"], reaction_rate=["reaction_rate", "tracers"], diffusion_j=["diffJ", "tracers"]),
    # keys of transportsetup.ini (openlbmpm_amd/config.read_transport) -> the fields they reach through Transport2DRK.  BetaInterface is one
    # value for all tracers; DiffusionXY / DiffusionYX use their first entry; crit has no key (the reference's 0.5)
    ini=dict(DiffusionX="diffusion_x", DiffusionY="diffusion_y", DiffusionXY="diffusion_xy", DiffusionYX="diffusion_yx", BetaInterface="beta_interface",
             ConcentrationInlet="inlet_concentration", DiffusionJ="diffusion_j", ReactionRate="reaction_rate", NumberTracers="num_tracers",
             InletType="dirichlet_inlet", OutletType="free_outlet"),
)
# instance axes beside the flow's: the tracer set (3 = three tracers with the reaction), the ends (dirichlet_inlet, free_outlet), the
# lattice ('tall': the one launch with both TR copies; 'short': the single-launch branch of launch_fused_tracer)
TRACER_AXES = dict(tracers=(1, 2, 3, 4), ends=((True, True), (False, False), (True, False), (False, True)), lattice=("tall", "short"))

RK2D_TR = dict(
    RK2D_CSF, name="rk2d-tr", tracer=TRACER, axes=TRACER_AXES,
    base=dict(RK2D_CSF["base"], tracers=3, ends=(True, True), lattice="tall"),
    # (the base holds three tracers with the reaction and both ends on: every tracer row is read there but the lists' fourth values)
    live=dict(RK2D_CSF["live"], tr_diffJ=dict(tracers=3), tr_reaction_rate=dict(tracers=3), tr_inlet_conc=dict(ends=(True, True))),
    # what a sensitivity run of this table measures: the concentrations alone (a flow parameter shows in them through the flow they ride)
    sensed=("C0", "C1", "C2", "C3"),
)
# a tracer row is named "tr_" + its keyword of configure_tracers (the flow has a beta of its own): params(RK2D_TR, "A", tr_beta=(...))
RK2D_TR["fields"] = dict(RK2D_CSF["fields"], **{f: ["tr_" + k if k in TRACER["defaults"] else k for k in ps] for f, ps in TRACER["fields"].items()})

TABLES = {t["name"]: t for t in (RK2D_CSF, RK2D_PERT, SC2D_EFS, SC2D_ORIGINAL, RK3D, RK3D_CSF, RK2D_TR)}

# config fields no table has a row for, and why
EXCLUDED_FIELDS = dict(nx="size", ny="size", nz="size", nz_local="size", nz_global="size", z_offset="size", slab_z0="size", global_nz="size",
                       device="device", variant="kernel variant: an instance axis, not a parameter", reserved="reserved",
                       ghost_lo="ghost-plane count", ghost_hi="ghost-plane count",
                       bulk_epsilon="opt-in approximation with its own test (test_rk3d_csf_gpu.py::test_the_opt_in_cut_of_a_colours_tail)")


def _cover(axes, rows):
    """instances from rows of indices into the axes' values"""
    names = list(axes)
    return [{n: axes[n][r[i]] for i, n in enumerate(names)} for r in rows]


# six binary axes, every pair of values of every two axes in some row: the zero row + the five rows of six distinct weight-3 columns
_CA6 = [(0, 0, 0, 0, 0, 0), (1, 1, 1, 1, 1, 1), (1, 1, 1, 0, 0, 0), (1, 0, 0, 1, 1, 0), (0, 1, 0, 1, 0, 1), (0, 0, 1, 0, 1, 1)]

RK2D_CSF["instances"] = _cover(dict(variant=(0, 1), relax=("SRT", "MRT"), wetting=(1, 2), tautype=(1, 2), inlet=("Neumann", "Dirichlet"),
                                    outlet=("Dirichlet", "Convective")), _CA6)


def _oa16():
    """16 rows over two four-valued and six binary axes in which every two axes meet in every pair of their values: the orthogonal array
    of GF(4) -- columns t, e, t + e, t + a e (a a generator, addition = XOR of the two bits, a (x1 x0) = (x1 ^ x0, x1)) -- whose last two
    columns are split into the three binary ones x0, x1, x0 ^ x1 each.  Row = (six binary indices, t, e); the first binary column is
    t0 ^ e0, the last x0 ^ x1 of t + a e."""
    rows = []
    for t in range(4):
        for e in range(4):
            c, d = t ^ e, t ^ ((((e >> 1) ^ e) & 1) << 1 | (e >> 1))
            rows.append((c & 1, c >> 1, (c ^ (c >> 1)) & 1, d & 1, d >> 1, (d ^ (d >> 1)) & 1, t, e))
    return rows


# relax, wetting, tautype, inlet, outlet, lattice are the binary axes; tracer set and ends the four-valued ones.  Every pair of values
# of every two axes is in some row (tests/test_param_points_cpu.py checks it), so in particular (relax, lattice), (relax, outlet) and
# (relax, tracer set).  The solver accepts every row: the reaction rides the tracer set 3, both lattices keep the rows 0 .. 3 free.
RK2D_TR["instances"] = _cover(dict(relax=("SRT", "MRT"), wetting=(1, 2), tautype=(1, 2), inlet=("Neumann", "Dirichlet"),
                                   outlet=("Dirichlet", "Convective"), lattice=TRACER_AXES["lattice"], tracers=TRACER_AXES["tracers"],
                                   ends=TRACER_AXES["ends"]), _oa16())
RK2D_PERT["instances"] = [dict(relax="SRT", inlet="Neumann", outlet="Dirichlet"), dict(relax="MRT", inlet="Neumann", outlet="Dirichlet"),
                          dict(relax="SRT", inlet="Dirichlet", outlet="Dirichlet"), dict(relax="SRT", inlet="Neumann", outlet="Convective"),
                          dict(relax="SRT", inlet="Dirichlet", outlet="Convective")]
# what the solver and its oracle accept: 'Freeflow' with the explicit forcing and SRT only, ExplicitScheme 8 / 10 with the explicit forcing
# only, 'Chang' with scheme 4 only, the original loop with SRT only (lbmpm_sc2d_create)
SC2D_EFS["instances"] = [dict(inter="EFS", relax="SRT", scheme=4, method="ZouHe", outlet="Dirichlet"),
                         dict(inter="EFS", relax="MRT", scheme=8, method="ZouHe", outlet="Convective"),
                         dict(inter="EFS", relax="SRT", scheme=10, method="ZouHe", outlet="Dirichlet"),
                         dict(inter="EFS", relax="SRT", scheme=8, method="ZouHe", outlet="Freeflow"),
                         dict(inter="EFS", relax="MRT", scheme=4, method="Chang", outlet="Dirichlet"),
                         dict(inter="EFS", relax="MRT", scheme=10, method="ZouHe", outlet="Dirichlet"),
                         dict(inter="EFS", relax="SRT", scheme=4, method="Chang", outlet="Convective"),
                         dict(inter="EFS", relax="MRT", scheme=4, method="ZouHe", outlet="Convective")]
SC2D_ORIGINAL["instances"] = [dict(inter="ShanChen", relax="SRT", scheme=4, method="ZouHe", outlet="Dirichlet"),
                              dict(inter="ShanChen", relax="SRT", scheme=4, method="Chang", outlet="Dirichlet"),
                              dict(inter="ShanChen", relax="SRT", scheme=4, method="Chang", outlet="Convective"),
                              dict(inter="ShanChen", relax="SRT", scheme=4, method="ZouHe", outlet="Convective")]
_VP = dict(inlet="Neumann", outlet="Dirichlet")          # velocity inlet + pressure outlet
_PC = dict(inlet="Dirichlet", outlet="Convective")       # pressure inlet + convective outlet
# (with the convective outlet the 38-value compact storage hands the lattice to the dense kernels, lbmpm_rk3d_create: its second instance
# is the pressure inlet with the pressure outlet)
_PP = dict(inlet="Dirichlet", outlet="Dirichlet")
# storage: q23 (23 values per cell; nx 64 the whole-segment instance, nx 70 the ragged one), dense, compact38 (nx a multiple of 64), and the
# split slab schedule of the q23 storage (three slabs through lbmpm_rk3d_step_slab)
RK3D["instances"] = [dict(storage=s, nx=nx, relax=r, **bc) for s, nx, picks in (
    ("q23", 64, (("SRT", _VP), ("MRT", _PC))), ("q23", 70, (("MRT", _VP), ("SRT", _PC))), ("dense", 70, (("SRT", _PC), ("MRT", _VP))),
    ("compact38", 64, (("MRT", _VP), ("SRT", _PP))), ("split", 70, (("MRT", _VP), ("SRT", _PC)))) for r, bc in picks]
RK3D_CSF["instances"] = _cover(dict(relax=("SRT", "MRT"), variant=(0, 1), inlet=("Neumann", "Dirichlet"), outlet=("Dirichlet", "Convective"),
                                    tautype=(1, 2), wetting=(0, 2)), _CA6)


def params(table, point, inst=None, **moved):
    """the parameter dict of `table` at `point` ('A' | 'B') in instance `inst` (default: the table's base), entries of `moved` replaced"""
    p = dict(table[point])
    p.update(table["base"] if inst is None else inst)
    if "tracer" in table:       # (entry "tr": the keyword arguments of configure_tracers at `point`, moved entries replaced)
        tr = {k[3:]: moved.pop(k) for k in list(moved) if k.startswith("tr_")}
        p.update(moved)
        p["tr"] = tracer_kwargs(table["tracer"], point, p["tracers"], p["ends"], **tr)
        return p
    p.update(moved)
    return p


def tracer_kwargs(tracer, point, nT, ends, **moved):
    """the keyword arguments of RK2DSolver.configure_tracers (and the tracer dict of oracle.tr.CoupledOracle) for nT tracers at `point` of
    the table `tracer`: the first nT values of every list; the reaction with three tracers only"""
    v = dict(tracer[point]); v.update(moved)
    kw = {k: tuple(v[k][:nT]) for k in tracer["per_tracer"]}
    kw.update(dXY=v["dXY"], dYX=v["dYX"], crit=v["crit"], reaction_rate=v["reaction_rate"] if nT == 3 else 0.0,
              dirichlet_inlet=bool(ends[0]), free_outlet=bool(ends[1]))
    return kw


def exact_shift(a, b):
    """(a + d, b - d) with the same rounded sum as (a, b): a pair moved with its sum (and mean) fixed bit for bit"""
    for k in range(1, 60):
        d = (abs(a) + abs(b)) * 2.0 ** -k
        a2, b2 = a + d, b - d
        if a2 != a and b2 != b and a2 + b2 == a + b and b2 + a2 == b + a:
            return a2, b2
    raise AssertionError("no exact shift for %r, %r" % (a, b))


# ------------------------------------------------------------------------------------------------ lattices
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def last_bit(a, seed_phase=0.0):
    """`a` rippled in the last bit (factor 1 + 1e-15 sin): the start of the conditioning runs"""
    idx = np.arange(a.size, dtype=np.float64).reshape(a.shape)
    return a * (1.0 + 1.0e-15 * np.sin(0.7 * idx + seed_phase))


def lattice_2d():
    """70 x 45: two tile columns (the second partial) and a partial tile row; discs of radius >= 3 and a ripple in the densities (no exact
    ties of the wetting rules, tests/test_ragged_sizes_gpu.py); the interface lies inside the porous image, across walls"""
    def make():
        from openlbmpm_amd.geometry import porous_disks, image_domain
        nx, ny, nbuf = 70, 45, 6
        img = porous_disks(nx, ny - 2 * nbuf, porosity=0.75, rmin=3.0, rmax=6.0, seed=nx + ny)
        dom = image_domain(img, nbuf, 0.5)
        assert dom.shape == (ny, nx)
        yy, xx = np.mgrid[0:ny, 0:nx]
        ripple = 1.0 + 1.0e-3 * np.sin(0.37 * xx + 0.11 * yy)
        fluid = dom == 1
        red = yy + 0.15 * xx < ny - 15
        return dom, np.where(fluid & red, 1.0, 0.0) * ripple, np.where(fluid & ~red, 1.0, 0.0) * ripple
    return _once("2d", make)


def lattice_2d_short():
    """70 x 20, the lattice of the single-launch branch of launch_fused_tracer (n_lo + n_hi >= tiles_y: ny <= 20 with 8-row tiles; see
    tracer_launch): the make of lattice_2d with 4 buffer rows on either side -- the rows 0 .. 3 and 16 .. 19 hold no solid (the convective
    outlet copies row 3 down, the boundary rows want none) -- and a 12-row porous image of six discs in between, across which the
    interface slants.
    The seed is chosen by the conditioning test of tests/test_param_points_cpu.py.  With the pressure inlet the colour front that leaves
    row 19 is uniform along x and meets the walls of row 15 three steps later; where a wall's normal is parallel to it, wetting rule 2
    divides by the sine of a vanishing angle (oracle/rk_oracle.c, rk_wetting2) and the oracle follows itself to 1e-8 only -- with most seeds
    that were tried, whatever the slant and the number of discs.  Seed 3 keeps every instance below 4e-13."""
    def make():
        from openlbmpm_amd.geometry import porous_disks, image_domain
        nx, ny, nbuf = 70, 20, 4
        img = porous_disks(nx, ny - 2 * nbuf, porosity=0.5, rmin=3.0, rmax=4.5, seed=3, max_disks=6)
        dom = image_domain(img, nbuf, 0.5)
        assert dom.shape == (ny, nx)
        yy, xx = np.mgrid[0:ny, 0:nx]
        ripple = 1.0 + 1.0e-3 * np.sin(0.37 * xx + 0.11 * yy)
        fluid = dom == 1
        red = yy + 0.1 * xx < ny - 7
        return dom, np.where(fluid & red, 1.0, 0.0) * ripple, np.where(fluid & ~red, 1.0, 0.0) * ripple
    return _once("2ds", make)


def lattice_tr(which):
    return {"tall": lattice_2d, "short": lattice_2d_short}[which]()


def concentrations(dom, nT):
    """[nT][ny][nx] initial concentrations that vary along x and along y and differ per tracer (a uniform field hides the diffusion tensor)"""
    yy, xx = np.mgrid[0:dom.shape[0], 0:dom.shape[1]]
    return np.stack([np.where(dom == 1, 0.3 + 0.1 * k + 0.2 * np.sin(0.29 * xx + 0.41 * yy + k) * np.cos(0.17 * xx - 0.23 * yy + 0.5 * k), 0.0)
                     for k in range(nT)])


def tracer_launch(ny, TH=8, H=3):
    """(n_lo, n_hi, tiles_y, single) of launch_fused_tracer (csrc/rk2d.hip) for a lattice of ny rows and tiles of TH rows: the tile rows
    from the bottom and from the top whose region (own rows + H rows of halo) holds one of the rows 0, 1, ny-2, ny-1, and whether they are
    all there are -- then one launch of rk2d_fused<., true, ., 1> does the step, else rk2d_fused_tracer with both copies of node_finish"""
    tiles_y = (ny + TH - 1) // TH
    n_lo = n_hi = 0
    for ty in range(tiles_y):
        if ty * TH - H <= 1:
            n_lo = ty + 1
        if ty * TH + TH - 1 + H >= ny - 2 and n_hi == 0:
            n_hi = tiles_y - ty
    return n_lo, n_hi, tiles_y, n_lo + n_hi >= tiles_y


def lattice_2d_mixed():
    """the 2-D lattice with both colours in every cell (perturbation and Shan-Chen runs: phi away from +-1, so beta, the solid phi and both
    colours' boundary values act from the first step)"""
    def make():
        dom, _, _ = lattice_2d()
        yy, xx = np.mgrid[0:dom.shape[0], 0:dom.shape[1]]
        w = 0.5 + 0.3 * np.sin(0.31 * xx + 0.47 * yy) * np.cos(0.13 * xx - 0.29 * yy)
        fluid = dom == 1
        return dom, np.where(fluid, w, 0.0), np.where(fluid, 1.05 - w, 0.0)
    return _once("2dm", make)


def lattice_sc():
    """the 2-D lattice for the Shan-Chen runs: both fluids in every cell, near the densities (1.0, 0.02) that the reference's pressure
    outlet hard-codes (ShanChenD2Q9.py O:555-585), rippled -- a start in pressure balance, so that |u| stays below 0.1 at G and Gs off their
    defaults; every fluid's inlet velocity, relaxation time and wall coupling acts on a density that is there"""
    def make():
        dom, _, _ = lattice_2d()
        yy, xx = np.mgrid[0:dom.shape[0], 0:dom.shape[1]]
        fluid = dom == 1
        return (dom, np.where(fluid, 1.0 * (1 + 0.01 * np.sin(0.31 * xx + 0.47 * yy)), 0.0),
                np.where(fluid, 0.02 * (1 + 0.3 * np.sin(0.23 * xx - 0.41 * yy)), 0.0))
    return _once("sc", make)


def sc_populations(dom, r0, r1):
    """populations [2][ny][nx][9] on the densities (r0, r1) that are no equilibrium at rest: the 'Chang' inlet reads the populations the last
    step left on its row only through o4 - 2 (o7 + o8), which is zero for f = w rho (tests/test_ragged_sizes_gpu.py::_populations)"""
    w = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)
    yy, xx = np.mgrid[0:dom.shape[0], 0:dom.shape[1]]
    f = np.empty((2,) + dom.shape + (9,))
    for k, r in enumerate((r0, r1)):
        for j in range(9):
            f[k, :, :, j] = w[j] * r * (1.0 + 1.0e-2 * np.sin(0.41 * xx + 0.23 * yy + j + 2 * k))
    return f


def lattice_3d(nx):
    """nx x 9 x 22 porous lattice without side walls, both colours in every cell: nx 64 the whole-segment and nx 70 the ragged instance of
    the 23-value storage, two row segments, rows that wrap, planes 0 .. 3 with one mask (the convective outlet copies plane 3 down)"""
    def make():
        from openlbmpm_amd.geometry import porous_spheres
        dom = porous_spheres(nx, 9, 22, porosity=0.72, rmin=2.0, rmax=4.0, seed=nx + 31, nbuf=4, walls=False)
        assert dom.shape == (22, 9, nx) and all(np.array_equal(dom[z], dom[3]) for z in range(3))
        zz, yy, xx = np.mgrid[0:22, 0:9, 0:nx]
        w = 0.5 + 0.3 * np.sin(0.31 * xx + 0.47 * yy + 0.23 * zz) * np.cos(0.17 * xx - 0.29 * zz)
        fluid = dom == 1
        return dom, np.where(fluid, w, 0.0), np.where(fluid, 1.05 - w, 0.0)
    return _once(("3d", nx), make)


def lattice_csf():
    from test_oracle_rk3d_csf import blob3
    return _once("csf", blob3)


def lattice_csf_slabs():
    """test_rk3d_csf_gpu._slab_case (restated: that module is a GPU module): a duct with obstacles and a slanted interface that cross the cuts"""
    def make():
        from openlbmpm_amd.RKColorGradientD3Q19 import duct
        nx, ny, nz = 22, 18, 44
        rng = np.random.default_rng(5)
        dom = duct(nx, ny, nz)
        for _ in range(7):
            z, y, x = rng.integers(5, nz - 9), rng.integers(2, ny - 5), rng.integers(2, nx - 6)
            dom[z:z + 4, y:y + 3, x:x + 4] = 0
        zz, yy, xx = np.mgrid[0:nz, 0:ny, 0:nx]
        fl = dom == 1
        red = zz + 0.3 * xx - 0.2 * yy < 0.55 * nz
        return dom, np.where(fl & red, 1.0, 0.0), np.where(fl & ~red, 1.0, 0.0)
    return _once("csf-slabs", make)


# ------------------------------------------------------------------------------------------------ compared fields
# scalars, vectors (components measured against the vector's largest magnitude), and K (where the colour gradient is alive)
COMPARED = {
    "rk2d-csf": dict(scalars=("fR", "fB", "rhoR", "rhoB", "phi"), vectors=(("vx", "vy"), ("Gx", "Gy"), ("Fx", "Fy")), K=True),
    "rk2d-pert": dict(scalars=("fR", "fB", "rhoR", "rhoB", "phi"), vectors=(("vx", "vy"),), K=False),
    "sc2d-efs": dict(scalars=("f0", "f1", "rho0", "rho1"), vectors=(("vx", "vy"), ("Fx0", "Fy0"), ("Fx1", "Fy1"), ("ueqx", "ueqy")), K=False),
    "sc2d-original": dict(scalars=("f0", "f1", "rho0", "rho1"), vectors=(("vx", "vy"), ("Fx0", "Fy0"), ("Fx1", "Fy1")), K=False),
    # (C0 .. C3: the tracers' concentrations, as many as the instance holds)
    "rk2d-tr": dict(scalars=("fR", "fB", "rhoR", "rhoB", "phi", "C0", "C1", "C2", "C3"), vectors=(("vx", "vy"), ("Gx", "Gy"), ("Fx", "Fy")), K=True),
    "rk3d": dict(scalars=("rhoR", "rhoB", "phi"), vectors=(("vx", "vy", "vz"),), K=False),
    "rk3dcsf": dict(scalars=("fR", "fB", "rhoR", "rhoB", "phi"), vectors=(("vx", "vy", "vz"), ("Gx", "Gy", "Gz"), ("Fx", "Fy", "Fz")), K=True),
}


def differences(name, got, ref, with_K=True):
    """{field: field-relative difference} of two field dicts of solver `name`; K, where it is compared, on ref's mask "K_live" """
    c = COMPARED[name]
    out = {f: rel_err(got[f], ref[f]) for f in c["scalars"] if f in ref}        # (a reference by reduction holds no populations)
    for vec in c["vectors"]:
        scale = max(max(float(np.max(np.abs(ref[f]))) for f in vec), 1e-300)
        for f in vec:
            out[f] = rel_err(got[f], ref[f], scale=scale)
    if c["K"] and with_K:
        live = ref["K_live"]
        out["K"] = rel_err(got["K"][live], ref["K"][live])
    return out


def worst(name, got, ref, with_K=True):
    d = differences(name, got, ref, with_K)
    f = max(d, key=d.get)
    return d[f], f


# ------------------------------------------------------------------------------------------------ oracle runs
def _solver_params(p, drop=()):
    return {k: v for k, v in p.items() if k not in drop}


def oracle_run(name, p, checkpoints=(1, STEPS), start=None, nx=None):
    """{step: fields} of the oracle of solver `name` with parameters p (see params()) from the lattice's densities, or from `start` =
    (densities of colour R / fluid 0, of colour B / fluid 1).  Compact 2-D fields, dense 3-D ones."""
    out = {}
    if name == "rk2d-csf":
        from oracle.rk import RKOracle
        dom, rR, rB = lattice_2d()
        rR, rB = start or (rR, rB)
        o = RKOracle(dom, _solver_params(p, ("variant",)), rR, rB)
        done = 0
        for n in checkpoints:
            o.run(n - done); done = n
            f = {k: getattr(o, k).copy() for k in ("fR", "fB", "rhoR", "rhoB", "phi", "vx", "vy", "Gx", "Gy", "Fx", "Fy", "K")}
            # K is a quotient by |G|: compared where the colour gradient is not vanishing (tests/test_ragged_sizes_gpu.py)
            f["K_live"] = np.hypot(f["Gx"], f["Gy"]) > 1e-6
            out[n] = f
    elif name == "rk2d-tr":
        from oracle.tr import CoupledOracle
        dom, rR, rB = lattice_tr(p["lattice"])
        conc = concentrations(dom, p["tracers"])
        rR, rB, conc = start or (rR, rB, conc)
        o = CoupledOracle(dom, {k: p[k] for k in list(RK2D_CSF["defaults"]) + list(RK2D_CSF["categorical"])}, rR, rB, conc, p["tr"])
        done = 0
        for n in checkpoints:
            o.run(n - done); done = n
            f = {k: getattr(o.flow, k).copy() for k in ("fR", "fB", "rhoR", "rhoB", "phi", "vx", "vy", "Gx", "Gy", "Fx", "Fy", "K")}
            f["K_live"] = np.hypot(f["Gx"], f["Gy"]) > 1e-6
            f.update({"C%d" % k: o.C[k].copy() for k in range(o.nT)})
            out[n] = f
    elif name == "rk2d-pert":
        from oracle.rk import RKPertOracle
        dom, rR, rB = lattice_2d_mixed()
        rR, rB = start or (rR, rB)
        if (p["inlet"], p["outlet"]) != ("Neumann", "Dirichlet"):
            return _pert_by_reduction(dom, rR, rB, p, checkpoints)
        o = RKPertOracle(dom, _solver_params(p, ("inlet", "outlet", "rhoRH", "rhoBH")), rhoR0=rR, rhoB0=rB)
        done = 0
        for n in checkpoints:
            o.run(n - done); done = n
            out[n] = {k: getattr(o, k).copy() for k in ("fR", "fB", "rhoR", "rhoB", "phi", "vx", "vy")}
    elif name in ("sc2d-efs", "sc2d-original"):
        from oracle.sc import SCOracle
        dom, r0, r1 = lattice_sc()
        r0, r1 = start or (r0, r1)
        o = SCOracle(dom, p, f_init=sc_populations(dom, r0, r1))
        for n in checkpoints:
            o.run(n - o.iterations)
            f = dict(vx=o.vx.copy(), vy=o.vy.copy(), ueqx=o.ux.copy(), ueqy=o.uy.copy())
            for k in range(2):
                f.update({"f%d" % k: o.f[k].copy(), "rho%d" % k: o.rho[k].copy(), "Fx%d" % k: o.Fx[k].copy(), "Fy%d" % k: o.Fy[k].copy()})
            out[n] = f
    elif name == "rk3d":
        from oracle.rk3d import RK3DOracle
        dom, rR, rB = lattice_3d(nx or p.get("nx", 70))
        rR, rB = start or (rR, rB)
        o = RK3DOracle(dom, rR, rB, _solver_params(p, ("storage", "nx")))
        done = 0
        for n in checkpoints:
            o.run(n - done); done = n
            o.macro()
            f = {k: o.field(k) for k in ("rhoR", "rhoB", "phi", "vx", "vy", "vz")}
            f["fR"], f["fB"] = o.field("fR"), o.field("fB")
            out[n] = f
    elif name == "rk3dcsf":
        from oracle.rk3dcsf import RK3DCSFOracle
        dom, rR, rB = lattice_csf()
        rR, rB = start or (rR, rB)
        o = RK3DCSFOracle(dom, rR, rB, dict(_solver_params(p, ("variant",)), crisp=CRISP))
        done = 0
        fl = dom == 1
        for n in checkpoints:
            o.run(n - done); done = n
            f = {k: o.field(k)[fl] for k in ("fR", "fB", "rhoR", "rhoB", "phi", "vx", "vy", "vz", "Gx", "Gy", "Gz", "Fx", "Fy", "Fz", "K")}
            f["K_live"] = np.ones(f["K"].shape, dtype=bool)       # against the crisp oracle K is compared everywhere (test_rk3d_csf_gpu.py)
            f["kind"], f["phi_dense"] = o.field("kind"), o.field("phi")
            out[n] = f
    else:
        raise KeyError(name)
    return out


def pert_unstreamed(dom, rR, rB):
    """dense populations [ny][nx][9] per colour whose first streaming gives the rest state w rho (tests/test_rk3d_reduction.py::unstream):
    the start of the 2-D perturbation step that corresponds to the densities the 3-D oracle starts from"""
    from oracle.rk import RKPertOracle
    o2 = RKPertOracle(dom, None, rhoR0=rR, rhoB0=rB)
    w = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)
    nb = o2.nbr.reshape(-1, 8)
    out = []
    for rho2 in (rR, rB):
        rho = rho2.reshape(-1)[o2.fluidNodes]
        g = np.empty((rho.size, 9))
        g[:, 0] = w[0] * rho
        for i in range(1, 9):
            q = nb[:, i - 1]
            g[:, i] = w[i] * np.where(q >= 0, rho[np.maximum(q, 0)], rho)
        d = np.zeros((dom.size, 9)); d[o2.fluidNodes] = g
        out.append(d.reshape(dom.shape + (9,)))
    return out


def _pert_by_reduction(dom, rR, rB, p, checkpoints):
    """The 2-D perturbation loop with the pressure inlet and / or the convective outlet, stated by oracle/rk3d_oracle.c on a lattice uniform
    along y with the projection-exact recolouring weights (tests/test_rk3d_reduction.py: every term of the D3Q19 step projects onto the
    D2Q9 one, SRT).  The 2-D step streams first, the 3-D one last: step n of the 2-D solver started from pert_unstreamed() has the
    densities and the velocity of the 3-D oracle after n - 1 steps and the head of the next.  Compact fields; no populations."""
    from oracle.rk3d import RK3DOracle
    assert p["relax"] == "SRT"
    ex = lambda a: np.ascontiguousarray(np.repeat(np.asarray(a)[:, None, :], 3, axis=1))
    sq2, sp = np.sqrt(2.0), p["solidPhi"]
    par3 = dict(AkR=p["AkR"], AkB=p["AkB"], beta=p["beta"], tauR=p["tauR"], tauB=p["tauB"], SolidRhoR=0.5 * (1. + sp), SolidRhoB=0.5 * (1. - sp),
                velocityZR=p["vyR"], velocityZB=p["vyB"], densityRL=p["rhoRL"], densityBL=p["rhoBL"], densityRH=p["rhoRH"], densityBH=p["rhoBH"],
                relax="SRT", inlet=p["inlet"], outlet=p["outlet"], recolor_axis=1. / 9. - 2. / (36. * sq2), recolor_diag=1. / (36. * sq2))
    o = RK3DOracle(ex(dom), ex(rR), ex(rB), par3)
    sel = dom.reshape(-1) == 1
    out, done = {}, 0
    for n in checkpoints:
        o.run(n - 1 - done); done = n - 1
        o.macro()
        out[n] = {k2: o.field(k3)[:, 0, :].reshape(-1)[sel] for k2, k3 in (("rhoR", "rhoR"), ("rhoB", "rhoB"), ("phi", "phi"), ("vx", "vx"), ("vy", "vz"))}
    return out


def start_of(name, nx=None, inst=None):
    """the two initial density arrays of solver `name`'s lattice (rk2d-tr: of the lattice of instance `inst`, and the concentrations)"""
    if name == "rk2d-tr":
        dom, rR, rB = lattice_tr(inst["lattice"])
        return dom, rR, rB, concentrations(dom, inst["tracers"])
    lat = {"rk2d-csf": lattice_2d, "rk2d-pert": lattice_2d_mixed, "sc2d-efs": lattice_sc, "sc2d-original": lattice_sc,
           "rk3d": lambda: lattice_3d(nx or 70), "rk3dcsf": lattice_csf}[name]()
    return lat[0], lat[1], lat[2]
