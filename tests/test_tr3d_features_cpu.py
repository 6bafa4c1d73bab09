"""What makes tests/test_rk3d_tracer_features_gpu.py mean something, without a GPU.  Every bound is TOL = 1e-10 of
tests/test_rk3d_tracer_gpu.py or a stated multiple of it.

1. with g = 0 the composition around the body-force recipe IS today's Coupled3DRef, bit for bit;
2. the hook sits where BodyForceRef.step_a() leaves u, and a hook leaves the flow's bits alone;
3. the composition around PeriodicRef is today's open-plane Coupled3DRef on the transposed lattice with D's x and z exchanged (0.1 TOL);
4. every case of the GPU comparison is well conditioned: started from densities rippled in the last bit the reference follows itself
   within 0.1 TOL at every compared step;
5. the mistakes the GPU comparison is there to catch each move a compared tracer field by >= 1000 TOL;
and tracer point B is off every default and off tracer_case."""
import numpy as np
import pytest

import body_force_ref as R
import param_points as P
import periodic_ref as PR
import test_rk3d_tracer_features_gpu as F
import test_rk3d_tracer_gpu as T
from helpers import rel_err
from tr3d_ref import Coupled3DRef, tracer_matrices3d

TOL = T.TOL
FLOW_FIELDS = ("fR", "fB", "rhoR", "rhoB", "phi", "vx", "vy", "vz", "Gx", "Gy", "Gz", "Fx", "Fy", "Fz", "K")


def tracer_difference(a, b, fl, nT):
    """the measure of compare_tracers: the largest field-relative difference over the tracers' concentrations and populations"""
    return max(max(rel_err(a.C[k][fl], b.C[k][fl]), rel_err(a.g[k][:, fl], b.g[k][:, fl])) for k in range(nT))


def rippled(c, seed_phase=0.3):
    return P.last_bit(c["rR"], seed_phase), P.last_bit(c["rB"], seed_phase + 1.0)


# ------------------------------------------------------------------------------------------------ tracer point B
def test_tracer_point_b_is_off_the_defaults_and_off_tracer_case():
    import inspect
    from openlbmpm_amd.rk3dcsf import tracer_config
    from tr3d_ref import DEFAULT_TRACER3D
    lib = {k: v.default for k, v in inspect.signature(tracer_config).parameters.items()}
    names = dict(diffusion_x="diffX", diffusion_y="diffY", diffusion_z="diffZ", diffusion_xy="dXY", diffusion_yx="dYX", diffusion_xz="dXZ", diffusion_zx="dZX",
                 diffusion_yz="dYZ", diffusion_zy="dZY", beta_interface="beta", criteria_rho="crit", inlet_concentration="inlet_conc", reaction_rate="reaction_rate",
                 diffusion_j="diffJ")
    for nT in (2, 3, 4):
        b, rb = T.tracer_point_b(nT, reaction_rate=0.05)
        a, _ = T.tracer_case(nT, reaction_rate=0.03)
        for key, rkey in names.items():
            vb, va = np.atleast_1d(b[key]), np.atleast_1d(a[key])
            assert np.all(vb != va), (key, vb, va)
            for default in (lib[key], DEFAULT_TRACER3D[rkey]):
                if default is None:                      # diffusion_y, diffusion_z: diffusion_x's values
                    default = b["diffusion_x"]
                assert np.all(vb != np.atleast_1d(default)), (key, vb, default)
            if key in ("diffusion_x", "diffusion_y", "diffusion_z"):
                assert np.all((vb >= 0.05) & (vb <= 0.25)), (key, vb)
        assert len({b["diffusion_" + n] for n in ("xy", "yx", "xz", "zx", "yz", "zy")}) == 6
        for k in range(nT):             # 1/2 + 3 D well conditioned
            D = np.array([[rb["diffX"][k], rb["dXY"], rb["dXZ"]], [rb["dYX"], rb["diffY"][k], rb["dYZ"]], [rb["dZX"], rb["dZY"], rb["diffZ"][k]]])
            assert np.linalg.cond(0.5 * np.eye(3) + 3. * D) < 2.5
        assert np.all(np.isfinite(tracer_matrices3d(rb)[1]))
    assert T.tracer_point_b(3)[0]["reaction_rate"] not in (0.0, T.tracer_case(3)[0]["reaction_rate"])


# ------------------------------------------------------------------------------------------------ 1. zero force
@pytest.mark.parametrize("i,tracers", [(0, "3 at B"), (1, "2 at tracer_case"), (2, "3 at B")], ids=["SRT", "MRT convective", "MRT"])
def test_without_a_force_the_composition_is_todays(i, tracers):
    c = F.bf_case(i, tracers)
    c["rR"], c["rB"] = P.lattice_csf()[1:]          # blob3() as it is
    new = F.bf_reference(c, g=F.NO_FORCE)
    old = Coupled3DRef(c["dom"], c["rR"], c["rB"], c["c0"], dict(c["opar"], crisp=R.CRISP), c["ref"])
    for n in range(1, 11):
        new.run(1); old.run(1)
        assert np.array_equal(new.g, old.g) and np.array_equal(new.C, old.C), n
        for f in FLOW_FIELDS:
            assert np.array_equal(new.flow.field(f), old.flow.field(f)), (n, f)
    assert float(np.max(np.abs(new.C - c["c0"]))) > 1e-3


# ------------------------------------------------------------------------------------------------ 2. hook timing
def test_the_hook_sees_what_step_a_leaves_and_leaves_the_flow_alone():
    c = F.bf_case(2, "3 at B")
    make = lambda: R.BodyForceRef(c["dom"], c["rR"], c["rB"], c["opar"], *c["g"])
    b, plain = make(), make()
    seen = []
    names = ("rhoR", "rhoB", "vx", "vy", "vz", "phi", "Gx", "Gy", "Gz")
    for n in range(5):
        b.step(lambda: seen.append({f: b.field(f) for f in names}))
        plain.step()
        twin = make().run(n)
        twin.step_a()
        assert len(seen) == n + 1
        for f in names:
            assert np.array_equal(seen[-1][f], twin.field(f)), (n, f)
        for f in FLOW_FIELDS:
            assert np.array_equal(b.field(f), plain.field(f)), (n, f)
    # ... and that u is not the one without the force's half, nor the one the second half leaves
    bare = R.BodyForceRef(c["dom"], c["rR"], c["rB"], c["opar"], *c["g"]).run(4)
    bare.o.step_a()
    fl = c["dom"] == 1
    assert rel_err(bare.field("vx")[fl], seen[-1]["vx"][fl]) > 1000 * TOL
    # the tracers ride on it without touching it
    with_tracers = F.bf_reference(c).run(5)
    for f in FLOW_FIELDS:
        assert np.array_equal(with_tracers.flow.field(f), plain.field(f)), f


# ------------------------------------------------------------------------------------------------ 3. periodic composition
@pytest.mark.parametrize("relax,tautype", F.PERIODIC_FLOWS)
def test_the_periodic_composition_is_the_open_plane_one_transposed(relax, tautype):
    """PeriodicRef's tracers against today's Coupled3DRef (the oracle, open planes) on the lattice with x and z exchanged: there the
    oracle's open planes are solid and the tracers' z is the wrapped x.  Not bit-equal: the exchange permutes the order of sums"""
    from test_tr3d_ref import exchange_field, exchange_populations, exchange_tracer
    c = F.periodic_case(relax, tautype, None)
    x = lambda f: exchange_field(f, "x", "z")
    new = F.periodic_reference(c)
    par = {k: v for k, v in c["par"].items() if k not in PR.FLOW_KEYS}
    old = Coupled3DRef(x(c["dom"]), x(c["rR"]), x(c["rB"]), x(c["c0"]), dict(par, crisp=R.CRISP), exchange_tracer(c["ref"], "x", "z"))
    assert not old.tr.t["free_outlet"] and not old.tr.t["dirichlet_inlet"]
    worst = 0.0
    for n in c["steps"]:
        new.run(n - new.steps); old.run(n - old.steps)
        worst = max(worst, rel_err(old.C, x(new.C)), rel_err(old.g, exchange_populations(new.g, "x", "z")))
    print("periodic composition against the transposed open-plane one, %s tautype %d: %.3e" % (relax, tautype, worst))
    assert worst < 0.1 * TOL, worst
    assert rel_err(new.C, c["c0"]) > 1e-2


# ------------------------------------------------------------------------------------------------ 4. conditioning
def _conditioning(what, one, two, steps, fl, nT):
    worst = 0.0
    for n in steps:
        one.run(n - one.steps); two.run(n - two.steps)
        worst = max(worst, tracer_difference(two, one, fl, nT))
    print("conditioning, %s: the reference against itself from a start rippled in the last bit, worst over the steps %s: %.3e" % (what, steps, worst))
    assert np.any(two.flow.field("fR") != one.flow.field("fR"))
    assert worst < 0.1 * TOL, (what, worst)


@pytest.mark.parametrize("i,tracers", F.BF_CASES, ids=["%d-%s" % c for c in F.BF_CASES])
def test_the_body_force_cases_are_well_conditioned(i, tracers):
    c = F.bf_case(i, tracers)
    _conditioning(c["what"], F.bf_reference(c), F.bf_reference(c, *rippled(c)), c["steps"], c["dom"] == 1, c["nT"])


@pytest.mark.parametrize("gset", ["G1", None])
@pytest.mark.parametrize("relax,tautype", F.PERIODIC_FLOWS)
def test_the_periodic_cases_are_well_conditioned(relax, tautype, gset):
    c = F.periodic_case(relax, tautype, gset)
    _conditioning(c["what"], F.periodic_reference(c), F.periodic_reference(c, *rippled(c)), c["steps"], c["dom"] == 1, 3)


@pytest.mark.parametrize("channel", ["A", "B"])
def test_the_channel_cases_are_well_conditioned(channel):
    c = F.channel_case()
    a = F.ANGLES[channel]
    _conditioning("two channels at %g, channel %s" % (a, channel), F.channel_reference(c, a), F.channel_reference(c, a, *rippled(c)), c["steps"],
                  c["cells"][channel] & (c["dom"] == 1), 2)


@pytest.mark.parametrize("flow", ["SRT", "MRT"])
def test_the_open_plane_cases_at_point_b_are_well_conditioned(flow):
    """the two cases test_against_the_restatement gained, with its flow, its lattice and the steps it compares them at (T.COMPARED)"""
    dom, rR, rB = T.LATTICES["obstacle"]()
    par = dict(theta=50.0, tauB=0.8, velocityZR=0.0, velocityZB=-1.0e-2, sigma=0.05, crisp=T.CRISP); par.update(T.FLOWS[flow])
    _, ref = T.tracer_point_b(3)
    c0 = T.concentrations(dom, 3)
    c = dict(rR=rR, rB=rB)
    one, two = Coupled3DRef(dom, rR, rB, c0, par, ref), Coupled3DRef(dom, *rippled(c), c0, par, ref)
    assert ("obstacle", flow, 3, T.POINT_B) in T.CASES
    _conditioning("obstacle %s, point B" % flow, one, two, T.COMPARED.get(("obstacle", flow, 3, T.POINT_B), (1, 2, T.STEPS)), dom == 1, 3)
    assert all(np.max(np.abs(one.C[k] - c0[k])) > 1e-2 for k in range(3))


# ------------------------------------------------------------------------------------------------ 5. sensitivity
def half_force(o, exchanged=False):
    """F_b / (2 rho) [3] in the solver's axes from the flow's densities as they stand; exchanged: with g_R and g_B exchanged"""
    f = o.flow
    rR, rB, fl = f.field("rhoR"), f.field("rhoB"), np.asarray(f.dom) == 1
    gr, gb = (f.g_b, f.g_r) if exchanged else (f.g_r, f.g_b)
    rho = np.where(fl, rR + rB, 1.0)
    return [np.where(fl, 0.5 * (rR * gr[a] + rB * gb[a]) / rho, 0.0) for a in range(3)]


def without_the_half(fields, o):
    h = half_force(o)
    return [fields[0]] + [fields[1 + a] - h[a] for a in range(3)] + fields[4:]


def with_the_other_colours_force(fields, o):
    h, x = half_force(o), half_force(o, exchanged=True)
    return [fields[0]] + [fields[1 + a] - h[a] + x[a] for a in range(3)] + fields[4:]


def _factors(what, good, bad, steps, fl, nT, after_b=False, least=1000.0, from_step=None):
    """the mistake's run against the right one at every compared step, in units of TOL; asserted from `from_step` on (default: all)"""
    out = []
    for n in steps:
        good.run(n - good.steps); bad.run(n - bad.steps, after_b=after_b)
        out.append(tracer_difference(bad, good, fl, nT) / TOL)
    print("sensitivity, %s: %s x TOL at the steps %s" % (what, ", ".join("%.3g" % v for v in out), steps))
    for n, v in zip(steps, out):
        if from_step is None or n >= from_step:
            assert v >= least, (what, n, v)
    return out


FORCE_MISTAKES = {"u without F_b / 2": dict(alter=without_the_half), "g_R and g_B exchanged": dict(alter=with_the_other_colours_force),
                  "the splice after the second half": dict()}


@pytest.mark.parametrize("mistake", sorted(FORCE_MISTAKES))
@pytest.mark.parametrize("i,tracers", [(0, "3 at B"), (2, "3 at B"), (1, "2 at tracer_case"), (3, "2 at tracer_case")], ids=["SRT A G1", "MRT B G2", "MRT A G1", "SRT B G2"])
def test_a_wrong_velocity_under_the_force_is_seen(i, tracers, mistake):
    c = F.bf_case(i, tracers)
    _factors("%s, %s" % (c["what"], mistake), F.bf_reference(c), F.bf_reference(c, **FORCE_MISTAKES[mistake]), c["steps"], c["dom"] == 1, c["nT"],
             after_b=mistake.startswith("the splice"))


@pytest.mark.parametrize("mistake", ["u without F_b / 2", "g_R and g_B exchanged"])
def test_a_wrong_velocity_under_the_force_is_seen_on_periodic_z(mistake):
    c = F.periodic_case("MRT", 2, "G1")
    _factors("%s, %s" % (c["what"], mistake), F.periodic_reference(c), F.periodic_reference(c, **FORCE_MISTAKES[mistake]), c["steps"], c["dom"] == 1, 3)


@pytest.mark.parametrize("gset", ["G1", None])
@pytest.mark.parametrize("relax,tautype", F.PERIODIC_FLOWS)
def test_a_cut_wrap_of_z_is_seen(relax, tautype, gset):
    """the tracers' pull along z stopped at the seam (bounce-back between plane nz-1 and plane 0)"""
    c = F.periodic_case(relax, tautype, gset)
    _factors("%s, no wrap of z" % c["what"], F.periodic_reference(c), F.periodic_reference(c, seam_wall=True), c["steps"], c["dom"] == 1, 3)


# every parameter of tracer point B, one at a time back at the default of configure_tracers (diffusion_y, diffusion_z: the value of
# diffusion_x, and 1/6).  name -> the override of tracer_point_b
def _defaults_one_at_a_time(nT=3):
    b = T.tracer_point_b(nT)[0]
    out = {}
    for t in range(nT):
        for key, default in (("diffusion_x", 1. / 6.), ("diffusion_y", 1. / 6.), ("diffusion_z", 1. / 6.), ("beta_interface", 0.0), ("inlet_concentration", 0.0),
                             ("diffusion_j", 0.0)):
            v = list(b[key]); v[t] = default
            out["%s[%d]" % (key, t)] = {key: tuple(v)}
        for key in ("diffusion_y", "diffusion_z"):
            v = list(b[key]); v[t] = b["diffusion_x"][t]
            out["%s[%d] = diffusion_x" % (key, t)] = {key: tuple(v)}
    for key in ("diffusion_xy", "diffusion_yx", "diffusion_xz", "diffusion_zx", "diffusion_yz", "diffusion_zy", "reaction_rate"):
        out[key] = {key: 0.0}
    out["criteria_rho"] = dict(criteria_rho=0.5)
    return out


DEFAULTS = _defaults_one_at_a_time()
# The periodic lattice and the obstacle box start with a sharp interface: in the first steps rho_R is near 0 or near 1 and no cell lies
# between the two criteria, so there criteria_rho shows at the last compared step only (the body-force cases start from a ramp for that
# reason, F.ramp_start, and see it at every step).
SHARP_START = ("criteria_rho",)


@pytest.mark.parametrize("name", sorted(DEFAULTS))
def test_a_parameter_of_point_b_at_its_default_is_seen(name):
    """on the body-force case (MRT, flow point B, G2) with three tracers, the tracers' open planes on"""
    c = F.bf_case(2, "3 at B")
    bad = dict(c, ref=T.tracer_point_b(3, **DEFAULTS[name])[1])
    _factors("%s at its default" % name, F.bf_reference(c), F.bf_reference(bad), c["steps"], c["dom"] == 1, 3)


@pytest.mark.parametrize("name", ["criteria_rho", "diffusion_x[0]"])
def test_a_parameter_of_point_b_at_its_default_is_seen_on_periodic_z_and_between_open_planes(name):
    c = F.periodic_case("MRT", 2, "G1")
    bad = dict(c, ref=T.tracer_point_b(3, dirichlet_inlet=False, free_outlet=False, **DEFAULTS[name])[1])
    _factors("periodic, %s at its default" % name, F.periodic_reference(c), F.periodic_reference(bad), c["steps"], c["dom"] == 1, 3,
             from_step=c["steps"][-1] if name in SHARP_START else None)
    dom, rR, rB = T.LATTICES["obstacle"]()
    par = dict(theta=50.0, tauB=0.8, velocityZR=0.0, velocityZB=-1.0e-2, sigma=0.05, crisp=T.CRISP, relax="MRT")
    c0 = T.concentrations(dom, 3)
    good, wrong = (Coupled3DRef(dom, rR, rB, c0, par, T.tracer_point_b(3, **over)[1]) for over in ({}, DEFAULTS[name]))
    _factors("obstacle, point B, %s at its default" % name, good, wrong, (1, 2, T.STEPS), dom == 1, 3, from_step=T.STEPS if name in SHARP_START else None)


@pytest.mark.parametrize("channel", ["A", "B"])
def test_the_other_channels_angle_is_seen(channel):
    c = F.channel_case()
    own, other = F.ANGLES[channel], F.ANGLES["B" if channel == "A" else "A"]
    _factors("channel %s with the angle %g instead of %g" % (channel, other, own), F.channel_reference(c, own), F.channel_reference(c, other), c["steps"],
             c["cells"][channel] & (c["dom"] == 1), 2)
