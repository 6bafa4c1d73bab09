"""The D3Q7 tracers' first-order reaction at solid walls on the GPU (lbmpm_rk3dcsf_tracer_set_wall_reaction, _tracer_wall_integrals; the
WALL instances of tr3d_step / tr3d_observe / the integrals' loader in csrc/rk3d_tracer.h, csrc/rk3d_tracer_wall.h).

The reference is tests/wall_reaction_ref.py (Tracer3DRef with the bounce-back line changed) inside tests/tr3d_ref.Coupled3DRef;
tests/test_wall_reaction_cpu.py holds it to the plain bounce-back, to the slit eigenmode and to its mass balance, and shows that the
cases of tests/wall_cases.py are well conditioned and that a wrong rate, class or tracer moves a compared field by >= 1000 TOL.
1. parity under a flow (open planes; periodic z with a body force), fields at TOL = 1e-10 and the uptake table;  2. k = 0, None and a
uniform map are bit-equal to what they should be;  3. the uptake table: links, sums, the mass balance on the device, the first state, a
NaN;  4. slabs, the bulk path, restart, a rate changed mid-run;  5. the slit eigenmode on the device;  6. errors leave the state alone.
Measured on the MI355X: see docs/EXPERIMENTS_r7.md, section W."""
import numpy as np
import pytest

import wall_cases as W
from helpers import rel_err
from test_rk3d_tracer_gpu import TOL, compare_tracers
from wall_reaction_ref import slit_case, slit_deviations

pytestmark = pytest.mark.gpu

RATE_BOUND, PROFILE_BOUND = 0.5e-2, 2e-3           # the CPU test's bounds (tests/test_wall_reaction_cpu.py)
SUM_TOL = 1e-12


def solver(c, **kw):
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    par = dict(c["par"], **kw.pop("par", {}))
    return RK3DCSFSolver(c["dom"], par, tracers=c["kw"], **kw)


def cluster(c, nslabs):
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster
    return RK3DCSFCluster(c["dom"], c["par"], nslabs=nslabs, tracers=c["kw"])


class Snap:
    def __init__(self, o):
        self.C, self.g, self.table = np.array(o.C), np.array(o.g), o.tr.table()


_REFS = {}


def reference(name, change_at=None, rates2=None):
    """{step: Snap} of the case's reference at W.STEPS.  With change_at: at change_at and 2 x change_at of a run whose rates become rates2
    once step change_at is computed on the device.  The rate belongs to the pull, and the pull that ends sub-step change_at is taken by
    whoever reads the stored populations next: the reference, which streams inside its sub-step, has the new rates from that sub-step on"""
    key = (name, change_at)
    if key not in _REFS:
        c = W.CASES[name]()
        o, out = W.reference(c), {}
        for n in (W.STEPS if change_at is None else (change_at - 1, change_at, 2 * change_at)):
            o.run(n - o.steps)
            if n == (change_at or 0) - 1:
                o.tr.set_rates(rates2)
            else:
                out[n] = Snap(o)
        _REFS[key] = (c, out)
    return _REFS[key]


def tables(s):
    return s.tracer_integrals().planes, s.tracer_wall_integrals().planes


def state(s, nT):
    return [s.get_tracer_pdf(k) for k in range(nT)] + [s.get_concentration(k) for k in range(nT)] + list(tables(s))


def same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), (what, i, float(np.max(np.abs(np.asarray(x) - np.asarray(y)))))


def compare_table(got, want, what):
    """links exact, no non-finite cell; -> the larger error of uptake and wall concentration per plane and tracer, relative to the
    column's largest entry"""
    assert got.shape == want.shape
    assert np.array_equal(got[:, :, 0], want[:, :, 0]), what
    eu, ec = rel_err(got[:, :, 1], want[:, :, 1]), rel_err(got[:, :, 2], want[:, :, 2])
    print("%s: uptake %.3e wall concentration %.3e (relative to the largest plane)" % (what, eu, ec))
    assert np.all(got[:, :, 3] == 0.0)
    return max(eu, ec)


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name", sorted(W.CASES))
def test_against_the_restatement_under_a_flow(name):
    """two tracers with distinct rates, one of them inf, on a three-class map: concentrations and populations after steps 1 and 10, and
    the uptake table against the reference's own sums.  Without the wall reaction the same run is elsewhere (what fails on a library
    that bounces everything back)"""
    c, ref = reference(name)
    fl, nT = c["dom"] == 1, c["nT"]
    s, plain = W.start(solver(c), c), W.start(solver(c), c, rates=None)
    assert s.wall_reaction.tolist() == W.RATES.tolist() and plain.wall_reaction is None
    worst = 0.0
    for n in W.STEPS:
        s.step(n - s.steps_done); plain.step(n - plain.steps_done)
        worst = max(worst, compare_tracers(s, ref[n], fl, nT, "%s, step %d" % (name, n)))
        err = compare_table(s.tracer_wall_integrals().planes, ref[n].table, "%s, step %d" % (name, n))
        assert err < TOL, err                 # (sums of populations held to TOL; the tight bound is test 3's, on the case conditioned to 7e-16)
        felt = max(rel_err(plain.get_tracer_pdf(k)[fl], s.get_tracer_pdf(k)[fl]) for k in range(nT))
        assert felt > 1000 * TOL, (n, felt)
    print("%s: worst field-relative difference %.3e; the reaction moved the populations by %.3e" % (name, worst, felt))
    s.close(); plain.close()


# ------------------------------------------------------------------------------------------------ 2. identities
@pytest.mark.parametrize("name", sorted(W.CASES))
def test_no_reaction_is_todays_run_bit_for_bit(name):
    """set_wall_reaction(0.0) (the WALL kernels with r = 1.0), set_wall_reaction(None) after a rate was set, and a run that never heard of
    it; a uniform map of class 1 equals the scalar call with class 1's rates"""
    c = W.CASES[name]()
    nT = c["nT"]
    plain = W.start(solver(c), c, rates=None)
    zero = W.start(solver(c), c, rates=0.0, minerals=None)
    zero_map = W.start(solver(c), c, rates=np.zeros(W.RATES.shape))          # (through the class words)
    off = W.start(solver(c), c)
    off.set_wall_reaction(None)
    assert zero.wall_reaction.tolist() == [[0.0] * nT] and off.wall_reaction is None
    scalar = W.start(solver(c), c, rates=W.RATES[1], minerals=None)
    uniform = W.start(solver(c), c, minerals=np.ones(c["dom"].shape, dtype=np.uint8))
    before = plain.device_bytes
    for n in (1, 2, 10):
        for x in (plain, zero, zero_map, off, scalar, uniform):
            x.step(n - x.steps_done)
        same(state(zero, nT), state(plain, nT), "k = 0, step %d" % n)
        same(state(zero_map, nT), state(plain, nT), "k = 0 on the map, step %d" % n)
        same(state(off, nT), state(plain, nT), "None, step %d" % n)
        same(state(uniform, nT), state(scalar, nT), "uniform map, step %d" % n)
        assert not np.array_equal(scalar.get_tracer_pdf(0), plain.get_tracer_pdf(0))
    assert np.all(plain.tracer_wall_integrals().planes[:, :, 1] == 0.0)           # r = 1: an uptake of exactly 0
    # the map costs 4 bytes per fluid cell while it is set (the tables of the integrals were allocated by state() everywhere)
    assert uniform.device_bytes - scalar.device_bytes == 4 * plain.num_fluid_nodes and scalar.device_bytes == plain.device_bytes
    assert before < plain.device_bytes
    uniform.set_wall_reaction(W.RATES[1])
    assert uniform.device_bytes == scalar.device_bytes
    for x in (plain, zero, zero_map, off, scalar, uniform):
        x.close()


# ------------------------------------------------------------------------------------------------ 3. the uptake table
def test_the_uptake_table_and_the_mass_balance_on_the_device():
    """the periodic case (a closed ring; the reference's own conditioning there is 7e-16): links exact, sums to 1e-12 of the reference's at
    every step 1 .. 20, zero uptake before the first step, and mass_0 - mass_20 of tracer_integrals() = the summed uptakes to 1e-12 of mass_0"""
    c = W.CASES["periodic"]()
    nT = c["nT"]
    o = W.reference(c)
    s = W.start(solver(c), c)
    first = s.tracer_wall_integrals()
    assert first.planes.shape == (c["dom"].shape[0], nT, 4)
    assert np.array_equal(first.planes[:, :, 0], o.tr.table()[:, :, 0]) and first.wall_links == int(o.tr.links.sum()) > 100
    assert np.all(first.planes[:, :, 1:] == 0.0)
    m0 = [s.tracer_integrals().mass(k) for k in range(nT)]
    taken, worst = [0.0] * nT, 0.0
    for n in range(1, 21):
        s.step(1); o.run(1)
        t = s.tracer_wall_integrals()
        worst = max(worst, compare_table(t.planes, o.tr.table(), "periodic, step %d" % n))
        for k in range(nT):
            taken[k] += t.uptake(k)
    assert worst < SUM_TOL, worst
    m = s.tracer_integrals()
    res = [abs(m0[k] - m.mass(k) - taken[k]) / abs(m0[k]) for k in range(nT)]
    lost = [(m0[k] - m.mass(k)) / m0[k] for k in range(nT)]
    print("mass balance on the device over 20 steps: lost %s of the initial mass, residual %s; the table against the reference %.3e" % (lost, res, worst))
    assert all(r < SUM_TOL for r in res), res
    assert all(abs(v) > 1e-3 for v in lost), lost
    assert t.mean_wall_concentration(0) > 0 and t.nonfinite == 0 and set(t.summary()) == {"uptake0", "wallC0", "uptake1", "wallC1"}
    s.close()


def test_a_nan_at_a_wall_lands_in_nonfinite_only():
    """tracer 1 starts with a NaN in one fluid cell with wall links: after one step that cell's stored populations are NaN, and the table
    counts the cell in NONFINITE and its links in LINKS; every sum stays finite and equals the clean run's without that cell's links"""
    c = W.CASES["periodic"]()
    dom, fl = c["dom"], c["dom"] == 1
    clean = W.start(solver(c), c)
    links = clean.tracer_wall_integrals()
    walls = np.argwhere(fl & (np.roll(dom, 1, axis=2) != 1) & (np.roll(dom, -1, axis=0) == 1))
    z, y, x = [int(v) for v in walls[len(walls) // 2]]
    c0 = np.array(c["c0"])
    c0[1, z, y, x] = np.nan
    s = W.start(solver(dict(c, c0=c0)), dict(c, c0=c0))
    s.step(1); clean.step(1)
    t, good = s.tracer_wall_integrals(), clean.tracer_wall_integrals()
    assert np.array_equal(t.planes[:, :, 0], links.planes[:, :, 0])
    assert np.all(np.isfinite(t.planes)) and t.nonfinite == 1 and t.planes[z, 1, 3] == 1.0 and good.nonfinite == 0
    assert np.array_equal(t.planes[:, 0], good.planes[:, 0])                                      # tracer 0 knows nothing of it
    other = [p for p in range(dom.shape[0]) if p != z]
    assert np.array_equal(t.planes[other, 1], good.planes[other, 1])
    assert good.planes[z, 1, 1] != t.planes[z, 1, 1] and good.planes[z, 1, 2] != t.planes[z, 1, 2]          # (the cell's links are left out)
    assert s.tracer_integrals().nonfinite >= 1
    s.close(); clean.close()


# ------------------------------------------------------------------------------------------------ 4. cuts, bulk path, restart, a changed rate
CHANGE_AT = 5
RATES2 = np.array([[0.5, 0.03], [W.INF, 0.2], [0.0, 0.08]])


@pytest.fixture(scope="module")
def undivided():
    """the open case (nz = 16) at the steps 5 and 10, its rates changed to RATES2 after step 5; the restart data of step 5 (the populations
    as the new rates' pull hands them out)"""
    c = W.CASES["open"]()
    s = W.start(solver(c), c)
    s.step(CHANGE_AT)
    at = dict(fR=s.get("fR"), fB=s.get("fB"), F=tuple(s.get(f) for f in ("Fx", "Fy", "Fz")), state=state(s, c["nT"]))
    s.set_wall_reaction(RATES2, c["minerals"])
    seen = state(s, c["nT"])               # the observers after the change: the new rates' pull of the stored populations
    at["g"] = seen[:c["nT"]]               # ... which is what a restart under the new rates continues from
    assert not np.array_equal(seen[0], at["state"][0])
    s.step(CHANGE_AT)
    out = dict(c=c, at=at, seen=seen, end=state(s, c["nT"]), fR=s.get("fR"))
    s.close()
    return out


@pytest.mark.parametrize("nslabs", [2, 3])
def test_slabs_equal_the_undivided_lattice(undivided, nslabs):
    u = undivided
    c, nT = u["c"], u["c"]["nT"]
    cl = W.start(cluster(c, nslabs), c)
    assert len(cl.slabs) == nslabs and all(g.z1 - g.z0 >= 4 for g in cl.geo) and cl.wall_reaction.tolist() == W.RATES.tolist()
    cl.step(CHANGE_AT)
    same(state(cl, nT), u["at"]["state"], "%d slabs, step %d" % (nslabs, CHANGE_AT))
    cl.set_wall_reaction(RATES2, c["minerals"])
    same(state(cl, nT), u["seen"], "%d slabs, after the change" % nslabs)
    cl.step(CHANGE_AT)
    same(state(cl, nT), u["end"], "%d slabs, step %d" % (nslabs, 2 * CHANGE_AT))
    assert np.array_equal(cl.get("fR"), u["fR"])
    cl.close()


def test_the_full_path_equals_the_bulk_path(undivided):
    """variant 1: no bulk skip, and the tracers' own table of source cells (tr3d_setup_src) in the place of the flow's"""
    u = undivided
    c, nT = u["c"], u["c"]["nT"]
    s = W.start(solver(c, par=dict(variant=1)), c)
    s.step(CHANGE_AT)
    same(state(s, nT), u["at"]["state"], "variant 1, step %d" % CHANGE_AT)
    s.set_wall_reaction(RATES2, c["minerals"])
    s.step(CHANGE_AT)
    same(state(s, nT), u["end"], "variant 1, step %d" % (2 * CHANGE_AT))
    s.close()


def test_a_restart_with_the_rates_given_again_continues_bit_for_bit(undivided):
    u = undivided
    c, nT = u["c"], u["c"]["nT"]
    s = solver(c)
    s.set_pdf(u["at"]["fR"], u["at"]["fB"], force=u["at"]["F"])
    s.set_wall_reaction(RATES2, c["minerals"])
    for k in range(nT):
        s.set_tracer_pdf(k, u["at"]["g"][k])          # (keeps the rates)
    assert s.wall_reaction.tolist() == RATES2.tolist()
    assert np.all(s.tracer_wall_integrals().planes[:, :, 1:] == 0.0)       # given populations stand where they are: no wall event yet
    s.step(CHANGE_AT)
    same(state(s, nT), u["end"], "restart")
    s.close()


def test_a_rate_changed_mid_run_follows_the_reference_doing_the_same(undivided):
    """what the observers hand out right after the change (the new rates' pull of step 5's populations) and step 10"""
    u = undivided
    c, nT, fl = u["c"], u["c"]["nT"], u["c"]["dom"] == 1
    _, ref = reference("open", CHANGE_AT, RATES2)
    for n, st in ((CHANGE_AT, u["seen"]), (2 * CHANGE_AT, u["end"])):
        for k in range(nT):
            eg, ec = rel_err(np.moveaxis(st[k], -1, 0)[:, fl], ref[n].g[k][:, fl]), rel_err(st[nT + k][fl], ref[n].C[k][fl])
            print("changed at step %d, step %d, tracer %d: concentration %.3e populations %.3e" % (CHANGE_AT, n, k, ec, eg))
            assert eg < TOL and ec < TOL, (n, k, eg, ec)
        assert compare_table(st[2 * nT + 1], ref[n].table, "changed at step %d, step %d" % (CHANGE_AT, n)) < TOL
    unchanged = reference("open")[1][W.STEPS[-1]]
    assert W.STEPS[-1] == 2 * CHANGE_AT and rel_err(u["end"][0][fl], np.moveaxis(unchanged.g[0], 0, -1)[fl]) > 1000 * TOL


# ------------------------------------------------------------------------------------------------ 5. the slit on the device
@pytest.mark.parametrize("k,D", [(0.05, 1. / 6.), (W.INF, 0.05)], ids=["k=0.05,D=1/6", "k=inf,D=0.05"])
def test_the_slit_eigenmode_on_the_device(k, D):
    """H = 16 between two reactive plates, one colour at rest with periodic z, 400 steps; mass from tracer_integrals(), the bounds of the CPU test"""
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    dom, conc, _, lam, mode = slit_case(k, D)
    s = RK3DCSFSolver(dom, dict(relax="MRT", inlet="Periodic", outlet="Periodic"),
                      tracers=dict(num_tracers=1, diffusion_x=D, beta_interface=0.0, dirichlet_inlet=False, free_outlet=False))
    s.set_macro(np.where(dom == 1, 1.0, 0.0), np.zeros(dom.shape))
    s.set_concentration(0, conc)
    s.set_wall_reaction(k)
    s.step(200)
    m200 = s.tracer_integrals().mass(0)
    s.step(200)
    m400 = s.tracer_integrals().mass(0)
    rate, prof = slit_deviations(m200, m400, s.get_concentration(0)[0, 0, 1:-1], D, lam, mode)
    print("slit on the device k = %g, D = %.4g: decay rate off by %.3e, profile off by %.3e; largest speed %.3e" % (k, D, rate, prof, s.integrals().max_speed))
    assert rate < RATE_BOUND and prof < PROFILE_BOUND, (k, D, rate, prof)
    s.close()


# ------------------------------------------------------------------------------------------------ 6. errors
def test_errors_leave_the_state_untouched():
    from openlbmpm_amd import _lib
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster, RK3DCSFSolver
    c = W.CASES["periodic"]()
    nT = c["nT"]
    bare = RK3DCSFSolver(c["dom"], c["par"])
    for call in (lambda: bare.set_wall_reaction(0.1), lambda: bare.tracer_wall_integrals(), lambda: bare.wall_reaction):
        with pytest.raises(_lib.LbmpmError) as e:
            call()
        assert e.value.status == _lib.ERR_STATE
    bare.close()
    s = solver(c)
    with pytest.raises(_lib.LbmpmError) as e:
        s.tracer_wall_integrals()                    # no state given yet
    assert e.value.status == _lib.ERR_STATE
    W.start(s, c)
    s.step(3)
    before = state(s, nT)
    too_high = np.array(c["minerals"])
    z, y, x = [int(v) for v in np.argwhere(c["dom"] != 1)[7]]
    too_high[z, y, x] = 3
    bad = [(lambda: s.set_wall_reaction(-0.1), _lib.LbmpmError), (lambda: s.set_wall_reaction((0.1, float("nan"))), _lib.LbmpmError),
           (lambda: s.set_wall_reaction(W.RATES, too_high), _lib.LbmpmError), (lambda: s.set_wall_reaction(W.RATES), _lib.LbmpmError),
           (lambda: s.set_wall_reaction((0.1, 0.2, 0.3)), ValueError), (lambda: s.set_wall_reaction(W.RATES, c["minerals"][1:]), ValueError),
           (lambda: s.set_wall_reaction(None, c["minerals"]), ValueError), (lambda: s.set_wall_reaction(0.1, c["minerals"].astype(float)), ValueError)]
    for call, kind in bad:
        with pytest.raises(kind) as e:
            call()
        if kind is _lib.LbmpmError:
            assert e.value.status == _lib.ERR_INVALID, str(e.value)
    with pytest.raises(_lib.LbmpmError, match=r"\(z, y, x\) = \(%d, %d, %d\)" % (z, y, x)):
        s.set_wall_reaction(W.RATES, too_high)
    fluid_only = np.array(c["minerals"])
    fluid_only[c["dom"] == 1] = 7                    # classes at fluid cells are not read
    s.set_wall_reaction(W.RATES, fluid_only)
    assert s.wall_reaction.tolist() == W.RATES.tolist() and s.steps_done == 3
    same(state(s, nT), before, "after the refused calls")
    s.close()
    cl = W.start(RK3DCSFCluster(c["dom"], c["par"], nslabs=2, tracers=c["kw"]), c)
    cl.step(1)
    before = state(cl, nT)
    far = np.array(c["minerals"])
    zs = [int(v) for v in np.argwhere(c["dom"][7] != 1)[3]]
    far[7, zs[0], zs[1]] = 5                         # a solid cell the first slab does not hold: no slab may change
    for call in (lambda: cl.set_wall_reaction(W.RATES, far), lambda: cl.set_wall_reaction(-1.0), lambda: cl.set_wall_reaction(W.RATES)):
        with pytest.raises(_lib.LbmpmError) as e:
            call()
        assert e.value.status == _lib.ERR_INVALID
    assert all(sl.wall_reaction.tolist() == W.RATES.tolist() for sl in cl.slabs)
    same(state(cl, nT), before, "cluster, after the refused calls")
    cl.close()
