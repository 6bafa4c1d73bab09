"""The paths of the 2-D Shan-Chen solver (csrc/sc2d.hip) that production runs take: the hipGraph replay of 64 captured steps
(run_steps: at most 2^18 nodes, ExplicitScheme 4, at least 192 steps per call) and runs with diagnostics off (keep_force == 0, what the
benchmark times).  A replayed run must equal the run of direct launches (LBMPM_NO_GRAPH=1) bit for bit, with every boundary kernel that
carries state from step to step (Chang inlet rows, convective outlet rows, the free-flow copy kernel), over repeated calls on one context;
a run without diagnostics must leave the same populations as a run with them.  Lattice: a seeded porous image 70 cells wide (two tile
columns, 64 + 6) and 82 rows high (tiles are 64 x 4: a partial tile row), 20 buffer rows at either end; the runs start from populations
on the densities of oracle.sc.initial_densities that vary along x and are no equilibrium at rest (test_ragged_sizes_gpu._populations:
only then do the rows that the Chang inlet keeps from step to step change its result)."""
import numpy as np
import pytest

from test_ragged_sizes_gpu import SC_ORIGINAL, SIZES_WIDE, TAUS, _image, _populations
from test_sc2d_gpu import _compare

pytestmark = pytest.mark.gpu

NX, NY, NBUF, SEED = 70, 82, 20, 11
DENS = dict(rho0=1.0, rho1=1.0, bg0=0.15, bg1=0.15)
SC = dict(SC_ORIGINAL)      # (tau0, tau1 != 1 here and below: see test_ragged_sizes_gpu.TAUS)
CONFIGS = {
    "sc-zouhe-dir": dict(SC, method="ZouHe", outlet="Dirichlet", tau0=1.0, tau1=1.0),      # (with TAUS the reference loop turns NaN after 500 steps)
    "sc-chang-conv": dict(SC, method="Chang", outlet="Convective"),
    "efs-srt-zouhe-dir": dict(inter="EFS", relax="SRT", method="ZouHe", outlet="Dirichlet", **TAUS),
    "efs-mrt-zouhe-conv": dict(inter="EFS", relax="MRT", method="ZouHe", outlet="Convective", tau0=1.0, tau1=0.8),
    "efs-srt-chang-dir": dict(inter="EFS", relax="SRT", method="Chang", outlet="Dirichlet", **TAUS),
    "efs-srt-zouhe-free": dict(inter="EFS", relax="SRT", method="ZouHe", outlet="Freeflow", **TAUS),
}
STATE = ("f0", "f1", "rho0", "rho1")
ALIAS = dict(ueqx="ux", ueqy="uy")


def _fields(par):
    return STATE + ("vx", "vy", "Fx0", "Fx1", "Fy0", "Fy1") + (("ueqx", "ueqy") if par["inter"] == "EFS" else ())


def _lattice(nx=NX, ny=NY, seed=SEED, populations=True):
    """the domain and its initial state: populations [2][ny][nx][9], or the densities themselves for set_density"""
    from oracle.sc import initial_densities
    dom = _image(nx, ny, seed, NBUF)
    rho = initial_densities(dom, True, dict(DENS))
    return dom, (_populations(dom, rho) if populations else rho)


def _solver(dom, init, par, diagnostics=True):
    from openlbmpm_amd.sc2d import SC2DSolver
    s = SC2DSolver(dom, dict(par, scheme=par.get("scheme", 4)), diagnostics=diagnostics)
    if init.ndim == 4:
        s.set_pdf(init[0], init[1])
    else:
        s.set_density(init[0], init[1])
    return s


def _direct(monkeypatch, s, n):
    """n steps of direct launches (the variable is read on every call of step())"""
    with monkeypatch.context() as m:
        m.setenv("LBMPM_NO_GRAPH", "1")
        s.step(n)


def _same(a, b, names, label):
    for f in names:
        x, y = a.get(f), b.get(f)
        assert np.isfinite(x).all(), (label, f)
        assert np.array_equal(x, y), "%s: field %s differs in %d values, max |diff| %.3e" % (label, f, np.count_nonzero(x != y), np.nanmax(np.abs(x - y)))


def _ripple(dom, rho):
    yy, xx = np.mgrid[0:dom.shape[0], 0:dom.shape[1]]
    return rho * (1.0 + 1.0e-2 * np.sin(0.41 * xx + 0.23 * yy))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_replay_equals_direct_launches_over_repeated_calls(name, monkeypatch):
    """step(200), step(1), step(200), step(192) on one context: the first long call captures the graph, the third starts on the other half
    of the fA / fB ping-pong (one more direct step before the replay), the fourth finds the graph where it was captured and reuses it.
    After every call all fields equal those of a context stepped by direct launches, bit for bit, and the counter of replays says which
    path ran; 200 steps in, the replayed run is also held against the CPU oracle."""
    from oracle.sc import SCOracle
    par = CONFIGS[name]
    dom, init = _lattice()
    G, D = _solver(dom, init, par), _solver(dom, init, par)
    total = 0
    for call, n in enumerate((200, 1, 200, 192)):
        before = G.graph_launches
        G.step(n)
        _direct(monkeypatch, D, n)
        total += n
        label = "%s call %d (%d steps)" % (name, call, total)
        assert G.steps_done == total and D.steps_done == total, label
        assert D.graph_launches == 0, label
        if n == 1:
            assert G.graph_launches == before, label
        else:
            assert G.graph_launches > before, label
        _same(G, D, _fields(par), label)
        if call == 0:
            o = SCOracle(dom, dict(par, **DENS), image=True, f_init=init).run(n)
            _compare(G, par["inter"] == "EFS", lambda f: getattr(o, ALIAS.get(f, f)), label)
    G.close(); D.close()


@pytest.mark.parametrize("name", ["sc-chang-conv", "efs-mrt-zouhe-conv"])
@pytest.mark.parametrize("extra", [0, 1], ids=["even", "odd"])
def test_new_densities_under_a_captured_graph(name, extra, monkeypatch):
    """set_density on a context that has replayed, then step(200): the first step is special again (EFS initialisation, the seed of the
    Chang rows, p.first of the convective outlet) and must not come from the graph; the result is that of a fresh context.  With one extra
    step before set_density the new run meets the graph on the other half of the ping-pong."""
    par = CONFIGS[name]
    dom, rho = _lattice(populations=False)
    other = _ripple(dom, rho)
    A = _solver(dom, _populations(dom, rho), par)
    A.step(200)
    if extra:
        A.step(extra)
    before = A.graph_launches
    assert before > 0
    A.set_density(other[0], other[1])
    A.step(200)
    assert A.graph_launches > before and A.steps_done == 200
    B = _solver(dom, other, par)
    B.step(200)
    _same(A, B, _fields(par), name + " re-initialised vs fresh (replayed)")
    C = _solver(dom, other, par)
    _direct(monkeypatch, C, 200)
    _same(A, C, _fields(par), name + " re-initialised vs fresh (direct)")
    A.close(); B.close(); C.close()


@pytest.mark.parametrize("name", ["sc-chang-conv", "efs-mrt-zouhe-conv"])
def test_graph_is_captured_again_when_diagnostics_are_switched_on(name, monkeypatch):
    """keep_force is frozen into the captured kernel arguments: a context created without diagnostics replays 200 steps, switches them
    on and replays 200 more from a new capture.  Populations and densities equal those of 400 direct steps with diagnostics on from the
    start."""
    par = CONFIGS[name]
    dom, init = _lattice()
    A = _solver(dom, init, par, diagnostics=False)
    A.step(200)
    first = A.graph_launches
    assert first > 0
    A.enable_diagnostics(True)
    A.step(200)
    assert A.graph_launches > first and A.steps_done == 400
    D = _solver(dom, init, par)
    _direct(monkeypatch, D, 400)
    assert D.graph_launches == 0
    _same(A, D, STATE, name)
    A.close(); D.close()


def _off_then_on(dom, init, par, n, monkeypatch, replayed=None):
    """n steps on a context that never enabled diagnostics, then diagnostics and one step, against n + 1 direct steps with diagnostics."""
    A = _solver(dom, init, par, diagnostics=False)
    A.step(n)
    if replayed is not None:
        assert (A.graph_launches > 0) == replayed
    A.enable_diagnostics(True)
    A.step(1)
    B = _solver(dom, init, par)
    _direct(monkeypatch, B, n + 1)
    assert A.steps_done == B.steps_done == n + 1
    # original Shan-Chen: u and F come from the force of the step itself.  EFS: u of a step is built with the force the step BEFORE
    # stored, which a diagnostics-off step does not keep (it stores row 3 for the convective outlet only) -- left out there
    _same(A, B, STATE if par["inter"] == "EFS" else _fields(par), "%s N=%d" % (sorted(par.items()), n))
    A.close(); B.close()


@pytest.mark.parametrize("n", [30, 200], ids=["direct", "replayed"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_diagnostics_off_runs_compute_the_same_state(name, n, monkeypatch):
    """The kernels' keep_force == 0 branches (no load of the last force, no store of this one): N steps without diagnostics, then
    enable_diagnostics and one step to read the state, equal N + 1 steps with diagnostics in f and rho of both components, bit for bit.
    For EFS vx, vy and F of that last step are not compared: they use the force the previous step stored, and a diagnostics-off
    step stores none."""
    dom, init = _lattice()
    _off_then_on(dom, init, CONFIGS[name], n, monkeypatch, replayed=(n >= 192))


@pytest.mark.parametrize("sweeps", ["1", "2"])
@pytest.mark.parametrize("relax", ["SRT", "MRT"])
@pytest.mark.parametrize("scheme", [8, 10])
def test_diagnostics_off_iso_schemes(scheme, relax, sweeps, monkeypatch):
    """the same for ExplicitScheme 8 / 10 in both schedules (sc2d_iso_fused; sc2d_iso_psi + sc2d_iso_collide); scheme 10 runs without
    boundary kernels, so only with the Dirichlet setting (as in test_iso_schemes_one_sweep_equals_two_sweeps)"""
    monkeypatch.setenv("LBMPM_SC2D_ISO_SWEEPS", sweeps)
    dom, init = _lattice()
    for outlet in ("Dirichlet", "Convective"):
        if scheme == 10 and outlet == "Convective":
            continue
        _off_then_on(dom, init, dict(inter="EFS", relax=relax, method="ZouHe", outlet=outlet, scheme=scheme, **TAUS), 30, monkeypatch, replayed=False)


@pytest.mark.parametrize("name", ["sc-chang-conv", "efs-mrt-zouhe-conv"])
def test_diagnostics_off_above_the_streaming_store_threshold(name, monkeypatch):
    """more than 2^18 nodes: the instantiation with non-temporal stores, tiles walked in staggered XCD bands"""
    nx, ny = SIZES_WIDE[-1]
    assert nx == 2241
    dom, init = _lattice(nx, ny + 30, nx * 3 + ny)
    assert (nx + 31) // 32 * 32 * dom.shape[0] > 1 << 18
    _off_then_on(dom, init, CONFIGS[name], 6, monkeypatch, replayed=False)
