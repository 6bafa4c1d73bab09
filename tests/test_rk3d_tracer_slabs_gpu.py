"""D3Q7 tracers on z-slabs of the 3-D CSF model (lbmpm_rk3dcsf_tracer_configure_slab; RK3DCSFCluster(..., tracers=...)): per tracer one
population crosses a z-face each way, and it rides the slabs' population message (LBMPM_CSF_MSG_PDF) behind the ten flow runs.

The yardstick is the undivided lattice on RK3DCSFSolver (held to the restatement and the 2-D oracle by tests/test_rk3d_tracer_gpu.py): slabs
do the same arithmetic on the same inputs in the same order, so every comparison is np.array_equal."""
import numpy as np
import pytest

from test_rk3d_csf_gpu import _slab_case, _SLAB_FIELDS
from test_rk3d_tracer_gpu import tracer_case, concentrations, porous_box

pytestmark = pytest.mark.gpu

PAR = dict(theta=55.0, tauB=0.8, velocityZR=0.0, velocityZB=-3.0e-3, sigma=0.06)
FLOW = ("fR", "phi", "Fz", "rec_rhoB", "rec_vz")
UNEVEN = [0, 9, 23, 44]
MSG_PDF, MSG_PHI, MSG_NORMAL = 0, 1, 2


def cut_walls(dom, cuts):
    """per cut c (between the planes c - 1 and c; the seam of the ring as c = 0): fluid cells of plane c - 1 under a solid of plane c,
    fluid cells of plane c above a solid of plane c - 1, fluid cells on both sides"""
    out = {}
    for c in cuts[:-1]:
        below, above = dom[c - 1] == 1, dom[c] == 1
        out[c] = (int((below & ~above).sum()), int((~below & above).sum()), int((below & above).sum()))
    return out


def test_the_cuts_of_the_sample_cross_walls():
    """what the comparison below rests on, from the mask alone: bounce-back across a cut in both directions, and fluid across every cut"""
    from openlbmpm_amd.rk3dcsf import slab_cuts
    dom, _, _ = _slab_case()
    four = cut_walls(dom, slab_cuts(dom.shape[0], 4))
    assert slab_cuts(dom.shape[0], 4) == [0, 11, 22, 33, 44]
    # (the three cuts; key 0 is the seam of the ring between the open planes nz - 1 and 0, which no obstacle reaches)
    assert four[22][0] == 12 and four[33][1] == 12 and all(four[z][2] == 308 for z in (11, 22, 33)) and four[0][2] == 320, four
    uneven = cut_walls(dom, UNEVEN)
    assert uneven[9][0] == 12 and uneven[23][0] == 12, uneven


def _start(s, rR, rB, c0):
    s.set_macro(rR, rB)
    for k in range(len(c0)):
        s.set_concentration(k, c0[k])


def _tracers_equal(a, c, nT, what):
    for k in range(nT):
        ca, cc = a.get_concentration(k), c.get_concentration(k)
        assert np.array_equal(ca, cc), (what, "concentration", k, float(np.max(np.abs(ca - cc))))
        ga, gc = a.get_tracer_pdf(k), c.get_tracer_pdf(k)
        assert np.array_equal(ga, gc), (what, "populations", k, float(np.max(np.abs(ga - gc))))


CASES = [
    # slabs or cuts, flow parameters, tracers, overrides of tracer_case
    (2, dict(relax="MRT"), 1, {}),
    (3, dict(relax="SRT"), 3, {}),
    (4, dict(relax="MRT"), 3, dict(dirichlet_inlet=False, free_outlet=False)),
    (UNEVEN, dict(relax="MRT", variant=1), 1, dict(dirichlet_inlet=False, free_outlet=False)),
    (4, dict(relax="SRT", variant=1), 3, {}),
    (UNEVEN, dict(relax="MRT", outlet="Convective"), 3, {}),
    (2, dict(relax="SRT"), 2, dict(dirichlet_inlet=False, free_outlet=False)),
    (4, dict(relax="MRT", inlet="Dirichlet", densityBH=1.0, densityRH=1e-8), 4, {}),
    (UNEVEN, dict(relax="SRT"), 3, dict(reaction_rate=0.0, beta_interface=(0.0, 0.0, 0.0))),
]


@pytest.mark.parametrize("cuts,flow,nT,over", CASES, ids=lambda v: None if isinstance(v, dict) else str(v).replace(" ", ""))
def test_cluster_equals_the_undivided_lattice(cuts, flow, nT, over):
    """every tracer's concentration and populations and the flow, bit for bit, after 1, 2, 3 and 36 steps: SRT and MRT, with and without
    the bulk skip, one to four tracers, the reaction, anisotropic D with off-diagonals, beta_interface != 0 (tracer_case), inlet + outlet
    on and off (off: the seam of the ring carries tracer), the flow's convective outlet and pressure inlet.  Bounce-back across a cut,
    the interface inside the edge planes and a moving, non-uniform concentration at every cut are asserted from the mask and the
    undivided run, so that a message that never arrived cannot go unnoticed."""
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster, RK3DCSFSolver, slab_cuts
    dom, rR, rB = _slab_case()
    nz = dom.shape[0]
    par = dict(PAR); par.update(flow)
    kw, _ = tracer_case(nT, **over)
    c0 = concentrations(dom, nT)
    a = RK3DCSFSolver(dom, par)
    a.configure_tracers(**kw)
    c = RK3DCSFCluster(dom, par, diagnostics=True, tracers=kw, **(dict(nslabs=cuts) if isinstance(cuts, int) else dict(cuts=cuts)))
    zc = slab_cuts(nz, cuts) if isinstance(cuts, int) else cuts
    assert c.cuts == zc and c.num_tracers == nT
    walls = cut_walls(dom, zc)
    assert all(v[2] > 0 for v in walls.values()), walls                      # fluid on both sides of every cut and of the seam
    if len(zc) - 1 == 4:
        assert any(v[0] > 0 for v in walls.values()) and any(v[1] > 0 for v in walls.values()), walls
    elif zc == UNEVEN:
        assert walls[9][0] > 0 and walls[23][0] > 0, walls
    for k in range(nT):                              # the initial concentration is not uniform across any cut or the seam
        for z in zc[:-1]:
            both = (dom[z - 1] == 1) & (dom[z] == 1)
            assert np.any(c0[k][z - 1][both] != c0[k][z][both]), (k, z)
    _start(a, rR, rB, c0); _start(c, rR, rB, c0)
    _tracers_equal(a, c, nT, "start")
    for n in (1, 2, 3, 36):
        a.step(n - a.steps_done); c.step(n - c.steps_done)
        _tracers_equal(a, c, nT, "step %d" % n)
        for f in FLOW:
            assert np.array_equal(a.get(f), c.get(f)), (n, f)
    # the interface lies inside the edge planes of a cut, and the tracers at every cut's edge planes have moved
    G = np.sqrt(a.get("Gx") ** 2 + a.get("Gy") ** 2 + a.get("Gz") ** 2)
    assert any(np.any(G[z - 1] > 1e-8) and np.any(G[z] > 1e-8) for z in zc[1:-1]), [float(G[z].max()) for z in zc[1:-1]]
    for k in range(nT):
        ck = a.get_concentration(k)
        assert np.all(np.isfinite(ck))
        for z in zc[1:-1]:
            for e in (z - 1, z):
                fl = dom[e] == 1
                assert np.any(ck[e][fl] != c0[k][e][fl]), (k, e)
    a.close(); c.close()


@pytest.mark.parametrize("relax,variant", [("MRT", 0), ("SRT", 0), ("MRT", 1)])
def test_the_flow_is_untouched_on_slabs(relax, variant):
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster
    dom, rR, rB = _slab_case()
    par = dict(PAR, relax=relax, variant=variant)
    kw, _ = tracer_case(2)
    c0 = concentrations(dom, 2)
    a = RK3DCSFCluster(dom, par, nslabs=3, diagnostics=True, tracers=kw)
    b = RK3DCSFCluster(dom, par, nslabs=3, diagnostics=True)
    _start(a, rR, rB, c0); b.set_macro(rR, rB)
    for n in (1, 2, 40):
        a.step(n - a.steps_done); b.step(n - b.steps_done)
        for f in _SLAB_FIELDS:
            assert np.array_equal(a.get(f), b.get(f)), (n, f)
        assert a.bulk_cells == b.bulk_cells
    a.close(); b.close()


@pytest.mark.parametrize("cuts", [[0, 11, 22, 33, 44], UNEVEN])
def test_message_sizes(cuts):
    """face_doubles(MSG_PDF) grows by one double per tracer and fluid cell of the edge plane (counted from the mask), the other two
    messages stay, and what a slab sends is what the slab across the cut (or the seam) expects"""
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster
    dom, _, _ = _slab_case()
    nz = dom.shape[0]
    cells = lambda z: int((dom[z % nz] == 1).sum())
    plain = RK3DCSFCluster(dom, PAR, cuts=cuts)
    for nT in (1, 3, 4):
        kw, _ = tracer_case(nT)
        c = RK3DCSFCluster(dom, PAR, cuts=cuts, tracers=kw)
        n = len(c.slabs)
        for k, (s, p) in enumerate(zip(c.slabs, plain.slabs)):
            z0, z1 = cuts[k], cuts[k + 1]
            # sent: the slab's own edge plane; received: the neighbour's edge plane beyond the face
            assert s.face_doubles(MSG_PDF, 0) - p.face_doubles(MSG_PDF, 0) == nT * cells(z0)
            assert s.face_doubles(MSG_PDF, 1) - p.face_doubles(MSG_PDF, 1) == nT * cells(z1 - 1)
            assert s.face_doubles_in(MSG_PDF, 0) - p.face_doubles_in(MSG_PDF, 0) == nT * cells(z0 - 1)
            assert s.face_doubles_in(MSG_PDF, 1) - p.face_doubles_in(MSG_PDF, 1) == nT * cells(z1)
            for m in (MSG_PHI, MSG_NORMAL):
                for face in (0, 1):
                    assert s.face_doubles(m, face) == p.face_doubles(m, face) and s.face_doubles_in(m, face) == p.face_doubles_in(m, face)
            up = c.slabs[(k + 1) % n]
            for m in (MSG_PDF, MSG_PHI, MSG_NORMAL):
                assert s.face_doubles(m, 1) == up.face_doubles_in(m, 0) and up.face_doubles(m, 0) == s.face_doubles_in(m, 1), (k, m)
        c.close()
    plain.close()


def test_restart_across_cuts():
    """the undivided lattice for 17 steps -> its tracer populations and flow state into a 3-slab cluster -> 13 more steps: the
    uninterrupted 30 steps, bit for bit; and the other way round"""
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster, RK3DCSFSolver
    dom, rR, rB = _slab_case()
    par = dict(PAR, relax="MRT")
    kw, _ = tracer_case(3)
    c0 = concentrations(dom, 3)

    def whole():
        s = RK3DCSFSolver(dom, par)
        s.configure_tracers(**kw)
        return s

    def hand_over(src, dst):
        dst.set_pdf(src.get("fR"), src.get("fB"), force=(src.get("Fx"), src.get("Fy"), src.get("Fz")))
        for k in range(3):
            dst.set_tracer_pdf(k, src.get_tracer_pdf(k))
        _tracers_equal(src, dst, 3, "handed over")

    ref = whole()
    _start(ref, rR, rB, c0)
    ref.step(17)
    c = RK3DCSFCluster(dom, par, nslabs=3, diagnostics=True, tracers=kw)
    hand_over(ref, c)
    ref.step(13); c.step(13)
    _tracers_equal(ref, c, 3, "undivided -> slabs")
    for f in FLOW:
        assert np.array_equal(ref.get(f), c.get(f)), f
    c.close()
    # the other way round
    c = RK3DCSFCluster(dom, par, nslabs=3, diagnostics=True, tracers=kw)
    _start(c, rR, rB, c0)
    c.step(17)
    b = whole()
    hand_over(c, b)
    b.step(13)
    _tracers_equal(ref, b, 3, "slabs -> undivided")
    for f in FLOW:
        assert np.array_equal(ref.get(f), b.get(f)), f
    ref.close(); b.close(); c.close()


@pytest.mark.parametrize("reaction", [False, True])
def test_conservation_on_the_ring(reaction):
    """tests/test_rk3d_tracer_gpu.py::test_conservation on three slabs: no open plane for the tracers, so what leaves a slab through a face
    enters its neighbour (the seam between the last and the first slab included) and the totals over the slabs stay, to that test's
    1e-11 relative"""
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster
    dom, rR, rB = porous_box()
    par = dict(relax="MRT", theta=50.0, tauB=0.8, velocityZR=0.0, velocityZB=-3.0e-3, sigma=0.05)
    kw, _ = tracer_case(3, reaction=reaction, dirichlet_inlet=False, free_outlet=False)
    c0 = concentrations(dom, 3)
    s = RK3DCSFCluster(dom, par, nslabs=3, tracers=kw)
    _start(s, rR, rB, c0)
    total = lambda: np.array([float(np.sum(s.get_concentration(k))) for k in range(3)])
    t0 = total()
    s.step(300)
    t1 = total()
    print("conservation on three slabs (reaction %s): totals %s -> %s" % (reaction, t0, t1))
    if not reaction:
        assert np.all(np.abs(t1 - t0) < 1e-11 * np.abs(t0)), (t0, t1)
    else:
        assert abs((t1[0] - t1[1]) - (t0[0] - t0[1])) < 1e-11 * abs(t0[0]) and abs((t1[0] + t1[2]) - (t0[0] + t0[2])) < 1e-11 * abs(t0[0] + t0[2]), (t0, t1)
        assert t0[0] - t1[0] > 1e-3 * t0[0]
    s.close()


def test_refusals():
    """every wrong call is refused with a status; none of them enqueues a wait (nothing here is ever connected)"""
    import ctypes as C
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster, RK3DCSFSolver, _SlabGeometry, tracer_config
    from openlbmpm_amd import _lib
    from openlbmpm_amd._lib import LbmpmError, ERR_UNSUPPORTED, ERR_INVALID, ERR_STATE
    dom, rR, rB = _slab_case()
    nz = dom.shape[0]
    L = _lib.lib()

    def configure_slab(s, **kw):
        cfg = tracer_config(**kw)
        return L.lbmpm_rk3dcsf_tracer_configure_slab(s._h, C.byref(cfg))

    def slab(z0, z1, **kw):
        g = _SlabGeometry(nz, z0, z1)
        return RK3DCSFSolver(g.cut(dom), PAR, slab=g.slab, **kw), g

    def status(fn, *a, **kw):
        with pytest.raises(LbmpmError) as e:
            fn(*a, **kw)
        return e.value.status

    whole = RK3DCSFSolver(dom, PAR)
    assert configure_slab(whole, num_tracers=1) == ERR_INVALID              # the undivided lattice: lbmpm_rk3dcsf_tracer_configure
    whole.close()
    s, g = slab(0, 22)
    assert configure_slab(s, num_tracers=5) == ERR_INVALID
    assert configure_slab(s, num_tracers=2, reaction_rate=0.1) == ERR_INVALID
    s.ipc_init()                                                            # the transport's shape exists: its slots hold no tracers
    assert configure_slab(s, num_tracers=1) == ERR_STATE
    s.transport_disconnect()
    assert configure_slab(s, num_tracers=1) == 0                            # (nothing of the refusals stuck)
    assert configure_slab(s, num_tracers=1) == ERR_STATE                    # once
    s.close()
    s, g = slab(0, 22)
    s.set_macro(g.cut(rR), g.cut(rB))
    s.stage(0)
    assert configure_slab(s, num_tracers=1) == ERR_STATE                    # inside a step
    s.stage(1); s.stage(2); s.sync()
    assert configure_slab(s, num_tracers=1) == ERR_STATE                    # after a step
    assert status(s.configure_tracers, num_tracers=1) == ERR_UNSUPPORTED    # the undivided lattice's call keeps refusing a slab
    s.close()
    # neighbours that carry different numbers of tracers
    one, g1 = slab(0, 22, tracers=dict(num_tracers=1))
    two, g2 = slab(22, nz, tracers=dict(num_tracers=2))
    for s, g in ((one, g1), (two, g2)):
        s.set_macro(g.cut(rR), g.cut(rB))
    assert status(one.send_to, 1, two, MSG_PDF) == ERR_INVALID and status(two.send_to, 0, one, MSG_PDF) == ERR_INVALID
    blobs = [one.ipc_init(), two.ipc_init()]
    assert status(one.ipc_connect, blobs[1], blobs[1]) == ERR_INVALID and status(two.ipc_connect, blobs[0], blobs[0]) == ERR_INVALID
    assert one.transport == "none" and two.transport == "none"             # nothing mapped
    for s in (one, two):                                                    # both still step by stages
        s.stage(0)
        s.transport_disconnect()
        s.sync()
        s.close()
    cl = RK3DCSFCluster(dom, PAR, nslabs=2, tracers=dict(num_tracers=1))
    with pytest.raises(LbmpmError) as e:
        cl.configure_tracers(num_tracers=1)
    assert e.value.status == ERR_UNSUPPORTED and "slabs" in str(e.value) and "tracers=" in str(e.value)
    cl.close()
