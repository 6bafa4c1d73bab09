"""The steady path of rk3dq_fused (csrc/rk3dq.h): a wave whose cells pull from one colour only, on a plane without a boundary rule, takes
rho_R = rho or 0 and phi = +-1 as constants of the colour and runs neither the Zou-He closures nor the division; rim cells in such a
neighbourhood take phi from the mask bit and the combined row flag.  Every dropped operation is exact (fma(1, g, s) = s + g, x / x = 1,
adding +0), so the kernel is held to what it was held to before -- the oracle, the 38-value kernels, the slab-decomposed run -- in
states where steady, mixed and Zou-He planes lie next to each other, and to the exact values the constants stand for.

Lattices: the two of tests/param_points.py (64 x 9 x 22 the whole-segment instance, 70 x 9 x 22 the ragged one) and 128 x 16 x 24 with
side walls (two tiles along x and along y: rim rows and rim columns of two tiles meet)."""
import numpy as np
import pytest

import param_points as P
from helpers import rel_err

pytestmark = pytest.mark.gpu
TOL_ORACLE = 1e-10               # the issue's; tests/test_rk3d_gpu.py::TOL
TOL_38 = 1e-11                   # tests/test_rk3d_gpu.py::test_q23_storage_equals_the_38_value_kernels_to_roundoff
FIELDS = ("rhoR", "rhoB", "phi", "vx", "vy", "vz")
CHECKPOINTS = (1, P.STEPS)

LATTICES = ("64", "70", "128w")
STATES = ("front", "red", "both")
_VP, _PP, _PC, _VC = P._VP, P._PP, P._PC, dict(inlet="Neumann", outlet="Convective")
# relaxation x inlet with the pressure outlet on every lattice; the convective outlet on the 64-wide one (the masks of its planes 0 .. 3 coincide)
CASES = [(lat, st, relax, bc) for lat in LATTICES for st in STATES for relax in ("SRT", "MRT") for bc in (_VP, _PP)] + \
        [("64", st, relax, bc) for st in STATES for relax, bc in (("MRT", _PC), ("SRT", _VC))]


def _id(v):
    return "%s-%s" % (v["inlet"][0], v["outlet"][0]) if isinstance(v, dict) else str(v)


_made = {}


def _lattice(lat):
    if lat not in _made:
        if lat == "128w":
            from openlbmpm_amd.geometry import porous_spheres
            dom = porous_spheres(128, 16, 24, porosity=0.72, rmin=2.0, rmax=4.0, seed=17, nbuf=4, walls=True)
            assert dom.shape == (24, 16, 128) and not dom[4:-4, 0].any() and not dom[4:-4, :, 0].any()       # (walls along the core planes)
            zz, yy, xx = np.mgrid[0:24, 0:16, 0:128]
            w = 0.5 + 0.3 * np.sin(0.31 * xx + 0.47 * yy + 0.23 * zz) * np.cos(0.17 * xx - 0.29 * zz)
            _made[lat] = dom, np.where(dom == 1, w, 0.0), np.where(dom == 1, 1.05 - w, 0.0)
        else:
            _made[lat] = P.lattice_3d(int(lat))
    return _made[lat]


def _state(lat, state):
    """front: red below a flat interface three planes from the inlet (the top), so that steady, mixed and Zou-He planes are adjacent"""
    dom, rR, rB = _lattice(lat)
    fluid = dom == 1
    if state == "both":
        return dom, rR, rB
    if state == "red":
        return dom, np.where(fluid, 1.0, 0.0), np.zeros(dom.shape)
    nz = dom.shape[0]
    red = np.arange(nz)[:, None, None] < nz - 1 - 3
    return dom, np.where(fluid & red, 1.0, 0.0), np.where(fluid & ~red, 1.0, 0.0)


def _par(relax, bc, **moved):
    p = P.params(P.RK3D, "A", dict(relax=relax, **bc), **moved)
    return {k: v for k, v in p.items() if k not in ("storage", "nx")}


def _run(dom, rR, rB, par, ranks=1, kernel="rk3dq_fused"):
    from openlbmpm_amd.rk3d import RK3DCluster
    c = RK3DCluster(dom, ranks, par)
    assert c.slabs[0].dominant_kernel == kernel, c.slabs[0].dominant_kernel
    c.set_density(rR, rB)
    out = {}
    for n in CHECKPOINTS:
        c.step(n - c.slabs[0].steps_done); c.observe()
        out[n] = {f: c.get(f) for f in FIELDS}
    c.close()
    return out


_single = {}


def _q23(lat, state, relax, bc, monkeypatch):
    """the single-domain run of the 23-value storage: computed once per case, shared by the tests, never changed"""
    key = (lat, state, relax, bc["inlet"], bc["outlet"])
    if key not in _single:
        for k in ("LBMPM_RK3D_LAYOUT", "LBMPM_RK3D_STORAGE"):
            monkeypatch.delenv(k, raising=False)
        dom, rR, rB = _state(lat, state)
        _single[key] = _run(dom, rR, rB, _par(relax, bc))
    return _single[key]


def _worst(got, ref):
    umax = max(max(float(np.max(np.abs(ref[f]))) for f in ("vx", "vy", "vz")), 1e-300)
    d = {f: rel_err(got[f], ref[f], scale=umax if f[0] == "v" else None) for f in FIELDS}
    f = max(d, key=d.get)
    return d[f], f


@pytest.mark.parametrize("lat,state,relax,bc", CASES, ids=_id)
def test_against_the_oracle(lat, state, relax, bc, monkeypatch):
    from oracle.rk3d import RK3DOracle
    got = _q23(lat, state, relax, bc, monkeypatch)
    dom, rR, rB = _state(lat, state)
    o = RK3DOracle(dom, rR, rB, _par(relax, bc))
    done = 0
    for n in CHECKPOINTS:
        o.run(n - done); done = n
        o.macro()
        e, f = _worst(got[n], {k: o.field(k) for k in FIELDS})
        print("%s %s %s %s step %d: %.2e (%s)" % (lat, state, relax, _id(bc), n, e, f))
        assert e < TOL_ORACLE, (f, e, n)


@pytest.mark.parametrize("lat,state,relax,bc", [c for c in CASES if c[0] != "70" and c[3]["outlet"] != "Convective"], ids=_id)
def test_against_the_38_value_kernels(lat, state, relax, bc, monkeypatch):
    """(the 38-value compact storage takes lattices of whole 64-cell segments and the pressure outlet)"""
    got = _q23(lat, state, relax, bc, monkeypatch)
    monkeypatch.setenv("LBMPM_RK3D_STORAGE", "38")
    dom, rR, rB = _state(lat, state)
    ref = _run(dom, rR, rB, _par(relax, bc), kernel="rk3dc_fused")
    for n in CHECKPOINTS:
        e, f = _worst(got[n], ref[n])
        print("%s %s %s %s step %d: %.2e (%s)" % (lat, state, relax, _id(bc), n, e, f))
        assert e < TOL_38, (f, e, n)


@pytest.mark.parametrize("lat,state,relax,bc", CASES, ids=_id)
def test_three_slabs_equal_the_single_domain_bitwise(lat, state, relax, bc, monkeypatch):
    want = _q23(lat, state, relax, bc, monkeypatch)
    dom, rR, rB = _state(lat, state)
    got = _run(dom, rR, rB, _par(relax, bc), ranks=3)
    for n in CHECKPOINTS:
        for f in FIELDS:
            assert np.array_equal(got[n][f], want[n][f]), (f, n)


@pytest.mark.parametrize("lat,relax,bc", [(lat, relax, _VP) for lat in LATTICES for relax in ("SRT", "MRT")] + [("64", "SRT", _VC), ("64", "MRT", _VC)],
                         ids=_id)
def test_an_all_red_lattice_stays_exactly_red(lat, relax, bc, monkeypatch):
    """After P.STEPS steps rho_B is exactly 0 and phi exactly 1 on every fluid cell that no blue can have reached -- the constants of the
    steady path, and what k + a = t and x / x = 1 gave before it.  The velocity inlet brings no blue (its blue velocity acts on a
    density that is not there).  The pressure outlet does: the library takes positive outlet densities only, so blue enters on plane
    z = 1 and streams one plane per step; with it the planes z >= 2 + P.STEPS are held, with the convective outlet every fluid cell."""
    for k in ("LBMPM_RK3D_LAYOUT", "LBMPM_RK3D_STORAGE"):
        monkeypatch.delenv(k, raising=False)
    dom, rR, rB = _state(lat, "red")
    got = _run(dom, rR, rB, _par(relax, bc))[P.STEPS]
    held = dom == 1
    if bc["outlet"] != "Convective":
        held[:2 + P.STEPS] = False
    assert held[2 + P.STEPS:].sum() > 1000
    assert np.all(got["rhoB"][held] == 0.0), float(np.max(np.abs(got["rhoB"][held])))
    assert np.all(got["phi"][held] == 1.0), float(np.max(np.abs(got["phi"][held] - 1.0)))
    assert np.all(got["rhoR"][held] > 0.5)
