"""The three working loops of the kernel-level drop-in path (tests/test_dropin_gpu.py: the same tables and kernel sequences) beyond one
block of 64 columns and on node counts that are no multiple of the 256-node tile, against the CPU oracles.

The golden captures of the real drivers stop at nx = 34, so no boundary-row kernel of these loops meets a second workgroup there.  The
oracles (oracle/rk.py, oracle/sc.py) are pinned to those captures at 1e-11 (tests/test_oracle_rk.py, tests/test_oracle_sc.py) and take
any domain: here porous images 130 columns wide -- three blocks of 64 columns, the last of two -- and a few tens of rows high.  The
tolerance is the 1e-9, field-relative, at which the fused solvers are held to the same oracles (test_rk2d_gpu.py,
test_ragged_sizes_gpu.py)."""
import numpy as np
import pytest

from helpers import rel_err
from test_dropin_gpu import (CSF_FIELDS, EFS_FIELDS, SC_FIELDS, csf_sequence, csf_table, efs_sequences, original_sequences, rt, run,  # noqa: F401
                             sc_table)
from test_ragged_sizes_gpu import SC_DENS, SC_ORIGINAL, TAUS, _image, _populations

pytestmark = pytest.mark.gpu
NX = 130
TOL = 1e-9


def compare(t, o, fields, alias, what):
    worst = {}
    for key, entry in fields.items():
        want = getattr(o, alias.get(key, key))
        assert np.isfinite(want).all(), (what, key)                # (rel_err masks what is not finite on both sides)
        worst[key] = rel_err(t.host(entry), want)
    print(what, " ".join("%s=%.1e" % kv for kv in worst.items()))
    for key, e in worst.items():
        assert e < TOL, "%s %s rel err %.3e" % (what, key, e)


# ------------------------------------------------------------------------------------------------ colour gradient, CSF
CSF_CONFIGS = {"vinlet-pout-w2-mrt": dict(inlet="Neumann", outlet="Dirichlet", wetting=2, relax="MRT"),
               "pinlet-conv-w1-srt": dict(inlet="Dirichlet", outlet="Convective", wetting=1, relax="SRT"),
               "vinlet-conv-w1-mrt": dict(inlet="Neumann", outlet="Convective", wetting=1, relax="MRT"),
               "pinlet-pout-w2-srt": dict(inlet="Dirichlet", outlet="Dirichlet", wetting=2, relax="SRT")}


@pytest.mark.parametrize("name", list(CSF_CONFIGS))
def test_colour_gradient_loop_wide(rt, name):
    """velocity / pressure inlet, pressure / convective outlet, wetting 1 / 2, SRT / MRT on 130 x 40 .. 43 porous images: all twelve fields after
    steps 1 and 12, the two neighbour tables as their kernels fill them against the oracle's set-up"""
    from openlbmpm_amd.geometry import initial_densities_rk
    ny = 40 + list(CSF_CONFIGS).index(name)
    dom = _image(NX, ny, NX + ny, 6)
    rR, rB = initial_densities_rk(dom, True, 6)
    yy, xx = np.mgrid[0:dom.shape[0], 0:dom.shape[1]]
    ripple = 1.0 + 1.0e-3 * np.sin(0.37 * xx + 0.11 * yy)          # (no exact ties in the wetting rules: see test_rk2d_ragged)
    par = dict(CSF_CONFIGS[name], theta=75.0, tauR=0.9, tauB=1.1)
    t, o = csf_table(rt, dom, par, rR * ripple, rB * ripple)
    assert o.nx == NX and o.N % 256 != 0 and o.N > 2 * 256 and o.W > 256 and o.Wf > 0, (o.N, o.W, o.Wf)
    assert np.array_equal(t.host("neighboringNodes"), o.nbr)
    assert np.array_equal(t.host("neighboringWettingNodes"), o.nbrWet[:8 * o.W])
    seq = csf_sequence(o.p, o.Wf > 0)
    done = 0
    for step in (1, 12):
        for _ in range(step - done):
            run(rt, "rk", t, seq)
        o.run(step - done)
        done = step
        compare(t, o, CSF_FIELDS, {}, "%s %s step %d" % (name, dom.shape, step))


# ------------------------------------------------------------------------------------------------ Shan-Chen family
def sc_case(dom, cfg):
    """parameters, the oracle and the compact populations [2][N][9] both start from: no equilibrium at rest, varying along x (_populations of
    test_ragged_sizes_gpu.py tells why the rows the Chang inlet keeps go unseen otherwise)"""
    from oracle.sc import DEFAULT_PARAMS, SCOracle, initial_densities
    par = dict(DEFAULT_PARAMS, **dict(cfg, **SC_DENS))
    f = _populations(dom, initial_densities(dom, True, par))
    o = SCOracle(dom, par, image=True, f_init=f)
    assert o.nx == NX and o.N % 256 != 0 and o.N > 2 * 256, o.N
    return par, o, np.ascontiguousarray(f.reshape(2, -1, 9)[:, dom.reshape(-1) == 1, :])


EFS_CONFIGS = {"scheme4-mrt-convective": dict(inter="EFS", relax="MRT", outlet="Convective", scheme=4, **TAUS),
               "scheme8-srt-dirichlet": dict(inter="EFS", relax="SRT", outlet="Dirichlet", scheme=8, **TAUS),
               "scheme10-srt": dict(inter="EFS", relax="SRT", outlet="Convective", scheme=10, **TAUS),
               "chang-inlet": dict(inter="EFS", relax="SRT", method="Chang", outlet="Convective", **TAUS),
               "freeflow-outlet": dict(inter="EFS", relax="SRT", method="ZouHe", outlet="Freeflow", **TAUS)}


@pytest.mark.parametrize("name", list(EFS_CONFIGS))
def test_explicit_forcing_loop_wide(rt, name):
    ny = 61 + list(EFS_CONFIGS).index(name)
    dom = _image(NX, ny, NX * 3 + ny, 20)
    par, o, f0 = sc_case(dom, EFS_CONFIGS[name])
    t, N, f0, tau, scheme = sc_table(rt, dom, par, True, f0=f0)
    assert N == o.N and np.array_equal(t.host("neighboringNodes"), o.nbr)
    if scheme != 4:
        assert np.array_equal(t.host("isoNodes"), o.nbrX)
    before, loop = efs_sequences(t, par, f0, tau, scheme)
    run(rt, "sc", t, before)                                   # (the oracle has done this part when it is made: sc_efs_prepare)
    for passes in (1, 10):
        for _ in range(passes - o.iterations):
            run(rt, "sc", t, loop)
        o.run(passes - o.iterations)
        compare(t, o, EFS_FIELDS, dict(ueqx="ux", ueqy="uy", fforce="ff"), "%s %s pass %d" % (name, dom.shape, passes))


SC_CONFIGS = {"zouhe-inlet": dict(SC_ORIGINAL, method="ZouHe", outlet="Convective"), "chang-inlet": dict(SC_ORIGINAL, method="Chang", outlet="Convective")}


@pytest.mark.parametrize("name", list(SC_CONFIGS))
def test_original_shan_chen_loop_wide(rt, name):
    ny = 63 + list(SC_CONFIGS).index(name)
    dom = _image(NX, ny, NX * 3 + ny, 20)
    par, o, f0 = sc_case(dom, SC_CONFIGS[name])
    t, N, f0, tau, _ = sc_table(rt, dom, par, False, f0=f0)
    assert N == o.N and np.array_equal(t.host("neighboringNodes"), o.nbr)
    head, tail = original_sequences(t, par)
    for passes in (1, 10):
        for _ in range(passes - o.iterations):
            run(rt, "sc", t, head + tail)
        o.run(passes - o.iterations)
        compare(t, o, SC_FIELDS, {}, "%s %s pass %d" % (name, dom.shape, passes))
