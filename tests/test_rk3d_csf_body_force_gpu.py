"""The body force of the 3-D CSF solver (lbmpm_rk3dcsf_set_body_force; BF instances of csf3d_collide / csf3d_collide_deep) on the GPU.

The reference is tests/body_force_ref.py, a recipe around the unchanged oracle whose own conditions tests/test_body_force_cpu.py holds.
1. parity with the recipe at the points A and B of tests/param_points.py;  2. the bulk path against the full path, bit for bit;
3. off means off;  4. slabs, two processes, the observers however the lattice is cut;  5. restart;  6. observers;  7. physics;
8. refusals."""
import os

import numpy as np
import pytest

import body_force_ref as R
import param_points as P
from helpers import rel_err
from test_rk3d_csf_gpu import TOL, _SLAB_FIELDS, _slab_case, compare_all, solver

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GR, GB = R.G_SETS["G1"]
TRACER = dict(num_tracers=1, diffusion_x=0.12, inlet_concentration=1.0)
ALL_FIELDS = _SLAB_FIELDS + ("rec_vx", "rec_vy")


def same(a, b, fields=ALL_FIELDS, what=""):
    for f in fields:
        x, y = (a[f] if isinstance(a, dict) else a.get(f)), (b[f] if isinstance(b, dict) else b.get(f))
        assert np.array_equal(x, y), (what, f, float(np.max(np.abs(x - y))))


def point_params(point, **over):
    return {k: v for k, v in P.params(P.TABLES["rk3dcsf"], point, **over).items()}


def porous_sample():
    """the sample of tests/test_rk3d_csf_gpu.py::test_porous_sample_against_the_oracle"""
    from openlbmpm_amd.geometry import porous_spheres, initial_densities_rk3d
    dom = porous_spheres(40, 24, 36, porosity=0.7, rmin=3.0, rmax=6.0, seed=7, nbuf=5)
    dom[0] = dom[1]; dom[-1] = dom[-2]
    return (dom,) + tuple(initial_densities_rk3d(dom, 5))


# ------------------------------------------------------------------------------------------------ 1. parity
def check_record(s, ref, what):
    """rec_*: what the first half of the next step makes of the state -- with the body force's half in u.  Uses the reference up"""
    fl = ref.fl
    rec = {f: s.get("rec_" + f) for f in ("fR", "fB", "rhoR", "rhoB", "vx", "vy", "vz", "phi")}
    ref.step_a()
    umax = max(float(np.max(np.abs(ref.field(c)[fl]))) for c in ("vx", "vy", "vz"))
    for f, a in rec.items():
        e = rel_err(a[fl], ref.field(f)[fl], scale=umax if f[0] == "v" else None)
        assert e < TOL, "record view %s: %s %.3e" % (what, f, e)


PARITY = [("blob3", "A", "G1", dict(relax="SRT", inlet="Neumann", outlet="Dirichlet")),
          ("blob3", "A", "G1", dict(relax="MRT", inlet="Dirichlet", outlet="Convective")),
          ("blob3", "B", "G2", dict(relax="MRT", inlet="Neumann", outlet="Dirichlet")),
          ("blob3", "B", "G2", dict(relax="SRT", inlet="Dirichlet", outlet="Convective")),
          ("blob3", "A", "G2", dict(relax="MRT", inlet="Neumann", outlet="Convective", tautype=1)),
          ("blob3", "B", "G1", dict(relax="SRT", inlet="Dirichlet", outlet="Dirichlet", wetting=0)),
          ("porous", "A", "G1", dict(relax="MRT", inlet="Neumann", outlet="Dirichlet")),
          ("porous", "B", "G2", dict(relax="SRT", inlet="Dirichlet", outlet="Convective"))]


@pytest.mark.parametrize("lattice,point,gset,inst", PARITY, ids=lambda v: ",".join(str(x) for x in v.values()) if isinstance(v, dict) else v)
def test_against_the_recipe(lattice, point, gset, inst):
    """every field compare_all holds, after step 1 and step 10, and the record view with the force's half in u; the instances without
    diagnostics and with a tracer leave the same bits"""
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    dom, rR, rB = P.lattice_csf() if lattice == "blob3" else porous_sample()
    par = point_params(point, **inst)
    gr, gb = R.G_SETS[gset]
    opar = {k: v for k, v in par.items() if k != "variant"}
    s = solver(dom, par)
    s.set_body_force(red=gr, blue=gb)
    assert s.body_force == (gr, gb)
    s.set_macro(rR, rB)
    lean = RK3DCSFSolver(dom, par, diagnostics=False, tracers=TRACER)
    lean.set_body_force(red=gr, blue=gb); lean.set_macro(rR, rB)
    lean.set_concentration(0, np.where(dom == 1, 0.5, 0.0))
    ref = R.BodyForceRef(dom, rR, rB, opar, gr, gb)
    first = R.BodyForceRef(dom, rR, rB, opar, gr, gb).run(1)
    s.step(1); ref.run(1)
    w1 = compare_all(s, ref, "%s %s %s, step 1" % (lattice, point, gset))
    check_record(s, first, "after step 1")
    s.step(P.STEPS - 1); ref.run(P.STEPS - 1)
    w10 = compare_all(s, ref, "%s %s %s, step %d" % (lattice, point, gset, P.STEPS))
    check_record(s, ref, "after step %d" % P.STEPS)
    print("%s %s %s %s: worst field-relative difference %.2e after step 1, %.2e after step %d" % (lattice, point, gset, inst, w1, w10, P.STEPS))
    lean.step(P.STEPS)
    same(s, lean, ("fR", "fB", "rhoR", "rhoB", "phi", "Gx", "Gy", "Gz", "Fx", "Fy", "Fz", "rec_vx", "rec_vy", "rec_vz"), "diagnostics off, one tracer")
    # the force is felt: without it the state differs by far more than the tolerance
    plain = solver(dom, par); plain.set_macro(rR, rB); plain.step(P.STEPS)
    assert rel_err(plain.get("fR"), s.get("fR")) > 1000 * TOL
    for x in (s, lean, plain):
        x.close()


# ------------------------------------------------------------------------------------------------ 2. the bulk path
BULK_FIELDS = ("fR", "fB", "rhoR", "rhoB", "phi", "Gx", "Gy", "Gz", "Fx", "Fy", "Fz", "K", "vx", "vy", "vz", "rec_vx", "rec_vy", "rec_vz", "rec_phi")


def bulk_duct():
    """the lattice of tests/test_rk3d_csf_gpu.py::test_the_bulk_skip_is_exact"""
    from openlbmpm_amd.RKColorGradientD3Q19 import duct
    dom = duct(34, 30, 120)
    dom[40:60, 8:20, 10:24] = 0
    zz = np.mgrid[0:120, 0:30, 0:34][0]
    fl = dom == 1
    return dom, np.where(fl & (zz < 84), 1.0, 0.0), np.where(fl & (zz >= 84), 1.0, 0.0)


def bulk_porous(seed=3):
    """... of test_the_bulk_skip_is_exact_in_a_porous_medium"""
    from openlbmpm_amd.geometry import porous_spheres, initial_densities_rk3d
    dom = porous_spheres(72, 56, 120, porosity=0.7, rmin=3.0, rmax=7.0, seed=seed, nbuf=6)
    dom[0] = dom[1]; dom[-1] = dom[-2]
    return (dom,) + tuple(initial_densities_rk3d(dom, 30))


@pytest.mark.parametrize("lattice,relax,on_at", [("duct", "MRT", 0), ("duct", "SRT", 0), ("duct", "MRT", 41), ("porous", "SRT", 3), ("porous", "MRT", 0)])
def test_the_bulk_path_equals_the_full_path(lattice, relax, on_at):
    """variant 0 (deep blocks through csf3d_collide_deep<.., BF>) against variant 1 (every cell through csf3d_collide), bit for bit, with
    both colours accelerated differently while a front moves; on_at > 0: the force comes on when blocks are deep already"""
    dom, rR, rB = bulk_duct() if lattice == "duct" else bulk_porous()
    par = dict(relax=relax, theta=55.0, tauB=0.8, velocityZR=0.0, velocityZB=-4.0e-3, sigma=0.05)
    a = solver(dom, par); b = solver(dom, dict(par, variant=1))
    a.set_macro(rR, rB); b.set_macro(rR, rB)
    shares = []
    for k in (1, 2, 3, 40, 41, 42, 90):
        if a.steps_done == on_at:
            assert on_at == 0 or a.bulk_cells > 0
            a.set_body_force(red=GR, blue=GB); b.set_body_force(red=GR, blue=GB)
        a.step(k - a.steps_done); b.step(k - b.steps_done)
        shares.append(a.bulk_cells / a.num_fluid_nodes)
        assert b.bulk_cells == 0
        same(a, b, BULK_FIELDS, (lattice, relax, on_at, k))
    assert a.bulk_cells > 0 and shares[1] > 0.2 and len(set(shares[1:])) > 1, shares      # the deep kernel ran, the set of deep blocks changed
    assert np.all(np.isfinite(a.get("vz")))
    off = solver(dom, par); off.set_macro(rR, rB); off.step(90)
    assert rel_err(off.get("fR"), a.get("fR")) > 1000 * TOL
    a.close(); b.close(); off.close()


# ------------------------------------------------------------------------------------------------ 3. off means off
@pytest.mark.parametrize("relax", ["SRT", "MRT"])
def test_off_means_off(relax):
    """no call, set_body_force(None), six zeros (negative zeros among them), a force set and removed before the first step: one and the
    same run, bit for bit, on both paths"""
    dom, rR, rB = bulk_duct()
    par = dict(relax=relax, theta=55.0, tauB=0.8, velocityZR=0.0, velocityZB=-4.0e-3, sigma=0.05)
    runs = []
    for how in ("no call", "None", "zeros", "set and removed"):
        s = solver(dom, par)
        if how == "None":
            s.set_body_force(None)
        elif how == "zeros":
            s.set_body_force(red=(0.0, -0.0, 0.0), blue=(-0.0, 0.0, 0.0))
        elif how == "set and removed":
            s.set_body_force(red=GR, blue=GB)
        s.set_macro(rR, rB)
        if how == "set and removed":
            s.set_body_force()
        assert s.body_force == ((0., 0., 0.), (0., 0., 0.))
        s.step(30)
        assert s.bulk_cells > 0
        runs.append(s)
    for s in runs[1:]:
        same(runs[0], s, BULK_FIELDS + ("Gx",), relax)
    for s in runs:
        s.close()


# ------------------------------------------------------------------------------------------------ 4. slabs
SLAB_PARAMS = dict(relax="MRT", theta=55.0, tauB=0.8, velocityZR=0.0, velocityZB=-3.0e-3, sigma=0.06)
SLAB_STEPS = 30


def observers(s):
    """integrals(), change(), clusters(props=True) and tracer_integrals() as arrays"""
    i, c, cl, t = s.integrals(), s.change(), s.clusters(props=True), s.tracer_integrals()
    if i is None:                # (RK3DCSFDistributed: rank 0 holds the whole lattice's tables)
        return {}
    return {"integrals": i.planes, "change": c.planes, "clusters": cl.table, "cluster props": cl.props, "tracer integrals": t.planes}


@pytest.fixture(scope="module")
def undivided():
    """_slab_case under the force with one tracer: the state after 10 steps, the fields and the observers' tables after SLAB_STEPS"""
    dom, rR, rB = _slab_case()
    conc = np.where(dom == 1, 0.5, 0.0)
    s = solver(dom, SLAB_PARAMS, tracers=TRACER)
    s.set_body_force(red=GR, blue=GB)
    s.set_macro(rR, rB); s.set_concentration(0, conc)
    s.step(10)
    s.mark_change()
    at10 = {f: s.get(f) for f in ("fR", "fB", "Fx", "Fy", "Fz")}
    at10["g"] = s.get_tracer_pdf(0)
    s.step(SLAB_STEPS - 10)
    out = dict(dom=dom, rR=rR, rB=rB, conc=conc, at10=at10, at30={f: s.get(f) for f in ALL_FIELDS}, observers=observers(s), conc30=s.get_concentration(0))
    s.close()
    return out


@pytest.mark.parametrize("cuts", [2, 3, "thinnest"])
def test_slabs_equal_the_undivided_lattice(undivided, cuts):
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster
    u = undivided
    nz = u["dom"].shape[0]
    kw = dict(cuts=[0, 4, 8, 12, nz - 4, nz]) if cuts == "thinnest" else dict(nslabs=cuts)
    c = RK3DCSFCluster(u["dom"], SLAB_PARAMS, diagnostics=True, tracers=TRACER, **kw)
    c.set_body_force(red=GR, blue=GB)
    assert c.body_force == (GR, GB) and all(s.body_force == (GR, GB) for s in c.slabs)
    c.set_macro(u["rR"], u["rB"]); c.set_concentration(0, u["conc"])
    c.step(10)
    c.mark_change()
    c.step(SLAB_STEPS - 10)
    same(c, u["at30"], what="slabs %s" % cuts)
    assert np.array_equal(c.get_concentration(0), u["conc30"])
    got = observers(c)
    for k, v in u["observers"].items():
        assert np.array_equal(got[k], v, equal_nan=True), (cuts, k)
    c.close()


_WORKER = '''
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np, torch, torch.distributed as dist
from test_rk3d_csf_gpu import _slab_case
from test_rk3d_csf_body_force_gpu import SLAB_PARAMS, SLAB_STEPS, TRACER, GR, GB, observers
from openlbmpm_amd.rk3dcsf import RK3DCSFDistributed
torch.cuda.set_device(0)
dist.init_process_group("gloo")
dom, rR, rB = _slab_case()
for transport in ("torch", "ipc"):
    d = RK3DCSFDistributed(dom, SLAB_PARAMS, device=0, transport=transport, tracers=TRACER)
    assert (d.transport == "torch") == (transport == "torch"), d.transport
    d.set_body_force(red=GR, blue=GB)
    assert d.body_force == (GR, GB)
    d.set_macro(rR, rB); d.set_concentration(0, np.where(dom == 1, 0.5, 0.0))
    d.step(10); d.mark_change(); d.step(SLAB_STEPS - 10); d.sync()
    for f in ("fR", "fB", "phi", "Fz", "rec_rhoB", "rec_vx", "rec_vy", "rec_vz"):
        g = d.gather(d.get(f))
        if dist.get_rank() == 0:
            np.save(os.path.join(%(out)r, "%%s_%%s.npy" %% (transport, f)), g)
    for k, v in observers(d).items():
        if dist.get_rank() == 0:
            np.save(os.path.join(%(out)r, "%%s_%%s.npy" %% (transport, k.replace(" ", "_"))), v)
    dist.barrier(); d.close(); dist.barrier()
dist.destroy_process_group()
'''


def test_two_processes_equal_the_undivided_lattice(undivided, tmp_path):
    """RK3DCSFDistributed on two ranks that share this GPU (started as tests/test_rk3d_csf_wettability_gpu.py starts them): the staged step with
    the messages through torch.distributed, and lbmpm_rk3dcsf_step_slab over the library's IPC transport"""
    import subprocess
    import sys
    from test_rk3d_gpu import _free_port
    u = undivided
    script = tmp_path / "w.py"
    script.write_text(_WORKER % dict(root=ROOT, out=str(tmp_path)))
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(script)], timeout=300)
    for transport in ("torch", "ipc"):
        for f in ("fR", "fB", "phi", "Fz", "rec_rhoB", "rec_vx", "rec_vy", "rec_vz"):
            assert np.array_equal(u["at30"][f], np.load(tmp_path / ("%s_%s.npy" % (transport, f)))), (transport, f)
        for k, v in u["observers"].items():
            assert np.array_equal(np.load(tmp_path / ("%s_%s.npy" % (transport, k.replace(" ", "_")))), v, equal_nan=True), (transport, k)


# ------------------------------------------------------------------------------------------------ 5. restart
def test_a_restart_with_the_force_continues_bit_for_bit(undivided):
    u = undivided
    s = solver(u["dom"], SLAB_PARAMS, tracers=TRACER)
    s.set_pdf(u["at10"]["fR"], u["at10"]["fB"], force=(u["at10"]["Fx"], u["at10"]["Fy"], u["at10"]["Fz"]))
    s.set_tracer_pdf(0, u["at10"]["g"])
    s.set_body_force(red=GR, blue=GB)
    s.step(SLAB_STEPS - 10)
    same(s, u["at30"], what="restart")
    assert np.array_equal(s.get_concentration(0), u["conc30"])
    s.close()


def test_a_force_changed_mid_run_equals_a_restart_with_the_new_force(undivided):
    u = undivided
    g2r, g2b = R.G_SETS["G2"]
    a = solver(u["dom"], SLAB_PARAMS)
    a.set_body_force(red=GR, blue=GB); a.set_macro(u["rR"], u["rB"]); a.step(10)
    a.set_body_force(red=g2r, blue=g2b)
    assert a.steps_done == 10 and a.body_force == (g2r, g2b)
    a.step(SLAB_STEPS - 10)
    b = solver(u["dom"], SLAB_PARAMS)
    b.set_body_force(red=g2r, blue=g2b)
    b.set_pdf(u["at10"]["fR"], u["at10"]["fB"], force=(u["at10"]["Fx"], u["at10"]["Fy"], u["at10"]["Fz"]))      # set_pdf keeps the force
    b.step(SLAB_STEPS - 10)
    same(a, b, what="changed at step 10")
    assert not np.array_equal(a.get("fR"), u["at30"]["fR"])
    a.close(); b.close()


def test_the_stored_force_is_the_csf_force_alone():
    """get("Fx" ...) against the recipe's CSF force: the oracle's Fx, which the recipe never adds the body force to"""
    dom, rR, rB = P.lattice_csf()
    par = point_params("A")
    s = solver(dom, par); s.set_body_force(red=GR, blue=GB); s.set_macro(rR, rB); s.step(P.STEPS)
    ref = R.BodyForceRef(dom, rR, rB, {k: v for k, v in par.items() if k != "variant"}, GR, GB).run(P.STEPS)
    fl = dom == 1
    scale = max(float(np.max(np.abs(ref.field(c)[fl]))) for c in ("Fx", "Fy", "Fz"))
    Fb = ref.body_force_density()
    for a, c in enumerate(("Fx", "Fy", "Fz")):
        assert rel_err(s.get(c)[fl], ref.field(c)[fl], scale=scale) < TOL, c
        assert rel_err(s.get(c)[fl], (ref.field(c) + Fb[a])[fl], scale=scale) > 1000 * TOL, c       # (the body part would be seen)
    s.close()


# ------------------------------------------------------------------------------------------------ 6. observers
def test_the_observers_carry_the_forces_half():
    """integrals().darcy_uz_* and get("rec_vz") agree with each other and with the recipe"""
    dom, rR, rB = P.lattice_csf()
    par = point_params("B")
    gr, gb = R.G_SETS["G2"]
    s = solver(dom, par); s.set_body_force(red=gr, blue=gb); s.set_macro(rR, rB); s.step(P.STEPS)
    ref = R.BodyForceRef(dom, rR, rB, {k: v for k, v in par.items() if k != "variant"}, gr, gb).run(P.STEPS)
    ref.step_a()
    fl = dom == 1
    t = s.integrals()
    cells = float(dom.size)
    uz, red = s.get("rec_vz"), s.get("rec_phi") > 0
    refuz, refred = ref.field("vz"), ref.field("phi") > 0
    assert np.array_equal(red[fl], refred[fl])
    scale = float(np.abs(refuz[fl]).sum()) / cells
    for k, mask in (("darcy_uz_R", fl & red), ("darcy_uz_B", fl & ~red)):
        got, own, recipe = getattr(t, k), float(uz[mask].sum()) / cells, float(refuz[mask].sum()) / cells
        # sums of ~ 3000 terms in another order: 1e-12 of the sum of magnitudes is rounding; the recipe's u is TOL away per cell
        assert abs(got - own) < 1e-12 * scale and abs(got - recipe) < TOL * scale, (k, got, own, recipe)
        assert abs(recipe) > 1e3 * TOL * scale, k
    # ... and the force's half is in it: without the force the same state's u differs
    bare = solver(dom, par); bare.set_pdf(s.get("fR"), s.get("fB"), force=(s.get("Fx"), s.get("Fy"), s.get("Fz")))
    assert abs(bare.integrals().darcy_uz_R - t.darcy_uz_R) > 1e3 * TOL * scale
    s.close(); bare.close()


def test_a_tracer_moves_with_a_purely_force_driven_flow():
    """open planes at equal pressure, no inlet velocity: the flow and the plume's displacement are the force's alone"""
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    from openlbmpm_amd.RKColorGradientD3Q19 import duct
    dom = duct(12, 10, 40)
    fl = dom == 1
    zz = np.mgrid[0:40, 0:10, 0:12][0]
    par = dict(relax="MRT", inlet="Dirichlet", outlet="Dirichlet", densityRH=1.0, densityBH=5e-8, densityRL=1.0, densityBL=5e-8, velocityZR=0.0, velocityZB=0.0)
    conc = np.where(fl & (zz >= 18) & (zz < 22), 1.0, 0.0)
    centre = {}
    for g in (None, (0.0, 0.0, -2.0e-4)):
        s = RK3DCSFSolver(dom, par, tracers=dict(num_tracers=1, diffusion_x=0.05, inlet_concentration=0.0))
        s.set_body_force(g)
        s.set_macro(np.where(fl, 1.0, 0.0), np.where(fl, 5e-8, 0.0)); s.set_concentration(0, conc)
        s.step(400)
        c = s.get_concentration(0)
        assert np.all(np.isfinite(c))
        centre[g] = float((c * zz).sum() / c.sum())
        if g is not None:
            assert float(s.get("rec_vz")[20, 5, 6]) < -1e-4
        s.close()
    assert abs(centre[None] - 19.5) < 0.05 and centre[None] - centre[(0.0, 0.0, -2.0e-4)] > 0.5, centre


# ------------------------------------------------------------------------------------------------ 7. physics
@pytest.mark.parametrize("relax", ["SRT", "MRT"])
@pytest.mark.parametrize("layers", [1, 2])
def test_hydrostatic_column(layers, relax):
    """bound: 0.5 % on the density drop across the gap against 3 sum F_b (tests/body_force_ref.py: hydrostatic_errors).  Measured, recipe and
    GPU alike: 0.338 % (one layer, SRT), 0.323 % (MRT), 0.340 % / 0.327 % (two layers); per pair of cells 0.44 - 0.46 %; max |u| 4.9e-5 and
    1.5e-5 = g / 2 of the fluid at the far wall.  The two layers are run without surface tension (hydrostatic_case says why)"""
    dom, rR, rB, par, g = R.hydrostatic_case(layers, relax)
    s = solver(dom, par); s.set_body_force(red=g[0], blue=g[1]); s.set_macro(rR, rB); s.step(R.HYDROSTATIC_STEPS)
    rhoR, rhoB = s.get("rhoR"), s.get("rhoB")
    Fb = np.where(dom == 1, rhoR * g[0][0] + rhoB * g[1][0], 0.0)
    drop, cell, umax = R.hydrostatic_errors(rhoR + rhoB, Fb, max(float(np.max(np.abs(s.get(c)))) for c in ("vx", "vy", "vz")))
    print("hydrostatic column, %d layer(s), %s: drop off 3 sum F_b by %.3f %%, per cell %.3f %%, max |u| %.2e" % (layers, relax, 100 * drop, 100 * cell, umax))
    assert drop < R.HYDROSTATIC_DROP_BOUND and cell < 2 * R.HYDROSTATIC_DROP_BOUND and umax < 1e-4
    s.close()


@pytest.mark.parametrize("relax", ["SRT", "MRT"])
def test_force_driven_poiseuille(relax):
    """bound: 2 % on the profile.  Measured, recipe and GPU alike: worst 1.08 % (SRT) and 0.74 % (MRT) at the wall cells, 0.13 % and 0.47 % at
    the centre"""
    dom, rR, rB, par, g = R.poiseuille_case(relax)
    s = solver(dom, par); s.set_body_force(g[0]); s.set_macro(rR, rB); s.step(R.POISEUILLE_STEPS)
    worst, centre = R.poiseuille_errors(s.get("vz"))
    print("force-driven Poiseuille, %s: worst deviation %.3f %%, at the centre %.3f %%" % (relax, 100 * worst, 100 * centre))
    assert worst < R.POISEUILLE_BOUND and centre < R.POISEUILLE_BOUND
    s.close()


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_force_state_and_counter_as_they_were(tmp_path):
    import ctypes as C
    from ini_fixtures import write_rk3d
    from openlbmpm_amd import config
    from openlbmpm_amd._lib import ERR_INVALID, ERR_STATE, LbmpmError
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver, _SlabGeometry
    from openlbmpm_amd.RKColorGradientD3Q19 import RKColorGradient3D
    dom, rR, rB = P.lattice_csf()
    par = dict(relax="MRT", tauB=0.8, theta=50.0)

    def run():
        s = solver(dom, par); s.set_body_force(red=GR, blue=GB); s.set_macro(rR, rB); s.step(5)
        return s
    never, s = run(), run()
    three = lambda v: (C.c_double * 3)(*v)
    for gr, gb in ((three(GR), None), (None, three(GB))):                          # one pointer NULL
        assert s._L.lbmpm_rk3dcsf_set_body_force(s._h, gr, gb) == ERR_INVALID
    for bad in (float("nan"), float("inf"), -float("inf")):
        for k in range(6):
            g = list(GR + GB); g[k] = bad
            with pytest.raises(LbmpmError) as e:
                s.set_body_force(red=g[:3], blue=g[3:])
            assert e.value.status == ERR_INVALID
    for bad in ((1., 2.), (1., 2., 3., 4.), 5.0, np.zeros((3, 3))):               # a wrong length
        with pytest.raises(ValueError):
            s.set_body_force(bad)
        with pytest.raises(ValueError):
            s.set_body_force(GR, blue=bad)
    assert s.body_force == (GR, GB) and s.steps_done == 5
    s.step(5); never.step(5)
    same(s, never, what="after refused calls")
    # a destroyed context
    gone = run(); gone.close()
    with pytest.raises(LbmpmError) as e:
        gone.set_body_force(GR)
    assert e.value.status == ERR_INVALID
    # between the stages of a step
    nz = dom.shape[0]
    geo = _SlabGeometry(nz, 0, nz // 2)
    slab = RK3DCSFSolver(geo.cut(dom), par, slab=geo.slab)
    slab.set_body_force(red=GR, blue=GB); slab.set_macro(geo.cut(rR), geo.cut(rB))
    slab.stage(0)
    with pytest.raises(LbmpmError) as e:
        slab.set_body_force(GB)
    assert e.value.status == ERR_STATE and slab.body_force == (GR, GB) and slab.steps_done == 0
    slab.sync(); slab.close()
    # the perturbation driver
    write_rk3d(str(tmp_path), nx=8, ny=8, nz=12, steps=4)
    with pytest.raises(config.ConfigError):
        RKColorGradient3D(str(tmp_path), body_force=GR)
    s.close(); never.close()


def test_the_driver_applies_the_force_and_records_it(tmp_path):
    """RKColorGradient3D(..., body_force=) and [BodyForce] of the ini: the run equals a stand-alone solver with the same force, the result
    file holds /BodyForce/Acceleration, a run continued from a checkpoint applies the force again"""
    from ini_fixtures import write_rk3d_csf
    from openlbmpm_amd import config
    from openlbmpm_amd.RKColorGradientD3Q19 import RKColorGradient3D, _CSFSlab, duct
    from openlbmpm_amd.geometry import initial_densities_rk3d
    from openlbmpm_amd.results import load_results
    write_rk3d_csf(str(tmp_path), theta=70.0, nx=14, ny=12, nz=32, steps=12, relax="MRT")
    dom = duct(14, 12, 32)
    sim = RKColorGradient3D(str(tmp_path), output_dir=str(tmp_path / "out"), record_every=6, body_force=dict(red=GR, blue=GB), checkpoint_every=6)
    res = load_results(sim.runRKColorGradient3D())
    assert np.array_equal(res["/BodyForce/Acceleration"], np.array([GR, GB]))
    p = config.read_rk3d(str(tmp_path))
    s = _CSFSlab(dom, p, 0).solver
    s.set_body_force(red=GR, blue=GB)
    s.set_macro(*initial_densities_rk3d(dom, 8, p["rho0R"], p["rho0B"]))
    s.step(12)
    last = sim.records - 1
    assert np.array_equal(res["/FluidMacro/FluidDensityRin%d" % last], s.get("rec_rhoR"))
    assert np.array_equal(res["/FluidVelocity/FluidVelocityZAt%d" % last], s.get("rec_vz"))
    again = RKColorGradient3D(str(tmp_path), output_dir=str(tmp_path / "out2"), record_every=6, body_force=dict(red=GR, blue=GB),
                              restart_from=sim.checkpoint_path)
    res2 = load_results(again.runRKColorGradient3D())
    assert np.array_equal(res2["/FluidVelocity/FluidVelocityZAt%d" % (again.records - 1)], s.get("rec_vz"))
    # the ini's section says the same
    with open(tmp_path / "RKtwophasesetup3D.ini", "a") as fh:
        fh.write("\n[BodyForce]\nisBodyForce = 'yes'\nbodyForceX = %r\nbodyForceY = %r\nbodyForceZ = %r\nbodyForceXB = %r\nbodyForceYB = %r\nbodyForceZB = %r\n" % (GR + GB))
    ini = RKColorGradient3D(str(tmp_path), output_dir=str(tmp_path / "out3"), record_every=6)
    res3 = load_results(ini.runRKColorGradient3D())
    assert np.array_equal(res3["/BodyForce/Acceleration"], np.array([GR, GB]))
    assert np.array_equal(res3["/FluidVelocity/FluidVelocityZAt%d" % (ini.records - 1)], s.get("rec_vz"))
    s.close()
