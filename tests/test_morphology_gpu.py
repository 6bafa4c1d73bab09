"""Phase morphology counted on the device (lbmpm_rk3d_morphology / lbmpm_rk3dcsf_morphology, csrc/rk3d_morphology.h) against the numpy
restatement of tests/test_morphology_cpu.py.  The classes the restatement starts from are taken from what the solver hands out -- phi
from get("phi") / get("rec_phi"), rho_R and rho_B from get("rhoR") .. / get("rec_rhoR") .. -- by the definition of include/lbmpm.h; the
phases are prescribed at step 0 (the patterns of tests/test_clusters_gpu.py), then seven real steps blur them.

Counts are integers: array_equal.  RHO_R, RHO_B per plane: within 2 (n - 1) 2^-53 sum|term| with n the plane's cells of that class, the
worst-case distance between two orders of summation of the same doubles (derived at the top of tests/test_integrals_gpu.py; the
terms rho_R + rho_B are the same doubles on both sides: the library is built with -ffp-contract=off).  Between two cuts of one lattice
the device's own order is the same: array_equal, RHO_* included.

The lattice is the 70 x 33 x 12 porous box of tests/test_integrals_gpu.py: rows of 64 + 6 cells, 2310 cells per plane = two chunks of the
reducer and a ragged one, a plane with five fluid cells, a solid row.
"""
import os

import numpy as np
import pytest

from test_clusters_gpu import CSF_PAR, PERT_PAR, SHARP, _box, _Csf, _Pert, densities
from test_drivers_gpu import _free_port
from test_morphology_cpu import C, cpu_morphology
from test_rk3d_csf_gpu import _slab_case

pytestmark = pytest.mark.gpu

S, R, B, N = 0, 1, 2, 3
RHO = (C["rho_R"], C["rho_B"])
COUNTS = [c for c in range(28) if c not in RHO]
# after seven steps no fluid cell has |phi| < 0.3: segment_boundary under the perturbation model -- its 57 red cells have dissolved, phi <= -0.3
# in all 24026 fluid cells -- and one_phase under the CSF model, red throughout as prescribed (measured: 0 N cells in both, 102 .. 16431 in
# the other twelve cases)
NO_BAND = {("perturbation", "segment_boundary"), ("csf", "one_phase")}


def rho_fields(m):
    """rho_R, rho_B as the solver hands them out"""
    pre = "rec_" if isinstance(m, _Csf) else ""
    return m.s.get(pre + "rhoR"), m.s.get(pre + "rhoB")


def classes(phi, rR, rB, dom, cut=0.0):
    """the class bytes by the definition of include/lbmpm.h"""
    fin = np.isfinite(phi) & np.isfinite(rR) & np.isfinite(rB)
    with np.errstate(invalid="ignore"):
        c = np.where(fin & (phi > cut), R, np.where(fin & (phi <= -cut), B, N))
    return np.where(dom == 1, c, S).astype(np.uint8)


def handed_out(m, cut=0.0):
    """(classes, rho_R + rho_B) of the state of the wrapper m"""
    rR, rB = rho_fields(m)
    return classes(m.phi(), rR, rB, m.dom, cut), rR + rB


def compare(planes, cls, rho, what, above=None):
    T = cpu_morphology(cls, np.where((cls == R) | (cls == B), rho, 0.0), above)
    assert planes.shape == T.shape and planes.dtype == np.float64, what
    for c in COUNTS:
        assert np.array_equal(planes[:, c], T[:, c]), (what, c, planes[:, c], T[:, c])
    for col, k, cells in ((C["rho_R"], R, C["cells_R"]), (C["rho_B"], B, C["cells_B"])):
        A = np.array([np.abs(rho[z][cls[z] == k]).sum() for z in range(cls.shape[0])])
        bound = 2.0 * np.maximum(T[:, cells] - 1.0, 0.0) * 2.0 ** -53 * A
        err = np.abs(planes[:, col] - T[:, col])
        print("%s col %d: worst error %.3e, bound there %.3e" % (what, col, err.max(), bound[np.argmax(err)]))
        assert np.all(err <= bound), (what, col, err, bound)
    return T


@pytest.fixture(scope="module")
def box():
    return _box()


@pytest.fixture(scope="module", params=["perturbation", "csf"])
def model(request, box):
    m = (_Pert if request.param == "perturbation" else _Csf)(box[0])
    yield m
    m.s.close()


# ---------------------------------------------------------------------------------------------- 1. patterns, at step 0 and after steps
@pytest.mark.parametrize("name", SHARP + ("graded",))
def test_pattern_at_step_0_and_after_7_steps(model, name):
    dom = model.dom
    kind = "csf" if isinstance(model, _Csf) else "perturbation"
    model.prescribe(*densities(name, dom))
    g = model.s.morphology()
    assert g.nx == 70 and g.ny == 33 and g.planes.shape == (12, 28)
    cls, rho = handed_out(model)
    T = compare(g.planes, cls, rho, "%s step 0" % name)
    assert T[5, :3].sum() == 5                               # the plane with five fluid cells
    model.step(7)
    for cut in (0.0, 0.3):
        g = model.s.morphology(phi_cut=cut)
        cls, rho = handed_out(model, cut)
        T = compare(g.planes, cls, rho, "%s step 7 cut %g" % (name, cut))
        print("%s step 7 cut %g: cells R %d B %d N %d, chi R %d B %d, RB faces %d" % (name, cut, g.cells("R"), g.cells("B"), g.cells("N"), g.euler("R"),
                                                                                     g.euler("B"), g.faces("RB")))
        assert np.array_equal(model.s.morphology(phi_cut=cut).planes, g.planes)          # the same call twice: the same bits
        if cut > 0:
            # the band must hold cells, or the case shows nothing -- but for the two of the fourteen cases that the steps leave with one
            # phase and so without an interface to cut a band from (NO_BAND, listed by name: any other case that loses its band fails)
            assert (T[:, C["cells_N"]].sum() > 0) == ((kind, name) not in NO_BAND), "no cell in the band: the case shows nothing"
        else:
            assert g.cells("R") == model.s.integrals().total("cells_R")                   # at phi_cut 0 the R cells are the integrals'


# ---------------------------------------------------------------------------------------------- 2. a cell that is not finite
def test_a_bad_cell_is_class_n_and_touches_its_elements_only(model, box):
    """rho_R = NaN in one fluid cell of plane 4 (as tests/test_integrals_gpu.py::_with_one_nan): it turns up in CELLS_N of plane 4; beside
    plane 4 only the elements of plane 3 that reach up to it can change -- z pairs, xz and yz squares, cubes"""
    dom, rR, rB = box
    y, x = np.argwhere(dom[4] == 1)[37]
    bad = rR.copy()
    bad[4, y, x] = np.nan
    model.prescribe(rR, rB)
    clean = model.s.morphology().planes
    compare(clean, *handed_out(model), "clean")
    model.prescribe(bad, rB)
    g = model.s.morphology()
    dirty = g.planes
    cls, rho = handed_out(model)
    assert cls[4, y, x] == N and int((cls == N).sum()) == 1
    compare(dirty, cls, rho, "one nan")
    assert np.all(np.isfinite(dirty)) and g.cells("N") == 1
    want = np.zeros(12); want[4] = 1
    assert np.array_equal(dirty[:, C["cells_N"]] - clean[:, C["cells_N"]], want)
    others = [z for z in range(12) if z not in (3, 4)]
    assert np.array_equal(dirty[others], clean[others])
    upwards = [C[n] for n in ("RR_z", "BB_z", "RB_z", "RS_z", "BS_z", "sq_R_xz", "sq_R_yz", "sq_B_xz", "sq_B_yz", "cube_R", "cube_B")]
    flat = [c for c in range(28) if c not in upwards]
    assert np.array_equal(dirty[3, flat], clean[3, flat])
    assert not np.array_equal(dirty[4], clean[4])


# ---------------------------------------------------------------------------------------------- 3. the plane above
def test_the_plane_above(model, box):
    from openlbmpm_amd._lib import ERR_INVALID, LbmpmError
    dom, rR, rB = box
    model.prescribe(rR, rB)
    model.step(2)
    cls, rho = handed_out(model)
    alone = model.s.morphology_part()
    compare(alone, cls, rho, "above = None")
    assert np.array_equal(model.s.morphology_face(), cls[0])
    red = np.full(dom.shape[1:], R, dtype=np.uint8)
    got = model.s.morphology_part(0.0, red)
    T = compare(got, cls, rho, "above = R", above=red)
    assert np.array_equal(got[:-1], alone[:-1]) and not np.array_equal(got[-1], alone[-1])      # only the top row changes
    assert np.array_equal(got[-1, COUNTS], T[-1, COUNTS])
    for name in ("RR_z", "sq_R_xz", "cube_R"):
        assert alone[-1, C[name]] == 0
    mixed = np.random.default_rng(4).integers(0, 4, size=dom.shape[1:]).astype(np.uint8)
    compare(model.s.morphology_part(0.0, mixed), cls, rho, "above = random classes", above=mixed)
    mixed[17, 69] = 4
    with pytest.raises(LbmpmError) as e:
        model.s.morphology_part(0.0, mixed)
    assert e.value.status == ERR_INVALID
    assert np.array_equal(model.s.morphology_part(), alone)


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_refusals(box):
    from openlbmpm_amd._lib import ERR_INVALID, ERR_STATE, LbmpmError
    dom, rR, rB = box
    for m in (_Pert(dom), _Csf(dom)):
        if isinstance(m, _Csf):
            for call in (m.s.morphology, m.s.morphology_face):
                with pytest.raises(LbmpmError) as e:
                    call()                                   # before set_macro / set_pdf
                assert e.value.status == ERR_STATE
        m.prescribe(rR, rB)
        for cut in (-0.1, float("nan"), float("inf")):
            for call in (m.s.morphology, m.s.morphology_face):
                with pytest.raises(LbmpmError) as e:
                    call(cut)
                assert e.value.status == ERR_INVALID, cut
        m.s.morphology()
        if isinstance(m, _Pert):
            m.s.step_single(1)
            for call in (m.s.morphology, m.s.morphology_face):
                with pytest.raises(LbmpmError) as e:
                    call()                                   # a step since the last phase_field(diagnostics=True)
                assert e.value.status == ERR_STATE and "stale" in str(e.value)
            m.s.phase_field(diagnostics=True)
        else:
            m.s.step(1)
        m.s.morphology()
        m.s.close()


# ---------------------------------------------------------------------------------------------- 5. a lattice smaller than a chunk
@pytest.mark.parametrize("make", [_Pert, _Csf], ids=["perturbation", "csf"])
def test_a_lattice_of_rows_that_wrap_after_a_few_cells(make):
    """5 x 4 cells per plane, all fluid, a random R / B assignment: every row wraps after five cells, every column after four, a plane is
    less than one chunk (eight planes: the fewest either library takes)"""
    dom = np.ones((8, 4, 5), dtype=np.uint8)
    red = np.random.default_rng(23).random(dom.shape) < 0.5
    m = make(dom)
    m.prescribe(np.where(red, 1.0, 0.0), np.where(red, 0.0, 1.0))
    cls, rho = handed_out(m)
    assert np.array_equal(cls[2:-2], np.where(red, R, B)[2:-2])
    g = m.s.morphology()
    T = compare(g.planes, cls, rho, "5 x 4 x 8")
    assert T[:, :2].sum() == dom.size and T[:, C["RB_x"]].sum() > 0
    m.s.close()


# ---------------------------------------------------------------------------------------------- 6. cut independence, bit for bit
@pytest.mark.parametrize("state", ["random", "steps"])
def test_perturbation_slabs_give_the_bits_of_the_undivided_lattice(box, state):
    """two and three slabs, as the integrals' and the clusters' tests cut the box; at step 0 also four slabs of three planes (a single own plane is
    refused by lbmpm_rk3d_create, which wants two, and by lbmpm_rk3dcsf_create, which wants four; the CPU's slab test has that case)"""
    from openlbmpm_amd.rk3d import RK3DCluster
    dom, rR, rB = box
    if state == "random":
        rR, rB = densities("random", dom)
    m = _Pert(dom)
    m.prescribe(rR, rB)
    if state == "steps":
        m.step(4)
    ref = {cut: m.s.morphology(cut).planes for cut in (0.0, 0.3)}
    compare(ref[0.0], *handed_out(m), "undivided, " + state)
    m.s.close()
    for k in (2, 3) + ((4,) if state == "random" else ()):
        c = RK3DCluster(dom, k, PERT_PAR)
        c.set_density(rR, rB)
        if state == "steps":
            c.step(4)
        for cut in (0.0, 0.3):
            got = c.morphology(cut)                          # (stale: observes first)
            assert got.planes.shape == (12, 28) and np.array_equal(got.planes, ref[cut]), (k, cut)
        c.close()


@pytest.mark.parametrize("state", ["random", "steps"])
def test_csf_slabs_give_the_bits_of_the_undivided_lattice(state):
    """the cuts of the integrals' and the clusters' tests, and one with a slab of four planes, the fewest a slab of this model owns"""
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster
    dom, rR, rB = _slab_case()
    if state == "random":
        rR, rB = densities("random", dom)
    m = _Csf(dom)
    m.prescribe(rR, rB)
    if state == "steps":
        m.step(4)
    ref = {cut: m.s.morphology(cut).planes for cut in (0.0, 0.3)}
    compare(ref[0.0], *handed_out(m), "undivided, " + state)
    m.s.close()
    for kw in (dict(nslabs=4), dict(cuts=[0, 9, 23, 44]), dict(cuts=[0, 9, 13, 23, 44])):
        c = RK3DCSFCluster(dom, CSF_PAR, **kw)
        c.set_macro(rR, rB)
        if state == "steps":
            c.step(4)
        for cut in (0.0, 0.3):
            got = c.morphology(cut)
            assert got.planes.shape == (44, 28) and np.array_equal(got.planes, ref[cut]), (kw, cut)
        c.close()


_WORKER = '''
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
import torch, torch.distributed as dist
import test_morphology_gpu as T
dist.init_process_group("gloo")
torch.cuda.set_device(0)
rank = dist.get_rank()
if %(tension)r == "CSF":
    from openlbmpm_amd.rk3dcsf import RK3DCSFDistributed
    dom, _, _ = T._slab_case()
    d = RK3DCSFDistributed(dom, T.CSF_PAR, device=0)
    d.set_macro(*T.densities("random", dom))
else:
    from openlbmpm_amd.rk3d import RK3DDistributed
    dom, _, _ = T._box()
    d = RK3DDistributed(dom, T.PERT_PAR, device=0, transport="callback")
    d.set_density(*T.densities("random", dom))
d.step(3)
d.sync()
out = {}
for cut in (0.0, 0.3):
    g = d.morphology(cut)
    assert (g is None) == (rank != 0)
    if g is not None:
        out["planes%%g" %% cut] = g.planes
if rank == 0:
    np.savez(%(npz)r, **out)
if hasattr(d, "close"):
    d.close()
dist.destroy_process_group()
'''


@pytest.mark.parametrize("tension", ["perturbation", "CSF"])
def test_two_ranks_give_the_bits_of_the_undivided_lattice(tmp_path, tension):
    """two ranks on this GPU over gloo: rank 0 gets the whole lattice's table, rank 1 None (a random pattern, three steps)"""
    import subprocess
    import sys
    tests = os.path.dirname(os.path.abspath(__file__))
    script = tmp_path / "w.py"
    script.write_text(_WORKER % dict(root=os.path.dirname(tests), tests=tests, tension=tension, npz=str(tmp_path / "two.npz")))
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(script)], env=dict(os.environ), timeout=600)
    two = np.load(str(tmp_path / "two.npz"))
    if tension == "CSF":
        dom = _slab_case()[0]
        m = _Csf(dom)
    else:
        dom = _box()[0]
        m = _Pert(dom)
    m.prescribe(*densities("random", dom))
    m.step(3)
    for cut in (0.0, 0.3):
        one = m.s.morphology(cut).planes
        compare(one, *handed_out(m, cut), "%s cut %g" % (tension, cut))
        assert np.array_equal(two["planes%g" % cut], one), cut
    m.s.close()


# ---------------------------------------------------------------------------------------------- 7. memory
def test_memory_is_the_class_array_allocated_by_the_first_call(box):
    dom, rR, rB = box
    nz, ny, nx = dom.shape
    for make in (_Pert, _Csf):
        quiet, m = make(dom), make(dom)
        for k in (quiet, m):
            k.prescribe(rR, rB)
            k.step(2)
            k.s.integrals()
        before = m.s.device_bytes
        assert quiet.s.device_bytes == before              # a context that never asks holds what it held
        m.s.morphology()
        assert m.s.device_bytes - before == (nz + 1) * ny * nx
        m.s.morphology(phi_cut=0.25)
        m.s.morphology_face()
        m.step(1)
        m.s.morphology_part(0.0, np.zeros((ny, nx), dtype=np.uint8))
        assert m.s.device_bytes - before == (nz + 1) * ny * nx          # allocated once; the reducer's partials live for a call
        quiet.step(1)
        assert quiet.s.device_bytes == before
        quiet.s.close(); m.s.close()
    # a slab: its own planes + 1, the ghost planes not counted
    from openlbmpm_amd.rk3dcsf import RK3DCSFCluster
    dom, rR, rB = _slab_case()
    c = RK3DCSFCluster(dom, CSF_PAR, cuts=[0, 9, 23, 44])
    c.set_macro(rR, rB)
    before = [s.device_bytes for s in c.slabs]
    c.morphology()
    assert [s.device_bytes - b for s, b in zip(c.slabs, before)] == [(n + 1) * 18 * 22 for n in (9, 14, 21)]
    c.close()
