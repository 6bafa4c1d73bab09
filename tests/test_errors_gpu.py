"""Error behaviour of the C ABI on a GPU box: every misuse returns a negative
status with a message in lbmpm_last_error(); nothing aborts, nothing falls back to a CPU path."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_rk2d_rejects_bad_configurations_and_shapes():
    from openlbmpm_amd._lib import LbmpmError
    from openlbmpm_amd.rk2d import RK2DSolver
    from openlbmpm_amd.geometry import simple_geometry
    dom = simple_geometry(20, 40)
    with pytest.raises((LbmpmError, ValueError, KeyError)):
        RK2DSolver(dom, dict(tauR=0.4))                       # tau <= 1/2
    with pytest.raises((LbmpmError, ValueError, KeyError)):
        RK2DSolver(dom, dict(wetting=7))                      # unknown WettingType
    s = RK2DSolver(dom, None)
    with pytest.raises(TypeError):
        s.set_macro(np.zeros((3, 3)), np.zeros((3, 3)))       # wrong shape
    with pytest.raises(LbmpmError) as e:
        s.get_tracer(0)                                       # no tracer configured
    assert "tracer" in str(e.value)
    s.set_macro(np.where(dom == 1, 1.0, 0.0), np.zeros(dom.shape))
    s.step(2)
    with pytest.raises(LbmpmError):
        s.configure_tracers()
        s.set_tracer(0, np.zeros(dom.shape))                  # tracer state must be set before the first step
    s.close()


def test_lattices_beyond_the_32_bit_plane_offsets_are_refused():
    """the 2-D kernels address a node inside a lattice plane with 32 bits (d2q9_device.h::pull_issue_asm): roundup(nx, 32) * ny must stay
    below 2^28 nodes, and create says so instead of wrapping an offset"""
    from openlbmpm_amd._lib import LbmpmError
    from openlbmpm_amd.rk2d import RK2DSolver
    from openlbmpm_amd.sc2d import SC2DSolver
    dom = np.ones((16400, 16384), dtype=np.uint8)             # 2^28 + 2^18 nodes; nothing is allocated on the device
    with pytest.raises(LbmpmError) as e:
        RK2DSolver(dom, None)
    assert "2^28" in str(e.value)
    with pytest.raises(LbmpmError) as e:
        SC2DSolver(dom, dict(inter="EFS"))
    assert "2^28" in str(e.value)


def test_sc2d_rejects_bad_configurations():
    from openlbmpm_amd._lib import LbmpmError
    from openlbmpm_amd.sc2d import SC2DSolver
    from openlbmpm_amd.geometry import simple_geometry
    dom = simple_geometry(20, 48)
    with pytest.raises((LbmpmError, ValueError)):
        SC2DSolver(dom, dict(inter="ShanChen", relax="MRT"))  # MRT exists for the explicit forcing scheme only
    with pytest.raises((LbmpmError, ValueError)):
        SC2DSolver(dom, dict(inter="ShanChen", scheme=8))     # iso-8 force belongs to EFS
    with pytest.raises((LbmpmError, ValueError)):
        SC2DSolver(dom, dict(scheme=6))
    s = SC2DSolver(dom, dict(inter="EFS"))
    s.set_density(np.where(dom == 1, 1.0, 0.0), np.where(dom == 1, 0.02, 0.0))
    s.step(1)
    with pytest.raises(LbmpmError) as e:
        s.get("rho0")                                         # EFS densities need the diagnostics switch
    assert "diagnostics" in str(e.value)
    s.close()


def test_rk3d_protocol_misuse_is_reported():
    from openlbmpm_amd import _lib
    from openlbmpm_amd._lib import LbmpmError
    from openlbmpm_amd.rk3d import RK3DSlab
    from openlbmpm_amd.geometry import porous_spheres, initial_densities_rk3d
    dom = porous_spheres(64, 16, 40, porosity=0.7, rmin=3.0, rmax=6.0, seed=3, nbuf=5)
    rR, rB = initial_densities_rk3d(dom, 5)
    with pytest.raises(LbmpmError):
        RK3DSlab(dom, 30, 20)                                 # slab outside the lattice
    with pytest.raises(LbmpmError):
        RK3DSlab(dom, 0, 40, params=dict(tauR=0.5))
    with pytest.raises(LbmpmError) as e:
        RK3DSlab(dom, 0, 40, params=dict(densityRL=0.0))      # the outlet rule divides by it
    assert "densityRL" in str(e.value)
    top = RK3DSlab(dom, 20, 20)
    top.set_density(rR[20:], rB[20:])
    with pytest.raises(LbmpmError) as e:
        top.step_single(1)                                    # a slab cannot step alone: it needs its neighbour's halo
    assert "single-slab" in str(e.value)
    top.collide_interior()
    with pytest.raises(LbmpmError):
        top.collide()                                         # the step was opened with collide_interior
    top.collide_boundary()
    with pytest.raises(LbmpmError) as e:
        top.get("rhoR")                                       # densities exist after phase_field(diagnostics=True) only
    assert "phase_field" in str(e.value)
    with pytest.raises(KeyError):
        top.buffer("no_such_buffer")
    ptr, n = C.c_void_p(), C.c_int64(0)
    assert _lib.lib().lbmpm_rk3d_buffer(top._h, 99, C.byref(ptr), C.byref(n)) < 0
    assert b"unknown buffer" in _lib.lib().lbmpm_last_error()
    top.close()


def test_empty_inputs():
    """zero steps are a no-op; lattices without a fluid node or below the minimum size are refused
    with a message instead of launching empty grids"""
    from openlbmpm_amd._lib import LbmpmError
    from openlbmpm_amd.rk2d import RK2DSolver
    from openlbmpm_amd.sc2d import SC2DSolver
    from openlbmpm_amd.rk3d import RK3DSlab
    from openlbmpm_amd.geometry import simple_geometry
    dom = simple_geometry(20, 40)
    rR = np.where(dom == 1, 1.0, 0.0)
    s = RK2DSolver(dom, None)
    s.set_macro(rR, np.zeros(dom.shape))
    before = s.get("fR")
    s.step(0)
    assert s.steps_done == 0 and np.array_equal(s.get("fR"), before)
    with pytest.raises(LbmpmError):
        s.step(-3)
    s.close()
    for make in (lambda d: RK2DSolver(d, None), lambda d: SC2DSolver(d, dict(inter="EFS"))):
        with pytest.raises(LbmpmError) as e:
            make(np.zeros((40, 20), dtype=np.uint8))                 # no fluid node at all
        assert "fluid" in str(e.value)
        with pytest.raises(LbmpmError):
            make(np.ones((4, 3), dtype=np.uint8))                    # smaller than the boundary rows need
    with pytest.raises(LbmpmError) as e:
        RK3DSlab(np.zeros((12, 8, 8), dtype=np.uint8), 0, 12)
    assert "fluid" in str(e.value)
    with pytest.raises(LbmpmError):
        RK3DSlab(np.ones((4, 4, 4), dtype=np.uint8), 0, 4)               # fewer than 8 planes


def test_stream_test_reports_plausible_rates():
    """lbmpm_hbm_stream_test (the measured ceiling quoted by bench.py): sane ordering and magnitude on an
    MI355X (spec 8 TB/s), bad arguments refused"""
    from openlbmpm_amd import _lib
    L = _lib.lib()
    a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
    assert L.lbmpm_hbm_stream_test(0, 1 << 30, 3, C.byref(a), C.byref(b), C.byref(c)) == 0
    assert 2000.0 < a.value < 8000.0 and 2000.0 < b.value < 8000.0 and 2000.0 < c.value < 8000.0
    assert L.lbmpm_hbm_stream_test(0, 16, 3, C.byref(a), C.byref(b), C.byref(c)) < 0
    assert L.lbmpm_hbm_stream_test(0, 1 << 30, 0, C.byref(a), C.byref(b), C.byref(c)) < 0


def test_device_memory_accounting():
    """lbmpm_*_device_bytes: two copies of the populations dominate; the compact 3-D storage holds less than
    the dense one on a porous sample"""
    from openlbmpm_amd.rk2d import RK2DSolver
    from openlbmpm_amd.sc2d import SC2DSolver
    from openlbmpm_amd.rk3d import RK3DSlab
    from openlbmpm_amd.geometry import simple_geometry, porous_spheres
    dom = simple_geometry(64, 96)
    for s in (RK2DSolver(dom, None), SC2DSolver(dom, dict(inter="EFS"))):
        assert 2 * 18 * 8 * dom.size <= s.device_bytes < 8 * 18 * 8 * dom.size
        s.close()
    vox = porous_spheres(64, 32, 40, porosity=0.6, rmin=3.0, rmax=6.0, seed=1, nbuf=4)
    compact = RK3DSlab(vox, 0, 40)
    assert compact.dominant_kernel == "rk3dq_fused"        # 23 doubles per fluid cell and buffer (csrc/rk3dq.h)
    os.environ["LBMPM_RK3D_LAYOUT"] = "dense"
    try:
        dense = RK3DSlab(vox, 0, 40)
    finally:
        del os.environ["LBMPM_RK3D_LAYOUT"]
    assert 2 * 23 * 8 * compact.num_fluid_nodes <= compact.device_bytes < dense.device_bytes
    compact.close(); dense.close()


def _duct3():
    """a 64 x 64 x 32 duct (solid side walls) with one solid block in it: the CSF context has wetting solids"""
    dom = np.ones((32, 64, 64), dtype=np.uint8)
    dom[:, 0, :] = dom[:, -1, :] = 0
    dom[:, :, 0] = dom[:, :, -1] = 0
    dom[12:20, 24:40, 24:40] = 0
    return dom


def contexts_with_every_optional_block(dom, dom3):
    """[(name, open solver)]: the four solver contexts after everything that allocates a device block on demand has run.  The 2-D
    colour-gradient solver comes twice: its perturbation model (with that model's diagnostics) and its tracers exclude each other."""
    from openlbmpm_amd.sc2d import SC2DSolver
    from openlbmpm_amd.rk2d import RK2DSolver
    from openlbmpm_amd.rk3d import RK3DSlab
    from openlbmpm_amd.rk3dcsf import RK3DCSFSolver
    from openlbmpm_amd.geometry import initial_densities_rk, initial_densities_rk3d
    fluid, fluid3 = (dom == 1).astype(np.float64), (dom3 == 1).astype(np.float64)
    rR, rB = initial_densities_rk(dom, False, 10)
    rR3, rB3 = initial_densities_rk3d(dom3, 5)
    out = []
    s = SC2DSolver(dom, dict(inter="EFS", scheme=8))
    s.set_density(fluid, 0.02 * fluid)
    s.step(1)                                                 # the EFS initialisation and its staging arrays
    s.enable_diagnostics(True); s.enable_diagnostics(False); s.enable_diagnostics(True)
    s.step(1)
    out.append(("sc2d", s))
    s = RK2DSolver(dom, None, diagnostics=True, perturbation=dict(AkR=0.007, AkB=0.009, solidPhi=0.5))
    s.set_macro(rR, rB)
    s.step(1)
    s.get("rhoR")
    out.append(("rk2d perturbation", s))
    s = RK2DSolver(dom, None, diagnostics=True)
    two = dict(diffX=(1. / 6.,) * 2, diffY=(1. / 6.,) * 2, beta=(1.0,) * 2, inlet_conc=(1.0,) * 2)
    s.configure_tracers(**two)
    s.configure_tracers(**two)                                # the second configure gives the first one's buffers back
    s.set_macro(rR, rB)
    for k in range(2):
        s.set_tracer(k, 0.1 * fluid)
    s.step(1)
    s.get_tracer(0); s.get("rhoR")
    out.append(("rk2d tracers", s))
    s = RK3DSlab(dom3, 0, dom3.shape[0])
    s.set_density(rR3, rB3)
    s.phase_field(diagnostics=True)
    s.integrals()
    s.clusters(labels=True)
    state, info = s.get_state()
    s.set_state(state, steps=info["steps"], post_collision=info["post_collision"])
    out.append(("rk3d", s))
    s = RK3DCSFSolver(dom3, None, diagnostics=True, tracers=dict(num_tracers=2))
    assert s.num_wetting_solids > 0
    s.set_macro(rR3, rB3)
    for k in range(2):
        s.set_concentration(k, 0.1 * fluid3)
    s.step(1)
    s.integrals()
    s.clusters(labels=True)
    s.tracer_integrals()
    s.get("rec_fR")
    s.get_tracer_pdf(0)
    out.append(("rk3dcsf", s))
    return out


def test_create_destroy_does_not_leak_device_memory():
    """Create / destroy cycles over every block a context allocates on demand: diagnostics (switched on and off), the EFS
    initialisation's staging arrays, the perturbation model's diagnostics, tracers (configured twice), the observe buffers, integral and
    cluster buffers, the state's and the populations' staging buffers.  EFS with an iso-8 force keeps a psi array (16 B per cell) that
    destroy once forgot; at these sizes (512 x 512, 64 x 64 x 32) a forgotten per-cell block of a byte per cell or more exceeds the cap
    within the ten cycles.  The small tables (integral tables, counters, cluster rows of the 2^17-cell duct's chunks) lie below what
    free memory can resolve: they are covered by construction -- a context's blocks all come from one owner (csrc/device_memory.h),
    which frees everything it handed out."""
    import torch
    from openlbmpm_amd.geometry import simple_geometry
    dom = simple_geometry(512, 512)
    dom3 = _duct3()

    def cycle():
        for _name, s in contexts_with_every_optional_block(dom, dom3):
            s.close()
    cycle()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(10):
        cycle()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 4 << 20, "device memory shrank by %d bytes over 10 create/destroy cycles" % (free0 - free1)


def test_device_bytes_round_trips():
    """lbmpm_*_device_bytes follows what is given back: diagnostics off returns it to its value before they were on, the EFS
    initialisation's staging arrays are not part of it, and tracers configured again count once"""
    from openlbmpm_amd.sc2d import SC2DSolver
    from openlbmpm_amd.rk2d import RK2DSolver
    from openlbmpm_amd.geometry import simple_geometry
    dom = simple_geometry(72, 96)
    fluid = (dom == 1).astype(np.float64)
    plane = 96 * 96                                           # rows are padded to a multiple of 32 nodes
    for s in (RK2DSolver(dom, None), SC2DSolver(dom, dict(inter="EFS", scheme=8))):
        before = s.device_bytes
        s.enable_diagnostics(True)
        on = s.device_bytes
        assert on >= before + 3 * 8 * plane
        s.enable_diagnostics(False)
        assert s.device_bytes == before
        s.enable_diagnostics(True)
        assert s.device_bytes == on
        s.close()
    s = SC2DSolver(dom, dict(inter="EFS", scheme=8))
    s.set_density(fluid, 0.02 * fluid)
    before = s.device_bytes
    s.step(1)                                                 # the first step initialises (38 planes of staging arrays come and go)
    assert s.device_bytes == before
    s.step(1)
    assert s.device_bytes == before
    s.close()

    def tracers(n):
        return dict(diffX=(1. / 6.,) * n, diffY=(1. / 6.,) * n, beta=(1.0,) * n, inlet_conc=(1.0,) * n)
    s, fresh = RK2DSolver(dom, None), RK2DSolver(dom, None)
    bare = s.device_bytes
    s.configure_tracers(**tracers(2))
    assert s.device_bytes == bare + 2 * 2 * 5 * 8 * plane      # two buffers of 5 populations per tracer
    s.configure_tracers(**tracers(3))
    fresh.configure_tracers(**tracers(3))
    assert s.device_bytes == fresh.device_bytes == bare + 2 * 3 * 5 * 8 * plane
    s.close(); fresh.close()


def test_rk3d_fields_are_refused_when_stale():
    from openlbmpm_amd._lib import LbmpmError
    from openlbmpm_amd.rk3d import RK3DSlab
    dom = np.ones((12, 8, 64), dtype=np.uint8)
    s = RK3DSlab(dom, 0, 12)
    s.set_density(np.ones(dom.shape), np.zeros(dom.shape))
    with pytest.raises(LbmpmError):
        s.get("phi")                                          # nothing observed yet
    s.step_single(2)
    with pytest.raises(LbmpmError) as e:
        s.get("phi")                                          # the fused kernel keeps phi in LDS
    assert "stale" in str(e.value)
    s.phase_field(diagnostics=True)
    assert np.allclose(s.get("phi")[4:8], 1.0) and np.allclose(s.get("rhoR")[4:8], 1.0)     # away from the open planes
    s.step_single(1)
    with pytest.raises(LbmpmError):
        s.get("rhoR")
    s.close()
