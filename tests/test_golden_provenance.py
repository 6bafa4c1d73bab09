"""The committed fixtures under tests/golden/ are what the committed generators produce from the REAL
reference (its drivers and kernels run under tests/golden/gen's numba stand-in): one scenario per
generator is regenerated here and compared bit for bit.  Container-only: skipped where
/root/reference does not exist (the GPU box)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tests", "golden", "gen")

pytestmark = pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="the reference tree is not on this machine")


@pytest.mark.parametrize("script,args,fixture", [
    ("make_golden_rk.py", ["csf_mrt_convective"], "rk_csf_mrt_convective.npz"),
    ("make_golden_sc.py", ["efs_srt_convective"], "sc_efs_srt_convective.npz"),
    ("make_golden_sc.py", ["efs_srt_freeflow"], "sc_efs_srt_freeflow.npz"),
    ("make_golden_sc.py", ["efs_srt_chang"], "sc_efs_srt_chang.npz"),
    ("make_golden_sc.py", ["sc_srt_chang"], "sc_sc_srt_chang.npz"),
    ("make_golden_tr.py", [], "tr_kernels.npz"),
    ("make_golden_rk_pert.py", ["kernels"], "rkpert_kernels.npz"),
    ("make_golden_rk_pert.py", ["srt_porous"], "rkpert_srt_porous.npz"),
    ("make_golden_rk_pert.py", ["mrt_capillary_literal"], "rkpert_mrt_capillary_literal.npz"),
    ("make_golden_rkb.py", [], "rkb_kernels.npz"),
    ("make_golden_dense.py", [], "dense_kernels.npz"),
    ("make_golden_tr_coupled.py", ["capillary"], "trc_capillary.npz"),
    ("make_golden_kats.py", ["rk"], "kats_rk.npz"),
    ("make_golden_kats.py", ["sc"], "kats_sc.npz"),
    ("make_golden_kats.py", ["tr"], "kats_tr.npz"),
])
def test_fixture_is_reproduced_from_the_reference(tmp_path, script, args, fixture):
    env = dict(os.environ, LBMPM_GOLDEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable, os.path.join(GEN, script)] + args, env=env, cwd=str(tmp_path),
                          stdout=subprocess.DEVNULL, timeout=600)
    new, old = np.load(tmp_path / fixture), np.load(os.path.join(ROOT, "tests", "golden", fixture))
    assert set(old.files) <= set(new.files)            # (later generator versions may record more parameters)
    for k in old.files:
        assert np.array_equal(new[k], old[k], equal_nan=new[k].dtype.kind == "f"), k


@pytest.mark.parametrize("tag", ["rk", "sc", "tr"])
def test_wide_known_answer_fixture_is_reproduced_from_the_reference(tmp_path, tag):
    """tests/golden/kats_wide_<tag>*.npz (the second geometry of make_golden_kats.py, 513 nodes; one file or parts of consecutive cases):
    regenerated and compared through the loader, case by case and bit for bit -- inputs, outputs, what is recorded as unchanged"""
    import glob
    from helpers import KatFile
    env = dict(os.environ, LBMPM_GOLDEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable, os.path.join(GEN, "make_golden_kats.py"), "wide_" + tag], env=env, cwd=str(tmp_path),
                          stdout=subprocess.DEVNULL, timeout=600)

    def load(folder):
        files = [KatFile(f) for f in sorted(glob.glob(os.path.join(str(folder), "kats_wide_%s*.npz" % tag)))]
        assert files
        cases = {case: f.case(case) for f in files for case in f.cases}
        assert len(cases) == sum(len(f.cases) for f in files)
        return cases, {k: v for f in files for k, v in f.raises.items()}

    def same(x, y):
        return (x is None and y is None) or (x is not None and y is not None and x.dtype == y.dtype and x.shape == y.shape
                                             and x.tobytes() == y.tobytes())

    (new, new_raises), (old, old_raises) = load(tmp_path), load(os.path.join(ROOT, "tests", "golden"))
    assert sorted(new) == sorted(old) and new_raises == old_raises
    for case in old:
        assert new[case][:3] == old[case][:3] and new[case][5] == old[case][5], case
        for k in (3, 4):
            assert list(new[case][k]) == list(old[case][k]), case
            for arg in old[case][k]:
                assert same(new[case][k][arg], old[case][k][arg]), (case, arg)


def test_every_kernel_of_the_five_kernel_modules_has_an_entry_point():
    """completeness of the kernel-level ABI: every function the reference compiles with @cuda.jit as a KERNEL (not
    device=True) in its five kernel modules has a same-named entry point in include/lbmpm_kernels.h, with the same
    parameter names in the same order"""
    import re
    from openlbmpm_amd._kernel_specs import KERNELS
    files = {"rk": "RKCG2D/AcceleratedRKGPU2D.py", "rkb": "RKCG2D/RKGPU2DBoundary.py", "sc": "ShanChen2D/OptimizedD2Q9GPU.py",
             "sc ": "ShanChen2D/ExplicitD2Q9GPU.py", "tr": "RKCG2D/AccelerateTransport2DRK.py"}
    total = 0
    for tag, rel in files.items():
        src = open(os.path.join("/root/reference", rel)).read()
        for m in re.finditer(r"@cuda\.jit\(([^@]*?)\)\s*\ndef (\w+)\(([^)]*)\)", src, re.S):
            if re.search(r"device\s*=\s*True", m.group(1)):
                continue
            name = m.group(2)
            params = tuple(p.strip() for p in m.group(3).replace("\\", " ").split(",") if p.strip())
            assert (tag.strip(), name) in KERNELS, "%s: %s has no entry point" % (rel, name)
            # the later definition of a name used twice is the one Python keeps (calRKCollision23GPU, A:244 / A:511)
            if src.count("def %s(" % name) == 1:
                assert KERNELS[(tag.strip(), name)][2] == params, (rel, name)
            total += 1
    assert total >= 155
    # the legacy dense file (north_star names it; SURVEY 8 a16 scopes it to its explicit-forcing pipeline :1336-2487 + :2698): the 15 entry
    # points of openlbmpm_amd/dropin/AccelerateGPU2D.py carry the reference kernels' own parameter lists
    src = open(os.path.join("/root/reference", "ShanChen2D/AccelerateGPU2D.py")).read()
    dense = {name: params for (tag, name), (_sym, _ct, params, _k) in KERNELS.items() if tag == "de"}
    assert len(dense) == 15
    found = 0
    for m in re.finditer(r"@cuda\.jit\(([^@]*?)\)\s*\ndef (\w+)\(([^)]*)\)", src, re.S):
        if m.group(2) in dense:
            assert dense[m.group(2)] == tuple(p.strip() for p in m.group(3).replace("\\", " ").split(",") if p.strip()), m.group(2)
            found += 1
    assert found == 15
