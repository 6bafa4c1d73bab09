"""python -m openlbmpm_amd rk3d ... --morphology-every N: the /Morphology group of the result file, for both 3-D models."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEPS = [0, 5, 10, 12]


def _write_ini(d, tension):
    from ini_fixtures import write_rk3d, write_rk3d_csf
    (write_rk3d_csf if tension == "CSF" else write_rk3d)(str(d), steps=12)          # the shipped sizes: 32 x 32 x 96


def _standalone(d, tension, phi_cut):
    """solver.morphology(phi_cut) of a stand-alone solver with the driver's set-up, stepped to the last of STEPS"""
    from openlbmpm_amd import config
    from openlbmpm_amd.RKColorGradientD3Q19 import PARAM_KEYS, _CSFSlab, duct
    from openlbmpm_amd.geometry import initial_densities_rk3d
    from openlbmpm_amd.rk3d import RK3DSlab
    p = config.read_rk3d(str(d))
    dom = duct(p["nx"], p["ny"], p["nz"])
    rR, rB = initial_densities_rk3d(dom, 10, p["rho0R"], p["rho0B"])
    if tension == "CSF":
        s = _CSFSlab(dom, p, 0).solver
        s.set_macro(rR, rB)
        s.step(STEPS[-1])
    else:
        s = RK3DSlab(dom, 0, dom.shape[0], {k: p[k] for k in PARAM_KEYS})
        s.set_density(rR, rB)
        s.step_single(STEPS[-1])
        s.phase_field(diagnostics=True)
    m = s.morphology(phi_cut)
    s.close()
    return m


@pytest.mark.parametrize("tension,phi_cut", [("perturbation", 0.0), ("CSF", 0.25)])
def test_the_cli_writes_the_morphology_group(tmp_path, tension, phi_cut, caplog):
    import logging
    from openlbmpm_amd.__main__ import main
    from openlbmpm_amd.integrals import column_names
    from openlbmpm_amd.morphology import COLUMNS
    from openlbmpm_amd.results import load_results
    _write_ini(tmp_path, tension)
    out = tmp_path / "out"
    with caplog.at_level(logging.INFO, logger="openlbmpm_amd"):
        assert main(["rk3d", str(tmp_path), "--out", str(out), "--morphology-every", "5"] + (["--morphology-phi-cut", str(phi_cut)] if phi_cut else [])) == 0
    files = os.listdir(out)
    assert len(files) == 1, files
    res = load_results(str(out / files[0]))
    assert np.array_equal(res["/Morphology/Steps"], np.array(STEPS, dtype=np.int64)) and res["/Morphology/Steps"].dtype == np.int64
    assert column_names(res["/Morphology/Columns"]) == COLUMNS
    assert sorted(k for k in res if k.startswith("/Morphology/")) == sorted(["/Morphology/Steps", "/Morphology/Columns"] + ["/Morphology/PlanesAtStep%d" % k for k in STEPS])
    for k in STEPS:
        t = res["/Morphology/PlanesAtStep%d" % k]
        assert t.shape == (96, 28) and t.dtype == np.float64, k
    want = _standalone(tmp_path, tension, phi_cut)
    last = res["/Morphology/PlanesAtStep%d" % STEPS[-1]]
    assert np.array_equal(last, want.planes)                 # bit for bit
    assert want.cells("R") > 0 and want.cells("B") > 0 and want.faces("RB") > 0 and (want.cells("N") > 0) == (phi_cut > 0)
    assert not np.array_equal(res["/Morphology/PlanesAtStep0"], last)
    lines = [r.getMessage() for r in caplog.records if " morphology step " in r.getMessage()]
    assert len(lines) == len(STEPS) and all(w in lines[-1] for w in ("areaRB", "wettedR", "eulerR", "eulerB", "capillaryPressure")), lines
    # without the option: no /Morphology group, the same records
    plain = tmp_path / "plain"
    assert main(["rk3d", str(tmp_path), "--out", str(plain)]) == 0
    ref = load_results(str(plain / os.listdir(plain)[0]))
    assert not any(k.startswith("/Morphology") for k in ref)
    assert set(ref) == {k for k in res if not k.startswith("/Morphology/")}
    for key in ref:
        assert np.array_equal(ref[key], res[key]), key
