"""The deduplicated known-answer case format of tests/helpers.py (write_kat_cases / KatFile / load_kat_cases, the format of
tests/golden/kats_wide_*.npz) on a small synthetic case set: what goes in comes out bit for bit, an array the launch left unchanged
comes back as None, and an array two cases share is stored once."""
import numpy as np

from helpers import KatFile, load_kat_cases, write_kat_cases


def _records():
    rng = np.random.default_rng(11)
    nodes = np.arange(7, dtype=np.int64) * 3
    rho = rng.uniform(0.1, 1.0, (2, 7)); rho[1, 3] = np.nan
    f = rng.uniform(0.0, 0.2, (2, 7, 9))
    mask = np.array([True, False, True, True, False, False, True])
    a = dict(case="first", module="sc", kernel="kernelA", args=["totalNodes", "tau", "fluidNodes", "fluidRho", "fluidPDF"],
             inputs=dict(totalNodes=7, tau=0.8, fluidNodes=nodes, fluidRho=rho, fluidPDF=f),
             outputs=dict(fluidNodes=nodes.copy(), fluidRho=rho.copy(), fluidPDF=f * 1.5))
    b = dict(case="first#variant", module="sc", kernel="kernelA", args=["totalNodes", "tau", "fluidNodes", "fluidRho", "fluidPDF"],
             inputs=dict(totalNodes=7, tau=1.1, fluidNodes=nodes, fluidRho=rho, fluidPDF=f),
             outputs=dict(fluidNodes=nodes.copy(), fluidRho=-rho, fluidPDF=f.copy()))
    c = dict(case="nothing", module="tr", kernel="kernelB", args=["totalNodes", "distriField", "fluidNodes"],
             inputs=dict(totalNodes=7, distriField=mask, fluidNodes=nodes), outputs=dict(distriField=mask.copy(), fluidNodes=nodes.copy()))
    # same bytes, another type: zeros of int64 and of float64 must not share a stored array
    d = dict(case="zeros", module="tr", kernel="kernelC", args=["n", "a", "b"], inputs=dict(n=2, a=np.zeros(2), b=np.zeros(2, dtype=np.int64)),
             outputs=dict(a=np.zeros(2), b=np.ones(2, dtype=np.int64)))
    return [a, b, c, d, dict(case="cannot", raises="IndexError")]


def _same(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def test_round_trip(tmp_path):
    path = str(tmp_path / "kats_wide_xx.npz")
    records = _records()
    write_kat_cases(path, records)
    f = KatFile(path)
    assert sorted(f.cases) == ["first", "first#variant", "nothing", "zeros"] and f.raises == {"cannot": "IndexError"}
    loaded = list(load_kat_cases(path))
    assert len(loaded) == 4
    for case, got in zip(f.cases, loaded):
        r = [r for r in records if r["case"] == case][0]
        module, kernel, args, inputs, outputs, noop = got
        assert (module, kernel, args) == (r["module"], r["kernel"], r["args"])
        assert list(inputs) == args and set(outputs) == set(r["outputs"])
        changed = 0
        for n in args:
            assert _same(inputs[n], r["inputs"][n]), (case, n)
            if n in outputs:
                if _same(r["outputs"][n], r["inputs"][n]):
                    assert outputs[n] is None, (case, n)                 # unchanged: recorded as that, not stored again
                else:
                    assert _same(outputs[n], r["outputs"][n]), (case, n)
                    changed += 1
        assert noop == (changed == 0)
    assert [g[5] for g in loaded] == [c == "nothing" for c in f.cases]
    assert inputs["a"].dtype == np.float64 and inputs["b"].dtype == np.int64 and outputs["a"] is None


def test_shared_arrays_are_stored_once(tmp_path):
    path = str(tmp_path / "kats_wide_xx.npz")
    write_kat_cases(path, _records())
    f = KatFile(path)
    for n in ("fluidNodes", "fluidRho", "fluidPDF"):
        assert f.index["first|in|" + n] == f.index["first#variant|in|" + n]
    assert f.index["first|in|fluidNodes"] == f.index["nothing|in|fluidNodes"]
    assert f.index["first|in|tau"] != f.index["first#variant|in|tau"]
    assert f.index["zeros|in|a"] != f.index["zeros|in|b"]
    stored = [k for k in f.d.files if k.startswith("blob|")]
    assert len(stored) == len(set(f.index.values()) - {"="})
    float_blobs = [k for k in stored if f.d[k].shape == (2, 7)]
    assert len(float_blobs) == 2                                         # rho (with its NaN) once, -rho once
