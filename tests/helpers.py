"""Shared helpers for the parity tests (oracle = checker; never the thing under test on
the product side)."""
import glob
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_files(prefix):
    return sorted(glob.glob(os.path.join(GOLDEN, prefix + "*.npz")))


def load_params(d):
    return {k[4:]: d[k].item() for k in d.files if k.startswith("par_")}


def rel_err(a, g, scale=None):
    """max |a-g| / max |g|  (field-relative, the north star's 'relative' tolerance).  `scale` replaces max |g|:
    the components of a vector field are measured against the magnitude of the vector, not each against itself
    (a component that is zero but for round-off has no scale of its own)."""
    a = np.asarray(a, dtype=np.float64); g = np.asarray(g, dtype=np.float64)
    if a.shape != g.shape:
        raise AssertionError("shape %s vs %s" % (a.shape, g.shape))
    if not np.all(np.isfinite(a) == np.isfinite(g)):
        return np.inf
    m = np.isfinite(g)
    scale = float(scale) if scale is not None else max(float(np.max(np.abs(g[m]))) if m.any() else 0.0, 1e-300)
    return float(np.max(np.abs(a[m] - g[m]))) / scale if m.any() else 0.0


# ---------------------------------------------------------------------------------------- known-answer case files, deduplicated
# One .npz per module: every distinct array once under "blob|<key>" (key: a hash of dtype, shape and bytes) and two parallel string
# arrays "index" / "keys" that map  <case>|kernel, <case>|module, <case>|args, <case>|noop, <case>|in|<arg>, <case>|out|<arg>  (and
# <case>|raises for a kernel the reference cannot run) to a key.  <case>|out|<arg> exists for every array argument; where the launch left
# the array as it was, bit for bit, its key is UNCHANGED and nothing is stored a second time.
UNCHANGED = "="


def _blob_key(a):
    h = hashlib.sha1()
    h.update(("%s|%s|" % (a.dtype.str, a.shape)).encode())
    h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:20]


def write_kat_cases(path, records):
    """records: dicts with case, module, kernel, args (names in order), inputs {arg: value} for every argument, outputs {arg: array after the
    launch} for every array argument -- or with case and raises alone"""
    blobs, index = {}, {}

    def put(name, value):
        a = np.array(value, copy=True)
        key = _blob_key(a)
        if key in blobs:
            assert blobs[key].dtype == a.dtype and blobs[key].shape == a.shape and blobs[key].tobytes() == a.tobytes(), name
        blobs.setdefault(key, a)
        assert name not in index, name
        index[name] = key

    for r in records:
        case = r["case"]
        if "raises" in r:
            put(case + "|raises", r["raises"])
            continue
        put(case + "|kernel", r["kernel"]); put(case + "|module", r["module"]); put(case + "|args", list(r["args"]))
        changed = 0
        for n in r["args"]:
            put("%s|in|%s" % (case, n), r["inputs"][n])
            if n in r["outputs"]:
                before, after = np.asarray(r["inputs"][n]), np.asarray(r["outputs"][n])
                same = before.dtype == after.dtype and before.shape == after.shape and before.tobytes() == after.tobytes()
                changed += not same
                if same:
                    index["%s|out|%s" % (case, n)] = UNCHANGED
                else:
                    put("%s|out|%s" % (case, n), after)
        put(case + "|noop", not changed)
    names = sorted(index)
    np.savez_compressed(path, index=np.array(names), keys=np.array([index[n] for n in names]), **{"blob|" + k: a for k, a in sorted(blobs.items())})


class KatFile:
    def __init__(self, path):
        self.path = path
        self.d = np.load(path)
        self.index = dict(zip((str(n) for n in self.d["index"]), (str(k) for k in self.d["keys"])))
        self.cases = [n[:-len("|kernel")] for n in self.index if n.endswith("|kernel")]
        self.raises = {n[:-len("|raises")]: str(self.d["blob|" + k]) for n, k in self.index.items() if n.endswith("|raises")}

    def get(self, name):
        return self.d["blob|" + self.index[name]]

    def case(self, case):
        """(module, kernel, args, inputs, outputs, noop): inputs {arg: value} for every argument, outputs {arg: array after the launch, or None
        where the launch left it unchanged} for every array argument"""
        args = [str(n) for n in self.get(case + "|args")]
        inputs = {n: self.get("%s|in|%s" % (case, n)) for n in args}
        outputs = {}
        for n in args:
            key = self.index.get("%s|out|%s" % (case, n))
            if key is not None:
                outputs[n] = None if key == UNCHANGED else self.d["blob|" + key]
        return str(self.get(case + "|module")), str(self.get(case + "|kernel")), args, inputs, outputs, bool(self.get(case + "|noop"))


def load_kat_cases(path):
    """yields (module, kernel, args, inputs, outputs_or_None, noop) per case of a file written by write_kat_cases, in the order of KatFile.cases"""
    f = KatFile(path)
    for case in f.cases:
        yield f.case(case)
