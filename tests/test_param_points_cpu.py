"""What tests/param_points.py promises about its two off-default points A and B, proved without a GPU on the oracles and the Python mapping:

(a) completeness   every key of a solver's DEFAULT_PARAMS and every field of its ctypes config struct has a row (or a written exclusion),
                   and moving a parameter moves exactly the config fields its row names;
(b) regime         at A and B the oracle stays finite, |u| < 0.1, rho_R + rho_B > 0 in every fluid cell, max |phi| <= 1 + 1e-12;
(c) sensitivity    moving any ONE parameter from A to its default, swapping a colour pair, swapping or moving a rate, changes a compared
                   field by >= 1000 x the GPU tolerance -- a kernel that ignores or mis-wires it misses the GPU test by three orders;
                   a declared degeneracy the other way round: the pair moved with its sum fixed leaves the oracle bit-equal;
(d) conditioning   the oracle restarted from densities rippled in the last bit follows itself within a tenth of the GPU tolerance, in
                   every instance the GPU module compares.
The bounds of (c) and (d) are conditions on the inputs of the GPU comparison, not measurements of any kernel."""
import ctypes as C

import numpy as np
import pytest

import param_points as P

NAMES = sorted(P.TABLES)
FACTOR = 1000.0


# ------------------------------------------------------------------------------------------------ (a) completeness
def _solver_defaults(name):
    from openlbmpm_amd import rk2d, rk3d, rk3dcsf, sc2d
    return {"rk2d-csf": rk2d, "rk2d-pert": rk2d, "sc2d-efs": sc2d, "sc2d-original": sc2d, "rk3d": rk3d, "rk3dcsf": rk3dcsf}[name].DEFAULT_PARAMS


@pytest.mark.parametrize("name", NAMES)
def test_the_table_covers_the_solvers_parameters(name):
    t = P.TABLES[name]
    D = _solver_defaults(name)
    rows = set(t["defaults"]) | set(t["categorical"]) | set(t.get("unread", ()))
    rows |= {"variant", "bulk_epsilon"} & set(D)            # (an instance axis; an opt-in approximation with its own test)
    rows |= {"inlet", "outlet"} & set(t["base"])
    assert set(D) == rows, (sorted(set(D) - rows), sorted(rows - set(D)))
    for k, v in t["defaults"].items():
        if k == "rates":
            assert D[k] is None               # None = the built-in rates: those of the oracle's DEFAULT_PARAMS
            from oracle.rk3dcsf import DEFAULT_PARAMS as O
            assert tuple(O["rates"]) == tuple(v)
        else:
            assert D[k] == v, k
    numeric = dict(t["defaults"], **t.get("extra_defaults", {}))
    assert set(t["A"]) == set(numeric) == set(t["B"])
    for k, d in numeric.items():
        a, b = t["A"][k], t["B"][k]
        if k == "rates":
            for r in (a, b):
                assert len(set(r)) == 6 and r[5] == 0.0
            assert all(x != y for x, y in zip(a[:5], b[:5])) and all(x != y for x, y in zip(a[:5], d[:5])) and all(x != y for x, y in zip(b[:5], d[:5]))
        else:
            assert a != d and b != d and a != b, k
    for r, b in t["pairs"]:
        for point in "AB":
            assert t[point][r] != t[point][b], (point, r, b)
    for r, b, why in t["degenerate"]:
        assert (r, b) in t["pairs"] and why
    for inst in t["instances"]:
        for k, v in inst.items():
            assert k in ("storage", "nx", "variant") or v in t["categorical"].get(k, (t["base"].get(k),)), (k, v)
    # every value of every instance axis is compared on the GPU (at both points: the GPU module runs every instance at A and at B)
    for k, values in t["categorical"].items():
        seen = {inst.get(k, t["base"].get(k)) for inst in t["instances"]}
        if name.startswith("sc2d"):
            other = P.TABLES["sc2d-original" if name == "sc2d-efs" else "sc2d-efs"]["instances"]
            seen |= {inst[k] for inst in other}
        assert seen == set(values), (k, seen)


class _Capture:
    """stands in for the loaded library: records the config structs the Python classes hand to *_create / *_set_perturbation"""

    def __init__(self):
        self.seen = {}

    def __getattr__(self, fn):
        def call(*args):
            if fn.endswith("_create") or fn.endswith("_set_perturbation"):
                cfg = args[1 if fn.endswith("_set_perturbation") else 0]._obj
                for f, _ in cfg._fields_:
                    v = getattr(cfg, f)
                    self.seen[f] = tuple(v) if isinstance(v, C.Array) else v
            return 0
        return call


def _config(name, p, monkeypatch):
    from openlbmpm_amd import _lib, rk2d, rk3d, rk3dcsf, sc2d
    cap = _Capture()
    monkeypatch.setattr(_lib, "lib", lambda: cap)
    if name == "rk2d-csf":
        rk2d.RK2DSolver(np.ones((8, 8), np.uint8), p)
    elif name == "rk2d-pert":
        pert = {k: p[k] for k in ("AkR", "AkB", "solidPhi")}
        rk2d.RK2DSolver(np.ones((8, 8), np.uint8), {k: v for k, v in p.items() if k not in pert}, perturbation=pert)
    elif name.startswith("sc2d"):
        sc2d.SC2DSolver(np.ones((8, 8), np.uint8), p)
    elif name == "rk3d":
        rk3d.RK3DSlab(np.ones((8, 8, 8), np.uint8), 0, 8, p)
    else:
        rk3dcsf.RK3DCSFSolver(np.ones((8, 8, 8), np.uint8), p)
    return cap.seen


def _struct_fields(name):
    from openlbmpm_amd import _lib
    S = {"rk2d-csf": (_lib.RK2DConfig,), "rk2d-pert": (_lib.RK2DPerturbation,), "sc2d-efs": (_lib.SC2DConfig,), "sc2d-original": (_lib.SC2DConfig,),
         "rk3d": (_lib.RK3DConfig,), "rk3dcsf": (_lib.RK3DCSFConfig,)}[name]
    return [f for s in S for f, _ in s._fields_]


@pytest.mark.parametrize("name", NAMES)
def test_every_config_field_has_a_row_and_every_row_moves_its_fields(name, monkeypatch):
    """a new config field without a row fails here; so does a row whose parameter the Python mapping drops or sends elsewhere"""
    t = P.TABLES[name]
    fields = _struct_fields(name)
    missing = [f for f in fields if f not in t["fields"] and f not in P.EXCLUDED_FIELDS]
    assert not missing, "config fields without a row in tests/param_points.py: %s" % missing
    assert not [f for f in t["fields"] if f not in fields]
    base = _config(name, P.params(t, "A"), monkeypatch)
    numeric = dict(t["defaults"], **t.get("extra_defaults", {}))
    moves = {k: numeric[k] for k in numeric}
    moves.update({k: next(v for v in values if v != t["base"].get(k)) for k, values in t["categorical"].items() if k != "variant"})
    for k, v in moves.items():
        moved = _config(name, P.params(t, "A", **{k: v}), monkeypatch)
        changed = {f for f in moved if moved[f] != base[f] and f in fields}
        want = {f for f, ps in t["fields"].items() if k in ps}
        if name == "rk2d-pert":                      # (RK2DSolver fills two structs: this table's is lbmpm_rk2d_perturbation)
            want |= {f for f, ps in P.RK2D_CSF["fields"].items() if k in ps and f in moved}
            changed = {f for f in moved if moved[f] != base[f]}
        assert changed == want and want, (k, sorted(changed), sorted(want))


# ------------------------------------------------------------------------------------------------ the oracle at A and B
_runs = {}


def _key(v):
    return tuple(sorted((k, _key(x) if isinstance(x, dict) else x) for k, x in v.items()))


def run(name, p, start=None, tag=None):
    """the oracle's fields after STEPS steps (cached for the unmoved points: every sensitivity run compares with them)"""
    key = (name, _key(p), tag)
    if start is not None or tag is None:
        return P.oracle_run(name, p, (P.STEPS,), start=start)[P.STEPS]
    if key not in _runs:
        _runs[key] = P.oracle_run(name, p, (P.STEPS,))[P.STEPS]
    return _runs[key]


def _instances(name):
    t = P.TABLES[name]
    seen, out = set(), []
    for inst in [t["base"]] + t["instances"]:
        inst = {k: v for k, v in inst.items() if k not in ("variant", "storage")}     # (the oracle knows neither)
        if _key(inst) not in seen:
            seen.add(_key(inst)); out.append(inst)
    return out


ALL_INSTANCES = [(n, i, p) for n in NAMES for i in _instances(n) for p in "AB"]


def _id(v):
    return ",".join(str(x) for x in v.values()) if isinstance(v, dict) else str(v)


@pytest.mark.parametrize("name,inst,point", ALL_INSTANCES, ids=_id)
def test_regime(name, inst, point):
    t = P.TABLES[name]
    f = run(name, P.params(t, point, inst), tag="ref")
    for k, a in f.items():
        if a.dtype.kind == "f":
            assert np.all(np.isfinite(a)), k
    vec = P.COMPARED[name]["vectors"][0]
    u = np.sqrt(sum(f[c] ** 2 for c in vec))
    assert float(u.max()) < 0.1, float(u.max())
    r = [f[k] for k in (("rho0", "rho1") if name.startswith("sc2d") else ("rhoR", "rhoB"))]
    fluid = slice(None) if r[0].ndim == 1 else (P.start_of(name, inst.get("nx"))[0] == 1)
    assert float((r[0] + r[1])[fluid].min()) > 0.0
    if "phi" in f:
        assert float(np.max(np.abs(f["phi"][fluid]))) <= 1.0 + 1e-12


@pytest.mark.parametrize("name,inst,point", ALL_INSTANCES, ids=_id)
def test_the_cases_of_the_gpu_comparison_are_well_conditioned(name, inst, point):
    """the pattern of tests/test_tr3d_ref.py: an oracle that does not follow ITSELF from a start that differs in the last bit cannot be
    followed by anything else.  A point that fails this is moved (contact angle, geometry), the GPU tolerance is not loosened."""
    t = P.TABLES[name]
    p = P.params(t, point, inst)
    _, a, b = P.start_of(name, inst.get("nx"))
    one = run(name, p, tag="ref")
    two = run(name, p, start=(P.last_bit(a), P.last_bit(b, 1.0)))
    assert any(np.any(one[k] != two[k]) for k in one if one[k].dtype.kind == "f")
    w, f = P.worst(name, two, one)
    print("%s %s %s: the oracle against itself from a start rippled in the last bit: %.2e (%s)" % (name, _id(inst), point, w, f))
    assert w < 0.1 * t["tol"], (w, f)


def _moves(name):
    t = P.TABLES[name]
    out = []
    for k in t["A"]:
        if k == "rates":
            out += [("rate %s -> default" % P.RATE_NAMES[i], "rate", i) for i in range(5)]
            out += [("rates %s <-> %s" % (P.RATE_NAMES[i], P.RATE_NAMES[j]), "rateswap", (i, j)) for i, j in P.RATE_SWAPS]
        else:
            out.append(("%s -> default" % k, "default", k))
    degenerate = {(r, b) for r, b, _ in t["degenerate"]}
    out += [("%s <-> %s" % pair, "swap", pair) for pair in t["pairs"] if pair not in degenerate]
    return [(name,) + m for m in out]


@pytest.mark.parametrize("name,what,kind,arg", [m for n in NAMES for m in _moves(n)], ids=lambda v: v if isinstance(v, str) else "")
def test_every_parameter_matters_at_A(name, what, kind, arg):
    t = P.TABLES[name]
    A = t["A"]
    numeric = dict(t["defaults"], **t.get("extra_defaults", {}))
    inst = dict(t["base"])
    if kind == "default":
        inst.update(t["live"].get(arg, {})); moved = {arg: numeric[arg]}
    elif kind == "swap":
        inst.update(t["live"].get(arg[0], {})); moved = {arg[0]: A[arg[1]], arg[1]: A[arg[0]]}
    else:
        r = list(A["rates"])
        if kind == "rate":
            r[arg] = numeric["rates"][arg]
        else:
            r[arg[0]], r[arg[1]] = r[arg[1]], r[arg[0]]
        moved = dict(rates=tuple(r))
    ref = run(name, P.params(t, "A", inst), tag="ref")
    got = run(name, P.params(t, "A", inst, **moved))
    w, f = P.worst(name, got, ref, with_K=False)          # (K is ill-conditioned where |G| is small: not counted)
    print("%s: %s moves %s by %.2e" % (name, what, f, w))
    assert w >= FACTOR * t["tol"], (what, w, f)


@pytest.mark.parametrize("name,r,b", [(n, r, b) for n in NAMES for r, b, _ in P.TABLES[n]["degenerate"]])
def test_a_declared_degeneracy_is_one(name, r, b):
    """the model reads the pair through its sum (or mean) alone: swapped, and moved with the sum fixed bit for bit, the oracle is bit-equal"""
    t = P.TABLES[name]
    A = t["A"]
    ref = run(name, P.params(t, "A"), tag="ref")
    r2, b2 = P.exact_shift(A[r], A[b])
    for moved in ({r: A[b], b: A[r]}, {r: r2, b: b2}):
        got = run(name, P.params(t, "A", **moved))
        for k in ref:
            assert np.array_equal(got[k], ref[k]), (moved, k)
