"""What tests/param_points.py promises about its two off-default points A and B, proved without a GPU on the oracles and the Python mapping:

(a) completeness   every key of a solver's DEFAULT_PARAMS and every field of its ctypes config struct has a row (or a written exclusion),
                   and moving a parameter moves exactly the config fields its row names;
(b) regime         at A and B the oracle stays finite, |u| < 0.1, rho_R + rho_B > 0 in every fluid cell, max |phi| <= 1 + 1e-12;
(c) sensitivity    moving any ONE parameter from A to its default, swapping a colour pair, swapping or moving a rate, changes a compared
                   field by >= 1000 x the GPU tolerance -- a kernel that ignores or mis-wires it misses the GPU test by three orders;
                   a declared degeneracy the other way round: the pair moved with its sum fixed leaves the oracle bit-equal;
(d) conditioning   the oracle restarted from densities rippled in the last bit follows itself within a tenth of the GPU tolerance, in
                   every instance the GPU module compares.
The bounds of (c) and (d) are conditions on the inputs of the GPU comparison, not measurements of any kernel.

The table of the 2-D tracers (rk2d-tr) takes part in all four with its flow rows and its sixteen instances; its tracer rows, its two
lattices (one per launch path of launch_fused_tracer), the cover of its instance axes and the keys of transportsetup.ini have tests of
their own at the end of the module, where a sensitivity counts in a concentration alone."""
import ctypes as C

import numpy as np
import pytest

import param_points as P

NAMES = sorted(P.TABLES)
FACTOR = 1000.0


# ------------------------------------------------------------------------------------------------ (a) completeness
def _solver_defaults(name):
    from openlbmpm_amd import rk2d, rk3d, rk3dcsf, sc2d
    return {"rk2d-csf": rk2d, "rk2d-pert": rk2d, "rk2d-tr": rk2d, "sc2d-efs": sc2d, "sc2d-original": sc2d, "rk3d": rk3d, "rk3dcsf": rk3dcsf}[name].DEFAULT_PARAMS


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
            assert k in ("storage", "nx", "variant") or v in t["categorical"].get(k, t.get("axes", {}).get(k, (t["base"].get(k),))), (k, v)
    # every value of every instance axis is compared on the GPU (at both points: the GPU module runs every instance at A and at B)
    for k, values in list(t["categorical"].items()) + list(t.get("axes", {}).items()):
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
            if fn.endswith("_create") or fn.endswith("_set_perturbation") or fn.endswith("_tracer_configure"):
                cfg = args[0 if fn.endswith("_create") else 1]._obj
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
    elif name == "rk2d-tr":
        s = rk2d.RK2DSolver(np.ones((8, 8), np.uint8), {k: v for k, v in p.items() if k in rk2d.DEFAULT_PARAMS})
        s.configure_tracers(**p["tr"])
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
    S = {"rk2d-csf": (_lib.RK2DConfig,), "rk2d-tr": (_lib.RK2DConfig, _lib.TracerConfig), "rk2d-pert": (_lib.RK2DPerturbation,), "sc2d-efs": (_lib.SC2DConfig,), "sc2d-original": (_lib.SC2DConfig,),
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
    if "tracer" in t:           # the tracer rows; the axes that reach the config (the lattice is its size: EXCLUDED_FIELDS)
        tr = t["tracer"]
        moves.update({"tr_" + k: (d,) * 4 if k in tr["per_tracer"] else d for k, d in tr["defaults"].items()})
        moves.update({k: next(v for v in values if v != t["base"][k]) for k, values in t["axes"].items() if k != "lattice"})
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
    _, a, b, *conc = P.start_of(name, inst.get("nx"), inst)
    one = run(name, p, tag="ref")
    two = run(name, p, start=(P.last_bit(a), P.last_bit(b, 1.0)) + tuple(P.last_bit(c, 2.0) for c in conc))
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
    _matters(name, what, got, ref)


def _matters(name, what, got, ref):
    t = P.TABLES[name]
    d = P.differences(name, got, ref, with_K=False)          # (K is ill-conditioned where |G| is small: not counted)
    d = {f: e for f, e in d.items() if f in t.get("sensed", d)}
    f = max(d, key=d.get)
    print("%s: %s moves %s by %.2e" % (name, what, f, d[f]))
    assert d[f] >= FACTOR * t["tol"], (what, d[f], f)
    return d[f]


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


# ------------------------------------------------------------------------------------------------ the tracer table (rk2d-tr)
TR = P.RK2D_TR["tracer"]


def test_the_tracer_rows_cover_configure_tracers_and_the_config_struct():
    """one row per keyword of RK2DSolver.configure_tracers and per field of lbmpm_tracer_config (the header and its ctypes mirror); the value
    rules of the two points"""
    import inspect
    import os
    import re
    from openlbmpm_amd import _lib, rk2d
    sig = inspect.signature(rk2d.RK2DSolver.configure_tracers).parameters
    keywords = {k: v.default for k, v in sig.items() if k != "self"}
    assert set(keywords) == set(TR["defaults"]) | {"free_outlet", "dirichlet_inlet"}, sorted(set(keywords) ^ set(TR["defaults"]))
    for k, d in TR["defaults"].items():
        assert keywords[k] == ((d,) if k in TR["per_tracer"] and k != "diffJ" else None if k == "diffJ" else d), k     # (diffJ None = 1/3 each)
    assert keywords["free_outlet"] is True and keywords["dirichlet_inlet"] is True and (True, True) in P.TRACER_AXES["ends"]
    fields = [f for f, _ in _lib.TracerConfig._fields_]
    assert set(fields) == set(TR["fields"]), sorted(set(fields) ^ set(TR["fields"]))
    header = open(os.path.join(os.path.dirname(rk2d.__file__), "..", "include", "lbmpm.h")).read()
    body = re.search(r"typedef struct lbmpm_tracer_config \{(.*?)\} lbmpm_tracer_config;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    in_header = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert in_header == fields, (in_header, fields)
    rows = {k for ps in TR["fields"].values() for k in ps}
    assert rows == set(TR["defaults"]) | {"tracers", "ends"}
    assert set(TR["ini"].values()) <= set(fields)
    # the value rules
    assert set(TR["A"]) == set(TR["defaults"]) == set(TR["B"])
    for k, d in TR["defaults"].items():
        a, b = TR["A"][k], TR["B"][k]
        if k in TR["per_tracer"]:
            assert len(a) == len(b) == 4 and len(set(a)) == 4 and len(set(b)) == 4, k
            assert all(x != y and x != d and y != d for x, y in zip(a, b)), k
        else:
            assert a != d and b != d and a != b, k
    for point in "AB":
        assert TR[point]["dXY"] != TR[point]["dYX"]
        for lattice in P.TRACER_AXES["lattice"]:        # crit strictly between the densities the lattice holds
            _, rR, _ = P.lattice_tr(lattice)
            assert rR.min() < TR[point]["crit"] < rR[rR > 0].min(), (point, lattice)
    for lattice in P.TRACER_AXES["lattice"]:            # the concentrations vary along x, along y, and from tracer to tracer
        dom = P.lattice_tr(lattice)[0]
        c = P.concentrations(dom, 4)
        both = (dom[:, 1:] == 1) & (dom[:, :-1] == 1), (dom[1:] == 1) & (dom[:-1] == 1)
        for k in range(4):
            assert np.abs(np.diff(c[k], axis=1))[both[0]].max() > 1e-2 and np.abs(np.diff(c[k], axis=0))[both[1]].max() > 1e-2 and c[k][dom == 1].min() > 0
            for j in range(k):
                assert np.abs(c[k] - c[j])[dom == 1].max() > 5e-2 and np.abs(c[k] / c[k][dom == 1].mean() - c[j] / c[j][dom == 1].mean())[dom == 1].max() > 5e-2, (j, k)


def test_the_instances_cover_every_pair_of_values_of_every_two_axes():
    t = P.RK2D_TR
    axes = dict(t["categorical"], **t["axes"])
    assert all(set(inst) == set(axes) for inst in t["instances"]) and len(t["instances"]) == 16
    names = sorted(axes)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            seen = {(inst[a], inst[b]) for inst in t["instances"]}
            assert seen == {(x, y) for x in axes[a] for y in axes[b]}, (a, b)


def test_the_two_lattices_take_the_two_launch_paths():
    """launch_fused_tracer (csrc/rk2d.hip) recomputed: the short lattice goes through the single launch of rk2d_fused<., true, ., 1>, the tall
    one through rk2d_fused_tracer with both copies of node_finish (and holds tile rows of either kind).  The formula is read off the
    source, so that a change there is met here."""
    import os
    from openlbmpm_amd import rk2d
    src = open(os.path.join(os.path.dirname(rk2d.__file__), "csrc", "rk2d.hip")).read()
    body = src[src.index("void launch_fused_tracer("):src.index("int launch_step(")]
    for line in ("constexpr int H = 3;", "if (ty * SH::TH - H <= 1) n_lo = ty + 1;", "if (ty * SH::TH + SH::TH - 1 + H >= c->ny - 2 && n_hi == 0) n_hi = tiles_y - ty;",
                 "if (n_lo + n_hi >= tiles_y) {", "launch_fused_tracer<FusedShape<8, 1>>(c, p);"):
        assert line in src and (line in body or "FusedShape" in line), line
    assert [ny for ny in range(8, 64) if P.tracer_launch(ny)[3]] == list(range(8, 21))
    dom, rR, rB = P.lattice_2d_short()
    assert dom.shape == (20, 70)
    n_lo, n_hi, tiles_y, single = P.tracer_launch(dom.shape[0])
    assert single and (n_lo, n_hi, tiles_y) == (1, 2, 3)
    tall = P.lattice_2d()[0]
    n_lo, n_hi, tiles_y, single = P.tracer_launch(tall.shape[0])
    assert not single and n_lo >= 1 and n_hi >= 1 and tiles_y - n_lo - n_hi >= 1, (n_lo, n_hi, tiles_y)
    assert tall.shape[1] % 64 != 0 and tall.shape[1] > 64          # a ragged second tile column
    # the short lattice: free boundary rows, a porous image with walls inside, the interface inside the image and across walls
    assert np.all(dom[:4] == 1) and np.all(dom[-4:] == 1) and 0.05 < 1.0 - dom[4:-4].mean() < 0.6
    red, blue = rR > 0, rB > 0
    rows = np.flatnonzero((red.any(axis=1)) & (blue.any(axis=1)))
    assert rows.min() >= 4 and rows.max() <= 15 and len(rows) >= 6, rows
    assert len(np.unique(rR[red])) > 100        # rippled densities: no exact ties in the wetting rules


class _Stop(Exception):
    pass


def _ini_config(tmp_path, monkeypatch, text, **driver):
    """the lbmpm_tracer_config that python -m openlbmpm_amd tr / Transport2DRK hands the library for the transportsetup.ini `text`"""
    import warnings
    from ini_fixtures import write_rk
    from openlbmpm_amd import _lib
    from openlbmpm_amd.Transport2DRK import Transport2DRK
    write_rk(str(tmp_path), nx=20, ny=48, steps=2, interval=25)
    (tmp_path / "transportsetup.ini").write_text(text)
    cap = _Capture()

    class Lib:
        def __getattr__(self, fn):
            if fn == "lbmpm_rk2d_tracer_set_concentration":
                raise _Stop()
            return getattr(cap, fn)
    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sim = Transport2DRK(str(tmp_path), output_dir=str(tmp_path / "out"), **driver)
        with pytest.raises(_Stop):
            sim.runTransport2DMPMCRKNew()
    return {f: cap.seen[f] for f, _ in _lib.TracerConfig._fields_}


def test_the_keys_of_the_transport_ini_reach_the_fields_of_their_rows(tmp_path, monkeypatch):
    """the ini reader behind Transport2DRK (config.read_transport) without a device: every key moved reaches exactly the field TR['ini']
    names, with the value of the file"""
    ini = """[SystemType]
Option = 'MPMC'
Reaction = 'yes'
Precipitation = 'no'
NumberSchemes = 5
[Reaction]
NumberReaction = 1
ReactionRate = 0.05
[TransportParameters]
NumberTracers = 3
DiffusionJ = 0.3, 0.4, 0.25
Tau = 1.0, 1.0, 1.0
BetaInterface = 0.8
[BoundaryCondition]
InletType = 'Dirichlet'
ConcentrationInlet = 0.9, 0.3, 0.6
OutletType = 'Freeflow'
[InitialCondition]
Type = 'Homogeneous'
TracerConc = 1.0, 0.5, 0.2
[FluidForTransport]
FluidType = 0
[RelaxationType]
Relaxation = 'MRT'
[TransportMRT]
DiffusionX = 0.12, 0.2, 0.15
DiffusionY = 0.21, 0.1, 0.14
DiffusionXY = 0.015, 0.015, 0.015
DiffusionYX = 0.03, 0.03, 0.03
"""
    base = _ini_config(tmp_path, monkeypatch, ini, inlet_concentration_from_ini=True)
    assert base == dict(num_tracers=3, diffusion_x=(0.12, 0.2, 0.15, 0.0), diffusion_y=(0.21, 0.1, 0.14, 0.0), diffusion_xy=0.015, diffusion_yx=0.03,
                        beta_interface=(0.8, 0.8, 0.8, 0.0), criteria_rho=0.5, inlet_concentration=(0.9, 0.3, 0.6, 0.0), dirichlet_inlet=1, free_outlet=1,
                        reaction_rate=0.05, diffusion_j=(0.3, 0.4, 0.25, 0.0))
    moved = {"DiffusionX": ("DiffusionX = 0.12, 0.2, 0.15", "DiffusionX = 0.12, 0.2, 0.17"), "DiffusionY": ("DiffusionY = 0.21", "DiffusionY = 0.22"),
             "DiffusionXY": ("DiffusionXY = 0.015", "DiffusionXY = 0.025"), "DiffusionYX": ("DiffusionYX = 0.03", "DiffusionYX = 0.04"),
             "BetaInterface": ("BetaInterface = 0.8", "BetaInterface = 0.55"), "ConcentrationInlet": ("ConcentrationInlet = 0.9, 0.3", "ConcentrationInlet = 0.9, 0.35"),
             "DiffusionJ": ("DiffusionJ = 0.3, 0.4", "DiffusionJ = 0.3, 0.45"), "ReactionRate": ("ReactionRate = 0.05", "ReactionRate = 0.08"),
             "InletType": ("InletType = 'Dirichlet'", "InletType = 'None'"), "OutletType": ("OutletType = 'Freeflow'", "OutletType = 'Dirichlet'")}
    assert set(moved) | {"NumberTracers"} == set(TR["ini"])
    for key, (old, new) in moved.items():
        assert ini.count(old) == 1, key
        got = _ini_config(tmp_path, monkeypatch, ini.replace(old, new), inlet_concentration_from_ini=True)
        changed = {f for f in got if got[f] != base[f]}
        if key == "InletType":              # (without the Dirichlet inlet the file's inlet values are not read: 1.0 each)
            changed -= {"inlet_concentration"}
        assert changed == {TR["ini"][key]}, (key, changed)
    two = ini.replace("Reaction = 'yes'", "Reaction = 'no'").replace("NumberTracers = 3", "NumberTracers = 2")
    for last in (", 0.25\n", ", 1.0\nBeta", ", 0.6\n", ", 0.2\n[Fluid", ", 0.15\n", ", 0.14\n", ", 0.015\nDiffusionYX", ", 0.03\n"):       # two values per list
        assert two.count(last) == 1, last
        two = two.replace(last, last[last.index("\n"):])
    got = _ini_config(tmp_path, monkeypatch, two, inlet_concentration_from_ini=True)
    assert got["num_tracers"] == 2 and got["reaction_rate"] == 0.0 and got["diffusion_x"] == (0.12, 0.2, 0.0, 0.0)
    # the reference's hard-coded inlet value of tracer 0 (Transport2DRK.py:1161), the driver's default
    assert _ini_config(tmp_path, monkeypatch, ini)["inlet_concentration"] == (1.0, 0.3, 0.6, 0.0)


def _tracer_moves():
    """(what, instance overrides, moved rows): every tracer parameter at its default, one value of a list at a time; two tracers' values of a
    list swapped; dXY <-> dYX; either end toggled.  The fourth value of a list is read with four tracers, the rest at the base (three
    tracers and the reaction); diffJ's fourth value is read by nothing (the reaction couples three tracers)"""
    A, D, live = TR["A"], TR["defaults"], P.RK2D_TR["live"]
    out = []
    for k in TR["per_tracer"]:
        for i in range(3 if k == "diffJ" else 4):
            v = list(A[k]); v[i] = D[k]
            out.append(("%s[%d] -> default" % (k, i), dict(tracers=4) if i == 3 else live.get("tr_" + k, {}), {"tr_" + k: tuple(v)}))
        for i, j in ((0, 1), (1, 2)) + (() if k == "diffJ" else ((2, 3),)):
            v = list(A[k]); v[i], v[j] = v[j], v[i]
            out.append(("%s[%d] <-> %s[%d]" % (k, i, k, j), dict(tracers=4) if j == 3 else live.get("tr_" + k, {}), {"tr_" + k: tuple(v)}))
    for k in ("dXY", "dYX", "crit", "reaction_rate"):
        out.append(("%s -> default" % k, live.get("tr_" + k, {}), {"tr_" + k: D[k]}))
    out.append(("dXY <-> dYX", {}, dict(tr_dXY=A["dYX"], tr_dYX=A["dXY"])))
    for name, ends in (("dirichlet_inlet off", (False, True)), ("free_outlet off", (True, False))):
        out.append((name, dict(ends=ends), None))
    return out


_sensitivities = {}


@pytest.mark.parametrize("what,over,moved", _tracer_moves(), ids=lambda v: v if isinstance(v, str) else "")
def test_every_tracer_parameter_matters_at_A(what, over, moved):
    t = P.RK2D_TR
    inst = dict(t["base"], **over)
    if moved is None:                   # an end toggled: against the base
        ref, got = run("rk2d-tr", P.params(t, "A"), tag="ref"), run("rk2d-tr", P.params(t, "A", inst))
    else:
        ref, got = run("rk2d-tr", P.params(t, "A", inst), tag="ref"), run("rk2d-tr", P.params(t, "A", inst, **moved))
    _sensitivities[what] = _matters("rk2d-tr", what, got, ref)


def test_the_table_of_tracer_moves_is_complete():
    whats = [m[0] for m in _tracer_moves()]
    for k in TR["defaults"]:
        assert any(w.startswith(k) and w.endswith("default") for w in whats), k
    if len(_sensitivities) == len(whats):
        w = min(_sensitivities, key=_sensitivities.get)
        print("rk2d-tr: the smallest sensitivity of a concentration to a tracer move: %.2e (%s)" % (_sensitivities[w], w))
