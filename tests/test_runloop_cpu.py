"""The run loop of the two 3-D drivers (openlbmpm_amd/runloop.py) without a GPU: the stop arithmetic against a brute force, and both
drivers end to end on a fake solver -- every call the solver receives, every dataset written and every progress call, in order, against
lists recorded from the drivers as they were before the loop was shared (docs/EXPERIMENTS_r7.md, section O)."""
import itertools

import numpy as np

NX, NY, NZ = 6, 5, 8


class Trace(list):
    """entries '<steps the fake has taken> <what>'"""
    at = 0

    def add(self, what):
        self.append("%d %s" % (self.at, what))


class FakeSolver:
    """What a driver opens as its solver: constant arrays, hand-made tables, every call into the trace.  It answers both to the names the
    drivers used on the solver behind `.solver` and to the names of the handle the loop talks to now."""
    trace, steady_from = None, None          # (set by _install) steady_from = k: the k-th table of change() and the later ones are steady
    rank, suffix, whole_arrays = 0, "", False
    slab = sim = property(lambda self: self)

    def __init__(self, dom, par, *rest, **kw):
        self.dom = np.asarray(dom)
        self.shape = self.dom.shape
        self.steps = self.tables = self.base_steps = 0
        self.solver = self
        self.z0, self.nzl = 0, self.shape[0]
        self.num_fluid_nodes = int(self.dom.sum())
        self.trace.at = 0

    def step(self, n):
        self.trace.add("step(%d)" % n)
        self.steps += n
        self.trace.at = self.steps

    step_single = step

    def observe(self):
        pass

    def gather(self, a):
        return a

    def sync(self):
        self.trace.add("sync")

    def close(self):
        pass

    def set_density(self, rR, rB):
        self.trace.add("set_density")

    def set_macro(self, *a):
        self.trace.add("set_macro")

    def set_pdf(self, *a, **kw):
        self.trace.add("set_pdf")

    def get(self, name):
        self.trace.add("get(%s)" % name)
        return np.full(self.shape, 0.5)

    def get_pdf(self):
        self.trace.add("get_pdf")
        return np.full(self.shape + (19,), 0.125), np.full(self.shape + (19,), 0.25)

    def get_state(self):
        self.trace.add("get_state")
        return np.full(self.shape + (41,), 0.75), dict(doubles_per_cell=41, steps=self.steps, post_collision=False)

    def set_state(self, st, steps, post_collision):
        assert np.shape(st) == self.shape + (41,) and np.all(np.asarray(st) == 0.75)
        self.trace.add("set_state(%d)" % steps)
        self.steps = self.trace.at = int(steps)

    def set_concentration(self, k, a):
        self.trace.add("set_concentration(%d)" % k)

    def get_concentration(self, k):
        self.trace.add("get_concentration(%d)" % k)
        return np.full(self.shape, 0.25)

    def integrals(self):
        from openlbmpm_amd.integrals import Integrals
        self.trace.add("integrals")
        planes = np.zeros((NZ, 12))
        planes[:, :4] = (12., 6., 6., 6.)
        return Integrals(planes, NX, NY)

    def tracer_integrals(self):
        from openlbmpm_amd.integrals import TracerIntegrals
        self.trace.add("tracer_integrals")
        planes = np.zeros((NZ, 2, 9))
        planes[:, :, :2] = (12., 3.)
        return TracerIntegrals(planes, NX, NY)

    def clusters(self, **kw):
        from openlbmpm_amd.clusters import PROP_COLUMNS, Clusters
        self.trace.add("clusters(%s)" % ", ".join("%s=%r" % kv for kv in sorted(kw.items())))
        table = np.array([[0, 1, 80, 0, 7], [5, 2, 16, 6, 7]], dtype=np.int64)
        props = None
        if kw.get("props"):
            props = np.zeros((2, len(PROP_COLUMNS)), dtype=np.int64)
            props[:, :3] = table[:, :3]
        return Clusters(table, NX, NY, NZ, props=props)

    def morphology(self, cut):
        from openlbmpm_amd.morphology import COLUMNS, Morphology
        self.trace.add("morphology(%r)" % cut)
        planes = np.zeros((NZ, len(COLUMNS)))
        planes[:, :5] = (6., 5., 1., 6., 5.)
        return Morphology(planes, NX, NY)

    def mark_change(self):
        self.trace.add("mark_change")

    def change(self):
        from openlbmpm_amd.change import COLUMNS, Change
        self.trace.add("change")
        self.tables += 1
        planes = np.zeros((NZ, len(COLUMNS)))
        planes[:, COLUMNS.index("cells")] = 12.
        planes[:, COLUMNS.index("u2_R")] = 1.
        if not (self.steady_from and self.tables >= self.steady_from):
            planes[:, COLUMNS.index("du2_R")] = 0.25
        return Change(planes, NX, NY, 4)


def _install(monkeypatch, steady_from=None):
    """The fake in the place of the solver that both drivers open, and ResultFile.write into the same trace.  The only lines of this
    module that know where a driver constructs its solver."""
    from openlbmpm_amd import RKColorGradientD3Q19, Transport3DRK, results
    trace = Trace()
    fake = type("Fake", (FakeSolver,), dict(trace=trace, steady_from=steady_from))
    monkeypatch.setattr(RKColorGradientD3Q19, "_CSFSlab", fake)
    monkeypatch.setattr(Transport3DRK, "_CSFTracerSlab", fake)
    write = results.ResultFile.write

    def traced(self, group, name, array):
        trace.add("write %s/%s" % (group, name))
        return write(self, group, name, array)
    monkeypatch.setattr(results.ResultFile, "write", traced)
    return trace


def _flow(tmp_path, monkeypatch, out="out", steady_from=None, **kw):
    from ini_fixtures import write_rk3d_csf
    from openlbmpm_amd.RKColorGradientD3Q19 import RKColorGradient3D
    trace = _install(monkeypatch, steady_from)
    write_rk3d_csf(str(tmp_path), nx=NX, ny=NY, nz=NZ, steps=12, relax="MRT")
    sim = RKColorGradient3D(str(tmp_path), output_dir=str(tmp_path / out), **kw)
    path = sim.runRKColorGradient3D(progress=lambda done: trace.add("progress(%d)" % done))
    assert path == sim.result_path and isinstance(sim.solver, FakeSolver)
    return sim, list(trace)


def _tracers(tmp_path, monkeypatch, steps, **kw):
    from ini_fixtures import write_rk3d_csf, write_transport
    from openlbmpm_amd.Transport3DRK import Transport3DRK
    trace = _install(monkeypatch)
    write_rk3d_csf(str(tmp_path), nx=NX, ny=NY, nz=NZ, steps=steps, relax="MRT")
    write_transport(str(tmp_path))
    sim = Transport3DRK(str(tmp_path), output_dir=str(tmp_path / "out"), **kw)
    paths = sim.runTransport3DMPMCRK(progress=lambda done: trace.add("progress(%d)" % done))
    assert paths == (sim.result_path, sim.concentration_path) and isinstance(sim.solver, FakeSolver)
    return sim, list(trace)


FLOW = dict(record_every=4, integrals_every=3, clusters_every=5, clusters_props=True, morphology_every=6, steady_every=4, checkpoint_every=6)
RESTART = dict(record_every=3, integrals_every=4, steady_every=3, checkpoint_every=6)


def _record(k):
    """the entries of record k: five fields taken, five datasets written"""
    return ["get(rhoR)", "get(rhoB)", "get(vx)", "get(vy)", "get(vz)", "write FluidMacro/FluidDensityRin%d" % k, "write FluidMacro/FluidDensityBin%d" % k,
            "write FluidVelocity/FluidVelocityXAt%d" % k, "write FluidVelocity/FluidVelocityYAt%d" % k, "write FluidVelocity/FluidVelocityZAt%d" % k]


def _tracer_record(k):
    return ["get_concentration(0)", "get_concentration(1)", "write TransportMacro/TracerConcType0in%d" % k, "write TransportMacro/TracerConcType1in%d" % k]


def _at(step, entries):
    return ["%d %s" % (step, e) for e in entries]


CHECKPOINT = ["sync", "get_state", "write Checkpoint/State", "write Checkpoint/Info"]
CLUSTERS = "clusters(connectivity=6, props=True)"

# ---- recorded from the drivers before the loop was shared (the commit docs/EXPERIMENTS_r7.md, section O, names); not regenerated since
FLOW_TRACE = ['0 set_density', '0 mark_change'] + \
    _at(0, _record(0)) + \
    ['0 integrals', '0 write Integrals/PlanesAtStep0', '0 clusters(connectivity=6, props=True)', '0 write Clusters/TableAtStep0',
     '0 write Clusters/PropsAtStep0', '0 morphology(0.0)', '0 write Morphology/PlanesAtStep0', '0 step(3)',
     '3 progress(3)', '3 integrals', '3 write Integrals/PlanesAtStep3', '3 step(1)',
     '4 progress(4)', '4 change', '4 write Steady/PlanesAtStep4'] + \
    _at(4, _record(1)) + \
    ['4 step(1)', '5 progress(5)', '5 clusters(connectivity=6, props=True)', '5 write Clusters/TableAtStep5',
     '5 write Clusters/PropsAtStep5', '5 step(1)'] + \
    _at(6, CHECKPOINT) + \
    ['6 progress(6)', '6 integrals', '6 write Integrals/PlanesAtStep6', '6 morphology(0.0)',
     '6 write Morphology/PlanesAtStep6', '6 step(2)', '8 progress(8)', '8 change',
     '8 write Steady/PlanesAtStep8'] + \
    _at(8, _record(2)) + \
    ['8 step(1)', '9 progress(9)', '9 integrals', '9 write Integrals/PlanesAtStep9',
     '9 step(1)', '10 progress(10)', '10 clusters(connectivity=6, props=True)', '10 write Clusters/TableAtStep10',
     '10 write Clusters/PropsAtStep10', '10 step(2)', '12 progress(12)'] + \
    _at(12, _record(3)) + \
    ['12 integrals', '12 write Integrals/PlanesAtStep12', '12 write Integrals/Steps', '12 write Integrals/Columns',
     '12 clusters(connectivity=6, props=True)', '12 write Clusters/TableAtStep12', '12 write Clusters/PropsAtStep12', '12 write Clusters/Steps',
     '12 write Clusters/Columns', '12 write Clusters/PropColumns', '12 morphology(0.0)', '12 write Morphology/PlanesAtStep12',
     '12 write Morphology/Steps', '12 write Morphology/Columns', '12 change', '12 write Steady/PlanesAtStep12',
     '12 write Steady/Steps', '12 write Steady/Columns', '12 write Steady/Criteria', '12 write Steady/CriteriaColumns',
     '12 sync']

EARLY_TRACE = ['0 set_density', '0 mark_change'] + \
    _at(0, _record(0)) + \
    ['0 integrals', '0 write Integrals/PlanesAtStep0', '0 clusters(connectivity=6, props=True)', '0 write Clusters/TableAtStep0',
     '0 write Clusters/PropsAtStep0', '0 morphology(0.0)', '0 write Morphology/PlanesAtStep0', '0 step(3)',
     '3 progress(3)', '3 integrals', '3 write Integrals/PlanesAtStep3', '3 step(1)',
     '4 progress(4)', '4 change', '4 write Steady/PlanesAtStep4'] + \
    _at(4, _record(1)) + \
    ['4 step(1)', '5 progress(5)', '5 clusters(connectivity=6, props=True)', '5 write Clusters/TableAtStep5',
     '5 write Clusters/PropsAtStep5', '5 step(1)'] + \
    _at(6, CHECKPOINT) + \
    ['6 progress(6)', '6 integrals', '6 write Integrals/PlanesAtStep6', '6 morphology(0.0)',
     '6 write Morphology/PlanesAtStep6', '6 step(2)', '8 progress(8)', '8 change',
     '8 write Steady/PlanesAtStep8'] + \
    _at(8, _record(2)) + \
    ['8 integrals', '8 write Integrals/PlanesAtStep8', '8 write Integrals/Steps', '8 write Integrals/Columns',
     '8 clusters(connectivity=6, props=True)', '8 write Clusters/TableAtStep8', '8 write Clusters/PropsAtStep8', '8 write Clusters/Steps',
     '8 write Clusters/Columns', '8 write Clusters/PropColumns', '8 morphology(0.0)', '8 write Morphology/PlanesAtStep8',
     '8 write Morphology/Steps', '8 write Morphology/Columns', '8 write Steady/Steps', '8 write Steady/Columns',
     '8 write Steady/Criteria', '8 write Steady/CriteriaColumns', '8 sync']

PLAIN_TRACE = ['0 set_density'] + \
    _at(0, _record(0)) + \
    ['0 step(4)', '4 progress(4)'] + \
    _at(4, _record(1)) + \
    ['4 step(4)', '8 progress(8)'] + \
    _at(8, _record(2)) + \
    ['8 step(4)', '12 progress(12)'] + \
    _at(12, _record(3)) + \
    ['12 sync']

RESTART_TRACE = ['0 set_state(6)', '6 mark_change'] + \
    _at(6, _record(2)) + \
    ['6 step(2)', '8 progress(8)', '8 integrals', '8 write Integrals/PlanesAtStep8',
     '8 step(1)', '9 progress(9)', '9 change', '9 write Steady/PlanesAtStep9'] + \
    _at(9, _record(3)) + \
    ['9 step(3)', '12 progress(12)'] + \
    _at(12, _record(4)) + \
    ['12 integrals', '12 write Integrals/PlanesAtStep12', '12 write Integrals/Steps', '12 write Integrals/Columns',
     '12 change', '12 write Steady/PlanesAtStep12', '12 write Steady/Steps', '12 write Steady/Columns',
     '12 write Steady/Criteria', '12 write Steady/CriteriaColumns', '12 sync']

TRACER_TRACE = ['0 set_density', '0 set_concentration(0)', '0 set_concentration(1)', '0 integrals',
     '0 write Integrals/PlanesAtStep0', '0 tracer_integrals', '0 write TracerIntegrals/PlanesAtStep0'] + \
    _at(0, _record(0)) + \
    ['0 step(1)'] + \
    _at(1, _tracer_record(0)) + \
    ['1 step(1)', '2 progress(2)', '2 integrals', '2 write Integrals/PlanesAtStep2',
     '2 tracer_integrals', '2 write TracerIntegrals/PlanesAtStep2', '2 step(1)'] + \
    _at(3, CHECKPOINT) + \
    ['3 progress(3)'] + \
    _at(3, _record(1)) + \
    ['3 step(1)'] + \
    _at(4, _tracer_record(1)) + \
    ['4 integrals', '4 write Integrals/PlanesAtStep4', '4 tracer_integrals', '4 write TracerIntegrals/PlanesAtStep4',
     '4 step(2)'] + \
    _at(6, CHECKPOINT) + \
    ['6 progress(6)', '6 integrals', '6 write Integrals/PlanesAtStep6', '6 tracer_integrals',
     '6 write TracerIntegrals/PlanesAtStep6'] + \
    _at(6, _record(2)) + \
    ['6 step(1)'] + \
    _at(7, _tracer_record(2)) + \
    ['7 progress(7)'] + \
    _at(7, _record(3)) + \
    _at(7, _tracer_record(3)) + \
    ['7 integrals', '7 write Integrals/PlanesAtStep7', '7 tracer_integrals', '7 write TracerIntegrals/PlanesAtStep7',
     '7 write Integrals/Steps', '7 write Integrals/Columns', '7 write TracerIntegrals/Steps', '7 write TracerIntegrals/Columns',
     '7 sync']

TRACER_EVERY_STEP_TRACE = ['0 set_density', '0 set_concentration(0)', '0 set_concentration(1)', '0 integrals',
     '0 write Integrals/PlanesAtStep0', '0 tracer_integrals', '0 write TracerIntegrals/PlanesAtStep0'] + \
    _at(0, _record(0)) + \
    ['0 step(1)'] + \
    _at(1, _tracer_record(0)) + \
    ['1 progress(1)'] + \
    _at(1, _record(1)) + \
    ['1 step(1)'] + \
    _at(2, _tracer_record(1)) + \
    ['2 integrals', '2 write Integrals/PlanesAtStep2', '2 tracer_integrals', '2 write TracerIntegrals/PlanesAtStep2',
     '2 progress(2)'] + \
    _at(2, _record(2)) + \
    ['2 step(1)'] + \
    _at(3, _tracer_record(2)) + \
    _at(3, CHECKPOINT) + \
    ['3 progress(3)'] + \
    _at(3, _record(3)) + \
    ['3 step(1)'] + \
    _at(4, _tracer_record(3)) + \
    ['4 integrals', '4 write Integrals/PlanesAtStep4', '4 tracer_integrals', '4 write TracerIntegrals/PlanesAtStep4',
     '4 progress(4)'] + \
    _at(4, _record(4)) + \
    _at(4, _tracer_record(4)) + \
    ['4 write Integrals/Steps', '4 write Integrals/Columns', '4 write TracerIntegrals/Steps', '4 write TracerIntegrals/Columns',
     '4 sync']


# ---- the stop arithmetic
def _brute(done, total, cadences):
    """the smallest n >= 1 such that done + n is the end of the run or a multiple of an active cadence"""
    n = 1
    while done + n != total and not any(c > 0 and (done + n) % c == 0 for c in cadences):
        n += 1
    return n


def test_the_stop_arithmetic_against_brute_force():
    from openlbmpm_amd.runloop import steps_to_stop
    further = [c for r in range(4) for c in itertools.combinations_with_replacement((0, 1, 3, 5, 7), r)]
    seen = 0
    for total in (1, 7, 12):
        for record in (1, 3, 4, 12, 20):
            for checkpoint in (0, 4):
                for more in further:
                    cadences = (record, checkpoint) + more
                    for done in range(total):
                        assert steps_to_stop(done, total, cadences) == _brute(done, total, cadences), (done, total, cadences)
                        seen += 1
                    assert steps_to_stop(total, total, cadences) == 0          # (the end of the run: nothing left to take)
    assert seen == (1 + 7 + 12) * 5 * 2 * 56
    assert steps_to_stop(2, 12, (20, 0, 0, 0)) == 10                           # a cadence of 0 adds no stop


# ---- both drivers on the fake
def test_flow_driver_trace(tmp_path, monkeypatch):
    from openlbmpm_amd.results import load_results
    sim, trace = _flow(tmp_path, monkeypatch, **FLOW)
    assert trace == FLOW_TRACE
    assert sim.integral_steps == [0, 3, 6, 9, 12] and sim.cluster_steps == [0, 5, 10, 12] and sim.morphology_steps == [0, 6, 12]
    assert sim.steady_steps == [4, 8, 12] and len(sim.steady_criteria) == 3 and sim.steady_step is None
    assert sim.records == 4 and sim._step_now == 12 and sim.checkpoint_path.startswith(str(tmp_path / "out"))
    assert sim.integrals.planes.shape == (NZ, 12) and sim.clusters.props.shape == (2, 14) and sim.morphology.planes.shape == (NZ, 28) and sim.change.steps == 4
    res = load_results(sim.result_path)
    assert {k.split("/")[1] for k in res} == {"FluidMacro", "FluidVelocity", "Integrals", "Clusters", "Morphology", "Steady"}
    assert list(res["/Steady/Steps"]) == [4, 8, 12] and res["/Steady/Criteria"].shape == (3, 8) and list(res["/Clusters/Steps"]) == [0, 5, 10, 12]


def test_flow_driver_stops_early_when_steady(tmp_path, monkeypatch):
    from openlbmpm_amd.results import load_results
    sim, trace = _flow(tmp_path, monkeypatch, steady_from=2, steady_tol=1e-3, **FLOW)
    assert trace == EARLY_TRACE
    assert "8 progress(8)" == [e for e in trace if "progress" in e][-1] and not any(e.startswith(("9 ", "10 ", "11 ", "12 ")) for e in trace)
    assert sim.steady_step == 8 and sim.steady_steps == [4, 8] and sim._step_now == 8
    # the break comes before that step's record: the tail takes it, and every table, at step 8
    tail = trace[trace.index("8 progress(8)") + 1:]
    assert tail[:2] == ["8 change", "8 write Steady/PlanesAtStep8"] and tail[2:12] == _at(8, _record(2)) and sim.records == 3
    assert sim.integral_steps == [0, 3, 6, 8] and sim.cluster_steps == [0, 5, 8] and sim.morphology_steps == [0, 6, 8]
    res = load_results(sim.result_path)
    assert list(res["/Steady/Steps"]) == [4, 8] and list(res["/Integrals/Steps"]) == [0, 3, 6, 8] and "/FluidMacro/FluidDensityRin2" in res


def test_flow_driver_with_every_cadence_off(tmp_path, monkeypatch):
    from openlbmpm_amd.results import load_results
    sim, trace = _flow(tmp_path, monkeypatch, record_every=4)
    assert trace == PLAIN_TRACE
    assert [e for e in trace if "step(" in e] == ["0 step(4)", "4 step(4)", "8 step(4)"]          # no extra stop
    assert {k.split("/")[1] for k in load_results(sim.result_path)} == {"FluidMacro", "FluidVelocity"}
    assert sim.integral_steps == sim.cluster_steps == sim.morphology_steps == sim.steady_steps == sim.steady_criteria == [] and sim.records == 4


def test_flow_driver_from_a_checkpoint(tmp_path, monkeypatch):
    first, _ = _flow(tmp_path, monkeypatch, **RESTART)
    assert first.records == 5 and first.steady_steps == [3, 6, 9, 12]
    sim, trace = _flow(tmp_path, monkeypatch, out="again", restart_from=first.checkpoint_path, **RESTART)
    assert trace == RESTART_TRACE
    # the first visit of the monitor after the restart marks; the record at step 6 (the checkpoint's counter precedes it) is taken again
    assert trace[:2] == ["0 set_state(6)", "6 mark_change"] and trace[2:12] == _at(6, _record(2))
    assert sim.steady_steps == [9, 12] and sim.records == 5 and sim.integral_steps == [8, 12]


def test_tracer_driver_trace(tmp_path, monkeypatch):
    sim, trace = _tracers(tmp_path, monkeypatch, 7, record_every=3, integrals_every=2, checkpoint_every=3, clusters_every=2, morphology_every=2, steady_every=2)
    assert trace == TRACER_TRACE
    assert sim.integral_steps == [0, 2, 4, 6, 7] and sim.records == 4 and sim.tracer_integrals.planes.shape == (NZ, 2, 9)
    assert len([e for e in trace if "progress" in e]) == 4                                      # one call per pass of the loop


def test_tracer_driver_recording_every_step(tmp_path, monkeypatch):
    sim, trace = _tracers(tmp_path, monkeypatch, 4, record_every=1, integrals_every=2, checkpoint_every=3)
    assert trace == TRACER_EVERY_STEP_TRACE
    assert [e for e in trace if "step(" in e] == ["0 step(1)", "1 step(1)", "2 step(1)", "3 step(1)"]           # the run to the next stop is empty
    assert sim.integral_steps == [0, 2, 4] and sim.records == 5                                  # (no step twice)


# ---- the order of visits, stated once more
ORDER = ("monitor", "record", "integrals", "clusters", "morphology")
TAIL_ORDER = ("record", "integrals", "clusters", "morphology", "monitor")
EVERY = dict(monitor=FLOW["steady_every"], record=FLOW["record_every"], integrals=FLOW["integrals_every"], clusters=FLOW["clusters_every"],
             morphology=FLOW["morphology_every"])


def _kind(what):
    if what.startswith(("mark_change", "change", "write Steady/")):
        return "monitor"
    if what.startswith(("get(", "get_pdf", "write FluidMacro/", "write FluidVelocity/", "write FluidPDF/")):
        return "record"
    for kind in ("integrals", "clusters", "morphology"):
        if what.startswith((kind, "write %s/" % kind.capitalize())):
            return kind
    return None


def _visits(entries):
    """{step: the kinds of visit in the order they came, each once}"""
    out = {}
    for e in entries:
        at, what = e.split(" ", 1)
        kind = _kind(what)
        if kind is not None:
            seen = out.setdefault(int(at), [])
            if not seen or seen[-1] != kind:
                seen.append(kind)
    return out


def test_the_order_of_visits_at_every_stop(tmp_path, monkeypatch):
    sim, trace = _flow(tmp_path, monkeypatch, **FLOW)
    last = max(i for i, e in enumerate(trace) if "progress" in e)
    loop, tail = _visits(trace[:last]), _visits(trace[last + 1:])
    stops = [s for s in range(12) if any(s % c == 0 for c in EVERY.values())]
    assert sorted(loop) == stops
    for s in stops:
        assert loop[s] == [k for k in ORDER if s % EVERY[k] == 0], s
    assert tail == {12: list(TAIL_ORDER)}                                      # (12 is a multiple of steady_every: the monitor's last visit)
    # between two stops nothing but the run of steps, the checkpoint when one is due, and the progress call
    rest = [e.split(" ", 1)[1] for e in trace[:last + 1] if _kind(e.split(" ", 1)[1]) is None]
    assert [e for e in rest if e not in CHECKPOINT and not e.startswith(("step(", "progress(", "set_"))] == []
