"""The step loop of the 3-D drivers (RKColorGradientD3Q19.py, Transport3DRK.py), once: a run is cut at the record cadence, the
checkpoint cadence and the cadence of every periodic analysis; at a stop the analyses that are due are visited in the order of the
driver's task list, the record is taken when one is due, then the solver runs to the next stop.  What differs between the analyses is
data of a PeriodicTask, what differs between the drivers is the `record` hook.  Under torchrun every visit and every record is a
collective: all ranks walk the same list in the same order.  Plain Python: nothing here touches the GPU or the library."""
import numpy as np


def steps_to_stop(done, total, cadences):
    """how many steps may run from `done` before the next stop: the end of the run, or the next multiple of a cadence (0: adds no stop)"""
    n = total - done
    for c in cadences:
        if c > 0:
            n = min(n, c - done % c)
    return n


class PeriodicTask:
    """One analysis a driver runs every `every` steps (0: never, no group, no stop).

    group           (name, description) of its group in a result file; file: which of the driver's files ("flow", "conc")
    here            the group exists on this rank (the tables are gathered: rank 0 holds the whole lattice's, the others get None)
    table()         takes the table (collective); it becomes owner.<attr>, the step joins owner.<steps_attr>
    datasets        ((name with %d for the step, attribute of the table), ...) written at every visit; an attribute that is None is left out
    report(step, t) what the guard or the log hears of the table (t = None off rank 0: a guard's verdict is collective); true: end the run
    closing()       [(name, array), ...] written behind <group>/Steps once the run is over
    mark            the monitor's way: the first visit calls mark() and takes no table
    before_record   visited before the stop's record, and in the tail after everything else (a verdict that ends the run must come
                    before the record: the tail then takes it, as at the end of a run of that many steps)
    only_multiples  the tail visits it only when the run's last step is a multiple of `every`
    joined          belongs to the stop of the task before it: the tail visits it before that one's closing datasets are written
    A step is never visited twice."""

    def __init__(self, owner, every, group, here, table, attr, steps_attr=None, file="flow", datasets=(("PlanesAtStep%d", "planes"),),
                 report=None, closing=None, mark=None, before_record=False, only_multiples=False, joined=False):
        self.owner, self.every, self.group, self.here, self.file = owner, int(every), group, bool(here), file
        self.table, self.attr, self.datasets, self.report, self.closing, self.mark = table, attr, datasets, report, closing, mark
        self.before_record, self.only_multiples, self.joined = before_record, only_multiples, joined
        self.out, self.steps, self.last = None, [], None
        if steps_attr:
            setattr(owner, steps_attr, self.steps)

    def due(self, done):
        return self.every > 0 and done % self.every == 0

    def visit(self, done):
        if self.last == done:
            return False
        self.last = done
        if self.mark is not None:
            self.mark()
            self.mark = None
            return False
        t = self.table()
        setattr(self.owner, self.attr, t)
        self.steps.append(int(done))
        if t is not None and self.out is not None:
            for name, field in self.datasets:
                if getattr(t, field) is not None:
                    self.out.write(self.group[0], name % done, getattr(t, field))
        return bool(self.report(done, t))

    def finish(self):
        if self.out is not None:
            self.out.write(self.group[0], "Steps", np.array(self.steps, dtype=np.int64))
            for name, a in self.closing():
                self.out.write(self.group[0], name, a)


def groups(tasks, file="flow"):
    """the groups the active tasks add to that result file on this rank"""
    return tuple(t.group for t in tasks if t.every > 0 and t.here and t.file == file)


def attach(tasks, out, file="flow"):
    """the opened result file (None: this rank writes none) to the tasks that write into it"""
    for t in tasks:
        if t.here and t.file == file:
            t.out = out


def run(tasks, done, total, record_every, checkpoint_every, record, step, checkpoint, progress=None):
    """Walk `done` to `total`; -> the step the run ended at (earlier than `total` when a task's verdict ended it).

    record(done, tail) -> done: takes the record of the state after `done` steps.  Inside the loop (tail = False) it may take steps of
    its own and return the new count -- the tracers' driver records the flow, takes one step and records the concentrations after it.
    step(n) runs n steps; checkpoint() writes one (the loop calls it only before the end of the run)."""
    tasks = [t for t in tasks if t.every > 0]
    early, late = [t for t in tasks if t.before_record], [t for t in tasks if not t.before_record]
    cadences = [record_every, checkpoint_every] + [t.every for t in tasks]

    def visit(some, done):
        return any([t.visit(done) for t in some if t.due(done)])          # (a list: every due task is visited, whatever the verdicts)

    def checkpoint_if_due(done):
        if checkpoint_every > 0 and done % checkpoint_every == 0 and done < total:
            checkpoint()

    while done < total:
        if visit(early, done):
            break                              # (before this step's record: the tail below takes it)
        stepped = False
        if done % record_every == 0:           # (a restarted run records its first step again: the counters of the checkpoint precede it)
            before, done = done, record(done, False)
            stepped = done != before
            if stepped:
                checkpoint_if_due(done)
        visit(tasks, done)
        # (a record that took a step and landed on the next record stop: that record comes first)
        n = 0 if stepped and done % record_every == 0 else steps_to_stop(done, total, cadences)
        if n:
            step(n)
            done += n
            checkpoint_if_due(done)
        if progress:
            progress(done)
    record(done, True)
    visited = []
    for t in late + early + [None]:
        if t is None or not t.joined:
            for v in visited:
                v.finish()
            visited = []
        if t is not None:
            if not t.only_multiples or t.due(done):
                t.visit(done)
            visited.append(t)
    return done
