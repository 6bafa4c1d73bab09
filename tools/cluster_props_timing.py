"""What clusters(props=True) costs on the bench lattice: the 512^3 porous medium of bench.py under the perturbation model, beside
clusters() and morphology() of the same build on the same state.  Not part of bench.py; there is no threshold, DESIGN.md keeps the numbers.

    python tools/cluster_props_timing.py [--size N] [--calls 7] [--states initial mixed random]

States: bench.py's `initial` and `mixed` (both colours in every cell: phi = 0, so the whole pore space is one B cluster) and `random`
(every cell R or B by a coin: two million clusters, the end where a workgroup meets more labels than its LDS table has rows).  Every call
ends in a stream synchronisation and is timed by the host clock; the four calls alternate, medians over `calls` rounds after a warm-up
round.  The atomics that the workgroup-level combine removes are counted on the host from the label field, as the kernel forms its runs:
`runs` = runs of equal labels inside a wave of 64 consecutive cells (what one add per run and column would issue), `chunk_labels` =
(label, workgroup) pairs (what is left after the combine, were no slot ever taken).  One JSON line per state.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--states", nargs="+", default=["initial", "mixed", "random"])
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import bench
    from openlbmpm_amd.rk3d import RK3DSlab
    n = a.size
    dom = bench.c5_domain((n, n, n))
    s = RK3DSlab(dom, 0, n, dict(relax="MRT"))
    for name in a.states:
        if name == "random":
            red = np.random.default_rng(1).random(dom.shape) < 0.5
            rR, rB = np.where((dom == 1) & red, 1.0, 0.0), np.where((dom == 1) & ~red, 1.0, 0.0)
        else:
            rR, rB = bench.c5_state(dom, 0, n, name)
        s.set_density(rR, rB)
        del rR, rB
        s.phase_field(diagnostics=True)
        c = s.clusters(props=True)              # the warm-up round: allocations, code objects
        s.morphology()
        count = c.table.shape[0]
        r = dict(state=name, size=n, fluid_cells=int(s.num_fluid_nodes), clusters=int(count), largest=int(c.table[:, 2].max()))
        calls = dict(clusters_ms=s.clusters, clusters_props_ms=lambda: s.clusters(props=True), props_alone_ms=lambda: s.cluster_props_part(count),
                     morphology_ms=s.morphology)
        ms = {k: [] for k in calls}
        for _ in range(a.calls):
            for k, call in calls.items():
                t = time.perf_counter()
                call()
                ms[k].append((time.perf_counter() - t) * 1e3)
        for k, v in ms.items():
            r[k] = dict(median=round(float(np.median(v)), 3), min=round(min(v), 3), max=round(max(v), 3))
        lab = s.clusters(labels=True).labels.reshape(-1)
        head = np.ones(lab.shape, dtype=bool)
        head[1:] = lab[1:] != lab[:-1]
        head[::64] = True
        runs = int(np.count_nonzero(head & (lab != NONE)))
        chunks = np.sort(np.concatenate([lab, np.full((-lab.size) % 1024, NONE, dtype=np.uint32)]).reshape(-1, 1024), axis=1)
        first = np.ones(chunks.shape, dtype=bool)
        first[:, 1:] = chunks[:, 1:] != chunks[:, :-1]
        per_chunk = np.count_nonzero(first & (chunks != NONE), axis=1)
        r.update(runs=runs, chunk_labels=int(per_chunk.sum()), most_labels_in_a_chunk=int(per_chunk.max()),
                 share_removed=round(1.0 - float(per_chunk.sum()) / max(runs, 1), 4))
        del lab, head, chunks, first
        print(json.dumps(r), flush=True)
    s.close()


if __name__ == "__main__":
    main()
