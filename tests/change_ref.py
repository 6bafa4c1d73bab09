"""numpy restatement of the change table (lbmpm_rk3d_change / lbmpm_rk3dcsf_change, csrc/rk3d_change.h) from fields the solvers hand out:
the expressions of the table in include/lbmpm.h evaluated left to right (numpy rounds every operation once, as the library built with
-ffp-contract=off does), the masks of test_integrals_gpu.restate, numpy's own order of summation."""
import numpy as np

NOW = ("rhoR", "rhoB", "vx", "vy", "vz", "phi")     # the six values the integrals test
OLD = ("vx", "vy", "vz", "phi")                     # the four a snapshot keeps
EXACT = (0, 1, 2, 8, 9, 10)
SUMS = (3, 4, 5, 6, 7)


def restate(dom, now, old):
    """the eleven columns per plane; now[name], old[name]: [nz][ny][nx] (now: NOW, old: at least OLD).  Returns (table, sum|term| per entry)"""
    nz = dom.shape[0]
    T, A = np.zeros((nz, 11)), np.zeros((nz, 11))
    for z in range(nz):
        fl = dom[z] == 1
        v = [np.asarray(now[k])[z][fl] for k in NOW]
        w = [np.asarray(old[k])[z][fl] for k in OLD]
        fin = np.ones(int(fl.sum()), dtype=bool)
        for a in v + w:
            fin &= np.isfinite(a)
        T[z, 0], T[z, 10] = fl.sum(), (~fin).sum()
        ux, uy, uz, phi = (a[fin] for a in v[2:])
        ux0, uy0, uz0, phi0 = (a[fin] for a in w)
        red = phi > 0
        T[z, 1] = red.sum()
        T[z, 2] = (red != (phi0 > 0)).sum()
        u2 = ux * ux + uy * uy + uz * uz
        dx, dy, dz = ux - ux0, uy - uy0, uz - uz0
        du2 = dx * dx + dy * dy + dz * dz
        d = phi - phi0
        terms = {3: u2[red], 4: u2[~red], 5: du2[red], 6: du2[~red], 7: d * d}
        for c, t in terms.items():
            T[z, c], A[z, c] = t.sum(), np.abs(t).sum()
        T[z, 8] = du2.max() if du2.size else 0.0
        T[z, 9] = np.abs(d).max() if d.size else 0.0
    return T, A


def compare(planes, dom, now, old, what):
    """columns 0, 1, 2, 8, 9, 10 equal exactly; the sums within 2 (n - 1) 2^-53 sum|term| per plane, the distance between two orders of
    summation of the same rounded terms (tests/test_integrals_gpu.py derives it).  Returns the restated table"""
    T, A = restate(dom, now, old)
    assert planes.shape == T.shape, what
    for c in EXACT:
        assert np.array_equal(planes[:, c], T[:, c]), (what, c, planes[:, c], T[:, c])
    n = T[:, 0]
    with np.errstate(invalid="ignore", over="ignore"):
        bound = 2.0 * np.maximum(n - 1.0, 0.0)[:, None] * 2.0 ** -53 * A
        err = np.abs(planes - T)
    for c in SUMS:
        print("%s col %d: worst error %.3e, bound there %.3e" % (what, c, err[:, c].max(), bound[np.argmax(err[:, c]), c]))
        # (equal entries first: a sum that overflowed is inf on both sides, and inf - inf is no distance)
        assert np.all((planes[:, c] == T[:, c]) | (err[:, c] <= bound[:, c])), (what, c, err[:, c], bound[:, c])
    return T
