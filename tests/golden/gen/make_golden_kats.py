#!/usr/bin/env python3
"""Known-answer vectors for the reference kernels that no working loop launches (kernels of the five
kernel modules outside the call stacks of section 3).  Every case is ONE launch of the real kernel body under the numba
stand-in; the arguments are looked up BY THE KERNEL'S OWN PARAMETER NAMES (inspect.signature of the reference function)
in a table of seeded inputs, so a case is just (module, kernel, overrides).  Stored per case:

    <case>|kernel, <case>|module, <case>|args (names, in order), <case>|in|<arg> for every argument,
    <case>|out|<arg> for every array argument after the launch.

tests/test_kats_gpu.py replays each case through the same-named HIP entry point.  Container-only.
Writes tests/golden/kats_<module tag>.npz.

`wide_rk`, `wide_sc`, `wide_tr` emit the same cases on a second geometry, 66 x 9 with 513 fluid nodes: two full tiles of 256 nodes and a
tile of one, two blocks of 64 columns for the boundary-row kernels.  Those go to tests/golden/kats_wide_<module tag>.npz in the
deduplicated format of tests/helpers.py (write_kat_cases): every distinct array once, outputs only where the launch changed the array;
a module whose file would pass 1e6 bytes is written as parts kats_wide_<module tag>_<i>.npz of consecutive cases.
"""
import inspect
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refenv  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from helpers import write_kat_cases  # noqa: E402

OUT = os.environ.get("LBMPM_GOLDEN_OUT") or os.path.dirname(HERE)

EX = np.array([0., 1., 0., -1., 0., 1., -1., -1., 1.]); EY = np.array([0., 0., 1., 0., -1., 1., 1., -1., -1.])
W9 = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)


WIDE = False                 # set by the wide_* targets


def geometry(nx=14, ny=18):
    """walls at x = 0 and x = nx-1, a disc, rows 0..3 and ny-4..ny-1 otherwise fluid"""
    if WIDE:
        return wide_geometry()
    dom = np.ones((ny, nx), dtype=np.int64)
    dom[:, 0] = 0; dom[:, -1] = 0
    yy, xx = np.mgrid[0:ny, 0:nx]
    dom[(xx - 6.5) ** 2 + (yy - 9.0) ** 2 <= 2.3 ** 2] = 0
    fluidNodes = np.flatnonzero(dom.reshape(-1) == 1).astype(np.int64)
    newIndex = -np.ones(ny * nx, dtype=np.int64)
    newIndex[fluidNodes] = np.arange(fluidNodes.size)
    return dom, fluidNodes, newIndex.reshape(ny, nx)


def wide_geometry(nx=66, ny=9):
    """walls at x = 0 and x = 65, a bar of solid cells in row 5; rows 0..3 and ny-2, ny-1 otherwise fluid.  513 = 2 * 256 + 1 fluid nodes:
    the last node, the one the row kernels reach through a solid neighbour, lies alone in the third tile; the second block of 64 columns
    holds column 64 (fluid) and 65 (wall)"""
    dom = np.ones((ny, nx), dtype=np.int64)
    dom[:, 0] = 0; dom[:, -1] = 0
    dom[5, 2:65] = 0
    fluidNodes = np.flatnonzero(dom.reshape(-1) == 1).astype(np.int64)
    assert fluidNodes.size == 513
    newIndex = -np.ones(ny * nx, dtype=np.int64)
    newIndex[fluidNodes] = np.arange(fluidNodes.size)
    return dom, fluidNodes, newIndex.reshape(ny, nx)


class Cases:
    def __init__(self, tag, module):
        self.tag, self.module, self.out = tag, module, {}

    def run(self, kernel, values, case=None, grid=None, block=(32, 1), module=None):
        case = case or kernel
        k = getattr(module or self.module, kernel)
        names = list(inspect.signature(k.py_func).parameters)
        missing = [n for n in names if n not in values]
        assert not missing, (kernel, missing)
        N = int(values[names[0]])
        xDim = int(values.get("xDim", 64))
        grid = grid or (xDim // block[0], -(-N // xDim))
        args = []
        for n in names:
            v = values[n]
            if isinstance(v, np.ndarray):
                v = np.array(v, copy=True)
            self.out["%s|in|%s" % (case, n)] = np.array(v, copy=True)
            args.append(v)
        k[grid, block](*args)
        for n, a in zip(names, args):
            if isinstance(a, np.ndarray):
                self.out["%s|out|%s" % (case, n)] = np.array(a, copy=True)
        self.out["%s|kernel" % case] = np.array(kernel)
        self.out["%s|module" % case] = np.array(self.tag)
        self.out["%s|args" % case] = np.array(names)
        changed = [n for n, a in zip(names, args) if isinstance(a, np.ndarray) and not np.array_equal(a, self.out["%s|in|%s" % (case, n)], equal_nan=True)]
        self.out["%s|noop" % case] = np.array(not changed)           # (a reference kernel that changes nothing: pinned as that)
        refenv.say("  %-44s changed: %s" % (case, ", ".join(changed) or "NOTHING"))
        return {n: a for n, a in zip(names, args)}

    def save(self):
        if WIDE:
            return self.save_wide()
        np.savez_compressed(os.path.join(OUT, "kats_%s.npz" % self.tag), **self.out)
        refenv.say("kats_%s: %d cases" % (self.tag, sum(1 for k in self.out if k.endswith("|kernel"))))


def rk_cases():
    import importlib
    A = importlib.import_module("AcceleratedRKGPU2D")
    rng = np.random.default_rng(1940)
    dom, fluidNodes, newIndex = geometry()
    ny, nx = dom.shape
    N = fluidNodes.size
    nbr = np.zeros(8 * N, dtype=np.int64)
    A.fillNeighboringNodes[(2, -(-N // 64)), (32, 1)](N, nx, ny, 64, fluidNodes, newIndex, nbr)
    nbr_solid = nbr.copy()                      # the colour-gradient loops mark non-fluid neighbours with -1 (RKD2Q9.py:632-655)
    fR = rng.uniform(0.01, 0.2, (N, 9)); fB = rng.uniform(0.01, 0.2, (N, 9))
    fB[: N // 3] *= 0.05; fR[-N // 3:] *= 0.05                 # red below, blue above, a mixed band between
    rR, rB = fR.sum(axis=1), fB.sum(axis=1)
    phi = (rR - rB) / (rR + rB)
    M = np.array([[1, 1, 1, 1, 1, 1, 1, 1, 1], [-4, -1, -1, -1, -1, 2, 2, 2, 2], [4, -2, -2, -2, -2, 1, 1, 1, 1], [0, 1, 0, -1, 0, 1, -1, -1, 1],
                  [0, -2, 0, 2, 0, 1, -1, -1, 1], [0, 0, 1, 0, -1, 1, 1, -1, -1], [0, 0, -2, 0, 2, 1, 1, -1, -1], [0, 1, -1, 1, -1, 0, 0, 0, 0],
                  [0, 0, 0, 0, 0, 1, -1, 1, -1]], dtype=np.float64)
    alphaR, alphaB = 0.2, 0.36
    cR = np.array([alphaR] + [(1. - alphaR) / 5.] * 4 + [(1. - alphaR) / 20.] * 4)
    cB = np.array([alphaB] + [(1. - alphaB) / 5.] * 4 + [(1. - alphaB) / 20.] * 4)
    T = dict(totalNodes=N, xDim=64, nx=nx, ny=ny, fluidNodes=fluidNodes, neighboringNodes=nbr_solid,
             delta=0.7, tauR=1.0, tauB=0.7, unitEX=EX, unitEY=EY, constantCR=cR, constantCB=cB, weightsCoeff=W9,
             physicalVX=rng.uniform(-0.03, 0.03, N), physicalVY=rng.uniform(-0.03, 0.03, N), fluidRhoR=rR, fluidRhoB=rB, fluidPDFR=fR, fluidPDFB=fB,
             transformationM=M, inverseTM=np.linalg.inv(M), collisionS=np.array([0., 1.64, 1.54, 0., 1.9, 0., 1.9, 1.0, 1.0]),
             betaCoeff=0.7, betaValue=0.7, AkR=7.0e-3, AkB=4.0e-3, solidDiff=0.35, solidPhi=0.4, surfaceTA=9.0e-3,
             constantB=np.array([-4. / 27.] + [2. / 27.] * 4 + [5. / 108.] * 4), schemeGradient=np.array([0.] + [4. / 12.] * 4 + [1. / 12.] * 4),
             CGX=np.zeros(N), CGY=np.ones(N), phiValue=phi, fluidPDFTotal=fR + fB, fluidPDFROld=rng.uniform(0., 1., (N, 9)),
             fluidPDFBOld=rng.uniform(0., 1., (N, 9)), collisionTotal1=np.zeros((N, 9)), collisionTotal2=np.zeros((N, 9)),
             gradientX=np.zeros(N), gradientY=np.zeros(N), forceX=rng.uniform(-1e-3, 1e-3, N), forceY=rng.uniform(-1e-3, 1e-3, N))
    # solid links as -1 for the kernels that test for it
    dx = EX[1:].astype(int); dy = EY[1:].astype(int)
    for k, loc in enumerate(fluidNodes):
        i, j = divmod(int(loc), nx)
        for d in range(8):
            if dom[(i + dy[d]) % ny, (j + dx[d]) % nx] != 1:
                nbr_solid[8 * k + d] = -1
    c = Cases("rk", A)
    c.run("calRKCollision1GPU2DSRT", T)
    c.run("calRKCollision1GPU2DMRT", T)
    c.run("calRKCollision23GPU", T)
    # a node with zero gradient takes the other branch of :553 and :574
    flat = dict(T, fluidRhoR=np.full(N, 0.6), fluidRhoB=np.full(N, 0.25), solidDiff=0.35)
    c.run("calRKCollision23GPU", flat, case="calRKCollision23GPU#flat")
    c.run("copyFluidPDFLastStep", T)
    c.run("copyFluidPDFRecoverOutlet", T)
    c.run("calNeumannPhiOutlet", dict(T, neighboringNodes=nbr))
    c.run("calModifiedPeriodicBoundary", T)
    s1 = c.run("calRKCollision1TotalGPU2DSRT", T)
    s2 = c.run("calRKCollision2TotalGPUNew", T)
    c.run("calRecoloringProcess", dict(T, collisionTotal1=s1["collisionTotal1"], collisionTotal2=s2["collisionTotal2"], gradientX=s2["gradientX"],
                                      gradientY=s2["gradientY"]))
    c.run("calPhysicalVelocityRKGPU2DVNew", T)
    c.run("calMacroDensityRKGPU2DNew", dict(T, fluidRhoR=np.zeros(N), fluidRhoB=np.zeros(N)))
    # Boundary rows next to a SOLID cell (an image geometry without all-fluid rows beside the inlet / outlet rows): these kernels index
    # with the neighbour id unlooked-at, and numba wraps the -1 of a solid neighbour like Python does -- the LAST node.
    dom2 = dom.copy(); dom2[1, 4] = 0; dom2[ny - 2, 9] = 0; dom2[2, 8] = 0
    if WIDE:
        dom2[1, 64] = 0                         # the second block of 64 columns meets a solid neighbour too
    fn2 = np.flatnonzero(dom2.reshape(-1) == 1).astype(np.int64)
    ni2 = -np.ones(ny * nx, dtype=np.int64); ni2[fn2] = np.arange(fn2.size)
    N2 = fn2.size
    nbr2 = np.zeros(8 * N2, dtype=np.int64)
    A.fillNeighboringNodes[(2, -(-N2 // 64)), (32, 1)](N2, nx, ny, 64, fn2, ni2.reshape(ny, nx), nbr2)
    for k, loc in enumerate(fn2):
        i, j = divmod(int(loc), nx)
        for d in range(8):
            if dom2[(i + dy[d]) % ny, (j + dx[d]) % nx] != 1:
                nbr2[8 * k + d] = -1
    f2R = rng.uniform(0.01, 0.2, (N2, 9)); f2B = rng.uniform(0.01, 0.2, (N2, 9))
    T2 = dict(T, totalNodes=N2, fluidNodes=fn2, neighboringNodes=nbr2, fluidPDFR=f2R, fluidPDFB=f2B, fluidRhoR=f2R.sum(axis=1), fluidRhoB=f2B.sum(axis=1),
              fluidPDFROld=rng.uniform(0., 1., (N2, 9)), fluidPDFBOld=rng.uniform(0., 1., (N2, 9)))
    for kern in ("ghostPointsConstPressureLowerRK", "ghostPointsConstantVelocityRK", "ghostPointsConstPressureInletRK", "convectiveOutletGPU",
                 "convectiveOutletGhost2GPU", "convectiveOutletGhost3GPU"):
        c.run(kern, T2, case=kern + "#solid_neighbour")
    c.save()


def sc_cases():
    import importlib
    O = importlib.import_module("OptimizedD2Q9GPU")
    E = importlib.import_module("ExplicitD2Q9GPU")
    rng = np.random.default_rng(1454)
    dom, fluidNodes, newIndex = geometry()
    ny, nx = dom.shape
    N = fluidNodes.size
    nbr = np.zeros(8 * N, dtype=np.int64)
    O.fillNeighboringNodes[(2, -(-N // 64)), (32, 1)](N, nx, ny, 64, fluidNodes, newIndex, nbr)      # -1 where the neighbour is solid
    assert (nbr == -1).any()
    f = rng.uniform(0.02, 0.2, (2, N, 9)); f[1] *= 0.3
    rho = f.sum(axis=2)
    G = np.array([[0.0, 0.9], [0.9, 0.05]])
    tau = np.array([1.0, 0.8])
    T = dict(totalNodes=N, totaNodes=N, totalNum=N, numFluids=2, xDim=64, nx=nx, ny=ny, fluidNodes=fluidNodes, neighboringNodes=nbr,
             weightInter=np.array([0.111, 0.112, 0.113, 0.114, 0.0271, 0.0272, 0.0273, 0.0274]), interactionCoeff=G, interCoeff=G,
             interactionSolid=np.array([-0.4, 0.35]), interSolid=np.array([-0.4, 0.35]), tau=tau, tauReverse=1. / tau,
             weightCoeff=W9, weightsCoeff=W9, weigthCoeff=W9, unitEX=EX, unitEY=EY, EX=EX, EY=EY,
             fluidRho=rho, fluidPotential=rho * rng.uniform(0.9, 1.1, (2, N)), fluidPsi=np.zeros((2, N)), fluidPDF=f,
             fluidPDFNew=rng.uniform(0.02, 0.2, (2, N, 9)), fluidPDFOld=rng.uniform(0.02, 0.2, (2, N, 9)),
             fEq=rng.uniform(0.02, 0.2, (2, N, 9)), fForce=rng.uniform(-1e-3, 1e-3, (2, N, 9)),
             forceX=rng.uniform(-1e-2, 1e-2, (2, N)), forceY=rng.uniform(-1e-2, 1e-2, (2, N)),
             mixtureVX=rng.uniform(-0.05, 0.05, N), mixtureVY=rng.uniform(-0.05, 0.05, N),
             equilibriumVX=rng.uniform(-0.05, 0.05, (2, N)), equilibriumVY=rng.uniform(-0.05, 0.05, (2, N)),
             physicalVX=rng.uniform(-0.05, 0.05, N), physicalVY=rng.uniform(-0.05, 0.05, N), totalVX=np.zeros(N), totalVY=np.zeros(N),
             fluidPressure=np.zeros(N), constR=1.0, temperatureT=0.05, temperature=0.05, coeffA=2. / 49., coeffB=2. / 21., coeffAlpha=1.0,
             constC0=6.0, constG=-1.0, bodyFX=1.0e-4, bodyFY=-2.0e-4, densityH=1.1, specificVY=np.array([-1.0e-3, -5.0e-4]),
             specificRhoH=1.05, specificRhoL=0.95)
    c = Cases("sc", O)
    c.run("calFluidPotentialGPUPR", T)
    c.run("calMacroPressure", T)
    c.run("calInteractionForce", T)
    c.run("addBodyForceGPU", T)
    c.run("calEquilibriumVGPU", T)
    c.run("calEquilibriumFuncGPU", T)
    c.run("calCollisionSRTGPU", T)
    c.run("constantPressureZouHeBoundaryHigher", T)
    c.run("ghostPointsConstantPressureInlet", T)
    c.run("calVelocityBoundaryHigherChangGPU", T)
    c.run("calPressureBoundaryHigherChangGPU", T)
    c.run("calPressureBoundaryLowerChangGPU", T)
    c.run("interactionCollisionEOFProcess", T)
    c.run("calStreaming1withLinkGPU", T)
    c.run("interactionForceGuo", T)
    c.run("calCollisionGuo", T)
    c.run("calMacroPressureEX", T, module=E)
    c.run("calEffectiveMassPR", T, module=E)
    c.run("calTotalVelocityGPU", T, module=E)
    c.run("calPressureExpGPU", T, module=E)
    s = c.run("convectiveOutletGPUEFS", T, module=E)                    # chained like the loop (ShanChenD2Q9.py:1865-1884)
    chain = dict(T, fluidPDFNew=s["fluidPDFNew"], fluidRho=s["fluidRho"], fForce=s["fForce"], fEq=s["fEq"])
    s = c.run("convectiveOutletGhost2GPUEFS", chain, module=E)
    chain = dict(T, fluidPDFNew=s["fluidPDFNew"], fluidRho=s["fluidRho"], fForce=s["fForce"], fEq=s["fEq"])
    c.run("convectiveOutletGhost3GPUEFS", chain, module=E)
    c.save()


def tr_cases():
    import importlib
    A = importlib.import_module("AcceleratedRKGPU2D")
    T = importlib.import_module("AccelerateTransport2DRK")
    rng = np.random.default_rng(1053)
    dom, fluidNodes, newIndex = geometry()
    ny, nx = dom.shape
    N = fluidNodes.size
    nbr4 = np.zeros(4 * N, dtype=np.int64); nbr8 = np.zeros(8 * N, dtype=np.int64)
    T.fillNeighboringNodesTransport[(2, -(-N // 64)), (32, 1)](N, nx, ny, 64, fluidNodes, newIndex, nbr4)
    A.fillNeighboringNodes[(2, -(-N // 64)), (32, 1)](N, nx, ny, 64, fluidNodes, newIndex, nbr8)
    nT = 2
    VX5 = np.array([0., 1., -1., 0., 0.]); VY5 = np.array([0., 0., 0., 1., -1.]); W5 = np.array([1. / 3.] + [1. / 6.] * 4)
    yrow = fluidNodes // nx
    mask = (yrow < (5 if WIDE else 9))                           # boolean masks: True in the lower half
    mask[rng.integers(0, N, 6)] ^= True
    C = rng.uniform(0.2, 1.0, (nT, N))
    g5 = C[:, :, None] * W5[None, None, :] * rng.uniform(0.8, 1.2, (nT, N, 5))
    g9 = C[:, :, None] * W9[None, None, :] * rng.uniform(0.8, 1.2, (nT, N, 9))
    newList = np.array(sorted(set(rng.choice(np.flatnonzero((yrow >= 2) & (yrow <= 4) if WIDE else (yrow >= 3) & (yrow <= 8)), 7).tolist())), dtype=np.int64)
    # every listed node needs a masked, unlisted surrounding node (the reference divides by their count, T:239)
    ok = []
    for n in newList:
        s = nbr8[8 * n: 8 * n + 8]
        if any(q >= 0 and mask[q] and q not in newList for q in s):
            ok.append(n)
    newList = np.array(ok, dtype=np.int64)
    assert newList.size >= 3
    M5 = np.array([[1, 1, 1, 1, 1], [0, 1, -1, 0, 0], [0, 0, 0, 1, -1], [-4, 1, 1, 1, 1], [0, 1, 1, -1, -1]], dtype=np.float64)
    A5 = np.stack([-np.linalg.inv(M5) @ np.diag(1. / np.array([1.0, 0.5 + 3 * d, 0.5 + 3 * d, 1.1, 1.2])) for d in (1. / 6., 0.12)])
    M9 = np.array([[1, 1, 1, 1, 1, 1, 1, 1, 1], [-4, -1, -1, -1, -1, 2, 2, 2, 2], [4, -2, -2, -2, -2, 1, 1, 1, 1], [0, 1, 0, -1, 0, 1, -1, -1, 1],
                   [0, -2, 0, 2, 0, 1, -1, -1, 1], [0, 0, 1, 0, -1, 1, 1, -1, -1], [0, 0, -2, 0, 2, 1, 1, -1, -1], [0, 1, -1, 1, -1, 0, 0, 0, 0],
                   [0, 0, 0, 0, 0, 1, -1, 1, -1]], dtype=np.float64)
    A9 = np.stack([-np.linalg.inv(M9) @ np.diag(1. / np.array([1.0, 1.1, 1.2, 0.5 + 3 * d, 1.3, 0.5 + 3 * d, 1.3, 1.4, 1.4])) for d in (1. / 6., 0.12)])
    J = np.stack([np.array([j] + [(1. - j) / 4.] * 4) for j in (1. / 3., 0.4)])
    vx, vy = rng.uniform(-0.04, 0.04, N), rng.uniform(-0.04, 0.04, N)
    vx[:5] = 0.0; vy[:5] = 0.0                                   # (nodes at rest: the other branch of T:513)
    V = dict(totalNodes=N, xDim=64, nx=nx, ny=ny, numTracers=nT, numScheme=5, fluidNodes=fluidNodes, neighboringNodes=nbr4, neighboringTRNodes=nbr4,
             surroundingNodes=nbr8, unitVX=VX5, unitVY=VY5, unitX=VX5, unitY=VY5, velocityVX=vx, velocityVY=vy, velocityX=vx, velocityY=vy,
             physicalVX=vx, physicalVY=vy, tauTransport=np.array([1.0, 0.86]), tauDiff=np.array([1.0, 0.86]), valueJDE=J, tracerConc=C,
             tracerConcNew=C * rng.uniform(0.9, 1.1, (nT, N)), tracerPDF=g5, tracerPDFNew=np.zeros((nT, N, 5)), criteriaFluid=0.5,
             fluidRhoR=rng.uniform(0., 1., N), distriField=mask, distrField=mask, transportDomain=mask, newFluidList=newList, oldFluidList=newList,
             newList=newList, randomPert=1.0e-3, sumOldConc=np.array([40., 25.]), sumOldList=np.array([3., 2.]), sumNewList=np.array([2.5, 2.2]),
             totalTracer=np.array([40., 25.]), totalOld=np.array([3., 2.]), weightsCoeff=W5, transportM=M5, inverseRelaxationMS=A5,
             concBoundary=np.array([1.0, 0.25]), betaTracer=np.array([0.8, 0.5]), valueTransportDomain=-(1. - mask.astype(np.float64)),
             unitEX=EX, unitEY=EY, gradientX=rng.uniform(-0.2, 0.2, N), gradientY=rng.uniform(-0.2, 0.2, N))
    V["gradientX"][:4] = 0.0; V["gradientY"][:4] = 0.0           # (no interface there: the other branch of T:1031)
    c = Cases("tr", T)
    c.run("calCollisionTransportGPU", V)
    c.run("calUpdateDistributionGPU", dict(V, distriField=np.zeros(N, dtype=bool)))
    c.run("calUpdateConcOnNewNodesGPU", V)
    c.run("calUpdateConcOnOldNodesGPU", V)
    c.run("calUpdateConcOnAllNewNodesGPU", V)
    c.run("calUpdateConcWholeDomainGPU", V)
    c.run("calTransportInterfaceGPU", V)
    c.run("calUpdatedPDFWithNewRho", V)
    c.run("calFreeConcBoundary1", V)
    c.run("calFreeConcBoundary2", V)
    c.run("calZeroConcenBoundary", V)
    c.run("calUpdateConcInTransportDomainByV", V)
    v5 = rng.uniform(-0.04, 0.04, 5)                             # T:624 indexes the 5-entry unitVY by node: five nodes at most
    five = dict(V, totalNodes=5, tracerConc=C[:, :5].copy(), tracerPDF=g5[:, :5].copy(), velocityVX=v5, velocityVY=v5[::-1].copy())
    c.run("calCollisionTransportQuadraticEqlMRTGPU", five)
    try:
        c.run("calCollisionTransportQuadraticEqlMRTGPU", V, case="discard")
        raise SystemExit("expected an IndexError")
    except IndexError:
        for k in [k for k in c.out if k.startswith("discard|")]:
            del c.out[k]
    c.run("calAntiCollisionConcBoundary", V)
    Q9 = dict(V, numScheme=9, unitVX=EX, unitVY=EY, weightsCoeff=W9, tracerPDF=g9, neighboringNodes=nbr8, transportM=M9, inverseRelaxationMS=A9)
    c.run("calCollisionQ9", Q9)
    s1 = c.run("calStreaming1GPU", dict(Q9, totalNum=N, numFluids=nT, fluidPDF=g9, fluidPDFNew=np.zeros((nT, N, 9))))
    c.run("calStreaming2GPU", dict(Q9, totalNum=N, numFluids=nT, fluidPDF=g9, fluidPDFNew=s1["fluidPDFNew"]))
    c.run("calTransportInterfaceQ9GPU", Q9)
    try:
        c.run("calUpdateConcInTransportDomainByVQ9", Q9, case="discard")
        raise SystemExit("expected an IndexError")
    except IndexError:                                           # T:938-939: 9 weights into a 5-entry shared array
        for k in [k for k in c.out if k.startswith("discard|")]:
            del c.out[k]
    c.out["calUpdateConcInTransportDomainByVQ9|raises"] = np.array("IndexError")
    c.run("calTransportWithInterfaceD2Q9", Q9)
    c.run("calCollisionTransportLinearEqlMRTGPUD2Q9", Q9)
    c.save()


PART_LIMIT = 1000000          # bytes; no committed file of this repository exceeds 1 MiB


def _save_wide(self):
    """kats_wide_<tag>.npz, or -- where that would exceed PART_LIMIT -- the fewest parts kats_wide_<tag>_<i>.npz of consecutive cases
    (equal counts) that all stay below it"""
    records = []
    for key in self.out:
        if key.endswith("|kernel"):
            case = key[:-len("|kernel")]
            names = [str(n) for n in self.out[case + "|args"]]
            records.append(dict(case=case, kernel=str(self.out[key]), module=str(self.out[case + "|module"]), args=names,
                                inputs={n: self.out["%s|in|%s" % (case, n)] for n in names},
                                outputs={n: self.out["%s|out|%s" % (case, n)] for n in names if "%s|out|%s" % (case, n) in self.out}))
        elif key.endswith("|raises"):
            records.append(dict(case=key[:-len("|raises")], raises=str(self.out[key])))
    for parts in range(1, len(records) + 1):
        per = -(-len(records) // parts)
        paths = [os.path.join(OUT, "kats_wide_%s%s.npz" % (self.tag, "_%d" % i if parts > 1 else "")) for i in range(parts)]
        for i, path in enumerate(paths):
            write_kat_cases(path, records[i * per: (i + 1) * per])
        if max(os.path.getsize(path) for path in paths) <= PART_LIMIT:
            break
        for path in paths:
            os.remove(path)
    refenv.say("kats_wide_%s: %d cases in %d file(s)" % (self.tag, sum(1 for r in records if "kernel" in r), parts))


Cases.save_wide = _save_wide


if __name__ == "__main__":
    refenv.setup()
    which = sys.argv[1:] or ["rk"]
    for w in which:
        WIDE = w.startswith("wide_")
        globals()[(w[5:] if WIDE else w) + "_cases"]()
