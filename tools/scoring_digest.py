#!/usr/bin/env python3
"""tools/scoring_digest.py -- one SHA-256 per output array of every scoring call (clone_loglik, clone_pair_loglik, clone_loglik_dm, clone_loglik_by_block,
project_cells, clone_evidence) over a fixed grid of small cases, in a fixed order: two builds of the library with the same ABI return the same bits exactly
when their outputs are the same, line for line.
   python tools/scoring_digest.py                                   (the tree's library)
   CLONEALIGN_HIP_LIB=build_ab/parent/libclonealign_hip.so python tools/scoring_digest.py

The grid varies one axis at a time around a base case (u8 storage, 257 cells x 130 genes, 7 clones, 2 factors, the constant, row-major, all cells):
storage (u8 with counts >= 255 -- one exactly 255, one in the last gene, one in a cell outside the cell range --, u16, f32 with a non-integer value), shape
((1, 1), (65, 17), (257, 130), (300, 1025)), columns ((C, D) = (2, 0), (7, 2), (12, 8) for 8, 16 and 32 table columns, and two column groups where the engine
takes that many clones), with_const, layout, cell range (all; lo = 63, 2 cells), the by-block labellings (one block; three contiguous blocks cut between genes
16 | 17 and at the last gene; g % 3; a labelling with an empty block), W = 1 and 8 pair weights, K = 1 and 16 concentrations with one above 2^100, K = 1 and 2
free factors, P = 0 and 1 covariates, max_iter = 3, Q = 1 and 5 nodes, the evidence at K = 0, and a two-rank group where two devices are visible.  E has a
clone with E = 0 at a gene some cell has counts in and one with E = 0 at a gene no cell has counts in; one cell has no counts at all.
The first line is the library's build id; a line "skipped ..." says what this machine or this engine could not run."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clonealign_amd import engine as _engine  # noqa: E402
from clonealign_amd.api import gauss_hermite_rule  # noqa: E402
from clonealign_amd.engine import HipEngine, HipGroupEngine  # noqa: E402


def sha(a):
    if a is None:
        return "none"
    a = np.ascontiguousarray(a)
    return f"{a.dtype.str}{list(a.shape)} " + hashlib.sha256(a.tobytes()).hexdigest()


def emit(case, call, res):
    for k in sorted(res) if isinstance(res, dict) else [None]:
        v = res[k] if k is not None else res
        if k != "pairs":
            print(f"{case} | {call}{'' if k is None else '.' + k} | {sha(v)}")


def problem(N, G, C, D, storage, seed):
    """Counts (80 % zeros), copy numbers, E with its two kinds of zeros, the factors, a covariate column and a prior."""
    rng = np.random.default_rng(seed)
    L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
    mu = rng.lognormal(-1.4, 1.0, G)
    Y = rng.poisson(mu[None, :] * L[:, rng.integers(0, C, N)].T).astype(np.int64)
    Y[:, 0] += 1                                                     # (no empty matrix)
    if storage == "u16":
        hot = rng.choice(N * G, size=max(1, N * G // 50), replace=False)
        Y.reshape(-1)[hot] = rng.integers(256, 60001, size=hot.size)
    E = mu[:, None] * L
    if G >= 17 and C >= 2:
        E[3, 0] = 0.0                                                # a clone with E = 0 where a cell has counts ...
        Y[min(2, N - 1), 3] = 2
        E[9, 1] = 0.0                                                # ... and one where no cell has any
        Y[:, 9] = 0
    if N > 4:
        Y[4, :] = 0                                                  # a cell with no counts at all
    if storage == "u8":                                              # the overflow list: one exactly 255, one in the last gene, one in a cell outside (63, 2)
        Y[0, G // 2] = 255
        Y[min(5, N - 1), G - 1] = 300
        Y[min(100, N - 1), min(1, G - 1)] = 1000
        Y[min(64, N - 1), min(6, G - 1)] = 70000                     # (and one inside it)
    if storage == "f32":
        Y = Y.astype(np.float32)
        Y[min(7, N - 1), min(2, G - 1)] = 2.5                        # a non-integer value
    else:
        Y = Y.astype(np.int32)
    U = rng.normal(size=(N, 8)) * 0.5
    V = rng.normal(size=(G, 8)) * 0.3
    lp = np.log(rng.dirichlet(np.ones(C), size=N))
    return Y, L, E, U, V, lp


def labellings(G):
    one = np.zeros(G, dtype=np.int32)
    three = np.minimum(np.arange(G) // 17, 1).astype(np.int32)       # cut between genes 16 | 17 ...
    three[G - 1] = 2                                                 # ... and at the last gene
    hole = (np.arange(G) % 2).astype(np.int32) * 2                   # labels 0 and 2 of three: block 1 is empty
    return [("one", one, 1), ("three", three, 3), ("mod3", (np.arange(G) % 3).astype(np.int32), 3), ("hole", hole, 3)]


def run_case(name, N, G, C, D, storage="u8", const=True, layout="row", cells=None, full=False, devices=None, seed=1):
    """The calls of one engine.  full: every call with every one of its own axes; else the calls at one setting each."""
    Y, L, E, U, V, lp = problem(N, G, C, D, storage, seed)
    f = np.asfortranarray if layout == "col" else np.ascontiguousarray
    kw = dict(y_storage=storage, layout=layout)
    try:
        if devices is None:
            eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, **kw)
        else:
            eng = HipGroupEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, devices=devices, **kw)
    except Exception as e:  # noqa: BLE001
        print(f"{name} | skipped: the engine refused the case ({type(e).__name__}: {str(e)[:120]})")
        return
    try:
        Uv, Vv = (None, None) if D == 0 else (f(U[:, :D]), f(V[:, :D]))
        Ef = f(E)
        emit(name, "clone_loglik", eng.clone_loglik(Ef, Uv, Vv, const=const))
        for lab, bg, B in (labellings(G) if full else labellings(G)[1:2] if G >= 17 else labellings(G)[:1]):
            emit(name, f"by_block[{lab}]", eng.clone_loglik_by_block(Ef, Uv, Vv, bg, B, const=const, cells=cells))
        for W in ((1, 8) if full else (2,)):
            if C >= 2:
                emit(name, f"pair[W={W}]", eng.clone_pair_loglik(Ef, Uv, Vv, weights=np.linspace(0.1, 0.9, W) if W > 1 else (0.5,), const=const, cells=cells))
        for Kc in ((1, 16) if full else (3,)):
            conc = np.geomspace(0.5, 500.0, Kc) if Kc > 1 else np.array([40.0])
            if Kc == 16:
                conc[-1] = 2.0 ** 101                                # above 2^100: no product route for the whole call
            emit(name, f"dm[K={Kc}]", eng.clone_loglik_dm(Ef, Uv, Vv, concentration=conc, const=const, cells=cells))
        if C + D > 32:                                               # (the moment kernels' column groups are not this case's subject)
            return
        for K, P in (((1, 0), (1, 1), (2, 0), (2, 1), (0, 1), (0, 0)) if full else ((1, min(D, 1)),)):
            if K + P > 8 or G < K + P:
                continue
            Vk, Xk = (f(V[:, :K + P]) if K + P else None), (f(U[:, 4:4 + P]) if P else None)
            ps = f(U[:, :K] * 0.1) if K else None
            emit(name, f"project[K={K},P={P}]", eng.project_cells(Ef, Vk, K, X=Xk, log_prior=f(lp), psi_start=ps, const=const, max_iter=3))
            for Q in ((1, 5) if full else (3,)):
                if K > 0:
                    nd, wt = gauss_hermite_rule(K, Q)
                    emit(name, f"evidence[K={K},P={P},Q={Q}]", eng.clone_evidence(Ef, Vk, K, X=Xk, psi_start=ps, nodes=nd, weights=wt, const=const, max_iter=3))
                elif Q == 1 or not full:
                    emit(name, f"evidence[K=0,P={P}]", eng.clone_evidence(Ef, Vk, 0, X=Xk, const=const))
    finally:
        eng.close()


def main():
    print(f"build id {_engine.build_id()}")
    base = dict(N=257, G=130, C=7, D=2)
    run_case("base u8 257x130 C7 D2", **base, full=True)
    for st in ("u16", "f32"):
        run_case(f"storage {st}", **base, storage=st)
    for N, G in ((1, 1), (65, 17), (300, 1025)):
        for st in ("u8", "u16", "f32") if G == 1025 else ("u8",):
            run_case(f"shape {N}x{G} {st}", N=N, G=G, C=min(7, max(G, 2)) if G > 1 else 2, D=2 if G > 1 else 0, storage=st)
    run_case("columns C2 D0", N=257, G=130, C=2, D=0, full=True)
    run_case("columns C12 D8", N=257, G=130, C=12, D=8)
    run_case("columns C28 D8 (two groups)", N=257, G=130, C=28, D=8)
    run_case("with_const 0", **base, const=False, full=True)
    run_case("layout col", **base, layout="col")
    run_case("layout col with_const 0 range", **base, layout="col", const=False, cells=(63, 65))
    run_case("range lo=63 cnt=2", **base, cells=(63, 65), full=True)
    import torch
    if torch.cuda.device_count() >= 2:
        run_case("group of two ranks", **base, devices=[0, 1], full=True)
        run_case("group of two ranks range", **base, devices=[0, 1], cells=(63, 200))
    else:
        print(f"group of two ranks | skipped: {torch.cuda.device_count()} device(s) visible")


if __name__ == "__main__":
    main()
