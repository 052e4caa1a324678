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
The first line is the library's build id; a line "skipped ..." says what this machine or this engine could not run.

Three layers, all by default or the ones named on the command line:
   engine   the six HipEngine methods (the grid above), then the refusals the methods make themselves;
   api      the public functions of clonealign_amd.api on throwaway engines (and once on the caller's engine);
   host     the same functions on an engine object that has only N, G and close: the float64 host forms, no GPU needed.
The api and host layers run clone_loglik, assign_cells, clone_loglik_by_block, assignment_support, clone_pair_loglik, detect_doublets, clone_loglik_dm,
estimate_concentration, assign_cells_dm (a value and "auto"), project_cells, clone_evidence, assign_cells_marginal and heldout_evidence (two fits with
different K) on a base case (257 x 130, C = 7, K = 1, P = 1, alpha, copy numbers above the saturation threshold, L = 0 against a positive count and against
none) and vary one axis at a time; then a fixed list of inputs with exactly one fault each: the call, the exception type and the message.  Two trees whose
Python computes the same print the same lines."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clonealign_amd import api  # noqa: E402
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


def digest(v):
    """One token for any returned value: arrays by their bytes, label arrays and lists by their joined strings, scalars by their repr."""
    if isinstance(v, np.ndarray) and v.dtype == object:
        return f"obj{list(v.shape)} " + hashlib.sha256("\x1f".join(str(e) for e in v.reshape(-1)).encode()).hexdigest()
    if isinstance(v, np.ndarray):
        return sha(v) + (" F" if v.ndim > 1 and v.flags.f_contiguous and not v.flags.c_contiguous else "")
    if isinstance(v, (list, tuple)):
        return f"list[{len(v)}] " + hashlib.sha256("\x1f".join(str(e) for e in v).encode()).hexdigest()
    if isinstance(v, (float, np.floating)):
        return "float " + float(v).hex()
    return f"{type(v).__name__} {v!r}"


def emit_any(case, call, res):
    if isinstance(res, dict):
        for k in sorted(res, key=str):
            emit_any(case, f"{call}.{k}", res[k])
    else:
        print(f"{case} | {call} | {digest(res)}")


def refusal(case, call, thunk):
    try:
        thunk()
        print(f"{case} | {call} | no refusal")
    except Exception as e:  # noqa: BLE001
        print(f"{case} | {call} | {type(e).__name__}: {e}")


class HostOnly:
    """An engine object without a scoring method: every call takes its host form."""

    def __init__(self, N, G):
        self.N, self.G = N, G

    def close(self):
        pass


def model(N=257, G=130, C=7, K=1, P=1, alpha=True, names=False, seed=1):
    """(fit, Y, L, x, extra) of an api case: problem()'s counts; L with values above the saturation threshold, 0 against a positive count and against none."""
    Y, L, _E, U, V, lp = problem(N, G, C, 2, "u8", seed)
    rng = np.random.default_rng(seed + 100)
    L.reshape(-1)[rng.choice(G * C, size=max(1, G * C // 10), replace=False)] = 8.0
    if G >= 17 and C >= 2:
        L[3, 0] = 0.0                                                # (problem() put a count at gene 3 and none at gene 9)
        L[9, 1] = 0.0
    ml = {"mu": rng.lognormal(-1.4, 1.0, G), "clone_probs": np.full((N, C), 1.0 / C)}
    if K:
        ml["W"], ml["psi"] = V[:, :K].copy(), U[:, :K].copy()
    if P:
        ml["beta"] = V[:, 4:4 + P].copy()
    if alpha:
        ml["alpha"] = rng.dirichlet(np.ones(C) * 3.0)
    fit = {"ml_params": ml}
    if names:
        fit["clone_names"] = [f"k{i}" for i in range(C)]
    return fit, Y, L, (U[:, 4:4 + P].copy() if P else None), lp


def other_k(fit):
    """The same fit with another number of factors: K = 0 for a fit with factors, K = 1 for one without."""
    ml = dict(fit["ml_params"])
    if ml.pop("W", None) is None:
        G, N = ml["mu"].shape[0], ml["clone_probs"].shape[0]
        rng = np.random.default_rng(9)
        ml["W"], ml["psi"] = rng.normal(size=(G, 1)) * 0.3, rng.normal(size=(N, 1)) * 0.5
    else:
        ml.pop("psi", None)
    return dict(fit, ml_params=ml)


def calls(fit, Y, L, eng, x=None, psi=None, extra=None, const=True, saturate=True, cells=None, chunk_cells=None, fit2=None):
    """(name, thunk) of every public scoring function on one input."""
    G = L.shape[0]
    blocks = np.array([f"chr{g // 50}" for g in range(G)], dtype=object)
    kw = dict(x=x, saturate=saturate, const=const, engine=eng)
    kp = dict(kw, psi=psi)
    exc = extra if cells is None or extra is None else extra[cells[0]:cells[1]]
    fits = {"a": fit, "b": other_k(fit) if fit2 is None else fit2}
    return [
        ("clone_loglik", lambda: api.clone_loglik(fit, Y, L, **kp)),
        ("assign_cells", lambda: api.assign_cells(fit, Y, L, extra_loglik=extra, **kp)),
        ("clone_loglik_by_block", lambda: api.clone_loglik_by_block(fit, Y, L, blocks, cells=cells, **kp)),
        ("assignment_support", lambda: api.assignment_support(fit, Y, L, blocks, extra_loglik=exc, cells=cells, **kp)),
        ("clone_pair_loglik", lambda: api.clone_pair_loglik(fit, Y, L, weights=(0.3, 0.5), **kp)),
        ("detect_doublets", lambda: api.detect_doublets(fit, Y, L, weights=(0.3, 0.5), extra_loglik=extra, chunk_cells=chunk_cells, **kp)),
        ("clone_loglik_dm", lambda: api.clone_loglik_dm(fit, Y, L, concentration=(5.0, 50.0, 500.0), **kp)),
        ("estimate_concentration", lambda: api.estimate_concentration(fit, Y, L, refine=1, extra_loglik=extra, **kp)),
        ("assign_cells_dm[40]", lambda: api.assign_cells_dm(fit, Y, L, 40.0, extra_loglik=extra, **kp)),
        ("assign_cells_dm[auto]", lambda: api.assign_cells_dm(fit, Y, L, "auto", refine=1, extra_loglik=extra, **kp)),
        ("project_cells", lambda: api.project_cells(fit, Y, L, extra_loglik=extra, max_iter=5, **kw)),
        ("clone_evidence", lambda: api.clone_evidence(fit, Y, L, max_iter=8, **kw)),
        ("assign_cells_marginal", lambda: api.assign_cells_marginal(fit, Y, L, extra_loglik=extra, max_iter=8, **kw)),
        ("heldout_evidence", lambda: api.heldout_evidence(fits, Y, L, extra_loglik=extra, max_iter=8, **kw)),
    ]


def api_case(layer, name, mk, only=None, **kw):
    fit, Y, L, x, _lp = mk
    eng = HostOnly(*Y.shape) if layer == "host" else None
    for call, thunk in calls(fit, Y, L, eng, x=x, **kw):
        if only is None or call in only:
            emit_any(f"{layer} {name}", call, thunk())


RANGE_CALLS = ("clone_loglik_by_block", "assignment_support")
PSI_CALLS = ("clone_loglik", "assign_cells", "clone_loglik_by_block", "assignment_support", "clone_pair_loglik", "detect_doublets", "clone_loglik_dm",
             "estimate_concentration", "assign_cells_dm[40]", "assign_cells_dm[auto]")
EXTRA_CALLS = ("assign_cells", "assignment_support", "detect_doublets", "estimate_concentration", "assign_cells_dm[40]", "assign_cells_dm[auto]",
               "project_cells", "assign_cells_marginal", "heldout_evidence")


def run_api(layer):
    """The public functions: a base case, then one axis at a time."""
    import pandas as pd
    import scipy.sparse as sps
    base = model()
    fit, Y, L, x, lp = base
    api_case(layer, "base 257x130 C7 K1 P1", base)
    api_case(layer, "K0", model(K=0))
    api_case(layer, "65x17 K2 P0", model(N=65, G=17, K=2, P=0))
    api_case(layer, "no alpha", model(alpha=False))
    api_case(layer, "extra_loglik", base, only=EXTRA_CALLS, extra=lp)
    api_case(layer, "no alpha extra_loglik", model(alpha=False), only=EXTRA_CALLS, extra=lp)
    api_case(layer, "const False", base, const=False)
    api_case(layer, "saturate False", base, saturate=False)
    api_case(layer, "psi fit", base, only=PSI_CALLS, psi="fit")
    api_case(layer, "psi array", base, only=PSI_CALLS, psi=fit["ml_params"]["psi"] * 0.5)
    api_case(layer, "cells (63, 65)", base, only=RANGE_CALLS, cells=(63, 65), extra=lp)
    api_case(layer, "chunk_cells 100", base, only=("detect_doublets",), chunk_cells=100, extra=lp)
    api_case(layer, "Y csr", (fit, sps.csr_matrix(Y), L, x, lp))
    api_case(layer, "Y int64", (fit, Y.astype(np.int64), L, x, lp))
    frame = pd.DataFrame(L, columns=[f"col{i}" for i in range(L.shape[1])])
    api_case(layer, "L DataFrame", (fit, Y, frame, x, lp))
    api_case(layer, "L DataFrame clone_names", (dict(fit, clone_names=[f"k{i}" for i in range(L.shape[1])]), Y, frame, x, lp))
    if layer == "api":                                               # the caller's engine: used as it is, for every call
        from clonealign_amd import hostprep
        eng = HipEngine(Y, hostprep.saturate(L, 6), np.zeros((Y.shape[0], 0)), None, 0)
        try:
            for call, thunk in calls(fit, Y, L, eng, x=x, extra=lp):
                emit_any("api caller's engine", call, thunk())
        finally:
            eng.close()
    api_refusals(layer, base)


def api_refusals(layer, base):
    """Inputs with exactly one fault each, through every function the fault can reach."""
    fit, Y, L, x, lp = base
    N, G = Y.shape
    eng = HostOnly(N, G) if layer == "host" else None
    ml = fit["ml_params"]

    def with_ml(**kv):
        return dict(fit, ml_params={k: v for k, v in dict(ml, **kv).items() if v is not None})

    def sweep(label, f=fit, Yv=Y, Lv=L, only=None, **kw):
        kw.setdefault("x", x)
        for call, thunk in calls(f, Yv, Lv, kw.pop("eng", eng), **kw):
            if only is None or call in only:
                refusal(f"{layer} refusal {label}", call, thunk)

    sweep("L with one gene less", Lv=L[:-1])
    sweep("mu of the wrong length", f=with_ml(mu=ml["mu"][:-1]), fit2=fit)
    sweep("x missing", x=None)
    sweep("x without beta", f=with_ml(beta=None), fit2=with_ml(beta=None, W=None, psi=None))
    sweep("psi with the wrong rows", only=PSI_CALLS, psi=ml["psi"][:-1])
    sweep("psi other", only=PSI_CALLS, psi="other")
    sweep("extra_loglik of the wrong shape", only=EXTRA_CALLS, extra=lp[:, :-1])
    refusal(f"{layer} refusal a bad weight", "clone_pair_loglik", lambda: api.clone_pair_loglik(fit, Y, L, weights=(0.3, 1.0), x=x, engine=eng))
    refusal(f"{layer} refusal a bad weight", "detect_doublets", lambda: api.detect_doublets(fit, Y, L, weights=(0.3, 1.0), x=x, engine=eng))
    refusal(f"{layer} refusal 17 concentrations", "clone_loglik_dm",
            lambda: api.clone_loglik_dm(fit, Y, L, concentration=np.geomspace(1.0, 1e4, 17), x=x, engine=eng))
    one = with_ml(alpha=np.ones(1))
    sweep("C = 1", f=one, Lv=L[:, :1], only=("assignment_support", "clone_pair_loglik", "detect_doublets"))
    if layer == "api":
        rng = np.random.default_rng(3)
        k3 = with_ml(W=rng.normal(size=(G, 3)) * 0.3, psi=rng.normal(size=(N, 3)))
        sweep("K = 3 on the device", f=k3, only=("project_cells", "clone_evidence", "assign_cells_marginal"))
        other = HipEngine(Y[:100], L, np.zeros((100, 0)), None, 0)
        try:
            sweep("an engine of another shape", eng=other)
        finally:
            other.close()


def engine_refusals():
    """What the six methods refuse before the library is called."""
    N, G, C = 65, 17, 3
    Y, L, E, U, V, lp = problem(N, G, C, 2, "u8", 1)
    eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0)
    bg = np.zeros(G, dtype=np.int32)
    nd, wt = gauss_hermite_rule(1, 3)
    ll_calls = [("clone_loglik", lambda E_, U_, V_: eng.clone_loglik(E_, U_, V_)),
                ("clone_pair_loglik", lambda E_, U_, V_: eng.clone_pair_loglik(E_, U_, V_)),
                ("clone_loglik_dm", lambda E_, U_, V_: eng.clone_loglik_dm(E_, U_, V_)),
                ("clone_loglik_by_block", lambda E_, U_, V_: eng.clone_loglik_by_block(E_, U_, V_, bg, 1))]
    lat_calls = [("project_cells", lambda E_, V_, K, **kw: eng.project_cells(E_, V_, K, **kw)),
                 ("clone_evidence", lambda E_, V_, K, **kw: eng.clone_evidence(E_, V_, K, **kw))]
    try:
        for name, f in ll_calls:
            refusal("engine refusal E of the wrong shape", name, lambda: f(E[:, :-1], U[:, :2], V[:, :2]))
            refusal("engine refusal U without V", name, lambda: f(E, U[:, :2], None))
            refusal("engine refusal U and V disagree", name, lambda: f(E, U[:, :2], V[:, :3]))
        for name, f in lat_calls:
            refusal("engine refusal E of the wrong shape", name, lambda: f(E[:, :-1], V[:, :1], 1))
            refusal("engine refusal V with fewer than K columns", name, lambda: f(E, V[:, :1], 2))
            refusal("engine refusal X of the wrong shape", name, lambda: f(E, V[:, :2], 1, X=U[:-1, 4:5]))
            refusal("engine refusal psi_start of the wrong shape", name, lambda: f(E, V[:, :1], 1, psi_start=U[:-1, :1]))
            refusal("engine refusal poll_every 0", name, lambda: f(E, V[:, :1], 1, poll_every=0))
        refusal("engine refusal log_prior of the wrong shape", "project_cells", lambda: eng.project_cells(E, V[:, :1], 1, log_prior=lp[:, :-1]))
        refusal("engine refusal nodes without weights", "clone_evidence", lambda: eng.clone_evidence(E, V[:, :1], 1, nodes=nd))
        refusal("engine refusal nodes of the wrong size", "clone_evidence", lambda: eng.clone_evidence(E, V[:, :1], 1, nodes=nd[:-1], weights=wt))
        refusal("engine refusal block_of_gene not integer", "clone_loglik_by_block", lambda: eng.clone_loglik_by_block(E, None, None, bg.astype(np.float64), 1))
    finally:
        eng.close()


def main():
    layers = sys.argv[1:] or ["engine", "api", "host"]
    if "host" in layers:
        run_api("host")
    if "api" in layers:
        print(f"build id {_engine.build_id()}")
        run_api("api")
    if "engine" in layers:
        run_engine()


def run_engine():
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
    engine_refusals()


if __name__ == "__main__":
    main()
