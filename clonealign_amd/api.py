"""User-facing API: ``clonealign()``, ``run_clonealign()``, ``plot_clonealign()`` and the ``clonealign_fit`` object.

Mirrors ``R/clonealign.R`` (exports in NAMESPACE:3-7) argument for argument; the only
compute-heavy callee, ``inference_tflow``, runs on the MI355X engine.
"""
import contextlib
import string
import warnings
from collections import Counter, namedtuple

import numpy as np

from . import hostprep
from .inference import inference_tflow


class ClonealignFit(dict):
    """The ``clonealign_fit`` S3 list (R/clonealign.R:303): a dict with attribute access."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __repr__(self):                                             # print.clonealign_fit, :348-357
        N = len(self["clone"])
        if "mu" not in self["ml_params"]:                            # assign_cells(): cells scored under another fit, no gene parameters
            return (f"A clonealign assignment of {N} cells to {self['ml_params']['clone_probs'].shape[1]} clones under a fitted model\n"
                    "To access clone assignments, call x$clone\n"
                    "To access the per-clone log-likelihoods, call x$clone_loglik\n")
        G = len(self["ml_params"]["mu"])
        C = self["ml_params"]["clone_probs"].shape[1]
        return (f"A clonealign_fit for {N} cells, {G} genes, and {C} clones\n"
                "To access clone assignments, call x$clone\n"
                "To access ML parameter estimates, call x$ml_params\n")

    __str__ = __repr__


def clone_assignment(gamma, clone_names, clone_assignment_probability=0.95):
    """R/inference-tflow.R:22-29: arg-max clone (first maximum) or ``"unassigned"``."""
    gamma = np.asarray(gamma)
    best = gamma.argmax(1)
    mx = gamma.max(1)
    names = np.asarray(list(clone_names), dtype=object)
    out = names[best]
    out[~(mx >= clone_assignment_probability)] = "unassigned"        # (a row of NaN, no clone possible, is unassigned too)
    return out


def recompute_clone_assignment(ca, clone_assignment_probability=0.95):
    """R/inference-tflow.R:36-46."""
    ca = ClonealignFit(ca)
    ca["clone"] = clone_assignment(ca["ml_params"]["clone_probs"], ca["clone_names"],
                                   clone_assignment_probability)
    return ca


def compute_correlations(Y, L, clones, clone_names):
    """R/clonealign.R:318-334: per-gene Pearson correlation of scaled counts vs the
    copy number of the assigned clone (NaN where undefined, like R's NA)."""
    Y = np.asarray(Y, dtype=np.float64)
    L = np.asarray(L, dtype=np.float64)
    clones = np.asarray(clones, dtype=object)
    unassigned = clones == "unassigned"
    Y = Y[~unassigned]
    clones = clones[~unassigned]
    idx = {c: i for i, c in enumerate(clone_names)}
    ci = np.array([idx[c] for c in clones], dtype=np.int64)
    G = Y.shape[1]
    out = np.full(G, np.nan)
    if Y.shape[0] < 2:
        return out
    Ys = hostprep.r_scale(Y)
    X = L[:, ci].T                                                  # [n, G]
    with np.errstate(divide="ignore", invalid="ignore"):
        xc = X - X.mean(0, keepdims=True)
        yc = Ys - Ys.mean(0, keepdims=True)
        num = (xc * yc).sum(0)
        den = np.sqrt((xc ** 2).sum(0) * (yc ** 2).sum(0))
        out = np.where(den > 0, num / den, np.nan)
    return out


def correlations_from_sums(T, Syy, L, clone_counts):
    """Pearson r per gene from the device-side sums (ca_clone_gene_sums): x = copy number of the assigned clone,
    y = counts, over assigned cells.  Equals compute_correlations() (R's scale() does not change r)."""
    T = np.asarray(T, dtype=np.float64)
    L = np.asarray(L, dtype=np.float64)
    nc = np.asarray(clone_counts, dtype=np.float64)
    n = nc.sum()
    out = np.full(T.shape[0], np.nan)
    if n < 2:
        return out
    Sx, Sxx = L @ nc, (L ** 2) @ nc
    Sy, Sxy = T.sum(1), (L * T).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        vx = n * Sxx - Sx ** 2
        vy = n * np.asarray(Syy, dtype=np.float64) - Sy ** 2
        den = np.sqrt(vx * vy)
        r = (n * Sxy - Sx * Sy) / den
    # constant x or y (R: NA with a warning); guard against round-off making a zero variance slightly positive
    ok = (vx > 1e-9 * np.maximum(n * Sxx, 1.0)) & (vy > 1e-9 * np.maximum(n * np.asarray(Syy), 1.0))
    out[ok] = r[ok]
    return out


def _is_sparse(a):
    import scipy.sparse as sps
    return sps.issparse(a)


def _fit_mse_host(Y, E, clone_idx, per_gene=False, chunk=4096):
    """Float64 host form of ``HipEngine.fit_mse`` (R/clonealign.R:429-432), for engines without it: Y [N, G] dense or scipy.sparse (densified
    ``chunk`` cells at a time), E [G, C] the predicted-expression table, ``clone_idx`` in [-1, C) with -1 = skip the cell.  Same return value."""
    E = np.asarray(E, dtype=np.float64)
    idx = np.asarray(clone_idx, dtype=np.int64).reshape(-1)
    N, G = Y.shape
    if E.shape[0] != G or idx.shape[0] != N:
        raise ValueError(f"fit_mse: Y is {N} x {G}, E has {E.shape[0]} rows, clone_idx {idx.shape[0]} entries")
    if idx.size and (idx.min() < -1 or idx.max() >= E.shape[1]):
        raise ValueError(f"fit_mse: clone index outside [-1, {E.shape[1]})")
    esum = E.sum(0)
    used = np.flatnonzero(idx >= 0)
    sse_gene = np.zeros(G)
    for lo in range(0, used.size, int(chunk)):
        rows = used[lo:lo + int(chunk)]
        Yc = Y[rows]
        Yc = np.asarray(Yc.toarray() if _is_sparse(Yc) else Yc, dtype=np.float64)
        a = Yc.sum(1) / esum[idx[rows]]                                  # normalizer, :429
        r = E[:, idx[rows]].T * a[:, None] - Yc                          # :430-432
        sse_gene += (r * r).sum(0)
    sse = float(sse_gene.sum())
    out = {"sse": sse, "n_cells": int(used.size), "mse": sse / (used.size * G) if used.size and G else float("nan")}
    if per_gene:
        out["sse_gene"] = sse_gene
    return out


def _cells_and_cnv(Y, L):
    """(Y, L, cn, N, G) of a call on the cells of ``Y`` and the copy numbers ``L``: the count matrix as the engine uploads it, ``L`` [G, C] parsed, the
    DataFrame's clone names or None; refuses an ``L`` for other genes."""
    L, cn = _parse_cnv(L)
    Y = _counts_array(Y.values if hasattr(Y, "columns") and hasattr(Y, "values") else Y)
    N, G = Y.shape
    if L.shape[0] != G:
        raise ValueError(f"L has {L.shape[0]} rows (genes) but Y has {G} columns (genes)")
    return Y, L, cn, N, G


def _clone_names(fit, cn, C):
    """The clone names of a result: the fit's, else the DataFrame's columns ``cn``, else ``clone_a`` ... ``clone_z``, ``clone_27`` ... (numbered beyond the
    26 letters, as ``_default_gene_names`` numbers genes)."""
    if "clone_names" in fit:
        return list(fit["clone_names"])
    lt = string.ascii_lowercase
    return cn if cn is not None else [f"clone_{lt[i]}" if i < 26 else f"clone_{i + 1}" for i in range(C)]


@contextlib.contextmanager
def _engine_lease(engine, method, Y, L, engine_opts):
    """The engine of a call on the resident matrix ``Y``: the caller's, used as it is and never closed, or a throwaway one built for the upload only
    (``K = 0``; ``engine_opts`` go to its constructor) and closed on every way out.  An engine that has ``method`` must hold a matrix of ``Y``'s shape."""
    N, G = Y.shape
    own = engine is None
    if own:
        from .engine import HipEngine
        engine = HipEngine(Y, L, np.zeros((N, 0)), None, 0, **(engine_opts or {}))
    try:
        if hasattr(engine, method) and (engine.N, engine.G) != (N, G):
            raise ValueError(f"the engine holds a {engine.N} x {engine.G} matrix but Y is {N} x {G}")
        yield engine
    finally:
        if own:
            engine.close()


def compute_ca_fit_mse(fit, Y, L, model_mu=False, random_clones=False, *, seed=None, drop_unassigned=False, per_gene=False,
                       engine=None, engine_opts=None):
    """Mean squared error of a clonealign fit on expression data under given clones, R/clonealign.R:415-434 (first five arguments as there):
    ``mean((t(L[, clones]) * rowSums(Y) / colSums(L[, clones]) - Y)^2)``, with ``mu * L`` in place of ``L`` when ``model_mu``.

    ``Y`` [cells, genes]: a dense array in any dtype the engine uploads, or a scipy.sparse matrix; it is evaluated on the device in one sweep
    (``HipEngine.fit_mse``) and never densified or copied as float64 on the host.  ``engine``: a live engine whose resident matrix is ``Y`` (used as
    it is); without it a throwaway engine is built for the upload and the fit constants only (``K=0``; ``engine_opts`` go to its constructor) and
    closed afterwards.  An engine without ``fit_mse`` gets the float64 host form.
    ``random_clones`` draws one label per cell, with replacement, from the distinct labels present, through ``numpy.random.default_rng(seed)``: the
    reference uses R's ``sample()``, whose stream cannot be reproduced here, so the labels (not their distribution) differ from R's under any seed.
    Cells labelled "unassigned": the reference fails on ``L[, "unassigned"]`` and so does this (ValueError) unless ``drop_unassigned=True``, which
    skips them and takes the mean over the cells that are left.
    Returns the MSE; with ``per_gene=True`` ``(mse, mse_gene[G])``, the same mean per gene."""
    Y, L, cn, N, G = _cells_and_cnv(Y, L)
    names = _clone_names(fit, cn, L.shape[1])
    if len(names) != L.shape[1]:
        raise ValueError(f"fit has {len(names)} clone names but L has {L.shape[1]} columns (clones)")
    clones = np.asarray(fit["clone"], dtype=object).reshape(-1)
    if random_clones:
        distinct = list(dict.fromkeys(clones.tolist()))              # unique(), in order of first appearance (:420)
        clones = np.asarray(distinct, dtype=object)[np.random.default_rng(seed).integers(0, len(distinct), size=N)]   # :421
    if clones.shape[0] != N:
        raise ValueError(f"fit has {clones.shape[0]} clone labels but Y has {N} rows (cells)")
    lut = {c: i for i, c in enumerate(names)}
    unknown = sorted({str(c) for c in clones if c not in lut and c != "unassigned"})
    if unknown:
        raise ValueError("clone labels that are no column of L: " + ", ".join(unknown))          # subscript out of bounds, :423
    idx = np.array([lut.get(c, -1) for c in clones], dtype=np.int32)
    if np.any(idx < 0) and not drop_unassigned:
        raise ValueError(f"{int((idx < 0).sum())} cells are \"unassigned\", which is no column of L (the reference fails at L[, clones]); "
                         "pass drop_unassigned=True to take the mean over the assigned cells")
    E = L
    if model_mu:
        mu = np.asarray(fit["ml_params"]["mu"], dtype=np.float64).reshape(-1)                  # :426-427
        if mu.shape[0] != G:
            raise ValueError(f"fit$ml_params$mu has length {mu.shape[0]} but L has {G} rows: evaluate on the retained genes")
        E = mu[:, None] * L
    with _engine_lease(engine, "fit_mse", Y, L, engine_opts) as eng:
        out = eng.fit_mse(idx, E, per_gene=per_gene) if hasattr(eng, "fit_mse") else _fit_mse_host(Y, E, idx, per_gene=per_gene)
    if per_gene:
        return out["mse"], (out["sse_gene"] / out["n_cells"] if out["n_cells"] else np.full(G, np.nan))
    return out["mse"]


def _ll_inputs(Y, E, U, V, what):
    """(E, U, V, D, esum) of a log-likelihood host form as float64 after the refusals the library makes (ValueError names the offender)."""
    E = np.asarray(E, dtype=np.float64)
    N, G = Y.shape
    if E.ndim != 2 or E.shape[0] != G:
        raise ValueError(f"{what}: Y is {N} x {G} but E is {E.shape}")
    D = 0
    if (U is None) != (V is None):
        raise ValueError(f"{what}: U and V go together (both, or neither)")
    if U is not None:
        U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
        if U.ndim != 2 or V.ndim != 2 or U.shape[0] != N or V.shape[0] != G or U.shape[1] != V.shape[1]:
            raise ValueError(f"{what}: U is {U.shape} and V is {V.shape}; expected ({N}, D) and ({G}, D)")
        D = U.shape[1]
    if D > 8:
        raise ValueError(f"{what}: D = {D} is outside [0, 8]")
    wrong = np.argwhere(~np.isfinite(E) | (E < 0))
    if wrong.size:
        raise ValueError(f"{what}: expected expression has a negative or non-finite entry (gene {wrong[0][0]}, clone {wrong[0][1]})")
    esum = E.sum(0)
    wrong = np.flatnonzero(~np.isfinite(esum) | (esum == 0))
    if wrong.size:
        raise ValueError(f"{what}: expected expression of clone {wrong[0]} sums to {esum[wrong[0]]} over the genes")
    for name, M, row in (("V", V, "gene"), ("U", U, "cell")):
        if D > 0 and not np.isfinite(M).all():
            r, d = np.argwhere(~np.isfinite(M))[0]
            raise ValueError(f"{what}: {name} has a non-finite entry ({row} {r}, factor {d})")
    return E, U, V, D, esum


def _cell_chunks(Y, chunk, E=None, U=None, V=None, order=None):
    """The cell walk of the host forms: yields ``(lo, Yc, eta, m, logz)`` per ``chunk`` cells of Y [N, G] dense or scipy.sparse, from cell ``lo`` on.
    ``Yc``: the chunk densified to float64 (in memory order ``order`` when given).  With ``U`` [N, D], D > 0: the exponent ``eta = U V^T`` [n, G] and,
    when ``E`` is given too, its largest value per cell ``m`` [n] and the whole-gene ``logz = m + log(exp(eta - m) @ E)`` [n, C]; None otherwise."""
    for lo in range(0, Y.shape[0], int(chunk)):
        Yc = Y[lo:lo + int(chunk)]
        Yc = np.asarray(Yc.toarray() if _is_sparse(Yc) else Yc, dtype=np.float64, order=order)
        eta = m = logz = None
        if U is not None:
            eta = U[lo:lo + int(chunk)] @ V.T
            if E is not None:
                m = eta.max(1)
                logz = m[:, None] + np.log(np.exp(eta - m[:, None]) @ E)
        yield lo, Yc, eta, m, logz


def _clone_loglik_host(Y, E, U=None, V=None, const=True, chunk=2048):
    """Float64 host form of ``HipEngine.clone_loglik`` for engines without it: Y [N, G] dense or scipy.sparse (densified ``chunk`` cells at a time), E
    [G, C], U [N, D] and V [G, D] or both None.  Same return value, same rules (xlogy, the shift by the largest exponent), same refusals (ValueError)."""
    from scipy.special import gammaln
    E, U, V, D, esum = _ll_inputs(Y, E, U, V, "clone_loglik")
    N, C = Y.shape[0], E.shape[1]
    zero = E == 0
    logE = np.log(np.where(zero, 1.0, E))                            # xlogy: 0 where E = 0, put right below
    ll = np.empty((N, C))
    for lo, Yc, eta, _m, logz in _cell_chunks(Y, chunk, E, U if D > 0 else None, V):
        s = Yc.sum(1)
        a = Yc @ logE
        if zero.any():
            a[((Yc > 0).astype(np.float64) @ zero.astype(np.float64)) > 0] = -np.inf
        if D > 0:
            a += (Yc * eta).sum(1)[:, None]
        else:
            logz = np.log(esum)[None, :]
        a -= np.where(s[:, None] > 0, s[:, None] * logz, 0.0)
        if const:
            a += (gammaln(s + 1.0) - gammaln(Yc + 1.0).sum(1))[:, None]
        ll[lo:lo + int(chunk)] = a
    return ll


_FitTables = namedtuple("_FitTables", "L E U V W beta K P x")


def _fit_tables(fit, L, N, x, psi, saturate, saturation_threshold, what="Y", free_psi=False):
    """The model tables of a fit for ``N`` cells, shared by the scoring calls and ``simulate_counts``: ``L`` [G, C] (parsed) saturated as asked,
    ``E = mu * L`` [G, C], ``U = [psi | x]`` [N, D] and ``V = [W | beta]`` [G, D] (both None when no exponent term is in play), and the pieces: ``W``
    [G, K], ``beta`` [G, P] and the checked ``x`` [N, P] (None without ``beta``).  ``psi``: None (the ``W`` term drops out), ``"fit"`` or an array
    [N, K]; ``x`` exactly when the fit has ``beta``.  ``what`` names the cells' owner in the refusals.  ``free_psi``: the call solves for ``psi``
    itself, so ``W``'s columns count towards the 8 exponent factors although no ``psi`` is given."""
    G = L.shape[0]
    ml = fit["ml_params"]
    mu = np.asarray(ml["mu"], dtype=np.float64).reshape(-1)
    if mu.shape[0] != G:
        raise ValueError(f"fit$ml_params$mu has length {mu.shape[0]} but L has {G} rows: evaluate on the retained genes")
    if "clone_names" in fit and len(fit["clone_names"]) != L.shape[1]:
        raise ValueError(f"fit has {len(fit['clone_names'])} clone names but L has {L.shape[1]} columns (clones)")
    if saturate:
        L = hostprep.saturate(L, saturation_threshold)               # :142-144
    E = mu[:, None] * L
    W = np.asarray(ml["W"], dtype=np.float64).reshape(G, -1) if ml.get("W") is not None else np.zeros((G, 0))
    beta = np.asarray(ml["beta"], dtype=np.float64).reshape(G, -1) if ml.get("beta") is not None else np.zeros((G, 0))
    K, P = W.shape[1], beta.shape[1]
    if (P > 0) != (x is not None):
        raise ValueError(f"x is required exactly when the fit has beta: the fit has {P} covariates and x is {'missing' if x is None else 'given'}")
    Ucols, Vcols = [], []
    if K > 0 and psi is not None:
        if isinstance(psi, str):
            if psi != "fit":
                raise ValueError("psi must be None (new cells: the prior mean 0), \"fit\" (the fit's own cells) or an array [cells, K]")
            psi = ml["psi"]
        psi = np.asarray(psi, dtype=np.float64)
        if psi.size != N * K or psi.reshape(-1, K).shape[0] != N:
            raise ValueError(f"psi has {psi.reshape(-1, K).shape[0] if psi.size % K == 0 else psi.size} rows (cells) but {what} has {N}")
        Ucols.append(psi.reshape(N, K))
        Vcols.append(W)
    if P > 0:
        x = np.asarray(x, dtype=np.float64)
        x = x.reshape(-1, 1) if x.ndim == 1 else x
        if x.shape != (N, P):
            raise ValueError(f"x is {x.shape} but {what} has {N} rows (cells) and the fit {P} covariates")
        Ucols.append(x)
        Vcols.append(beta)
    U = np.concatenate(Ucols, axis=1) if Ucols else None
    V = np.concatenate(Vcols, axis=1) if Vcols else None
    D = (0 if U is None else U.shape[1]) + (K if free_psi else 0)
    if D > 8:
        raise ValueError(f"the fit has {D} exponent factors (K + P); at most 8 are supported")
    return _FitTables(L, E, U, V, W, beta, K, P, x if P > 0 else None)


def clone_loglik(fit, Y, L, *, x=None, psi=None, saturate=True, saturation_threshold=6, const=True, engine=None, engine_opts=None):
    """Log-likelihood ``ll`` [cells, clones] of the cells of ``Y`` under every clone of a fitted model, taken at the fit's point estimates: the
    reference's ``p_y_on_c`` (R/inference-tflow.R:288-296) with the draw of ``mu`` replaced by ``fit["ml_params"]["mu"]``, i.e.
    ``Multinomial(total = s_n, probs ~ mu * L[:, c] * exp(psi_n W^T + x_n beta^T)).log_prob(y_n)``.  The cells need not be the ones the fit saw.

    ``Y`` [cells, genes]: a dense array in any dtype the engine uploads, or a scipy.sparse matrix; it is evaluated on the device in one float64 sweep
    (``HipEngine.clone_loglik``) and never densified or copied as float64 on the host.  ``L`` [genes, clones] is given for the fit's retained genes and
    saturated as ``inference_tflow`` does by default (:142-144); ``saturate=False`` is for fits made that way.
    ``psi``, for fits with ``K > 0`` (the default ``clonealign()`` fit has ``K = 1``): ``None`` means the cells are NEW -- their ``psi`` is taken at its
    prior mean 0 (:318), so the ``W`` term drops out; ``"fit"`` takes ``fit["ml_params"]["psi"]`` (the cells are the fit's own, in its order); an array
    [cells, K] is used as given.  ``x`` [cells, P]: the covariates, required exactly when the fit has ``beta``.
    ``const=False`` leaves out the clone-independent ``lgamma(s + 1) - sum(lgamma(y + 1))``.
    ``engine``: a live engine whose resident matrix is ``Y`` (used as it is); without it a throwaway engine is built for the upload only (``K=0``;
    ``engine_opts`` go to its constructor) and closed afterwards.  An engine without ``clone_loglik`` gets the chunked float64 host form.
    A positive count on a gene where a clone has copy number 0 makes that entry exactly ``-inf``; a zero count there adds nothing."""
    Y, L, _cn, N, _G = _cells_and_cnv(Y, L)
    t = _fit_tables(fit, L, N, x, psi, saturate, saturation_threshold)
    with _engine_lease(engine, "clone_loglik", Y, t.L, engine_opts) as eng:
        if hasattr(eng, "clone_loglik"):
            return eng.clone_loglik(t.E, t.U, t.V, const=const)
        return _clone_loglik_host(Y, t.E, t.U, t.V, const=const)


def assign_cells(fit, Y, L, clone_assignment_probability=0.95, *, extra_loglik=None, x=None, psi=None, saturate=True, saturation_threshold=6,
                 const=True, engine=None, engine_opts=None):
    """Assign the cells of ``Y`` to the clones of a fitted model without refitting: ``clone_probs = softmax_c(ll + log alpha + extra_loglik)`` with
    ``ll = clone_loglik(fit, Y, L, ...)`` (same keywords), the exact optimum of ``q(z)`` given the fit's other parameters
    (R/inference-tflow.R:308,322,333).  ``extra_loglik`` [cells, clones]: an addend such as the allele-specific term.

    Returns a :class:`ClonealignFit` with ``clone_probs`` [cells, clones], ``clone`` (through ``clone_assignment`` at
    ``clone_assignment_probability``), ``loglik`` [cells] (the logsumexp of the same sum: the cell's marginal log-likelihood), ``clone_loglik``
    [cells, clones] and ``clone_names``; ``recompute_clone_assignment`` works on it.  A cell whose ``ll`` is ``-inf`` in every clone gets NaN
    probabilities and the label "unassigned"; ``-inf`` in some clones gives probability 0 there."""
    ll = clone_loglik(fit, Y, L, x=x, psi=psi, saturate=saturate, saturation_threshold=saturation_threshold, const=const, engine=engine,
                      engine_opts=engine_opts)
    return _assign_from_loglik(fit, ll, L, extra_loglik, clone_assignment_probability)


def _prior_terms(fit, extra_loglik, N, C):
    """The addends of the clone posterior next to the log-likelihood, for the caller to add in its own order: ``(log alpha [1, C] or None when the fit
    has no alpha, extra_loglik [N, C] as float64 or None)``; refuses an ``extra_loglik`` of another shape."""
    alpha = fit["ml_params"].get("alpha")
    with np.errstate(divide="ignore"):
        la = None if alpha is None else np.log(np.asarray(alpha, dtype=np.float64).reshape(1, C))   # :308
    ex = None if extra_loglik is None else np.asarray(extra_loglik, dtype=np.float64)
    if ex is not None and ex.shape != (N, C):
        raise ValueError(f"extra_loglik is {ex.shape} but the log-likelihood is {N} x {C}")
    return la, ex


def _log_prior(fit, extra_loglik, N, C):
    """The [N, C] (or [1, C]) addend ``log alpha + extra_loglik`` of the clone posterior, formed before it meets the log-likelihood."""
    la, ex = _prior_terms(fit, extra_loglik, N, C)
    lp = np.zeros((1, C)) if la is None else la
    with np.errstate(invalid="ignore"):
        return lp if ex is None else lp + ex


def _lse_clones(t):
    """logsumexp over axis 1 of ``t`` [N, C, ...]; ``-inf`` where every clone is (no NaN)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        m = t.max(1)
        return np.where(np.isneginf(m), -np.inf, m + np.log(np.exp(t - np.where(np.isneginf(m), 0.0, m)[:, None]).sum(1)))


def _assign_from_loglik(fit, ll, L, extra_loglik, clone_assignment_probability):
    """``assign_cells``' result from the log-likelihood ``ll`` [cells, clones]: the sum is formed as ``(ll + log alpha) + extra_loglik``, and the
    logsumexp is its own -- a row of ``-inf`` is to give NaN probabilities."""
    N, C = ll.shape
    names = _clone_names(fit, _parse_cnv(L)[1], C)
    la, ex = _prior_terms(fit, extra_loglik, N, C)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ll + (0.0 if la is None else la)
        if ex is not None:
            t = t + ex
        m = t.max(1, keepdims=True)
        lse = m + np.log(np.exp(t - m).sum(1, keepdims=True))        # (a row of -inf: NaN - no clone is possible)
        probs = np.exp(t - lse)
    loglik = np.where(np.isneginf(m[:, 0]), -np.inf, lse[:, 0])
    return ClonealignFit(clone_probs=probs, clone=clone_assignment(probs, names, clone_assignment_probability), loglik=loglik, clone_loglik=ll,
                         clone_names=names, ml_params={"clone_probs": probs})


def _block_labels(blocks, G):
    """(block_names, block_of_gene [G] int32) of a length-G sequence of labels (chromosome names, segment ids): blocks in order of first appearance;
    ``None`` / NaN labels form a last block ``"NA"``."""
    labels = list(blocks.tolist() if hasattr(blocks, "tolist") else blocks)
    if len(labels) != G:
        raise ValueError(f"blocks has {len(labels)} labels but there are {G} genes")
    index, names, missing = {}, [], []
    bg = np.empty(G, dtype=np.int32)
    for g, v in enumerate(labels):
        if v is None or (isinstance(v, (float, np.floating)) and np.isnan(v)):
            missing.append(g)
            continue
        if v not in index:
            index[v] = len(names)
            names.append(v)
        bg[g] = index[v]
    if missing:
        bg[missing] = len(names)
        names.append("NA")
    return names, bg


def _clone_loglik_by_block_host(Y, E, U, V, block_of_gene, n_blocks, const=True, chunk=2048):
    """Float64 host form of ``HipEngine.clone_loglik_by_block`` for engines without it: Y [N, G] dense or scipy.sparse (densified ``chunk`` cells at a time),
    E [G, C], U [N, D] and V [G, D] or both None, ``block_of_gene`` [G] in ``[0, n_blocks)``.  Same return value (``{"A" [N, B, C], "logZ" [N, B, C],
    "s" [N, B], "lg" [N, B] or None}``), same rules (xlogy, the shift by the block's largest exponent, an empty block gives 0, 0, 0 and ``-inf``), same
    refusals (ValueError)."""
    from scipy.special import gammaln
    what = "clone_loglik_by_block"
    E, U, V, D, _esum = _ll_inputs(Y, E, U, V, what)
    N, G = Y.shape
    C, B = E.shape[1], int(n_blocks)
    if B < 1:
        raise ValueError(f"{what}: n_blocks = {B} is below 1")
    bg = np.asarray(block_of_gene).reshape(-1)
    if bg.shape[0] != G:
        raise ValueError(f"{what}: block_of_gene has {bg.shape[0]} labels but there are {G} genes")
    wrong = np.flatnonzero((bg < 0) | (bg >= B))
    if wrong.size:
        raise ValueError(f"{what}: block_of_gene[{wrong[0]}] = {bg[wrong[0]]} is outside [0, {B})")
    genes = [np.flatnonzero(bg == b) for b in range(B)]              # (ascending within a block)
    zero = E == 0
    logE = np.log(np.where(zero, 1.0, E))                            # xlogy: 0 where E = 0, put right below
    A, logZ = np.zeros((N, B, C)), np.full((N, B, C), -np.inf)
    s, lg = np.zeros((N, B)), (np.zeros((N, B)) if const else None)
    for lo, Yc, eta, _m, _logz in _cell_chunks(Y, chunk, None, U if D > 0 else None, V):
        hi = lo + Yc.shape[0]
        for b, idx in enumerate(genes):
            if idx.size == 0:
                continue
            Yb = Yc[:, idx]
            a = Yb @ logE[idx]
            if zero[idx].any():
                a[((Yb > 0).astype(np.float64) @ zero[idx].astype(np.float64)) > 0] = -np.inf
            with np.errstate(divide="ignore"):
                if D > 0:
                    eb = eta[:, idx]
                    m = eb.max(1)
                    logZ[lo:hi, b] = m[:, None] + np.log(np.exp(eb - m[:, None]) @ E[idx])
                    a += (Yb * eb).sum(1)[:, None]
                else:
                    logZ[lo:hi, b] = np.log(E[idx].sum(0))[None, :]
            A[lo:hi, b] = a
            s[lo:hi, b] = Yb.sum(1)
            if const:
                lg[lo:hi, b] = gammaln(Yb + 1.0).sum(1)
    return {"A": A, "logZ": logZ, "s": s, "lg": lg}


def _excluding_each(x, axis, op, empty):
    """``op`` over all entries of ``axis`` but one, for every one left out, by a prefix and a suffix scan: no difference ``total - x`` is ever formed."""
    x = np.moveaxis(x, axis, 0)
    pre, suf = np.full_like(x, empty), np.full_like(x, empty)
    for b in range(1, x.shape[0]):
        pre[b] = op(pre[b - 1], x[b - 1])
        suf[-1 - b] = op(suf[-b], x[-b])
    return np.moveaxis(op(pre, suf), 0, axis)


def _by_block_terms(A, logZ, s, lg):
    """``within`` [n, B, C], ``between`` [n, C], ``without`` [n, B, C] and ``clone_loglik`` [n, C] from the four sufficient statistics per (cell, block)
    (``lg`` None: without the multinomial coefficients).  ``s * logZ`` with ``s = 0`` is 0 even where ``logZ = -inf``; where ``A = -inf`` (a positive
    count against ``E = 0``) the result is ``-inf`` whatever ``logZ`` is, so no ``inf - inf`` is formed; the sums and logsumexps over the other blocks
    come from prefix / suffix scans, O(n B C)."""
    from scipy.special import gammaln
    sb = s[:, :, None]

    def times(cnt, lz):                                              # cnt * lz, 0 where cnt = 0
        return np.where(cnt > 0, cnt * np.where(cnt > 0, lz, 0.0), 0.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        within = np.where(np.isneginf(A), -np.inf, A - times(sb, np.where(np.isneginf(A), 0.0, logZ)))
        lz_all = np.logaddexp.reduce(logZ, axis=1)                   # [n, C]
        st = s.sum(1)
        between = times(sb, logZ - lz_all[:, None, :]).sum(1)
        a_wo = _excluding_each(A, 1, np.add, 0.0)
        s_wo = _excluding_each(s, 1, np.add, 0.0)[:, :, None]
        lz_wo = _excluding_each(logZ, 1, np.logaddexp, -np.inf)
        without = np.where(np.isneginf(a_wo), -np.inf, a_wo - times(s_wo, np.where(np.isneginf(a_wo), 0.0, lz_wo)))
        if lg is not None:
            within = within + (gammaln(s + 1.0) - lg)[:, :, None]
            between = between + (gammaln(st + 1.0) - gammaln(s + 1.0).sum(1))[:, None]
            without = without + (gammaln(s_wo[:, :, 0] + 1.0) - _excluding_each(lg, 1, np.add, 0.0))[:, :, None]
    return {"within": within, "between": between, "without": without, "clone_loglik": within.sum(1) + between}


def _by_block_call(engine, Y, t, bg, B, const, cells):
    """The result dict of ``clone_loglik_by_block`` under the tables ``t`` but for the names: through the engine's method, or through the host form when it
    has none."""
    lo, hi = (0, Y.shape[0]) if cells is None else (int(cells[0]), int(cells[1]))
    if hasattr(engine, "clone_loglik_by_block"):
        st = engine.clone_loglik_by_block(t.E, t.U, t.V, bg, B, const=const, cells=(lo, hi))
    else:
        if not 0 <= lo <= hi <= Y.shape[0]:
            raise ValueError(f"clone_loglik_by_block: the cell range [{lo}, {hi}) is outside [0, {Y.shape[0]}]")
        st = _clone_loglik_by_block_host(Y[lo:hi], t.E, None if t.U is None else t.U[lo:hi], t.V, bg, B, const=const)
    out = _by_block_terms(st["A"], st["logZ"], st["s"], st["lg"])
    out["counts"] = st["s"]
    return out


def clone_loglik_by_block(fit, Y, L, blocks, *, x=None, psi=None, saturate=True, saturation_threshold=6, const=True, cells=None, engine=None,
                          engine_opts=None):
    """WHICH PART OF THE GENOME carries a cell's likelihood: ``clone_loglik`` split exactly over a partition of the genes into blocks (chromosomes, arms,
    copy-number segments).  The multinomial factorises as ``ll[n][c] = sum_b within[n][b][c] + between[n][c]``: ``within`` is the conditional multinomial
    of block b's counts given their total ("what block b alone says"), ``between`` the multinomial of the block totals ("how the cell's reads are split
    between blocks"); ``without[n][b][c]`` is the log-likelihood of the cell with block b's genes deleted -- again a multinomial, over the remaining genes.
    Everything comes from ONE sweep over the resident matrix (``HipEngine.clone_loglik_by_block``; include/clonealign_hip.h has the four sums it returns),
    not from one engine per block.

    ``blocks``: a length-G sequence of labels; block order is order of first appearance, ``None`` / NaN labels form a last block ``"NA"``.  Any
    labelling is legal; one whose genes are not sorted by block is only slower.  ``cells`` = ``(lo, hi)`` restricts the call to that range of cells.
    Every other keyword as for ``clone_loglik``, with the same refusals and the same throwaway-engine rule; an engine without the method gets the chunked
    float64 host form.

    Returns a dict: ``block_names`` [B], ``counts`` [n, B] (reads per block), ``within`` [n, B, C] (0 where the cell has no reads in b), ``between``
    [n, C], ``without`` [n, B, C], ``clone_loglik`` [n, C] (``sum_b within + between``: ``clone_loglik``'s value up to rounding).  ``-inf`` exactly where a
    positive count meets copy number 0 among the genes that enter; no NaN."""
    Y, L, _cn, N, G = _cells_and_cnv(Y, L)
    block_names, bg = _block_labels(blocks, G)
    t = _fit_tables(fit, L, N, x, psi, saturate, saturation_threshold)
    with _engine_lease(engine, "clone_loglik_by_block", Y, t.L, engine_opts) as eng:
        out = _by_block_call(eng, Y, t, bg, len(block_names), const, cells)
    out["block_names"] = block_names
    return out


def _margin(t, cstar):
    """``t[..., c*] - max_{c != c*} t[..., c]`` along the last axis (``cstar`` [n] indexes the first): ``+inf`` where every rival is ``-inf``, NaN where
    ``c*`` is too."""
    idx = cstar.reshape((-1,) + (1,) * (t.ndim - 1))
    own = np.take_along_axis(t, np.broadcast_to(idx, t.shape[:-1] + (1,)), axis=-1)[..., 0]
    rivals = np.where(np.arange(t.shape[-1]) == idx, -np.inf, t)
    with np.errstate(invalid="ignore"):
        return own - rivals.max(-1)


def assignment_support(fit, Y, L, blocks, clone_assignment_probability=0.95, *, extra_loglik=None, x=None, psi=None, saturate=True, saturation_threshold=6,
                       const=True, cells=None, engine=None, engine_opts=None):
    """``assign_cells`` with the evidence behind every call, by block of genes: does a call rest on one amplified segment, or is it supported by every
    segment where the clones differ?  ``blocks`` as for ``clone_loglik_by_block``, every other argument as for ``assign_cells`` (``cells`` = ``(lo, hi)``
    restricts both to that range; ``extra_loglik`` then has the range's rows).  One upload: a throwaway engine serves both sweeps.

    Returns a :class:`ClonealignFit` that holds everything ``assign_cells`` returns, identically (``clone_probs``, ``clone``, ``loglik``,
    ``clone_loglik``, ``clone_names``), plus, with ``t = ll + log alpha + extra_loglik`` and ``c*`` its argmax on the full data:
    ``block_names`` [B]; ``probs_without`` [n, B, C] and ``clone_without`` [n, B]: posterior and label with block b left out; ``margin`` [n]:
    ``t[c*] - max_{c != c*} t[c]``, the log odds of the call against its best rival; ``margin_without`` [n, B]: the same odds, still for ``c*``, with block
    b left out -- negative means the call flips without b; ``margin_within`` [n, B]: the same difference of block b's ``within`` term alone (the evidence
    of b's genes given their total; no prior enters); ``n_flips`` [B]: cells whose argmax changes without b.  Rivals all ``-inf`` give ``+inf``; a cell
    with every clone ``-inf`` gets NaN margins and is "unassigned".  ``C < 2`` is a ValueError."""
    Y, Lm, _cn, N, G = _cells_and_cnv(Y, L)
    block_names, bg = _block_labels(blocks, G)
    ft = _fit_tables(fit, Lm, N, x, psi, saturate, saturation_threshold)
    C = Lm.shape[1]
    if C < 2:
        raise ValueError(f"assignment_support: C = {C} clones: a margin needs at least 2")
    lo, hi = (0, N) if cells is None else (int(cells[0]), int(cells[1]))
    with _engine_lease(engine, "clone_loglik_by_block", Y, ft.L, engine_opts) as eng:
        by = _by_block_call(eng, Y, ft, bg, len(block_names), const, (lo, hi))
        if hasattr(eng, "clone_loglik"):
            ll = eng.clone_loglik(ft.E, ft.U, ft.V, const=const)[lo:hi]
        else:
            ll = _clone_loglik_host(Y[lo:hi], ft.E, None if ft.U is None else ft.U[lo:hi], ft.V, const=const)
    n = ll.shape[0]
    base = _assign_from_loglik(fit, ll, ft.L, extra_loglik, clone_assignment_probability)   # (the parsed L: a DataFrame's column names do not name the clones here)
    names = base["clone_names"]
    prior = np.zeros((n, C)) + _log_prior(fit, extra_loglik, n, C)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ll + prior
        cstar = np.argmax(np.where(np.isnan(t), -np.inf, t), axis=1)
        tw = by["without"] + prior[:, None, :]
        m = tw.max(2, keepdims=True)
        probs_without = np.exp(tw - (m + np.log(np.exp(tw - m).sum(2, keepdims=True))))   # (a row of -inf: NaN, as in assign_cells)
    B = len(block_names)
    clone_without = np.stack([clone_assignment(probs_without[:, b], names, clone_assignment_probability) for b in range(B)], axis=1) if B else np.empty((n, 0), dtype=object)
    alive = ~np.isneginf(t.max(1))
    flips = (np.argmax(tw, axis=2) != cstar[:, None]) & alive[:, None] & ~np.isneginf(m[:, :, 0])
    base.update(block_names=block_names, counts=by["counts"], within=by["within"], between=by["between"], without=by["without"],
                probs_without=probs_without, clone_without=clone_without, margin=_margin(t, cstar), margin_without=_margin(tw, cstar),
                margin_within=_margin(by["within"], cstar), n_flips=flips.sum(0).astype(np.int64))
    return base


def bootstrap_gene_weights(G, n_rep, *, seed=0, blocks=None):
    """Gene weights of ``n_rep`` bootstrap replicates, [n_rep, G] float64: how often each gene was drawn when G genes are resampled with replacement
    (a row is ``Multinomial(G, 1/G)`` and sums to G).  With ``blocks`` (a length-G labelling as for ``clone_loglik_by_block``: chromosome arms, copy-number
    segments) WHOLE BLOCKS are drawn with replacement, as many draws as there are blocks, and a gene carries its block's count: the genes of a copy-number
    segment move together and are not independent evidence.  The draws come from the counter-based generator of ``rng`` (``rng.index_draw``), stream =
    replicate, so a replicate's weights depend on ``(seed, replicate)`` alone -- the same bits on every run, and the first rows of a larger ``n_rep``."""
    from . import rng
    G, n_rep = int(G), int(n_rep)
    if G < 1 or n_rep < 0:
        raise ValueError(f"bootstrap_gene_weights: G = {G} and n_rep = {n_rep}; expected G >= 1 and n_rep >= 0")
    if blocks is None:
        B, bg = G, np.arange(G)
    else:
        names, bg = _block_labels(blocks, G)
        B = len(names)
    w = np.empty((n_rep, G), dtype=np.float64)
    for r in range(n_rep):
        w[r] = np.bincount(rng.index_draw(seed, r, B, B), minlength=B).astype(np.float64)[bg]
    return w


def _reweighted_weights(weights, G, what="clone_loglik_reweighted"):
    """The replicate weights of a reweighted call as [R, G] float64 after the library's refusals (ValueError names the offender)."""
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64))
    if w.ndim != 2 or w.shape[1] != G:
        raise ValueError(f"{what}: weights is {w.shape}; expected (R, {G})")
    if w.shape[0] < 1:
        raise ValueError(f"{what}: R = {w.shape[0]} replicates is below 1")
    wrong = np.argwhere(~np.isfinite(w) | (w < 0))
    if wrong.size:
        raise ValueError(f"{what}: the weights have a negative or non-finite entry (replicate {wrong[0][0]}, gene {wrong[0][1]})")
    wrong = np.flatnonzero(~(w > 0).any(1))
    if wrong.size:
        raise ValueError(f"{what}: the weights of replicate {wrong[0]} are all zero (genes 0 .. {G - 1})")
    return w


def _clone_loglik_reweighted_host(Y, E, U, V, weights, log_prior=None, cells=None, want_ll=True, chunk=256, with_scale=False):
    """Float64 host form of ``HipEngine.clone_loglik_reweighted`` for engines without it, and its yardstick: Y [N, G] dense or scipy.sparse (densified
    ``chunk`` cells at a time), E [G, C], U [N, D] and V [G, D] or both None, ``weights`` [R, G], ``log_prior`` [N, C] / [1, C] or None.  Same return value
    and rules: ``ll_r = sum_g w_rg xlogy(y, E) - s_r log sum_g w_rg E exp(eta)`` (no ``sum w y eta``, no lgamma constant: the same for every clone),
    ``-inf`` exactly where a positive count with a positive weight meets ``E = 0``, 0 where ``s_r = 0``, no NaN; ``votes`` by ``np.argmax`` of
    ``ll_r + log_prior``; a replicate with every clone at ``-inf`` adds nothing to ``prob_sum`` / ``prob_sq``.  ``with_scale``: also ``"scale"``
    [n, R, C], the sum of the terms' magnitudes (the tests' bar)."""
    E, U, V, D, _esum = _ll_inputs(Y, E, U, V, "clone_loglik_reweighted")
    N, G = Y.shape
    C = E.shape[1]
    W = _reweighted_weights(weights, G)
    R = W.shape[0]
    lo0, hi0 = (0, N) if cells is None else (int(cells[0]), int(cells[1]))
    if lo0 < 0 or hi0 < lo0 or hi0 > N:
        raise ValueError(f"clone_loglik_reweighted: the cell range [{lo0}, {lo0} + {hi0 - lo0}) is outside [0, {N}]")
    n = hi0 - lo0
    lp = None if log_prior is None else np.broadcast_to(np.asarray(log_prior, dtype=np.float64), (N, C))
    if lp is not None and (np.isnan(lp) | (lp == np.inf)).any():
        r, c = np.argwhere(np.isnan(lp) | (lp == np.inf))[0]
        raise ValueError(f"clone_loglik_reweighted: log_prior has a NaN or +inf entry (cell {r}, clone {c}); -inf excludes a clone")
    zero = E == 0
    logE = np.log(np.where(zero, 1.0, E))
    B1 = (W.T[:, :, None] * logE[:, None, :]).reshape(G, R * C)
    Bz = ((W.T > 0)[:, :, None] & zero[:, None, :]).astype(np.float64).reshape(G, R * C)
    B2 = (W.T[:, :, None] * E[:, None, :]).reshape(G, R * C)
    with np.errstate(divide="ignore"):
        logz0 = np.log(W @ E)[None]                                    # D = 0: [1, R, C]
    out = {"votes": np.zeros((n, C), dtype=np.int32), "prob_sum": np.zeros((n, C)), "prob_sq": np.zeros((n, C)), "reads": np.empty((n, R)),
           "ll": np.empty((n, R, C)) if want_ll else None}
    if with_scale:
        out["scale"] = np.empty((n, R, C))
    Ys = Y[lo0:hi0]
    Us = None if D == 0 else U[lo0:hi0]
    for lo, Yc, eta, _m, _lz in _cell_chunks(Ys, chunk, None, Us, V):
        k = Yc.shape[0]
        s = Yc @ W.T                                                   # [k, R]
        a = (Yc @ B1).reshape(k, R, C)
        ninf = ((Yc > 0).astype(np.float64) @ Bz).reshape(k, R, C) > 0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            if D > 0:
                m = eta.max(1)
                logz = m[:, None, None] + np.log((np.exp(eta - m[:, None]) @ B2).reshape(k, R, C))
            else:
                logz = np.broadcast_to(logz0, (k, R, C))
            pos = (s > 0)[:, :, None]
            ll = np.where(ninf, -np.inf, np.where(pos, a - s[:, :, None] * np.where(pos, logz, 0.0), 0.0))
            t = ll if lp is None else ll + lp[lo0 + lo:lo0 + lo + k, None, :]
            mx = t.max(2, keepdims=True)
            alive = ~np.isneginf(mx)
            e = np.where(t == mx, 1.0, np.exp(t - np.where(alive, mx, 0.0)))
            p = np.where(alive, e / e.sum(2, keepdims=True), 0.0)
        best = np.argmax(t, axis=2)                                    # [k, R]
        out["votes"][lo:lo + k] = (best[:, :, None] == np.arange(C)).sum(1)
        out["prob_sum"][lo:lo + k] = p.sum(1)
        out["prob_sq"][lo:lo + k] = (p * p).sum(1)
        out["reads"][lo:lo + k] = s
        if want_ll:
            out["ll"][lo:lo + k] = ll
        if with_scale:
            with np.errstate(invalid="ignore"):
                out["scale"][lo:lo + k] = (Yc @ np.abs(B1)).reshape(k, R, C) + s[:, :, None] * np.where(np.isfinite(logz), np.abs(logz), 0.0)
    return out


def _reweighted_call(engine, Y, t, weights, log_prior, cells, want_ll):
    """The cells ``cells`` under the tables ``t`` through the engine's ``clone_loglik_reweighted``, or through the host form when it has none."""
    if hasattr(engine, "clone_loglik_reweighted"):
        return engine.clone_loglik_reweighted(t.E, t.U, t.V, weights, log_prior=log_prior, cells=cells, want_ll=want_ll)
    return _clone_loglik_reweighted_host(Y, t.E, t.U, t.V, weights, log_prior=log_prior, cells=cells, want_ll=want_ll)


def clone_loglik_reweighted(fit, Y, L, weights, *, x=None, psi=None, saturate=True, saturation_threshold=6, extra_loglik=None, cells=None, want_ll=True,
                            engine=None, engine_opts=None):
    """``clone_loglik`` with the genes REWEIGHTED, for every row of ``weights`` [R, genes] at once (``bootstrap_gene_weights`` makes them): the replicates of
    a bootstrap over genes, all in two float64 matrix products against the resident matrix (``HipEngine.clone_loglik_reweighted``).
    ``ll_r[n, c] = sum_g w_rg xlogy(y_ng, E_gc) - s_r[n] log sum_g w_rg E_gc exp(eta_ng)`` with ``s_r[n] = sum_g w_rg y_ng``: for integer weights
    ``clone_loglik(const=False)`` of the matrix with gene g repeated ``w_rg`` times, minus ``sum_g w_rg y_ng eta_ng`` -- that term and the lgamma constant are
    the same for every clone of a cell and are left out.  ``fit``, ``Y``, ``L``, ``x``, ``psi``, ``saturate``, ``engine`` as for ``clone_loglik``;
    ``extra_loglik`` [cells, clones] (all cells of ``Y``) joins ``log alpha`` in the prior; ``cells`` = ``(lo, hi)`` restricts the call to that range.
    Returns a dict: ``votes`` [n, C] int32 (replicates whose argmax of ``ll_r + log alpha + extra_loglik`` is c), ``prob_sum`` and ``prob_sq`` [n, C]
    (sums over the replicates of the posterior and of its square), ``reads`` [n, R] (``s_r``), ``ll`` [n, R, C] (None unless ``want_ll``).  A positive
    count with a positive weight against copy number 0 gives exactly ``-inf``; ``s_r = 0`` gives ``ll_r = 0``; no NaN.  An engine without
    ``clone_loglik_reweighted`` gets the chunked float64 host form."""
    Y, L, _cn, N, G = _cells_and_cnv(Y, L)
    t = _fit_tables(fit, L, N, x, psi, saturate, saturation_threshold)
    C = t.L.shape[1]
    w = _reweighted_weights(weights, G)
    prior = np.ascontiguousarray(np.broadcast_to(_log_prior(fit, extra_loglik, N, C), (N, C)))
    with _engine_lease(engine, "clone_loglik_reweighted", Y, t.L, engine_opts) as eng:
        return _reweighted_call(eng, Y, t, w, prior, cells, want_ll)


def bootstrap_assignments(fit, Y, L, n_rep=100, clone_assignment_probability=0.95, support_threshold=0.95, *, seed=0, blocks=None, weights=None,
                          extra_loglik=None, x=None, psi=None, saturate=True, saturation_threshold=6, const=True, engine=None, engine_opts=None):
    """``assign_cells`` with BOOTSTRAP SUPPORT for every call: the genes are resampled with replacement ``n_rep`` times (``bootstrap_gene_weights``; whole
    ``blocks`` when given; or the caller's ``weights`` [R, genes]), every replicate is called again, and a cell's support is the share of replicates that
    repeat its call -- what phylogenetics does with sites.  A multinomial over thousands of genes pushes almost every posterior to 0.999...; when the
    counts are overdispersed many of those calls are wrong, and their support is visibly lower.  One upload: a throwaway engine serves both calls, and all
    replicates are one ``clone_loglik_reweighted`` on the device.  Every other argument as for ``assign_cells``.

    Returns a :class:`ClonealignFit` that holds everything ``assign_cells`` returns, identically, plus: ``support`` [N] (the share of replicates whose
    argmax is the cell's own -- the argmax of ``ll + log alpha + extra_loglik`` on the full data), ``clone_support`` [N, C] (the share per clone),
    ``mean_probs`` and ``sd_probs`` [N, C] (mean and standard deviation of the replicates' posteriors), ``clone_bootstrap`` (``clone``, or
    ``"unassigned"`` where ``support < support_threshold``), ``n_newly_unassigned`` (calls that ``clone`` makes and ``clone_bootstrap`` withholds),
    ``weights_seed`` (``seed``; None with the caller's ``weights``) and ``n_rep``."""
    Y, Lm, _cn, N, G = _cells_and_cnv(Y, L)
    ft = _fit_tables(fit, Lm, N, x, psi, saturate, saturation_threshold)
    C = ft.L.shape[1]
    own = weights is None
    w = _reweighted_weights(bootstrap_gene_weights(G, n_rep, seed=seed, blocks=blocks) if own else weights, G, "bootstrap_assignments")
    R = w.shape[0]
    prior = np.ascontiguousarray(np.broadcast_to(_log_prior(fit, extra_loglik, N, C), (N, C)))
    with _engine_lease(engine, "clone_loglik_reweighted", Y, ft.L, engine_opts) as eng:
        ll = eng.clone_loglik(ft.E, ft.U, ft.V, const=const) if hasattr(eng, "clone_loglik") else _clone_loglik_host(Y, ft.E, ft.U, ft.V, const=const)
        rw = _reweighted_call(eng, Y, ft, w, prior, None, False)
    base = _assign_from_loglik(fit, ll, ft.L, extra_loglik, clone_assignment_probability)   # (the parsed L: a DataFrame's column names do not name the clones here)
    with np.errstate(invalid="ignore"):
        t = ll + prior
    cstar = np.argmax(np.where(np.isnan(t), -np.inf, t), axis=1)
    clone_support = rw["votes"] / float(R)
    support = clone_support[np.arange(N), cstar]
    mean = rw["prob_sum"] / R
    sd = np.sqrt(np.maximum(rw["prob_sq"] / R - mean * mean, 0.0))
    clone = np.asarray(base["clone"], dtype=object)
    boot = np.where(support >= support_threshold, clone, "unassigned").astype(object)
    base.update(support=support, clone_support=clone_support, mean_probs=mean, sd_probs=sd, clone_bootstrap=boot,
                n_newly_unassigned=int(((clone != "unassigned") & (boot == "unassigned")).sum()), weights_seed=int(seed) if own else None, n_rep=int(R))
    return base


def _pair_weights(weights, what="clone_pair_loglik", limit=8):
    """The mixture weights of a pair call: 1 to 8 finite values in the open interval (0, 1) (ValueError names the offender otherwise)."""
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if not 1 <= w.shape[0] <= limit:
        raise ValueError(f"{what}: n_weights = {w.shape[0]} is outside [1, 8]")
    for i, v in enumerate(w):
        if not (np.isfinite(v) and 0.0 < v < 1.0):
            raise ValueError(f"{what}: weight {i} is {v}: not inside the open interval (0, 1)")
    return w


def _pair_weight_grid(weights, what="clone_pair_loglik"):
    """``weights`` closed under ``w -> 1 - w`` and sorted (values closer than 1e-12 are one; at most 8 after that): the pairs are unordered, so an
    asymmetric grid would favour one parent."""
    w = _pair_weights(weights, what, limit=1 << 30)
    both = np.sort(np.concatenate([w, 1.0 - w]))
    return _pair_weights(both[np.concatenate([[True], np.diff(both) > 1e-12])], what)


def _clone_pair_loglik_host(Y, E, U=None, V=None, weights=(0.5,), const=True, chunk=512):
    """Float64 host form of ``HipEngine.clone_pair_loglik`` for engines without it: Y [N, G] dense or scipy.sparse (densified ``chunk`` cells at a time), E
    [G, C], U [N, D] and V [G, D] or both None, ``weights`` as given.  Same return value (``{"ll", "pair_ll" [N, M, W], "pairs" [M, 2]}``), same rules
    (the per-pair shift by ``min(log Z_a, log Z_b)``, zero counts skipped, ``-inf`` exactly where both clones have ``E = 0`` against a positive count, no
    NaN), same refusals (ValueError)."""
    from scipy.special import gammaln
    w = _pair_weights(weights)
    ll = _clone_loglik_host(Y, E, U, V, const=const, chunk=max(int(chunk), 1))      # (and its refusals on E, U and V)
    E = np.asarray(E, dtype=np.float64)
    N, G = Y.shape
    C = E.shape[1]
    if C < 2:
        raise ValueError(f"clone_pair_loglik: C = {C} clones: a pair needs at least 2")
    D = 0 if U is None else np.asarray(U).shape[1]
    if D > 0:
        U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    pairs = hostprep.pair_list(C)
    M, W = pairs.shape[0], w.shape[0]
    pll = np.empty((N, M, W))
    logz0 = np.log(E.sum(0))
    for lo, Yc, eta, _m, logz in _cell_chunks(Y, chunk, E, U if D > 0 else None, V):
        n = Yc.shape[0]
        pos = Yc > 0
        s = Yc.sum(1)
        base = np.zeros(n)
        if D > 0:
            base += (Yc * eta).sum(1)
        else:
            logz = np.broadcast_to(logz0[None, :], (n, C))
        if const:
            base += gammaln(s + 1.0) - gammaln(Yc + 1.0).sum(1)
        for p, (a, b) in enumerate(pairs):
            lz = np.minimum(logz[:, a], logz[:, b])
            ca, cb = np.exp(lz - logz[:, a]), np.exp(lz - logz[:, b])
            for k, wk in enumerate(w):
                br = (wk * ca)[:, None] * E[None, :, a] + ((1.0 - wk) * cb)[:, None] * E[None, :, b]
                with np.errstate(divide="ignore"):
                    lb = np.log(br, where=pos, out=np.zeros_like(br))          # zero counts are skipped: 0 * log 0 is never formed
                    t = (Yc * lb).sum(1)
                pll[lo:lo + n, p, k] = t + base - np.where(s > 0, s * lz, 0.0)
    return {"ll": ll, "pair_ll": pll, "pairs": pairs}


def _pair_setup(fit, Y, L, weights, x, psi, saturate, saturation_threshold, what):
    """(Y, model tables, weight grid, clone names) of a pair call named ``what``."""
    Y, L, cn, N, _G = _cells_and_cnv(Y, L)
    if L.shape[1] < 2:
        raise ValueError(f"{what}: C = {L.shape[1]} clones: a pair needs at least 2")
    grid = _pair_weight_grid(weights, what)
    return Y, _fit_tables(fit, L, N, x, psi, saturate, saturation_threshold), grid, _clone_names(fit, cn, L.shape[1])


def _pair_call(engine, Y, t, grid, const, lo, hi):
    """Cells [lo, hi) under the tables ``t`` through the engine's ``clone_pair_loglik``, or through the host form when it has none."""
    if hasattr(engine, "clone_pair_loglik"):
        return engine.clone_pair_loglik(t.E, t.U, t.V, weights=grid, const=const, cells=(lo, hi))
    return _clone_pair_loglik_host(Y[lo:hi], t.E, None if t.U is None else t.U[lo:hi], t.V, weights=grid, const=const)


def clone_pair_loglik(fit, Y, L, *, weights=(0.3, 0.5, 0.7), x=None, psi=None, saturate=True, saturation_threshold=6, const=True, engine=None, engine_opts=None):
    """Log-likelihood of the cells of ``Y`` under every MIXTURE of two clones of a fitted model -- a heterotypic doublet: two cells of clones ``a < b`` in one
    droplet, whose summed counts are multinomial in ``w p_a + (1 - w) p_b`` -- at the fit's point estimates, for every weight of a grid
    (``HipEngine.clone_pair_loglik``; include/clonealign_hip.h has the formula and the rules).  ``Y``, ``L``, ``x``, ``psi``, ``saturate``, ``const``,
    ``engine`` and ``engine_opts`` as for ``clone_loglik``.  ``weights``: 1 to 8 values in (0, 1) after being closed under ``w -> 1 - w`` and sorted (the
    pairs are unordered, so an asymmetric grid would favour one parent); ``w`` is the share of the pair's first clone.

    Returns ``{"ll" [cells, clones] (clone_loglik's), "pair_ll" [cells, M, W], "pairs" [M, 2] (lexicographic), "weights" [W] (the grid used)}``.  An engine
    without ``clone_pair_loglik`` gets the chunked float64 host form."""
    Y, t, grid, _names = _pair_setup(fit, Y, L, weights, x, psi, saturate, saturation_threshold, "clone_pair_loglik")
    with _engine_lease(engine, "clone_pair_loglik", Y, t.L, engine_opts) as eng:
        out = _pair_call(eng, Y, t, grid, const, 0, Y.shape[0])
    out["weights"] = grid
    return out


def detect_doublets(fit, Y, L, doublet_rate=0.05, doublet_probability=0.5, clone_assignment_probability=0.95, *, weights=(0.3, 0.5, 0.7), extra_loglik=None,
                    x=None, psi=None, saturate=True, saturation_threshold=6, const=True, engine=None, engine_opts=None, chunk_cells=None):
    """Heterotypic doublets under a fitted model, without refitting: the exact posterior of every cell of ``Y`` over the hypotheses {singlet of clone c} and
    {doublet of the clone pair (a, b)}, from ``clone_pair_loglik`` (same keywords).  Priors, with ``rho = doublet_rate``, ``alpha`` the fit's clone
    prevalences (uniform when it has none) and ``het = 1 - sum_c alpha_c^2``: singlet ``c``: ``(1 - rho) alpha_c``; pair ``(a, b)``:
    ``rho 2 alpha_a alpha_b / het`` (a homotypic doublet is indistinguishable from a singlet and counts as one); the weights of the grid: uniform.
    ``extra_loglik`` [cells, clones] is added to the singlets; a pair gets ``logaddexp(extra_a, extra_b) - log 2``.  The cells are walked in ranges of
    ``chunk_cells`` (default: so that a range's ``pair_ll`` block stays under 256 MB on the host).

    Returns a :class:`ClonealignFit` with ``p_doublet`` [cells], ``pair_probs`` [cells, M], ``doublet_pair`` (``"A+B"`` for the cells labelled
    ``"doublet"``, else None), ``doublet_weight`` (the posterior mean of ``w`` under the most probable pair: the share of its first-named clone),
    ``clone_probs`` [cells, clones] (renormalised over the singlets: ``assign_cells``'s, so ``recompute_clone_assignment`` works), ``clone``
    (``"doublet"`` where ``p_doublet >= doublet_probability``, else ``assign_cells``'s label), ``loglik`` [cells] (the marginal over all hypotheses),
    ``log_bayes_factor`` [cells] (doublet against singlet, ``rho`` left out), ``clone_loglik``, ``clone_names``, ``pairs`` and ``weights``.  A cell that
    is ``-inf`` under every hypothesis gets NaN probabilities and ``"unassigned"``; no other cell sees a NaN."""
    rho = float(doublet_rate)
    if not (np.isfinite(rho) and 0.0 <= rho <= 1.0):
        raise ValueError(f"detect_doublets: doublet_rate = {doublet_rate} is outside [0, 1]")
    Y, ft, grid, names = _pair_setup(fit, Y, L, weights, x, psi, saturate, saturation_threshold, "detect_doublets")
    N, C = Y.shape[0], ft.E.shape[1]
    pairs = hostprep.pair_list(C)
    M, W = pairs.shape[0], grid.shape[0]
    alpha = fit["ml_params"].get("alpha")
    alpha = np.full(C, 1.0 / C) if alpha is None else np.asarray(alpha, dtype=np.float64).reshape(C)   # (uniform where the fit has none)
    _la, ex = _prior_terms(fit, extra_loglik, N, C)
    step = int(chunk_cells) if chunk_cells else max(1, (1 << 28) // (8 * M * W))
    ll = np.empty((N, C))
    pair_log = np.empty((N, M))                                      # log p(y | pair), the weights marginalised (uniform on the grid)
    w_mean = np.empty((N, M))
    with _engine_lease(engine, "clone_pair_loglik", Y, ft.L, engine_opts) as eng, np.errstate(divide="ignore", invalid="ignore"):
        for lo in range(0, N, step):
            hi = min(N, lo + step)
            r = _pair_call(eng, Y, ft, grid, const, lo, hi)
            ll[lo:hi] = r["ll"]
            pl = r["pair_ll"]
            m = pl.max(2, keepdims=True)
            e = np.exp(pl - np.where(np.isneginf(m), 0.0, m))        # (a pair at -inf for every weight: all zeros, no NaN)
            tot = e.sum(2)
            pair_log[lo:hi] = np.where(np.isneginf(m[:, :, 0]), -np.inf, m[:, :, 0] + np.log(tot)) - np.log(W)
            w_mean[lo:hi] = (e * grid[None, None, :]).sum(2) / tot
    with np.errstate(divide="ignore", invalid="ignore"):
        het = 1.0 - (alpha ** 2).sum()
        t_s = ll + np.log(alpha)[None, :]                            # singlets, rho left out
        t_p = pair_log + (np.log(2.0 * alpha[pairs[:, 0]] * alpha[pairs[:, 1]]) - np.log(het) if het > 0 else np.full(M, -np.inf))[None, :]
        if ex is not None:
            t_s = t_s + ex
            t_p = t_p + np.logaddexp(ex[:, pairs[:, 0]], ex[:, pairs[:, 1]]) - np.log(2.0)
        ls, lp = _lse_clones(t_s), _lse_clones(t_p)
        a_s, a_p = np.log1p(-rho) + ls, np.log(rho) + lp
        loglik = np.where(np.isneginf(a_s) & np.isneginf(a_p), -np.inf, np.logaddexp(a_s, a_p))
        dead = np.isneginf(loglik)
        clone_probs = np.exp(t_s - ls[:, None])                      # (a row of -inf: NaN - no clone is possible)
        pair_probs = np.exp(np.log(rho) + t_p - loglik[:, None])
        pair_probs[dead] = np.nan
        p_doublet = np.where(dead, np.nan, np.exp(a_p - loglik))
        lbf = np.where(np.isneginf(ls) & np.isneginf(lp), np.nan, lp - ls)
    clone = clone_assignment(clone_probs, names, clone_assignment_probability)
    clone[dead] = "unassigned"
    is_d = p_doublet >= doublet_probability                          # (NaN: False)
    clone[is_d] = "doublet"
    best = np.where(np.isneginf(lp), 0, np.argmax(np.where(np.isnan(t_p), -np.inf, t_p), axis=1))
    pair_names = np.asarray([f"{names[a]}+{names[b]}" for a, b in pairs], dtype=object)
    doublet_pair = np.full(N, None, dtype=object)
    doublet_pair[is_d] = pair_names[best[is_d]]
    doublet_weight = np.where(np.isneginf(lp), np.nan, w_mean[np.arange(N), best])
    return ClonealignFit(clone_probs=clone_probs, clone=clone, p_doublet=p_doublet, pair_probs=pair_probs, doublet_pair=doublet_pair,
                         doublet_weight=doublet_weight, loglik=loglik, log_bayes_factor=lbf, clone_loglik=ll, clone_names=names, pairs=pairs,
                         weights=grid, ml_params={"clone_probs": clone_probs})


MIX_CMAX = 32                                                       # components of a mixture call, extra profiles included (include/clonealign_hip.h)


def _mixture_start(start, n, C, lo=0, what="clone_mixture"):
    """The start of a mixture call as [n, C] float64 after the library's refusals (ValueError names the offender), or None."""
    if start is None:
        return None
    st = np.asarray(start, dtype=np.float64)
    if st.ndim == 1 and st.shape[0] == C:
        st = np.broadcast_to(st, (n, C))
    if st.shape != (n, C):
        raise ValueError(f"{what}: start is {st.shape}; expected ({n}, {C})")
    wrong = np.argwhere(~np.isfinite(st) | (st < 0))
    if wrong.size:
        raise ValueError(f"{what}: start has a negative or non-finite entry (cell {lo + wrong[0][0]}, clone {wrong[0][1]})")
    off = np.flatnonzero(~(np.abs(st.sum(1) - 1.0) <= 1e-9))
    if off.size:
        raise ValueError(f"{what}: the start of cell {lo + off[0]} sums to {st[off[0]].sum()}: off 1 by more than 1e-9")
    return np.ascontiguousarray(st)


def _mixture_settings(C, max_iter, tol, what="clone_mixture"):
    """(max_iter, tol) of a mixture call after the library's refusals."""
    if C > MIX_CMAX:
        raise ValueError(f"{what}: C = {C} clones: a mixture takes at most {MIX_CMAX}")
    if int(max_iter) < 0:
        raise ValueError(f"{what}: max_iter = {max_iter} is negative")
    if not (np.isfinite(tol) and tol >= 0):
        raise ValueError(f"{what}: tol_nats = {tol} is negative or not finite")
    return int(max_iter), float(tol)


def _mix_chol_solve(A, b):
    """``x`` with ``A x = b`` for a batch of symmetric matrices [n, C, C] by Cholesky (the lower triangle is read), and ``ok`` [n]: every pivot positive and
    finite.  Rows that break down return garbage that the caller ignores."""
    n, C, _ = A.shape
    Lw = A.copy()
    ok = np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        for k in range(C):
            p = Lw[:, k, k]
            good = (p > 0) & np.isfinite(p)
            ok &= good
            l = np.sqrt(np.where(good, p, 1.0))
            Lw[:, k, k] = l
            Lw[:, k + 1:, k] /= l[:, None]
            Lw[:, k + 1:, k + 1:] -= Lw[:, k + 1:, k, None] * Lw[:, None, k + 1:, k]
        x = b.copy()
        for k in range(C):
            x[:, k] /= Lw[:, k, k]
            x[:, k + 1:] -= Lw[:, k + 1:, k] * x[:, k, None]
        for k in range(C - 1, -1, -1):
            x[:, k] /= Lw[:, k, k]
            x[:, :k] -= Lw[:, k, :k] * x[:, k, None]
    return x, ok


def _clone_mixture_host(Y, E, U=None, V=None, start=None, max_iter=50, tol=1e-3, const=True, cells=None, want_ll=True, want_grad=True, chunk=128):
    """Float64 host form of ``HipEngine.clone_mixture`` for engines without it, the same algorithm in numpy (include/clonealign_hip.h has the formulas, the
    round and the rules): Y [N, G] dense or scipy.sparse (densified ``chunk`` cells at a time), E [G, C], U [N, D] and V [G, D] or both None, ``start``
    [n, C] for the cells of the range or None (uniform).  Same return value, same rules (unsupported entries left out and ``mix_ll = -inf``, the uniform
    restart of a start that excludes the data, ``max_iter = 0`` evaluates), same refusals (ValueError).  Every cell of a chunk is evaluated in every round
    and a stopped cell's weights are frozen, so a cell's values do not depend on when the others stop: T rounds are T calls of one round, bit for bit."""
    from scipy.special import gammaln
    E, U, V, D, esum = _ll_inputs(Y, E, U, V, "clone_mixture")
    N, G = Y.shape
    C = E.shape[1]
    max_iter, tol = _mixture_settings(C, max_iter, tol)
    lo0, hi0 = (0, N) if cells is None else (int(cells[0]), int(cells[1]))
    if lo0 < 0 or hi0 < lo0 or hi0 > N:
        raise ValueError(f"clone_mixture: the cell range [{lo0}, {lo0} + {hi0 - lo0}) is outside [0, {N}]")
    n = hi0 - lo0
    st = _mixture_start(start, n, C, lo0)
    Ys = Y[lo0:hi0]
    Us = None if D == 0 else U[lo0:hi0]
    out = {"ll": _clone_loglik_host(Ys, E, Us, V if D > 0 else None, const=const) if want_ll else None, "weights": np.empty((n, C)),
           "grad": np.empty((n, C)) if want_grad else None, "mix_ll": np.empty(n), "bound": np.empty(n), "rounds": np.zeros(n, dtype=np.int32)}
    steps = (1.0, 0.5, 0.25, 0.125)
    for lo, Yc, eta, _m, logz in _cell_chunks(Ys, chunk, E, Us, V):
        k = Yc.shape[0]
        s = Yc.sum(1)
        base = (Yc * eta).sum(1) if D > 0 else np.zeros(k)
        if D == 0:
            logz = np.broadcast_to(np.log(esum)[None, :], (k, C))
        if const:
            base = base + gammaln(s + 1.0) - gammaln(Yc + 1.0).sum(1)
        lz = logz.min(1)
        q = E[None, :, :] * np.exp(lz[:, None] - logz)[:, None, :]   # [k, G, C], every factor <= 1
        pos = Yc > 0
        usable = pos & (q.sum(2) > 0)
        ninf = (pos & ~usable).any(1)
        seff = np.where(usable, Yc, 0.0).sum(1)
        ssafe = np.where(seff > 0, seff, 1.0)
        ysafe = np.where(pos, Yc, 1.0)

        def evaluate(pi, hess):
            m = np.einsum("ngc,nc->ng", q, pi)
            good = usable & (m > 0)
            bad = (usable & ~good).any(1)
            msafe = np.where(good, m, 1.0)
            f = (Yc * np.log(msafe)).sum(1)                          # (log 1 = 0 where an entry is left out)
            r = np.where(good, Yc / msafe, 0.0)
            g = np.einsum("ng,ngc->nc", r, q)
            H = np.matmul(q.transpose(0, 2, 1), q * (r * r / ysafe)[:, :, None]) if hess else None
            gap = np.maximum(g.max(1) - (pi * g).sum(1), 0.0)
            bound = np.where(seff > 0, np.where(bad, np.inf, gap), 0.0)
            return good, bad, f, g, H, bound

        pi = np.full((k, C), 1.0 / C) if st is None else st[lo:lo + k].copy()
        good, bad, f, g, H, bound = evaluate(pi, max_iter > 0)
        if max_iter > 0 and bad.any():                               # a start whose zeros exclude the data: the uniform start
            pi[bad] = 1.0 / C
            good, bad, f, g, H, bound = evaluate(pi, True)
        rounds = np.zeros(k, dtype=np.int32)
        done = np.zeros(k, dtype=bool)
        while True:
            done |= ~(seff > 0) | (bound <= tol) | (rounds >= max_iter)
            if done.all():
                break
            with np.errstate(all="ignore"):
                gam = g - seff[:, None]
                hcc = np.einsum("ncc->nc", H).copy()
                hsafe = np.where(hcc > 0, hcc, 1.0)
                term = np.where(hcc > 0, np.abs(pi - np.maximum(pi + gam / hsafe, 0.0)), pi)
                eps = np.minimum(1e-3, term.max(1))
                active = (pi <= eps[:, None]) & (gam < 0)
                nF = C - active.sum(1)
                ridge = np.where(nF > 0, 1e-12 * np.where(active, 0.0, hcc).sum(1) / np.maximum(nF, 1), 0.0)
                A = np.where(active[:, :, None] | active[:, None, :], 0.0, H)
                ii = np.arange(C)
                A[:, ii, ii] = np.where(active, 1.0, hcc + ridge[:, None])
                dF, ok = _mix_chol_solve(A, np.where(active, 0.0, gam))
                d = np.where(active, np.where(hcc > 0, gam / hsafe, -1.0), dF)
                ok &= np.isfinite(d).all(1)
                d = np.where(ok[:, None], d, 0.0)
                phi0 = f - seff * pi.sum(1)
                pn = pi * g / ssafe[:, None]                         # the EM step, unless a trial point passes
                taken = np.zeros(k, dtype=bool)
                for t in steps:                                      # descending: the largest step that passes
                    tr = np.maximum(pi + t * d, 0.0)
                    mt = np.einsum("ngc,nc->ng", q, tr)
                    ft = np.where(good, Yc * np.log(np.where(good, mt, 1.0)), 0.0).sum(1)
                    ph = ft - seff * tr.sum(1)
                    passes = ok & ~taken & np.isfinite(ph) & (ph >= phi0 + 1e-4 * (gam * (tr - pi)).sum(1))
                    pn = np.where(passes[:, None], tr, pn)
                    taken |= passes
                tot = pn.sum(1)
                pn = np.where(((tot > 0) & np.isfinite(tot))[:, None], pn / np.where(tot > 0, tot, 1.0)[:, None], pn)
            pi = np.where(done[:, None], pi, pn)
            rounds += ~done
            good, bad, f, g, H, bound = evaluate(pi, True)
        out["weights"][lo:lo + k] = pi
        if want_grad:
            out["grad"][lo:lo + k] = np.where(seff[:, None] > 0, g / ssafe[:, None], 0.0)
        out["mix_ll"][lo:lo + k] = np.where(ninf | bad, -np.inf, f + base - np.where(s > 0, s * lz, 0.0))
        out["bound"][lo:lo + k] = bound
        out["rounds"][lo:lo + k] = rounds
    out["converged"] = out["bound"] <= tol
    return out


def _extra_profiles(extra_profiles, G, what):
    """(profiles [G, M] float64, names) of ``extra_profiles``: a [G, M] matrix (or a length-G vector) of non-negative expected expression, or a dict of name to
    vector; None gives M = 0."""
    if extra_profiles is None:
        return np.zeros((G, 0)), []
    if isinstance(extra_profiles, dict):
        names = [str(k) for k in extra_profiles]
        X = np.stack([np.asarray(v, dtype=np.float64).reshape(-1) for v in extra_profiles.values()], axis=1) if names else np.zeros((G, 0))
    else:
        X = np.asarray(extra_profiles, dtype=np.float64)
        X = X.reshape(-1, 1) if X.ndim == 1 else X
        names = [f"extra_{i + 1}" for i in range(X.shape[1] if X.ndim == 2 else 0)]
    if X.ndim != 2 or X.shape[0] != G:
        raise ValueError(f"{what}: extra_profiles is {X.shape}; expected ({G}, M): one column of expected expression per profile")
    wrong = np.argwhere(~np.isfinite(X) | (X < 0))
    if wrong.size:
        raise ValueError(f"{what}: extra_profiles has a negative or non-finite entry (gene {wrong[0][0]}, profile {names[wrong[0][1]]})")
    return X, names


def clone_mixture(fit, Y, L, *, start=None, max_iter=50, tol=1e-3, extra_profiles=None, x=None, psi=None, saturate=True, saturation_threshold=6, const=True,
                  cells=None, engine=None, engine_opts=None):
    """The maximum-likelihood MIXTURE of the clones of a fitted model for every row of ``Y``: a spatial spot or a bulk sample (clone prevalences), a droplet
    with ambient RNA or a tumour clone with a normal cell (``extra_profiles``), a doublet at any weights, a triplet.  The sum of multinomial rows of several
    clones is multinomial in ``sum_c pi_c p_n.c``; the weights ``pi`` on the simplex are found per row by projected Newton on the device
    (``HipEngine.clone_mixture``; include/clonealign_hip.h has the formulas, the round and the rules) and come with a CERTIFIED bound: no other weights
    gain more than ``bound`` nats (concavity), and a row stops when ``bound <= tol`` or after ``max_iter`` rounds.  ``Y``, ``L``, ``x``, ``psi``,
    ``saturate``, ``const``, ``engine`` and ``engine_opts`` as for ``clone_loglik``; ``cells`` = ``(lo, hi)`` restricts the call to that range.

    ``extra_profiles``: a [genes, M] matrix of non-negative expected expression, or a dict of name to vector -- an ambient profile, a diploid ``2 mu`` --
    that become further columns of the table (scale does not matter: every column is normalised by its own ``Z``; the cell's exponent term applies to them
    too); ``C + M <= 32``.  A throwaway engine is built with ``C + M`` columns; an engine passed in must hold that many.  ``start`` [rows, C + M] on the
    simplex (None: uniform); a start whose zeros exclude the data is replaced by the uniform one; ``max_iter=0`` evaluates at the start.

    Returns a dict: ``weights`` [n, C + M], ``mix_ll`` [n], ``ll`` [n, C + M] (``clone_loglik``'s, one column per component), ``grad`` [n, C + M]
    (``g_c / s_eff``: 1 on the support of an optimum), ``bound`` [n], ``rounds`` [n], ``converged`` [n] (``bound <= tol``), ``component_names`` and
    ``log_lr_single`` [n] = ``mix_ll - max_c ll``: by how many nats the mixture beats the best single component.  An engine without ``clone_mixture`` gets
    the float64 host form."""
    return _mixture_api(fit, Y, L, start, max_iter, tol, extra_profiles, x, psi, saturate, saturation_threshold, const, cells, engine, engine_opts, "clone_mixture")


def _mixture_api(fit, Y, L, start, max_iter, tol, extra_profiles, x, psi, saturate, saturation_threshold, const, cells, engine, engine_opts, what):
    Y, Lm, cn, N, G = _cells_and_cnv(Y, L)
    t = _fit_tables(fit, Lm, N, x, psi, saturate, saturation_threshold)
    C = t.L.shape[1]
    X, xnames = _extra_profiles(extra_profiles, G, what)
    M = X.shape[1]
    if C + M > MIX_CMAX:
        raise ValueError(f"{what}: C + M = {C} + {M} components: a mixture takes at most {MIX_CMAX}")
    max_iter, tol = _mixture_settings(C + M, max_iter, tol, what)
    names = list(_clone_names(fit, cn, C)) + xnames
    E = np.ascontiguousarray(np.concatenate([t.E, X], axis=1))
    Lall = np.ascontiguousarray(np.concatenate([t.L, np.ones((G, M))], axis=1))   # (the engine's own L is not read by a scoring call: it sets the column count)
    lo, hi = (0, N) if cells is None else (int(cells[0]), int(cells[1]))
    if lo < 0 or hi < lo or hi > N:
        raise ValueError(f"{what}: the cell range [{lo}, {lo} + {hi - lo}) is outside [0, {N}]")
    st = _mixture_start(start, hi - lo, C + M, lo, what)
    if engine is not None and hasattr(engine, "clone_mixture") and getattr(engine, "C", C + M) != C + M:
        raise ValueError(f"{what}: the engine holds {engine.C} columns but the call has {C} clones + {M} extra profiles = {C + M} components; "
                         "build the engine with that many columns")
    with _engine_lease(engine, "clone_mixture", Y, Lall, engine_opts) as eng:
        if hasattr(eng, "clone_mixture"):
            out = eng.clone_mixture(E, t.U, t.V, start=st, max_iter=max_iter, tol=tol, const=const, cells=(lo, hi))
        else:
            out = _clone_mixture_host(Y, E, t.U, t.V, start=st, max_iter=max_iter, tol=tol, const=const, cells=(lo, hi))
    with np.errstate(invalid="ignore"):
        best = out["ll"].max(1) if C + M else np.zeros(hi - lo)
        out["log_lr_single"] = np.where(np.isneginf(out["mix_ll"]) & np.isneginf(best), np.nan, out["mix_ll"] - best)
    out["component_names"] = names
    out["n_clones"] = C
    return out


def mixture_loglik(fit, Y, L, weights, *, extra_profiles=None, x=None, psi=None, saturate=True, saturation_threshold=6, const=True, cells=None, engine=None,
                   engine_opts=None):
    """``clone_mixture`` in EVALUATION mode: the mixture log-likelihood of every row of ``Y`` at the given ``weights`` [rows, C + M] (or one row for all), zeros
    included, with the gradient and the bound at those weights and no round taken.  A one-hot row reproduces ``clone_loglik``'s value, ``(w, 1 - w)`` on a
    pair ``clone_pair_loglik``'s.  Same return value as ``clone_mixture`` (``rounds`` is 0)."""
    return _mixture_api(fit, Y, L, weights, 0, 0.0, extra_profiles, x, psi, saturate, saturation_threshold, const, cells, engine, engine_opts, "mixture_loglik")


def deconvolve_clones(fit, Y, L, *, extra_profiles=None, min_weight=0.05, start=None, max_iter=50, tol=1e-3, x=None, psi=None, saturate=True,
                      saturation_threshold=6, const=True, cells=None, engine=None, engine_opts=None):
    """Clone composition of every row of ``Y`` under a fitted model, from ``clone_mixture`` (same keywords): what a spot, a bulk sample or a contaminated
    droplet is made of.  Returns everything ``clone_mixture`` returns, except that ``weights`` [n, C] holds the clones' columns and ``weights_extra``
    [n, M] those of ``extra_profiles`` (``weights_all`` [n, C + M] is the solver's row), plus: ``dominant`` [n] (the name of the largest component),
    ``n_components`` [n] (weights at or above ``min_weight``), ``is_mixed`` [n] (more than one such component) and ``prevalence`` [C + M]: the
    read-weighted mean weight per component over the rows -- the bulk deconvolution when ``Y`` has one row (rows without reads, or that no component can
    explain, carry no weight)."""
    if not (np.isfinite(min_weight) and 0.0 <= min_weight <= 1.0):
        raise ValueError(f"deconvolve_clones: min_weight = {min_weight} is outside [0, 1]")
    out = _mixture_api(fit, Y, L, start, max_iter, tol, extra_profiles, x, psi, saturate, saturation_threshold, const, cells, engine, engine_opts, "deconvolve_clones")
    w = out["weights"]
    C = out["n_clones"]
    Yc = _counts_array(Y.values if hasattr(Y, "columns") and hasattr(Y, "values") else Y)
    lo, hi = (0, Yc.shape[0]) if cells is None else (int(cells[0]), int(cells[1]))
    reads = np.asarray(Yc[lo:hi].sum(1), dtype=np.float64).reshape(-1)
    reads = np.where(np.isfinite(out["mix_ll"]), reads, 0.0)
    names = np.asarray(out["component_names"], dtype=object)
    n_comp = (w >= min_weight).sum(1)
    out.update(weights_all=w, weights=w[:, :C], weights_extra=w[:, C:], dominant=names[np.argmax(w, axis=1)] if w.shape[1] else np.empty(w.shape[0], dtype=object),
               n_components=n_comp, is_mixed=n_comp > 1, min_weight=float(min_weight),
               prevalence=(reads[:, None] * w).sum(0) / reads.sum() if reads.sum() > 0 else np.full(w.shape[1], np.nan))
    return out


DM_DEFAULT_GRID = tuple(10.0 ** np.arange(1.0, 4.75, 0.5))         # 8 concentrations, 10 .. 10^4.5


def _dm_concentrations(concentration, what="clone_loglik_dm", limit=16):
    """The concentrations of a Dirichlet-multinomial call: 1 to 16 finite values > 0 (ValueError names the offender otherwise)."""
    phi = np.asarray(concentration, dtype=np.float64).reshape(-1)
    if not 1 <= phi.shape[0] <= limit:
        raise ValueError(f"{what}: n_conc = {phi.shape[0]} is outside [1, 16]")
    for i, v in enumerate(phi):
        if not (np.isfinite(v) and v > 0.0):
            raise ValueError(f"{what}: concentration {i} is {v}: not finite and > 0")
        if v > 1e300:
            raise ValueError(f"{what}: concentration {i} is above 1e300: lgamma of it overflows")
    return phi


def _clone_loglik_dm_host(Y, E, U=None, V=None, concentration=(100.,), const=True, chunk=512, with_scale=False):
    """Float64 host form of ``HipEngine.clone_loglik_dm`` (numpy and ``scipy.special.gammaln`` over the non-zero counts): Y [N, G] dense or scipy.sparse
    (densified ``chunk`` cells at a time), E [G, C], U [N, D] and V [G, D] or both None, ``concentration`` as given.  Same return value (``{"ll", "dm_ll"
    [N, C, n_conc]}``), same rules (zero counts never visited, ``-inf`` exactly where ``a = phi p`` is 0 against a positive count, ``0 + const`` for a
    cell without counts, no NaN), same refusals (ValueError).  It is the yardstick of the device form and the only CPU route.  ``with_scale`` adds
    ``"scale"`` [N, C, n_conc]: per entry the sum of the magnitudes that went into it -- ``|gammaln(y + a)| + |gammaln(a)| + 1 + |eta| + |log Z|`` per
    non-zero count (the relative error of ``a`` enters each term with a factor of about 1), ``|gammaln(phi)| + |gammaln(phi + s)|`` and, with the constant,
    ``gammaln(s + 1) + sum gammaln(y + 1)`` -- against which the tests bound the rounding error of another evaluation."""
    from scipy.special import gammaln
    phi = _dm_concentrations(concentration)
    ll = _clone_loglik_host(Y, E, U, V, const=const, chunk=max(int(chunk), 1))      # (and its refusals on E, U and V)
    E = np.asarray(E, dtype=np.float64)
    N, C = Y.shape[0], E.shape[1]
    D = 0 if U is None else np.asarray(U).shape[1]
    if D > 0:
        U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    K = phi.shape[0]
    dm = np.empty((N, C, K))
    scale = np.empty((N, C, K)) if with_scale else None
    logz0 = np.log(E.sum(0))
    for lo, Yc, eta, m, logz in _cell_chunks(Y, chunk, E, U if D > 0 else None, V):
        n = Yc.shape[0]
        s = Yc.sum(1)
        r, g = np.nonzero(Yc > 0)                                    # the non-zero counts, rows ascending and genes ascending within a row
        y = Yc[r, g]
        if D > 0:
            t = np.exp(eta[r, g] - m[r])
        else:
            m, logz, t = np.zeros(n), np.broadcast_to(logz0[None, :], (n, C)), np.ones(y.shape[0])
        head = np.where(s[:, None] > 0, gammaln(phi)[None, :] - gammaln(phi[None, :] + s[:, None]), 0.0)
        hsc = np.abs(gammaln(phi))[None, :] + np.abs(gammaln(phi[None, :] + s[:, None]))
        if const:
            lg = gammaln(Yc + 1.0).sum(1)
            head = head + (gammaln(s + 1.0) - lg)[:, None]
            hsc = hsc + (gammaln(s + 1.0) + lg)[:, None]
        aeta = np.abs(eta[r, g]) if D > 0 else 0.0
        for c in range(C):
            a = (np.exp(m - logz[:, c])[r] * E[g, c] * t)[:, None] * phi[None, :]            # phi p, [non-zero counts, K]
            with np.errstate(divide="ignore", invalid="ignore"):
                g1, g0 = gammaln(y[:, None] + a), gammaln(a)
                term = np.where(a > 0, g1 - g0, -np.inf)
            for k in range(K):
                dm[lo:lo + n, c, k] = np.bincount(r, weights=term[:, k], minlength=n) + head[:, k]
            if scale is not None:                                    # the magnitudes of what was added, per entry (the tests' yardstick of rounding)
                per = np.abs(g1) + np.abs(g0) + (1.0 + aeta + np.abs(logz[r, c]))[:, None]
                for k in range(K):
                    scale[lo:lo + n, c, k] = np.bincount(r, weights=per[:, k], minlength=n) + hsc[:, k]
    return {"ll": ll, "dm_ll": dm} if scale is None else {"ll": ll, "dm_ll": dm, "scale": scale}


def _dm_call(engine, Y, t, phi, const):
    """All cells under the tables ``t`` through the engine's ``clone_loglik_dm``, or through the host form when it has none."""
    if hasattr(engine, "clone_loglik_dm"):
        return engine.clone_loglik_dm(t.E, t.U, t.V, concentration=phi, const=const)
    return _clone_loglik_dm_host(Y, t.E, t.U, t.V, concentration=phi, const=const)


def clone_loglik_dm(fit, Y, L, *, concentration, x=None, psi=None, saturate=True, saturation_threshold=6, const=True, engine=None, engine_opts=None):
    """DIRICHLET-MULTINOMIAL log-likelihood of the cells of ``Y`` under every clone of a fitted model at every value of ``concentration`` (1 to 16 finite
    values ``phi`` > 0): ``DirichletMultinomial(total = s_n, alpha = phi * p_n.c).log_prob(y_n)`` with ``p_n.c`` the multinomial probabilities of
    ``clone_loglik`` -- the same model with overdispersed counts; ``phi -> inf`` gives ``clone_loglik`` back (``HipEngine.clone_loglik_dm``;
    include/clonealign_hip.h has the formula and the rules).  ``Y``, ``L``, ``x``, ``psi``, ``saturate``, ``const``, ``engine`` and ``engine_opts`` as for
    ``clone_loglik``.

    Returns ``{"ll" [cells, clones] (clone_loglik's), "dm_ll" [cells, clones, n_conc], "concentration" [n_conc]}``.  An engine without
    ``clone_loglik_dm`` gets the chunked float64 host form."""
    phi = _dm_concentrations(concentration)
    Y, Lm, _cn, N, _G = _cells_and_cnv(Y, L)
    t = _fit_tables(fit, Lm, N, x, psi, saturate, saturation_threshold)
    with _engine_lease(engine, "clone_loglik_dm", Y, t.L, engine_opts) as eng:
        out = _dm_call(eng, Y, t, phi, const)
    out["concentration"] = phi
    return out


def _estimate_concentration(fit, engine, Y, t, grid, refine, extra_loglik, const):
    """``estimate_concentration`` on a live engine; also returns the log-likelihoods at the chosen concentration (``assign_cells_dm`` reuses them)."""
    grid = np.unique(_dm_concentrations(DM_DEFAULT_GRID if grid is None else grid, "estimate_concentration", limit=1 << 30))
    lp = _log_prior(fit, extra_loglik, Y.shape[0], t.E.shape[1])
    seen, ll = {}, None                                              # concentration -> (marginal, dm_ll [N, C])

    def visit(values):
        nonlocal ll
        for lo in range(0, len(values), 16):                         # (16 concentrations per device call)
            phi = np.asarray(values[lo:lo + 16], dtype=np.float64)
            r = _dm_call(engine, Y, t, phi, const)
            ll = r["ll"]
            cell = _lse_clones(r["dm_ll"] + lp[:, :, None])         # [N, n_conc]
            for k, v in enumerate(phi):
                seen[float(v)] = (cell[:, k], r["dm_ll"][:, :, k].copy())
    visit(grid)
    multi = _lse_clones(ll + lp)
    live = ~np.isneginf(multi)                                       # a cell that is impossible under every clone says nothing about phi

    def marginal(v):
        return float(seen[v][0][live].sum())
    best = max(grid.tolist(), key=marginal)                          # (the first maximum)
    at_edge = len(grid) > 1 and best in (float(grid[0]), float(grid[-1])) or len(grid) == 1
    for _ in range(0 if at_edge else int(refine)):
        vs = sorted(seen)
        i = vs.index(best)
        visit(np.geomspace(vs[i - 1], vs[i + 1], 10)[1:-1].tolist())  # 8 log-spaced values between the maximum's two neighbours, one device call
        best = max(sorted(seen), key=marginal)
    vs = np.asarray(sorted(seen))
    return {"concentration": float(best), "grid": vs, "marginal_loglik": np.asarray([marginal(float(v)) for v in vs]),
            "multinomial_marginal_loglik": float(multi[live].sum()), "at_edge": bool(at_edge), "n_cells_used": int(live.sum())}, seen[best][1], ll


def estimate_concentration(fit, Y, L, *, grid=None, refine=2, extra_loglik=None, x=None, psi=None, saturate=True, saturation_threshold=6, const=True,
                           engine=None, engine_opts=None):
    """The Dirichlet-multinomial concentration ``phi`` of the cells of ``Y`` under a fitted model, by marginal likelihood over a grid, without refitting:
    ``M(phi) = sum_n logsumexp_c(log alpha_c + extra_loglik_nc + dm_ll[n, c, phi])`` with ``dm_ll`` of ``clone_loglik_dm`` (same keywords).  ``grid``:
    the concentrations tried first (default 8 values, ``10 ** arange(1, 4.75, 0.5)``; more than 16 take several device calls); each of ``refine``
    rounds then makes one more device call on 8 log-spaced values between the two neighbours of the best value so far.

    Returns a dict: ``concentration`` (the arg-max), ``grid`` (every value visited, ascending) and ``marginal_loglik`` (``M`` at each),
    ``multinomial_marginal_loglik`` (the same sum under ``clone_loglik``: the limit ``phi -> inf``, from the same call), ``at_edge`` -- True when the
    arg-max of the first grid is its largest value (no detectable overdispersion: the multinomial is adequate) or its smallest; no refinement is made then --
    and ``n_cells_used`` (cells that are ``-inf`` under every clone are left out of every sum)."""
    Y, Lm, _cn, N, _G = _cells_and_cnv(Y, L)
    t = _fit_tables(fit, Lm, N, x, psi, saturate, saturation_threshold)
    with _engine_lease(engine, "clone_loglik_dm", Y, t.L, engine_opts) as eng:
        return _estimate_concentration(fit, eng, Y, t, grid, refine, extra_loglik, const)[0]


def assign_cells_dm(fit, Y, L, concentration="auto", clone_assignment_probability=0.95, *, grid=None, refine=2, extra_loglik=None, x=None, psi=None,
                    saturate=True, saturation_threshold=6, const=True, engine=None, engine_opts=None):
    """``assign_cells`` under the DIRICHLET-MULTINOMIAL likelihood of ``clone_loglik_dm``: posteriors that allow for the overdispersion of the counts, so
    that the threshold ``clone_assignment_probability`` rejects what a multinomial over thousands of genes calls certain.  ``concentration``: a value
    > 0, or ``"auto"`` for ``estimate_concentration`` (``grid``, ``refine``) on the same engine -- the matrix is uploaded once.  Other keywords as for
    ``assign_cells``.

    Returns everything ``assign_cells`` returns, computed from ``dm_ll`` at the chosen concentration (``clone_loglik`` holds it), plus ``concentration``,
    ``multinomial_clone_loglik``, ``multinomial_clone_probs`` and ``multinomial_clone`` (``assign_cells``'s own answer, from the same device call),
    ``n_calls_changed`` (cells whose label differs between the two), ``n_newly_unassigned`` (cells the multinomial assigns and this does not) and, with
    ``"auto"``, ``concentration_estimate`` (``estimate_concentration``'s dict)."""
    auto = isinstance(concentration, str)
    if auto and concentration != "auto":
        raise ValueError(f"assign_cells_dm: concentration must be a value > 0 or \"auto\", got {concentration!r}")
    phi = None if auto else _dm_concentrations([concentration], "assign_cells_dm")
    Yc, Lm, _cn, N, _G = _cells_and_cnv(Y, L)
    t = _fit_tables(fit, Lm, N, x, psi, saturate, saturation_threshold)
    with _engine_lease(engine, "clone_loglik_dm", Yc, t.L, engine_opts) as eng:
        if auto:
            est, dm, ll = _estimate_concentration(fit, eng, Yc, t, grid, refine, extra_loglik, const)
        else:
            r = _dm_call(eng, Yc, t, phi, const)
            est, dm, ll = None, r["dm_ll"][:, :, 0], r["ll"]
    out = _assign_from_loglik(fit, dm, L, extra_loglik, clone_assignment_probability)
    multi = _assign_from_loglik(fit, ll, L, extra_loglik, clone_assignment_probability)
    out.update(concentration=est["concentration"] if auto else float(phi[0]), multinomial_clone_loglik=ll, multinomial_clone_probs=multi["clone_probs"],
               multinomial_clone=multi["clone"], n_calls_changed=int((out["clone"] != multi["clone"]).sum()),
               n_newly_unassigned=int(((out["clone"] == "unassigned") & (multi["clone"] != "unassigned")).sum()))
    if auto:
        out["concentration_estimate"] = est
    return out


def _project_cells_host(Y, E, V, K, P, X, log_prior, psi_start, const=True, max_iter=25, tol=1e-9, max_step=1.0, chunk=2048):
    """Float64 numpy restatement of ``HipEngine.project_cells`` (ca_project_cells; the algorithm is stated in include/clonealign_hip.h), step for step,
    ``chunk`` cells at a time: Y [N, G] dense or scipy.sparse, E [G, C], V = [W | beta] [G, K + P] or None, X [N, P] or None, log_prior [N, C] or None,
    psi_start [N, K] or None.  Any K (the device takes K <= 2).  Same return value, same rules, same refusals (ValueError)."""
    from scipy.special import gammaln
    E = np.asarray(E, dtype=np.float64)
    N, G = Y.shape
    K, P = int(K), int(P)
    D = K + P
    if E.ndim != 2 or E.shape[0] != G:
        raise ValueError(f"project_cells: Y is {N} x {G} but E is {E.shape}")
    C = E.shape[1]
    if K < 0:
        raise ValueError(f"project_cells: K = {K} is negative")
    if P < 0 or D > 8:
        raise ValueError(f"project_cells: K + P = {D} is outside [0, 8]")
    if D > 0 and V is None:
        raise ValueError(f"project_cells: K + P = {D} needs V (genes x (K + P))")
    if P > 0 and X is None:
        raise ValueError(f"project_cells: P = {P} needs X (cells x P)")
    if max_iter < 0:
        raise ValueError(f"project_cells: max_iter = {max_iter} is negative")
    for name, v in (("tol", tol), ("max_step", max_step)):
        if not (np.isfinite(v) and v > 0):
            raise ValueError(f"project_cells: {name} = {v} is not a positive finite number")
    V = np.zeros((G, 0)) if D == 0 else np.asarray(V, dtype=np.float64)
    X = np.zeros((N, 0)) if P == 0 else np.asarray(X, dtype=np.float64)
    psi = np.zeros((N, K)) if psi_start is None or K == 0 else np.array(psi_start, dtype=np.float64)
    if V.shape != (G, D) or X.shape != (N, P) or psi.shape != (N, K):
        raise ValueError(f"project_cells: V is {V.shape}, X {X.shape}, psi_start {psi.shape}; expected ({G}, {D}), ({N}, {P}), ({N}, {K})")
    wrong = np.argwhere(~np.isfinite(E) | (E < 0))
    if wrong.size:
        raise ValueError(f"project_cells: expected expression has a negative or non-finite entry (gene {wrong[0][0]}, clone {wrong[0][1]})")
    esum = E.sum(0)
    wrong = np.flatnonzero(~np.isfinite(esum) | (esum == 0))
    if wrong.size:
        raise ValueError(f"project_cells: expected expression of clone {wrong[0]} sums to {esum[wrong[0]]} over the genes")
    for name, M, row, colname in (("V", V, "gene", "factor"), ("psi_start", psi, "cell", "factor"), ("X", X, "cell", "covariate")):
        if M.size and not np.isfinite(M).all():
            r, d = np.argwhere(~np.isfinite(M))[0]
            raise ValueError(f"project_cells: {name} has a non-finite entry ({row} {r}, {colname} {d})")
    lp = None
    if log_prior is not None:
        lp = np.asarray(log_prior, dtype=np.float64)
        if lp.shape != (N, C):
            raise ValueError(f"project_cells: log_prior is {lp.shape}; expected ({N}, {C})")
        wrong = np.argwhere(np.isnan(lp) | np.isposinf(lp))
        if wrong.size:
            raise ValueError(f"project_cells: log_prior has a NaN or +inf entry (cell {wrong[0][0]}, clone {wrong[0][1]}); -inf excludes a clone")
    zero = E == 0
    logE = np.log(np.where(zero, 1.0, E))                            # xlogy: 0 where E = 0, put right below
    W = V[:, :K]
    tri = [(k, l) for k in range(K) for l in range(k, K)]
    out = {"psi": psi, "ll": np.empty((N, C)), "clone_probs": np.empty((N, C)), "objective": np.empty(N), "rounds": np.zeros(N, dtype=np.int32),
           "converged": np.zeros(N, dtype=bool)}
    for lo, Yc, _eta, _m, _logz in _cell_chunks(Y, chunk):
        n = Yc.shape[0]
        s = Yc.sum(1)
        A = Yc @ logE                                                # the sweep: A, B, s and the constant
        if zero.any():
            A[((Yc > 0).astype(np.float64) @ zero.astype(np.float64)) > 0] = -np.inf
        if const:
            A += (gammaln(s + 1.0) - gammaln(Yc + 1.0).sum(1))[:, None]
        B = Yc @ V
        U = np.concatenate([psi[lo:lo + n], X[lo:lo + n]], axis=1)
        lpc = 0.0 if lp is None else lp[lo:lo + n]
        frozen = np.zeros(n, dtype=bool)

        def evaluate(i, moments):
            """steps 1-2 (and the moments of step 3) for the cells i of the chunk"""
            eta = U[i] @ V.T
            m = eta.max(1) if G else np.zeros(i.size)
            w = np.exp(eta - m[:, None])
            Z0 = w @ E
            with np.errstate(divide="ignore", invalid="ignore"):
                ll = A[i] + (U[i] * B[i]).sum(1)[:, None] - np.where(s[i, None] > 0, s[i, None] * (m[:, None] + np.log(Z0)), 0.0)
                t = ll + (lpc if lp is None else lpc[i])
                M = t.max(1)
                lse = M + np.log(np.exp(t - M[:, None]).sum(1))       # (a row of -inf: NaN - no clone is possible)
                gamma = np.exp(t - lse[:, None])
            if not moments:
                return ll, gamma, lse, M, None, None
            mean = np.empty((i.size, C, K))
            cov = np.empty((i.size, C, K, K))
            for k in range(K):
                wk = w * W[:, k]
                mean[:, :, k] = (wk @ E) / Z0
                for l in range(k, K):
                    cov[:, :, k, l] = cov[:, :, l, k] = ((wk * W[:, l]) @ E) / Z0
            cov -= mean[:, :, :, None] * mean[:, :, None, :]
            return ll, gamma, lse, M, mean, cov

        def settle(i, ll, gamma, lse, M, ok, used):
            """freeze the cells i with this evaluation's outputs"""
            dead = np.isneginf(M)
            j = lo + i
            out["ll"][j], out["clone_probs"][j] = ll, gamma
            out["objective"][j] = np.where(dead, -np.inf, lse - 0.5 * (U[i, :K] ** 2).sum(1))
            out["rounds"][j] = np.where(dead, 0, used)
            out["converged"][j] = ok & ~dead
            frozen[i] = True

        for t in range(int(max_iter) if K > 0 else 0):
            i = np.flatnonzero(~frozen)
            if i.size == 0:
                break
            ll, gamma, lse, M, mean, cov = evaluate(i, True)
            dead = np.isneginf(M)
            g0 = np.where(dead[:, None], 0.0, gamma)                 # (a cell without a possible clone takes no step)
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                g = B[i, :K] - s[i, None] * np.einsum("nc,nck->nk", g0, mean) - U[i, :K]
                H = np.eye(K)[None] + s[i, None, None] * np.einsum("nc,nckl->nkl", g0, cov)
                if K == 1:
                    d = g / H[:, 0]
                elif K == 2:                                             # the closed form the device uses
                    det = H[:, 0, 0] * H[:, 1, 1] - H[:, 0, 1] * H[:, 0, 1]
                    d = np.stack([(H[:, 1, 1] * g[:, 0] - H[:, 0, 1] * g[:, 1]) / det, (H[:, 0, 0] * g[:, 1] - H[:, 0, 1] * g[:, 0]) / det], axis=1)
                else:
                    d = np.linalg.solve(H, g[:, :, None])[:, :, 0]
                dmax = np.abs(d).max(1)
            nan = ~(dmax < np.inf)                                        # a step that is no number: the cell stops where it is, not converged
            stop = dead | nan | (dmax <= tol)
            if stop.any():
                settle(i[stop], ll[stop], gamma[stop], lse[stop], M[stop], (dmax <= tol)[stop], t + 1)
            go = ~stop
            f = np.where(dmax[go] > max_step, max_step / dmax[go], 1.0)
            U[i[go], :K] += d[go] * f[:, None]
        i = np.flatnonzero(~frozen)
        if i.size:                                                   # the cells that never froze: ll and the posterior at the psi they hold
            ll, gamma, lse, M, _m, _c = evaluate(i, False)
            settle(i, ll, gamma, lse, M, np.full(i.size, K == 0), int(max_iter) if K > 0 else 0)
        psi[lo:lo + n] = U[:, :K]
    return out


def project_cells(fit, Y, L, clone_assignment_probability=0.95, *, extra_loglik=None, x=None, psi_start=None, saturate=True, saturation_threshold=6,
                  const=True, max_iter=25, tol=1e-9, max_step=1.0, engine=None, engine_opts=None):
    """Place cells the fit never saw: for every cell of ``Y`` the MAP value of its latent factor ``psi`` under the fit's gene-level parameters (``mu``,
    ``W``, ``beta``, ``alpha``) and the exact clone posterior at it, without refitting -- ``assign_cells`` with the ``W`` term switched on.  Per cell it
    maximises ``F(psi) = logsumexp_c(ll_c(psi) + log alpha_c + extra_loglik_c) - |psi|^2 / 2`` (``ll`` is ``clone_loglik``'s; the prior is the
    reference's ``Normal(0, 1)``, R/inference-tflow.R:318-319) by generalised EM with one safeguarded Newton step per round, from ``psi_start`` (default
    0); a cell stops when its step falls to ``tol`` or after ``max_iter`` rounds (include/clonealign_hip.h states the algorithm).

    ``Y``, ``L``, ``x``, ``saturate``, ``const``, ``engine`` and ``engine_opts`` as for ``clone_loglik``: one float64 sweep over the matrix on the device,
    then two launches per round that do not read it (``HipEngine.project_cells``); an engine without the method gets the chunked float64 host form.
    The device takes fits with ``K <= 2`` (ValueError otherwise).
    Returns a :class:`ClonealignFit` with ``psi`` [cells, K], ``clone_probs``, ``clone``, ``loglik`` (``F + |psi|^2 / 2``: the cell's marginal over the
    clones at its psi), ``objective`` (``F``), ``clone_loglik`` [cells, clones], ``rounds``, ``converged`` and ``clone_names``;
    ``recompute_clone_assignment`` works on it.  A fit with ``K = 0`` returns what ``assign_cells`` returns, plus an empty ``psi``."""
    Y, Lm, cn, N, _G = _cells_and_cnv(Y, L)
    t = _fit_tables(fit, Lm, N, x, None, saturate, saturation_threshold, free_psi=True)
    K, C = t.K, Lm.shape[1]
    if K == 0:
        out = assign_cells(fit, Y, L, clone_assignment_probability, extra_loglik=extra_loglik, x=x, saturate=saturate,
                           saturation_threshold=saturation_threshold, const=const, engine=engine, engine_opts=engine_opts)
        out.update(psi=np.zeros((N, 0)), objective=out["loglik"].copy(), rounds=np.zeros(N, dtype=np.int32), converged=np.isfinite(out["loglik"]))
        out["ml_params"] = {"psi": out["psi"], "clone_probs": out["clone_probs"]}
        return out
    names = _clone_names(fit, cn, C)
    if psi_start is not None:
        psi_start = np.asarray(psi_start, dtype=np.float64)
        if psi_start.size != N * K:
            raise ValueError(f"psi_start has {psi_start.size} entries but Y has {N} rows (cells) and the fit K = {K}")
        psi_start = psi_start.reshape(N, K)
    V = np.concatenate([t.W, t.beta], axis=1)
    lp = None
    if fit["ml_params"].get("alpha") is not None or extra_loglik is not None:
        lp = np.zeros((N, C)) + _log_prior(fit, extra_loglik, N, C)
    with _engine_lease(engine, "project_cells", Y, t.L, engine_opts) as eng:
        if hasattr(eng, "project_cells"):
            if K > 2:
                raise ValueError(f"the fit has K = {K} latent factors; the device form of project_cells takes K <= 2")
            r = eng.project_cells(t.E, V, K, X=t.x, log_prior=lp, psi_start=psi_start, const=const, max_iter=max_iter, tol=tol, max_step=max_step)
        else:
            r = _project_cells_host(Y, t.E, V, K, t.P, t.x, lp, psi_start, const, max_iter, tol, max_step)
    psi, probs = r["psi"], r["clone_probs"]
    return ClonealignFit(psi=psi, clone_probs=probs, clone=clone_assignment(probs, names, clone_assignment_probability),
                         loglik=r["objective"] + 0.5 * (psi ** 2).sum(1), objective=r["objective"], clone_loglik=r["ll"], rounds=r["rounds"],
                         converged=r["converged"], clone_names=names, ml_params={"psi": psi, "clone_probs": probs})


def gauss_hermite_rule(K, n_nodes=8):
    """A quadrature rule for the standard normal measure in ``K`` dimensions: the tensor product of the ``n_nodes``-point Gauss-Hermite rule per axis
    (``numpy.polynomial.hermite_e.hermegauss``), weights normalised to sum 1.  Returns ``(nodes [n_nodes ** K, K], weights [n_nodes ** K])``; ``K = 0``
    gives the single empty node with weight 1."""
    K, n = int(K), int(n_nodes)
    if K < 0 or n < 1:
        raise ValueError(f"gauss_hermite_rule: K = {K} and n_nodes = {n} must be >= 0 and >= 1")
    z, w = np.polynomial.hermite_e.hermegauss(n)
    w = w / w.sum()
    if K == 0:
        return np.zeros((1, 0)), np.ones(1)
    grids = np.meshgrid(*([z] * K), indexing="ij")
    nodes = np.stack([g.reshape(-1) for g in grids], axis=1)
    weights = np.ones(n ** K)
    for k, g in enumerate(np.meshgrid(*([w] * K), indexing="ij")):
        weights = weights * g.reshape(-1)
    return nodes, weights / weights.sum()


def _evidence_rule(K, nodes, weights):
    """(nodes [Q, K], weights [Q]) of a ``clone_evidence`` call after the library's refusals (ValueError names the offender)."""
    if nodes is None or weights is None:
        raise ValueError(f"clone_evidence: {'nodes' if nodes is None else 'weights'} is None (n_nodes x K nodes and n_nodes weights are needed)")
    wt = np.asarray(weights, dtype=np.float64).reshape(-1)
    Q = wt.shape[0]
    if Q < 1 or Q > 64:
        raise ValueError(f"clone_evidence: n_nodes = {Q} is outside [1, 64]")
    nd = np.asarray(nodes, dtype=np.float64)
    if nd.size != Q * K:
        raise ValueError(f"clone_evidence: nodes is {nd.shape}; {Q} weights and K = {K} need ({Q}, {K})")
    nd = nd.reshape(Q, K)
    for q in range(Q):
        if not np.isfinite(nd[q]).all():
            raise ValueError(f"clone_evidence: node {q} has a non-finite coordinate (factor {int(np.flatnonzero(~np.isfinite(nd[q]))[0])})")
        if not (np.isfinite(wt[q]) and wt[q] > 0):
            raise ValueError(f"clone_evidence: weight {q} is {wt[q]}: not positive and finite")
    total = 0.0
    for q in range(Q):
        total += float(wt[q])
    if not abs(total - 1.0) <= 1e-12:
        raise ValueError(f"clone_evidence: the weights sum to {total}: off 1 by more than 1e-12")
    return nd, wt


def _clone_evidence_host(Y, E, V, K, P, X, psi_start, nodes, weights, const=True, max_iter=50, tol=1e-9, max_step=1.0, chunk=None):
    """Float64 numpy restatement of ``HipEngine.clone_evidence`` (ca_clone_evidence; the algorithm is stated in include/clonealign_hip.h), step for step,
    ``chunk`` cells at a time (None: so that cells x clones x genes stays near 4e6), vectorised over the (cell, clone) pairs and the genes: Y [N, G] dense
    or scipy.sparse, E [G, C], V = [W | beta] [G, K + P] or None, X [N, P] or None, psi_start [N, K] or None, nodes [Q, K], weights [Q].  Any K (general
    solve and Cholesky beyond the device's closed forms for K <= 2).  Same return value, same rules, same refusals (ValueError)."""
    from scipy.special import gammaln
    E = np.asarray(E, dtype=np.float64)
    N, G = Y.shape
    K, P = int(K), int(P)
    D = K + P
    what = "clone_evidence"
    if E.ndim != 2 or E.shape[0] != G:
        raise ValueError(f"{what}: Y is {N} x {G} but E is {E.shape}")
    C = E.shape[1]
    if K < 0:
        raise ValueError(f"{what}: K = {K} is negative")
    if P < 0 or D > 8:
        raise ValueError(f"{what}: K + P = {D} is outside [0, 8]")
    if D > 0 and V is None:
        raise ValueError(f"{what}: K + P = {D} needs V (genes x (K + P))")
    if P > 0 and X is None:
        raise ValueError(f"{what}: P = {P} needs X (cells x P)")
    if max_iter < 0:
        raise ValueError(f"{what}: max_iter = {max_iter} is negative")
    for name, v in (("tol", tol), ("max_step", max_step)):
        if not (np.isfinite(v) and v > 0):
            raise ValueError(f"{what}: {name} = {v} is not a positive finite number")
    nd, wt = _evidence_rule(K, nodes, weights)
    Q = wt.shape[0]
    V = np.zeros((G, 0)) if D == 0 else np.asarray(V, dtype=np.float64)
    X = np.zeros((N, 0)) if P == 0 else np.asarray(X, dtype=np.float64)
    start = np.zeros((N, K)) if psi_start is None or K == 0 else np.array(psi_start, dtype=np.float64)
    if V.shape != (G, D) or X.shape != (N, P) or start.shape != (N, K):
        raise ValueError(f"{what}: V is {V.shape}, X {X.shape}, psi_start {start.shape}; expected ({G}, {D}), ({N}, {P}), ({N}, {K})")
    wrong = np.argwhere(~np.isfinite(E) | (E < 0))
    if wrong.size:
        raise ValueError(f"{what}: expected expression has a negative or non-finite entry (gene {wrong[0][0]}, clone {wrong[0][1]})")
    esum = E.sum(0)
    wrong = np.flatnonzero(~np.isfinite(esum) | (esum == 0))
    if wrong.size:
        raise ValueError(f"{what}: expected expression of clone {wrong[0]} sums to {esum[wrong[0]]} over the genes")
    for name, M, row, colname in (("V", V, "gene", "factor"), ("psi_start", start, "cell", "factor"), ("X", X, "cell", "covariate")):
        if M.size and not np.isfinite(M).all():
            r, d = np.argwhere(~np.isfinite(M))[0]
            raise ValueError(f"{what}: {name} has a non-finite entry ({row} {r}, {colname} {d})")
    NH = K * (K + 1) // 2
    tri = [(k, l) for k in range(K) for l in range(k, K)]
    out = {"evidence": np.empty((N, C)), "laplace": np.empty((N, C)), "psi_mode": np.zeros((N, C, K)), "psi_prec": np.zeros((N, C, NH)),
           "rounds": np.zeros((N, C), dtype=np.int32), "converged": np.zeros((N, C), dtype=bool)}
    if K == 0:                                                       # nothing to integrate: clone_loglik's value
        ll = _clone_loglik_host(Y, E, X if P > 0 else None, V if P > 0 else None, const=const)
        out["evidence"][:], out["laplace"][:] = ll, ll
        out["converged"][:] = ~np.isneginf(ll)
        return out
    zero = E == 0
    logE = np.log(np.where(zero, 1.0, E))                            # xlogy: 0 where E = 0, put right below
    W, beta = V[:, :K], V[:, K:]
    Et = np.ascontiguousarray(E.T)
    step = int(chunk) if chunk is not None else max(1, 4_000_000 // max(1, C * G))
    for lo, Yc, _eta, _m, _logz in _cell_chunks(Y, step, order="C"):   # (one memory order: the products below sum the same way)
        n = Yc.shape[0]
        s = Yc.sum(1)
        A = Yc @ logE                                                # the sweep: A, B, s and the constant
        if zero.any():
            A[((Yc > 0).astype(np.float64) @ zero.astype(np.float64)) > 0] = -np.inf
        if const:
            A += (gammaln(s + 1.0) - gammaln(Yc + 1.0).sum(1))[:, None]
        B = Yc @ V
        xB = (X[lo:lo + n] * B[:, K:]).sum(1)
        xbeta = X[lo:lo + n] @ beta.T                                # [n, G]: the covariates' part of the exponent, once per (cell, gene)
        ni, ci = np.repeat(np.arange(n), C), np.tile(np.arange(C), n)   # the pairs, cell-major
        Ap, sp = A[ni, ci], s[ni]
        psi = start[lo:lo + n][ni].copy()
        dead = np.isneginf(Ap)
        frozen = dead.copy()
        rounds = np.zeros(n * C, dtype=np.int32)
        conv = np.zeros(n * C, dtype=bool)
        fstar = np.full(n * C, -np.inf)
        H = np.zeros((n * C, K, K)) + np.eye(K)

        def moments(i, ps, full):
            """m, Z0 (and mean, cov) of the pairs i at their psi ``ps``"""
            eta = xbeta[ni[i]].copy() if P > 0 else np.zeros((i.size, G))
            for k in range(K):
                eta += ps[:, k, None] * W[None, :, k]
            m = eta.max(1)
            wE = np.exp(eta - m[:, None]) * Et[ci[i]]
            Z0 = wE.sum(1)
            if not full:
                return m, Z0, None, None
            mean = np.empty((i.size, K))
            cov = np.empty((i.size, K, K))
            for k in range(K):
                wk = wE * W[:, k]
                mean[:, k] = wk.sum(1) / Z0
                for l in range(k, K):
                    cov[:, k, l] = cov[:, l, k] = (wk * W[:, l]).sum(1) / Z0
            cov -= mean[:, :, None] * mean[:, None, :]
            return m, Z0, mean, cov

        def fval(i, ps, m, Z0):
            with np.errstate(divide="ignore", invalid="ignore"):
                return Ap[i] + ((ps * B[ni[i], :K]).sum(1) + xB[ni[i]]) - np.where(sp[i] > 0, sp[i] * (m + np.log(Z0)), 0.0) - 0.5 * (ps ** 2).sum(1)

        def newton(i):
            m, Z0, mean, cov = moments(i, psi[i], True)
            f = fval(i, psi[i], m, Z0)
            g = B[ni[i], :K] - sp[i, None] * mean - psi[i]
            Hi = np.eye(K)[None] + sp[i, None, None] * cov
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                if K == 1:
                    d = g / Hi[:, 0]
                elif K == 2:                                         # the closed form the device uses
                    det = Hi[:, 0, 0] * Hi[:, 1, 1] - Hi[:, 0, 1] * Hi[:, 0, 1]
                    d = np.stack([(Hi[:, 1, 1] * g[:, 0] - Hi[:, 0, 1] * g[:, 1]) / det, (Hi[:, 0, 0] * g[:, 1] - Hi[:, 0, 1] * g[:, 0]) / det], axis=1)
                else:
                    d = np.linalg.solve(Hi, g[:, :, None])[:, :, 0]
            return f, Hi, d

        for t in range(int(max_iter)):
            i = np.flatnonzero(~frozen)
            if i.size == 0:
                break
            f, Hi, d = newton(i)
            dmax = np.abs(d).max(1)
            nan = ~(dmax < np.inf)                                   # a step that is no number: the pair stops where it is, not converged
            stop = nan | (dmax <= tol)
            j = i[stop]
            frozen[j], rounds[j], conv[j], fstar[j], H[j] = True, t + 1, (dmax <= tol)[stop], f[stop], Hi[stop]
            go = ~stop
            sc = np.where(dmax[go] > max_step, max_step / dmax[go], 1.0)
            psi[i[go]] += d[go] * sc[:, None]
        i = np.flatnonzero(~frozen)
        if i.size:                                                   # the pairs that never froze: f and H at the psi they hold
            f, Hi, _d = newton(i)
            frozen[i], rounds[i], fstar[i], H[i] = True, int(max_iter), f, Hi
        a = np.flatnonzero(~dead)
        lap = np.full(n * C, -np.inf)
        ev = np.full(n * C, -np.inf)
        if a.size:
            Ha = H[a]
            if K == 1:
                Lc = np.sqrt(Ha)
            elif K == 2:                                             # the closed form the device uses
                l00 = np.sqrt(Ha[:, 0, 0])
                l10 = Ha[:, 0, 1] / l00
                l11 = np.sqrt(Ha[:, 1, 1] - l10 * l10)
                Lc = np.zeros_like(Ha)
                Lc[:, 0, 0], Lc[:, 1, 0], Lc[:, 1, 1] = l00, l10, l11
            else:
                Lc = np.linalg.cholesky(Ha)
            hld = np.zeros(a.size)
            for k in range(K):
                hld = hld + np.log(Lc[:, k, k])
            lap[a] = fstar[a] - hld
            M = np.full(a.size, -np.inf)
            S = np.zeros(a.size)
            for q in range(Q):                                       # psi_q = psi* + L^-T z_q; the sum under a running maximum, q ascending
                z = nd[q]
                if K == 1:
                    y = (z[0] / Lc[:, 0, 0])[:, None]
                elif K == 2:
                    y1 = z[1] / Lc[:, 1, 1]
                    y = np.stack([(z[0] - Lc[:, 1, 0] * y1) / Lc[:, 0, 0], y1], axis=1)
                else:
                    y = np.linalg.solve(np.swapaxes(Lc, 1, 2), np.broadcast_to(z, (a.size, K))[:, :, None])[:, :, 0]
                pq = psi[a] + y
                m, Z0, _m, _c = moments(a, pq, False)
                tq = fval(a, pq, m, Z0) - fstar[a] + 0.5 * float((z * z).sum())
                with np.errstate(invalid="ignore"):
                    up = tq > M
                    S = np.where(up, S * np.exp(np.where(up, M - tq, 0.0)), S)
                    M = np.where(up, tq, M)
                    S = S + wt[q] * np.exp(tq - M)
            ev[a] = lap[a] + (M + np.log(S))
        sl = slice(lo, lo + n)
        out["evidence"][sl], out["laplace"][sl] = ev.reshape(n, C), lap.reshape(n, C)
        out["psi_mode"][sl] = psi.reshape(n, C, K)
        out["psi_prec"][sl] = np.stack([H[:, k, l] for k, l in tri], axis=1).reshape(n, C, NH)
        out["rounds"][sl], out["converged"][sl] = rounds.reshape(n, C), conv.reshape(n, C)
    return out


def _prec_to_cov(prec, K):
    """[N, C, K, K] inverse of the precision matrices given by their entries k <= l [N, C, K (K + 1) / 2]."""
    N, C = prec.shape[:2]
    H = np.zeros((N, C, K, K))
    for j, (k, l) in enumerate([(k, l) for k in range(K) for l in range(k, K)]):
        H[:, :, k, l] = H[:, :, l, k] = prec[:, :, j]
    return np.linalg.inv(H) if K else H


def _clone_evidence_on(engine, fit, Y, Lm, n_nodes, x, psi_start, saturate, saturation_threshold, const, max_iter, tol, max_step):
    """``clone_evidence`` of one fit on a live engine (or the host form for an engine without the method)."""
    N = Y.shape[0]
    t = _fit_tables(fit, Lm, N, x, None, saturate, saturation_threshold, free_psi=True)
    E, K, P, X = t.E, t.K, t.P, t.x
    if psi_start is not None:
        psi_start = np.asarray(psi_start, dtype=np.float64)
        if psi_start.size != N * K:
            raise ValueError(f"psi_start has {psi_start.size} entries but Y has {N} rows (cells) and the fit K = {K}")
        psi_start = psi_start.reshape(N, K)
    per_axis = int(n_nodes) if n_nodes is not None else (8 if K <= 1 else 5)
    nodes, weights = gauss_hermite_rule(K, per_axis)
    V = np.concatenate([t.W, t.beta], axis=1) if K + P > 0 else None
    if hasattr(engine, "clone_evidence"):
        if K > 2:
            raise ValueError(f"the fit has K = {K} latent factors; the device form of clone_evidence takes K <= 2")
        r = engine.clone_evidence(E, V, K, X=X, psi_start=psi_start, nodes=nodes, weights=weights, const=const, max_iter=max_iter, tol=tol,
                                  max_step=max_step)
    else:
        r = _clone_evidence_host(Y, E, V, K, P, X, psi_start, nodes, weights, const, max_iter, tol, max_step)
    r = dict(r)
    r["psi_cov"] = _prec_to_cov(r.pop("psi_prec"), K)
    return r


def clone_evidence(fit, Y, L, *, n_nodes=None, x=None, psi_start=None, saturate=True, saturation_threshold=6, const=True, max_iter=50, tol=1e-9,
                   max_step=1.0, engine=None, engine_opts=None):
    """The EVIDENCE of the cells of ``Y`` under every clone of a fitted model, with the cell's latent factor integrated out:
    ``evidence[n, c] = log Integral Normal(psi; 0, I) Multinomial(y_n | clone c, psi) dpsi`` under the fit's gene-level parameters.  Unlike the value at
    the MAP ``psi`` (``project_cells``: a maximum over ``psi``, which a fit with more factors never loses) this can be compared between fits on held-out
    cells, so it chooses the number of factors ``K`` (``heldout_evidence``); it also gives each cell's posterior uncertainty in ``psi``.  On easy data the
    clone calls barely move against ``project_cells`` -- the value of this is model choice and uncertainty, not new calls.

    Per (cell, clone): the mode of the integrand by safeguarded Newton from ``psi_start`` (default 0), the Laplace value, and a Gauss-Hermite tensor rule
    of ``n_nodes`` points per axis (default 8 for K <= 1, 5 for K = 2; at most 64 nodes in all) centred at the mode and scaled by the Cholesky factor of the
    precision (include/clonealign_hip.h states the algorithm).  Other keywords as for ``project_cells``.  One float64 sweep over the matrix on the
    device, then launches that do not read it (``HipEngine.clone_evidence``, ``K <= 2``); an engine without the method gets the float64 host form.

    Returns a dict: ``evidence`` and ``laplace`` [cells, clones], ``psi_mode`` [cells, clones, K], ``psi_cov`` [cells, clones, K, K] (the inverse
    precision at the mode: the Laplace covariance), ``rounds`` and ``converged`` [cells, clones].  A pair with ``converged`` False (``max_iter`` reached)
    holds a value that is deterministic but NOT to be trusted."""
    Yc, Lm, _cn, _N, _G = _cells_and_cnv(Y, L)
    with _engine_lease(engine, "clone_evidence", Yc, hostprep.saturate(Lm, saturation_threshold) if saturate else Lm, engine_opts) as eng:
        return _clone_evidence_on(eng, fit, Yc, Lm, n_nodes, x, psi_start, saturate, saturation_threshold, const, max_iter, tol, max_step)


def _marginal_from_evidence(fit, r, L, extra_loglik, clone_assignment_probability):
    """``assign_cells_marginal``'s result from ``clone_evidence``'s."""
    out = _assign_from_loglik(fit, r["evidence"], L, extra_loglik, clone_assignment_probability)
    probs = out["clone_probs"]
    g = np.where(np.isfinite(probs), probs, 0.0)
    mode, cov = r["psi_mode"], r["psi_cov"]
    K = mode.shape[2]
    psi = np.einsum("nc,nck->nk", g, mode)                           # the mixture of Laplace Gaussians: its mean and its marginal standard deviations
    second = np.einsum("nc,nck->nk", g, np.einsum("nckk->nck", cov) + mode ** 2) if K else np.zeros_like(psi)
    sd = np.sqrt(np.maximum(second - psi ** 2, 0.0))
    out.update(laplace_loglik=r["laplace"], clone_evidence=r["evidence"], psi=psi, psi_sd=sd,
               converged=(r["converged"] | ~(g > 1e-12)).all(1) & np.isfinite(out["loglik"]), rounds=r["rounds"])
    out["ml_params"] = {"psi": psi, "clone_probs": probs}
    return out


def assign_cells_marginal(fit, Y, L, clone_assignment_probability=0.95, *, extra_loglik=None, n_nodes=None, x=None, psi_start=None, saturate=True,
                          saturation_threshold=6, const=True, max_iter=50, tol=1e-9, max_step=1.0, engine=None, engine_opts=None):
    """``assign_cells`` with the cell's latent factor INTEGRATED OUT clone by clone: ``clone_probs = softmax_c(evidence + log alpha + extra_loglik)`` with
    ``clone_evidence``'s value (same keywords), so that every clone is judged at its own best ``psi`` and with its own volume, not at one ``psi`` shared
    by all clones (``project_cells``) or at ``psi = 0`` (``assign_cells``).  On easy data the calls barely move; what is new is ``loglik`` -- the cell's
    evidence, comparable between fits (``heldout_evidence``) -- and the uncertainty of ``psi``.

    Returns a :class:`ClonealignFit` with ``clone_probs``, ``clone``, ``loglik`` [cells] (the logsumexp of the same sum), ``clone_loglik`` and
    ``clone_evidence`` [cells, clones] (the evidence), ``laplace_loglik``, ``psi`` [cells, K] (the posterior-weighted mean of the clones' modes),
    ``psi_sd`` [cells, K] (from the mixture of the clones' Laplace Gaussians), ``rounds`` [cells, clones], ``converged`` [cells] (every clone with
    posterior above 1e-12 converged) and ``clone_names``; ``recompute_clone_assignment`` works on it."""
    r = clone_evidence(fit, Y, L, n_nodes=n_nodes, x=x, psi_start=psi_start, saturate=saturate, saturation_threshold=saturation_threshold, const=const,
                       max_iter=max_iter, tol=tol, max_step=max_step, engine=engine, engine_opts=engine_opts)
    return _marginal_from_evidence(fit, r, L, extra_loglik, clone_assignment_probability)


def heldout_evidence(fits, Y, L, *, x=None, extra_loglik=None, n_nodes=None, saturate=True, saturation_threshold=6, const=True, max_iter=50, tol=1e-9,
                     max_step=1.0, engine=None, engine_opts=None):
    """Compare fitted models on cells none of them saw: for every fit of ``fits`` (a dict name -> fit, or a list; the numbers of factors K may differ) the
    held-out evidence ``sum_n logsumexp_c(evidence_nc + log alpha_c + extra_loglik_nc)`` with ``clone_evidence``'s value (same keywords).  ONE engine and
    ONE upload of ``Y`` serve all fits.

    Returns a dict ``name -> {"total", "per_cell" [cells], "n_unconverged" (pairs), "delta" (total minus the best total, <= 0), "delta_se" (the paired
    standard error of that difference: sqrt(cells) times the standard deviation of the per-cell differences; 0 for the best fit)}`` plus ``"best"`` (the
    name with the largest total) and ``"ranking"`` (names, best first).  Cells that are impossible under every clone of some fit are left out of every sum."""
    items = list(fits.items()) if isinstance(fits, dict) else [(i, f) for i, f in enumerate(fits)]
    if not items:
        raise ValueError("heldout_evidence: no fit given")
    Yc, Lm, _cn, N, _G = _cells_and_cnv(Y, L)
    res = {}
    with _engine_lease(engine, "clone_evidence", Yc, hostprep.saturate(Lm, saturation_threshold) if saturate else Lm, engine_opts) as eng:
        for name, fit in items:
            r = _clone_evidence_on(eng, fit, Yc, Lm, n_nodes, x, None, saturate, saturation_threshold, const, max_iter, tol, max_step)
            cell = _lse_clones(r["evidence"] + _log_prior(fit, extra_loglik, N, r["evidence"].shape[1]))
            res[name] = {"per_cell": cell, "n_unconverged": int((~r["converged"] & np.isfinite(r["evidence"])).sum())}
    live = np.ones(N, dtype=bool)
    for v in res.values():
        live &= np.isfinite(v["per_cell"])
    for v in res.values():
        v["total"] = float(v["per_cell"][live].sum())
    ranking = sorted(res, key=lambda k: -res[k]["total"])
    best = ranking[0]
    for v in res.values():
        d = (v["per_cell"] - res[best]["per_cell"])[live]
        v["delta"] = float(d.sum())
        v["delta_se"] = float(np.sqrt(d.size) * d.std(ddof=1)) if d.size > 1 else 0.0
    res["best"], res["ranking"] = best, ranking
    return res


def _model_inputs_host(E, V, U, clone, total, what="simulate_counts"):
    """The arguments of the handle-free model calls as float64 / int64 arrays, with ``ca_simulate_counts``'s refusals about them as ValueError (``what``
    names the call).  Returns ``(E, V, U, clone, total, N, G, C, D)``."""
    E = np.asarray(E, dtype=np.float64)
    if E.ndim != 2:
        raise ValueError(f"{what}: E is {E.shape}; expected (genes, clones)")
    G, C = E.shape
    clone = np.asarray(clone, dtype=np.int64).reshape(-1)
    N = clone.shape[0]
    total = np.array(np.broadcast_to(np.asarray(total, dtype=np.int64), (N,)))
    if (U is None) != (V is None):
        raise ValueError(f"{what}: U and V go together (both, or neither)")
    D = 0
    if U is not None:
        U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
        if U.ndim != 2 or V.ndim != 2 or U.shape[0] != N or V.shape[0] != G or U.shape[1] != V.shape[1]:
            raise ValueError(f"{what}: U is {U.shape} and V is {V.shape}; expected ({N}, D) and ({G}, D)")
        D = U.shape[1]
    if D > 8:
        raise ValueError(f"{what}: D = {D} is outside [0, 8]")
    wrong = np.argwhere(~np.isfinite(E) | (E < 0))
    if wrong.size:
        raise ValueError(f"{what}: E has a negative or non-finite entry (gene {wrong[0][0]}, clone {wrong[0][1]})")
    for name, M, row in (("V", V, "gene"), ("U", U, "cell")):
        if D > 0 and not np.isfinite(M).all():
            r, d = np.argwhere(~np.isfinite(M))[0]
            raise ValueError(f"{what}: {name} has a non-finite entry ({row} {r}, factor {d})")
    wrong = np.flatnonzero((clone < 0) | (clone >= C))
    if wrong.size:
        raise ValueError(f"{what}: clone[{wrong[0]}] = {clone[wrong[0]]} is outside [0, {C})")
    wrong = np.flatnonzero((total < 0) | (total > 2 ** 31 - 1))
    if wrong.size:
        raise ValueError(f"{what}: total[{wrong[0]}] = {total[wrong[0]]} is outside [0, 2^31 - 1]")
    wrong = np.flatnonzero((total > 0) & ~(E > 0).any(0)[clone])
    if wrong.size:
        raise ValueError(f"{what}: total[{wrong[0]}] = {total[wrong[0]]} but E is zero in every gene of the cell's clone {clone[wrong[0]]}")
    return E, V, U, clone, total, N, G, C, D


def _simulate_counts_host(E, V, U, clone, total, seed, draw=0, cell_offset=0, chunk=1 << 20, _cumsum=None):
    """Numpy float64 restatement of ``ca_simulate_counts`` (include/clonealign_hip.h states the sampler): rows ``y_n ~ Multinomial(total[n], p_n)`` with
    ``p_ng ~ E[g, clone[n]] exp(U[n] . V[g])``.  Per cell: ``eta`` summed factor by factor, the shift by its maximum over the genes with ``E > 0``,
    ``w = E exp(eta - m)``, the SEQUENTIAL ``np.cumsum``; per draw ``j`` the Philox4x32-10 block ``j >> 1`` of ``rng.philox4x32`` (key = the seed's halves,
    counter = ``(j >> 1, q lo, draw lo, draw bits 32..47 | (q >> 32) << 16)`` with ``q = cell_offset + n``; words (0, 1) for even ``j``, (2, 3) for odd),
    ``u = ((hi << 21 | lo >> 11) + 0.5) 2^-53``, ``t = min(u cum[-1], nextafter(cum[-1], 0))`` and ``np.searchsorted(cum, t, side="right")``.
    Returns ``(Y int32 [N, G], flagged int64 [N])``: ``flagged[n]`` counts the cell's draws whose ``t`` lies within ``1e-12 cum[-1]`` of a cumulative
    boundary next to it -- the only draws where another grouping of the float64 sums, or the last bit of ``exp``, may pick the neighbouring gene.
    ``chunk``: Philox blocks generated at a time.  Refusals are ``ca_simulate_counts``'s, as ValueError.  ``_cumsum``: another cumulative sum (tests)."""
    from .rng import philox4x32
    E, V, U, clone, total, N, G, C, D = _model_inputs_host(E, V, U, clone, total)
    seed, draw, cell_offset = int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw), int(cell_offset)
    if cell_offset < 0 or cell_offset + N > 2 ** 48 or not 0 <= draw < 2 ** 48:
        raise ValueError("simulate_counts: cell_offset + N must lie in [0, 2^48] and draw in [0, 2^48)")
    cumsum = np.cumsum if _cumsum is None else _cumsum
    key = (seed & 0xFFFFFFFF, seed >> 32)
    Y = np.zeros((N, G), dtype=np.int32)
    flagged = np.zeros(N, dtype=np.int64)
    nblk = (total + 1) // 2
    lo = 0
    while lo < N:                                                    # cells [lo, hi): about `chunk` Philox blocks, at least one cell
        hi = lo + max(1, int(np.searchsorted(np.cumsum(nblk[lo:]), int(chunk), side="right")))
        hi = min(hi, N)
        nb = nblk[lo:hi]
        first = np.concatenate([[0], np.cumsum(nb)])
        ctr = np.zeros((int(first[-1]), 4), dtype=np.uint32)
        q = np.repeat(np.arange(lo, hi, dtype=np.int64) + cell_offset, nb)
        ctr[:, 0] = np.arange(first[-1], dtype=np.int64) - np.repeat(first[:-1], nb)     # j >> 1
        ctr[:, 1] = q & 0xFFFFFFFF
        ctr[:, 2] = draw & 0xFFFFFFFF
        ctr[:, 3] = ((draw >> 32) & 0xFFFF) | ((q >> 32) << 16)
        r = philox4x32(ctr, key).astype(np.uint64)
        x = np.stack([(r[:, 1] << np.uint64(21)) | (r[:, 0] >> np.uint64(11)), (r[:, 3] << np.uint64(21)) | (r[:, 2] >> np.uint64(11))], axis=1)
        u_all = ((x.astype(np.float64) + 0.5) * 2.0 ** -53).reshape(-1)                  # draws 2b, 2b + 1 of every block, cell after cell
        for n in range(lo, hi):
            if total[n] == 0:
                continue
            e = E[:, clone[n]]
            if D > 0:
                eta = U[n, 0] * V[:, 0]
                for d in range(1, D):
                    eta = eta + U[n, d] * V[:, d]
                m = eta[e > 0].max()
                with np.errstate(over="ignore"):
                    w = np.where(e > 0, e * np.exp(np.where(e > 0, eta - m, 0.0)), 0.0)
            else:
                w = e
            cum = cumsum(w)
            u = u_all[2 * first[n - lo]:2 * first[n - lo] + total[n]]
            t = np.minimum(u * cum[-1], np.nextafter(cum[-1], 0.0))
            g = np.searchsorted(cum, t, side="right")
            Y[n] = np.bincount(g, minlength=G)
            tol = 1e-12 * cum[-1]
            near = (cum[g] - t <= tol) | ((g > 0) & (t - cum[np.maximum(g - 1, 0)] <= tol))
            flagged[n] = int(near.sum())
        lo = hi
    return Y, flagged


def simulate_counts(fit, L, *, n_cells=None, clones=None, total_counts=None, psi=None, x=None, seed=0, draw=0, saturate=True, saturation_threshold=6,
                    device=0, host=False):
    """Simulate a count matrix from a fitted model on the device: the model's generative direction, ``y_n ~ Multinomial(total_counts[n], p_n)`` with
    ``p_ng ~ mu_g L[g, z_n] exp(psi_n W_g^T + x_n beta_g^T)`` at the fit's point estimates (``engine.simulate_counts`` / ``ca_simulate_counts``;
    include/clonealign_hip.h states the sampler).  ``L`` [genes, clones] for the fit's retained genes, saturated as ``clone_loglik`` does.

    ``total_counts`` (required): a scalar or an array [cells] of library sizes; passing the OBSERVED row sums of a matrix gives posterior predictive
    replicates of it.  ``clones``: an array [cells] of clone names or indices; default: drawn from the fit's ``alpha`` (uniform without it) with
    ``numpy.random.Generator(PCG64(seed))``.  ``psi`` [cells, K]: default, for fits with ``K > 0``: ``Normal(0, 1)`` draws (the model's prior) from the
    same generator, after the clones.  ``x`` [cells, P]: the covariates, required exactly when the fit has ``beta``.  ``n_cells`` is needed only when no
    array gives the number of cells.  ``clones=fit["clone"], psi=fit["ml_params"]["psi"]`` replicates the fit's own cells; cells labelled
    "unassigned" have no clone to draw from and are refused (ValueError) -- subset them away first.
    ``seed`` and ``draw`` also key the counter-based stream of the draws: the same arguments give the same matrix bit for bit, another ``draw`` an
    independent replicate with the same row sums.  ``host=True`` runs the numpy restatement (``_simulate_counts_host``) instead of the device; there
    is no silent fallback otherwise.
    Returns a dict: ``counts`` int32 [cells, genes], ``clone`` (names), ``clone_index``, ``psi`` [cells, K] and ``total_counts`` as used."""
    Lm, cn = _parse_cnv(L)
    G, C = Lm.shape
    if total_counts is None:
        raise ValueError("total_counts is required: a scalar or one library size per cell (the observed row sums give posterior predictive replicates)")
    names = _clone_names(fit, cn, C)
    if len(names) != C:
        raise ValueError(f"fit has {len(names)} clone names but L has {C} columns (clones)")
    ml = fit["ml_params"]
    if np.asarray(ml["mu"]).size != G:
        raise ValueError(f"fit$ml_params$mu has length {np.asarray(ml['mu']).size} but L has {G} rows: simulate on the retained genes")
    K = 0 if ml.get("W") is None else int(np.asarray(ml["W"]).size // G)           # (_fit_tables checks the shapes)
    total = np.asarray(total_counts)
    sizes = {"n_cells": None if n_cells is None else int(n_cells), "clones": None if clones is None else int(np.asarray(clones, dtype=object).reshape(-1).shape[0]),
             "total_counts": int(total.reshape(-1).shape[0]) if total.ndim > 0 else None,
             "psi": None if psi is None or isinstance(psi, str) or K == 0 else int(np.asarray(psi).size // K),
             "x": None if x is None else int(np.asarray(x).shape[0])}
    given = {k: v for k, v in sizes.items() if v is not None}
    if not given:
        raise ValueError("the number of cells is not given: pass n_cells, or clones, psi, x or total_counts as an array")
    if len(set(given.values())) != 1:
        raise ValueError("the arguments disagree on the number of cells: " + ", ".join(f"{k} {v}" for k, v in given.items()))
    N = next(iter(given.values()))
    if not np.all(np.isfinite(total.astype(np.float64))) or np.any(total != np.floor(total)):
        raise ValueError("total_counts must be whole numbers")
    total = np.array(np.broadcast_to(total.astype(np.int64).reshape(-1) if total.ndim > 0 else total.astype(np.int64), (N,)))
    gen = np.random.Generator(np.random.PCG64(int(seed)))
    if clones is None:
        alpha = ml.get("alpha")
        p = np.full(C, 1.0 / C) if alpha is None else np.asarray(alpha, dtype=np.float64).reshape(-1)
        if p.shape[0] != C or not np.all(np.isfinite(p)) or np.any(p < 0) or p.sum() <= 0:
            raise ValueError(f"fit$ml_params$alpha must hold {C} non-negative clone prevalences")
        idx = gen.choice(C, size=N, p=p / p.sum()).astype(np.int32)
    else:
        cl = np.asarray(clones).reshape(-1)
        if cl.dtype.kind in "iu":
            if cl.size and (cl.min() < 0 or cl.max() >= C):
                raise ValueError(f"clone index outside [0, {C})")
            idx = cl.astype(np.int32)
        else:
            lut = {c: i for i, c in enumerate(names)}
            n_un = sum(1 for c in cl if c == "unassigned")
            if n_un:
                raise ValueError(f"{n_un} cells are \"unassigned\": they have no clone to simulate from; pass the assigned cells only")
            unknown = sorted({str(c) for c in cl if c not in lut})
            if unknown:
                raise ValueError("clone labels that are no column of L: " + ", ".join(unknown))
            idx = np.array([lut[c] for c in cl], dtype=np.int32)
    if K > 0 and psi is None:
        psi = gen.standard_normal((N, K))
    _Ls, E, U, V = _fit_tables(fit, Lm, N, x, psi if K > 0 else None, saturate, saturation_threshold, what="the simulation")[:4]
    psi_out = U[:, :K].copy() if K > 0 else np.zeros((N, 0))
    if host:
        counts, _flagged = _simulate_counts_host(E, V, U, idx, total, seed, draw)
    else:
        from . import engine as _engine
        counts = _engine.simulate_counts(E, V, U, idx, total, seed, draw, device=device)
    return {"counts": counts, "clone": np.asarray(names, dtype=object)[idx], "clone_index": idx, "psi": psi_out, "total_counts": total}


def predictive_fit_mse(fit, Y, L, n_rep=20, *, seed=0, model_mu=False, x=None, engine_opts=None):
    """Posterior predictive check of ``compute_ca_fit_mse``: the observed MSE of the fit's called clones beside the same statistic on ``n_rep`` count
    matrices simulated from the fitted model itself, which gives the number a scale.  Cells labelled "unassigned" are left out on both sides.  A replicate
    keeps the assigned cells' clones, their ``psi`` (``fit["ml_params"]["psi"]`` when the fit has ``K > 0``), their OBSERVED row sums and ``x``, and is
    drawn by ``simulate_counts(..., seed=seed, draw=r)`` for ``r = 0 .. n_rep - 1``; each one is uploaded and evaluated as the observed matrix is
    (``compute_ca_fit_mse`` -> ``HipEngine.fit_mse``; ``engine_opts`` go to the engines' constructor).  ``Y`` and ``L`` as for ``compute_ca_fit_mse``.
    Returns a dict: ``observed``, ``replicates`` [n_rep], ``z`` = (observed - mean(replicates)) / sd(replicates) (sample sd), and per gene
    ``observed_gene``, ``replicate_gene_mean``, ``replicate_gene_sd`` [genes].  A large positive ``z`` says the data are further from the fit than the
    fit's own data would be."""
    n_rep = int(n_rep)
    if n_rep < 2:
        raise ValueError("n_rep must be at least 2 (the replicates' spread is the scale)")
    Lm, cn = _parse_cnv(L)
    Ya = _counts_array(Y.values if hasattr(Y, "columns") and hasattr(Y, "values") else Y)
    N = Ya.shape[0]
    clones = np.asarray(fit["clone"], dtype=object).reshape(-1)
    if clones.shape[0] != N:
        raise ValueError(f"fit has {clones.shape[0]} clone labels but Y has {N} rows (cells)")
    used = np.flatnonzero(clones != "unassigned")
    if used.size == 0:
        raise ValueError("every cell is \"unassigned\": there is nothing to evaluate")
    obs, obs_gene = compute_ca_fit_mse(fit, Ya, L, model_mu=model_mu, drop_unassigned=True, per_gene=True, engine_opts=engine_opts)
    rows = np.asarray(Ya.sum(axis=1)).reshape(-1)[used]
    ml = fit["ml_params"]
    has_psi = ml.get("W") is not None and np.asarray(ml["W"]).size > 0
    psi = np.asarray(ml["psi"], dtype=np.float64).reshape(N, -1)[used] if has_psi else None
    xs = None
    if x is not None:
        xs = np.asarray(x, dtype=np.float64)
        xs = (xs.reshape(-1, 1) if xs.ndim == 1 else xs)[used]
    sub = {k: v for k, v in fit.items() if k != "clone"}
    sub["clone"] = clones[used]
    reps, rep_gene = np.empty(n_rep), np.empty((n_rep, Lm.shape[0]))
    for r in range(n_rep):
        sim = simulate_counts(fit, L, clones=clones[used], total_counts=rows, psi=psi, x=xs, seed=seed, draw=r)
        reps[r], rep_gene[r] = compute_ca_fit_mse(sub, sim["counts"], L, model_mu=model_mu, per_gene=True, engine_opts=engine_opts)
    sd = reps.std(ddof=1)
    return {"observed": float(obs), "replicates": reps, "z": float((obs - reps.mean()) / sd) if sd > 0 else float("nan"),
            "observed_gene": obs_gene, "replicate_gene_mean": rep_gene.mean(0), "replicate_gene_sd": rep_gene.std(0, ddof=1)}


def _predictive_stats_host(E, V, U, clone, total, seed, draw0=0, n_rep=1, cell_offset=0, gene_totals=True, chunk=2048):
    """Numpy float64 restatement of ``ca_predictive_stats`` (include/clonealign_hip.h states the outputs): replicate ``r`` is the matrix
    ``_simulate_counts_host(..., seed, draw=draw0 + r, cell_offset)`` returns; ``ll_rep[n, r] = gammaln(total_n + 1) - sum_g gammaln(y_g + 1) +
    sum over y_g > 0 of y_g (log E[g, c_n] + eta_g - m - log Z_n)`` with ``m`` the largest ``eta`` over the genes with ``E > 0`` and ``Z_n = sum_g E
    exp(eta_g - m)`` (a sequential sum here); ``T_rep[r, g, c]`` = the rows of the cells of clone ``c`` summed.  ``total_n = 0`` gives exactly 0.
    Returns ``(ll_rep float64 [N, n_rep], T_rep int64 [n_rep, G, C] or None)``.  Refusals are ``ca_predictive_stats``'s, as ValueError."""
    from scipy.special import gammaln
    n_rep, draw0 = int(n_rep), int(draw0)
    if n_rep < 1:
        raise ValueError(f"predictive_stats: n_rep = {n_rep} is below 1")
    if draw0 < 0 or draw0 + n_rep > 2 ** 48:
        raise ValueError(f"predictive_stats: draw0 = {draw0} with n_rep = {n_rep}: draw0 + n_rep must lie in [0, 2^48]")
    rows = [_simulate_counts_host(E, V, U, clone, total, seed, draw0 + r, cell_offset)[0] for r in range(n_rep)]   # (also: every refusal on the inputs)
    E = np.asarray(E, dtype=np.float64)
    G, C = E.shape
    clone = np.asarray(clone, dtype=np.int64).reshape(-1)
    N = clone.shape[0]
    total = np.array(np.broadcast_to(np.asarray(total, dtype=np.int64), (N,)))
    ll = np.zeros((N, n_rep))
    for lo in range(0, N, int(chunk)):
        sl = slice(lo, min(lo + int(chunk), N))
        e = E[:, clone[sl]].T                                        # [cells, G]
        pos = e > 0
        eta = np.zeros(e.shape)
        if U is not None:
            Uc, Vm = np.asarray(U, dtype=np.float64)[sl], np.asarray(V, dtype=np.float64)
            for d in range(Uc.shape[1]):
                eta = eta + Uc[:, d:d + 1] * Vm[None, :, d]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            m = np.where(pos, eta, -np.inf).max(1, keepdims=True)
            x = np.where(pos, eta - m, 0.0)
            lw = np.where(pos, np.log(np.where(pos, e, 1.0)) + x, 0.0)
            log_z = np.log(np.where(pos, e * np.exp(x), 0.0).sum(1))
        live = total[sl] > 0                                         # (a cell without counts: exactly 0, whatever its clone)
        for r in range(n_rep):
            y = rows[r][sl].astype(np.float64)
            with np.errstate(invalid="ignore"):
                v = gammaln(total[sl] + 1.0) - gammaln(y + 1.0).sum(1) + (y * lw).sum(1) - total[sl] * log_z
            ll[sl, r] = np.where(live, v, 0.0)
    T = None
    if gene_totals:
        T = np.zeros((n_rep, G, C), dtype=np.int64)
        for r in range(n_rep):
            np.add.at(T[r].T, clone, rows[r])
    return ll, T


_PredictiveInputs = namedtuple("_PredictiveInputs", "Y L Ls E U V idx used rows Uu N G")


def _predictive_inputs(fit, Y, L, x, saturate, saturation_threshold):
    """What ``predictive_check`` and ``predictive_moments`` make of their arguments, with their refusals: the count matrix and the parsed ``L``, the fit's
    tables (``Ls``: ``L`` saturated as asked; ``E``, ``U``, ``V`` for all cells), the clone index per cell (-1: "unassigned"), the cells used, their observed
    row sums and their rows of ``U``."""
    Ya, Lm, cn, N, G = _cells_and_cnv(Y, L)
    names = _clone_names(fit, cn, Lm.shape[1])
    if len(names) != Lm.shape[1]:
        raise ValueError(f"fit has {len(names)} clone names but L has {Lm.shape[1]} columns (clones)")
    clones = np.asarray(fit["clone"], dtype=object).reshape(-1)
    if clones.shape[0] != N:
        raise ValueError(f"fit has {clones.shape[0]} clone labels but Y has {N} rows (cells)")
    lut = {c: i for i, c in enumerate(names)}
    unknown = sorted({str(c) for c in clones if c not in lut and c != "unassigned"})
    if unknown:
        raise ValueError("clone labels that are no column of L: " + ", ".join(unknown))
    idx = np.array([lut.get(c, -1) for c in clones], dtype=np.int32)
    used = np.flatnonzero(idx >= 0)
    if used.size == 0:
        raise ValueError("every cell is \"unassigned\": there is nothing to evaluate")
    ml = fit["ml_params"]
    has_psi = ml.get("W") is not None and np.asarray(ml["W"]).size > 0
    Ls, E, U, V = _fit_tables(fit, Lm, N, x, "fit" if has_psi else None, saturate, saturation_threshold)[:4]
    rows = np.asarray(Ya.sum(axis=1)).reshape(-1)
    if np.any(rows != np.floor(rows)):
        raise ValueError("Y must hold whole numbers: a replicate keeps the observed row sums")
    rows = rows.astype(np.int64)[used]
    Uu = None if U is None else U[used]
    return _PredictiveInputs(Ya, Lm, Ls, E, U, V, idx, used, rows, Uu, N, G)


def predictive_check(fit, Y, L, n_rep=50, *, seed=0, x=None, saturate=True, saturation_threshold=6, gene_totals=True, engine_opts=None, host=False):
    """Posterior predictive check of a fit on the model's own scale, per cell and per (gene, clone): the multinomial log-likelihood of every assigned
    cell at its called clone, and the per-clone pseudo-bulk totals, beside the same statistics of ``n_rep`` count matrices drawn from the fitted model.
    The replicates are drawn AND reduced on the device (``engine.predictive_stats`` / ``ca_predictive_stats``): no replicate matrix is stored, copied
    or uploaded.  Cells labelled "unassigned" are left out on both sides (all of them: ValueError); ``n_rep`` is at least 2.

    ``Y`` [cells, genes] and ``L`` [genes, clones] as for ``clone_loglik``; the cells are the fit's own (``fit["clone"]``, ``fit["ml_params"]["psi"]``
    when the fit has ``K > 0``, ``x`` exactly when it has ``beta``).  Observed side, one engine with ``Y`` resident (``engine_opts`` go to its
    constructor): ``ll_observed[n] = clone_loglik(...)[n, called clone]`` with ``const=True``, ``T_observed`` from ``clone_gene_sums``.  A replicate
    keeps the used cells' clones, ``psi``, ``x`` and OBSERVED row sums; replicate ``r`` is the matrix ``predictive_fit_mse(seed=seed)`` evaluates as
    its replicate ``r`` (``seed``, ``draw = r``).  ``host=True`` runs the numpy restatements on both sides instead of the device; there is no silent
    fallback otherwise.

    Returns a dict.  ``cells``: the indices used.  Per used cell: ``ll_observed``, ``ll_replicate_mean``, ``ll_replicate_sd`` (sample sd),
    ``z_cell`` = (observed - mean) / sd (NaN where the sd is 0: a cell without counts), ``p_cell`` = (1 + #{r: ll_rep <= ll_obs}) / (n_rep + 1).
    Over all used cells: ``ll_total_observed``, ``ll_total_replicates`` [n_rep], ``z``.  With ``gene_totals``: ``T_observed``,
    ``T_replicate_mean``, ``T_replicate_sd``, ``z_gene_clone`` [genes, clones] (NaN where the sd is 0) and ``p_gene_clone`` = min(1, 2 min(p_low,
    p_high)) with the same +1 rule on both tails.

    What the numbers mean: a very negative ``z_cell`` (``p_cell`` at its floor 1 / (n_rep + 1)) is a cell the fitted model explains worse than it
    explains its own data -- a cell of a clone absent from the copy-number data, a doublet, a contaminating normal cell --, also when every clone fits
    it badly and the posterior probabilities say nothing.  A large ``|z_gene_clone|`` is a gene that departs from the dosage model in that clone.
    What they do not mean: the clone and ``psi`` were chosen to fit the observed cell, so the observed side is favoured and the check is conservative;
    and real counts are overdispersed against a multinomial, so on real data ``z_cell`` is a ranking on a depth-aware scale, not a calibrated test."""
    n_rep = int(n_rep)
    if n_rep < 2:
        raise ValueError("n_rep must be at least 2 (the replicates' spread is the scale)")
    Ya, Lm, Ls, E, U, V, idx, used, rows, Uu, N, G = _predictive_inputs(fit, Y, L, x, saturate, saturation_threshold)
    if host:
        ll_all = _clone_loglik_host(Ya, E, U, V, const=True)
        T_obs = None
        if gene_totals:
            T_obs = np.zeros((G, Lm.shape[1]))
            dense = Ya[used].toarray() if _is_sparse(Ya) else np.asarray(Ya)[used]
            np.add.at(T_obs.T, idx[used], dense.astype(np.float64))
        ll_rep, T_rep = _predictive_stats_host(E, V, Uu, idx[used], rows, seed, 0, n_rep, gene_totals=gene_totals)
    else:
        from . import engine as _engine
        opts = dict(engine_opts or {})
        eng = _engine.HipEngine(Ya, Ls, np.zeros((N, 0)), None, 0, **opts)
        try:
            ll_all = eng.clone_loglik(E, U, V, const=True)
            T_obs = np.ascontiguousarray(eng.clone_gene_sums(idx)[0]) if gene_totals else None
        finally:
            eng.close()
        ll_rep, T_rep = _engine.predictive_stats(E, V, Uu, idx[used], rows, seed, 0, n_rep, device=int(opts.get("device", 0)), gene_totals=gene_totals)
    ll_obs = ll_all[used, idx[used]]
    mean, sd = ll_rep.mean(1), ll_rep.std(1, ddof=1)
    tot_rep = ll_rep.sum(0)
    tot_sd = tot_rep.std(ddof=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        z_cell = np.where(sd > 0, (ll_obs - mean) / sd, np.nan)
    out = {"cells": used, "ll_observed": ll_obs, "ll_replicate_mean": mean, "ll_replicate_sd": sd, "z_cell": z_cell,
           "p_cell": (1.0 + (ll_rep <= ll_obs[:, None]).sum(1)) / (n_rep + 1.0),
           "ll_total_observed": float(ll_obs.sum()), "ll_total_replicates": tot_rep,
           "z": float((ll_obs.sum() - tot_rep.mean()) / tot_sd) if tot_sd > 0 else float("nan")}
    if gene_totals:
        T_mean, T_sd = T_rep.mean(0), T_rep.std(0, ddof=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            z_gc = np.where(T_sd > 0, (T_obs - T_mean) / T_sd, np.nan)
        p_low = (1.0 + (T_rep <= T_obs[None]).sum(0)) / (n_rep + 1.0)
        p_high = (1.0 + (T_rep >= T_obs[None]).sum(0)) / (n_rep + 1.0)
        out.update({"T_observed": T_obs, "T_replicate_mean": T_mean, "T_replicate_sd": T_sd, "z_gene_clone": z_gc,
                    "p_gene_clone": np.minimum(1.0, 2.0 * np.minimum(p_low, p_high))})
    return out


def _predictive_moments_host(E, V, U, clone, total, chunk=2048):
    """Numpy float64 restatement of ``ca_predictive_moments`` (include/clonealign_hip.h states the outputs): per cell ``eta`` summed factor by factor, the
    shift ``m`` by its maximum over the genes with ``E > 0``, ``w = E exp(eta - m)``, ``Z = sum_g w``, ``p = w / Z``, ``lp = log E + (eta - m) - log Z`` (``log1p(-(the others' w) / Z)`` for a gene with ``p > 1/2``);
    ``cell_mean = total h`` with ``h = sum_g p lp``, ``cell_var = total sum_g p (lp - h)^2``; ``T_mean``, ``T_var``, ``T_cum3`` [G, C] = the sums over a
    clone's cells of ``total p``, ``total p (1 - p)`` and ``total p (1 - p)(1 - 2p)``.  A cell without counts gives exactly 0 and joins no sum.  ``chunk``
    cells at a time: no [cells, genes] array is larger.  Returns ``(cell_mean, cell_var, T_mean, T_var, T_cum3)``; refusals are
    ``ca_predictive_moments``'s, as ValueError."""
    E, V, U, clone, total, N, G, C, D = _model_inputs_host(E, V, U, clone, total, "predictive_moments")
    cell_mean, cell_var = np.zeros(N), np.zeros(N)
    T = np.zeros((3, G, C))
    for lo in range(0, N, int(chunk)):
        rows = lo + np.flatnonzero(total[lo:lo + int(chunk)] > 0)
        if rows.size == 0:
            continue
        e = E[:, clone[rows]].T                                      # [cells, G]
        pos = e > 0
        eta = np.zeros(e.shape)
        for d in range(D):
            eta = eta + U[rows, d:d + 1] * V[None, :, d]
        with np.errstate(over="ignore", invalid="ignore"):
            m = np.where(pos, eta, -np.inf).max(1, keepdims=True)
            x = np.where(pos, eta - m, 0.0)
            w = np.where(pos, e * np.exp(x), 0.0)
        top = w.argmax(1)[:, None]                                   # the largest w (the first such gene) goes last into the sum
        w_top = np.take_along_axis(w, top, 1)
        rest = w.copy()
        np.put_along_axis(rest, top, 0.0, 1)
        rest = rest.sum(1, keepdims=True)
        Z = rest + w_top
        p = w / Z
        lp = np.where(pos, np.log(np.where(pos, e, 1.0)) + x - np.log(Z), 0.0)
        big = w_top / Z > 0.5                                        # p > 1/2: the difference above cancels; log1p of the others' share does not
        np.put_along_axis(lp, top, np.where(big, np.log1p(-rest / Z), np.take_along_axis(lp, top, 1)), 1)
        h = (p * lp).sum(1, keepdims=True)
        t = total[rows].astype(np.float64)
        cell_mean[rows] = t * h[:, 0]
        cell_var[rows] = t * (p * (lp - h) ** 2).sum(1)
        tp = t[:, None] * p
        tpq = tp * (1.0 - p)
        for c in np.unique(clone[rows]):
            sel = clone[rows] == c
            T[0][:, c] += tp[sel].sum(0)
            T[1][:, c] += tpq[sel].sum(0)
            T[2][:, c] += (tpq[sel] * (1.0 - 2.0 * p[sel])).sum(0)
    return cell_mean, cell_var, T[0], T[1], T[2]


def refined_normal_cdf(t, mean, var, cum3):
    """``P(T <= t)`` for an integer-valued sum of independent terms with the given mean, variance and third cumulant, by the normal approximation with
    the continuity correction and the first Edgeworth (skewness) term: ``F(t) = Phi(x) - gamma (x^2 - 1) phi(x) / 6`` with ``x = (t + 0.5 - mean) / sd``
    and ``gamma = cum3 / sd^3``, clipped to [0, 1].  A variance of 0 is a point mass at ``mean``.  Arrays broadcast.  Against the exact distribution of
    a sum of binomials its absolute error is about 0.03 / variance (tests/test_predictive_moments_host.py), so it screens and ranks; it is no tail
    probability below about 1e-3."""
    from scipy.special import ndtr
    t, mean, var, cum3 = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (t, mean, var, cum3)))
    ok = var > 0
    sd = np.sqrt(np.where(ok, var, 1.0))
    x = (t + 0.5 - mean) / sd
    F = ndtr(x) - (cum3 / sd ** 3) * (x * x - 1.0) * np.exp(-0.5 * x * x) / (6.0 * np.sqrt(2.0 * np.pi))
    return np.where(ok, np.clip(F, 0.0, 1.0), (t >= mean).astype(np.float64))


def predictive_moments(fit, Y, L, *, x=None, saturate=True, saturation_threshold=6, engine_opts=None, host=False):
    """``predictive_check`` without the Monte Carlo where none is needed: given the called clones and the observed row sums -- what its replicates
    condition on -- a replicate row is one multinomial draw, so the per-clone totals ``T[g, c]`` are sums of independent binomials and the linear part
    of a row's log-likelihood is a linear statistic; their moments are sums over (cell, gene) of functions of ``p_ng``, taken in one pass on the device
    that reads no counts (``engine.predictive_moments`` / ``ca_predictive_moments``; include/clonealign_hip.h states them).

    Arguments, label checks and the treatment of "unassigned" cells are ``predictive_check``'s.  Observed side, one engine with ``Y`` resident
    (``engine_opts`` go to its constructor): ``stat_observed[n] = clone_loglik(const=False)[n, called clone]``, ``T_observed`` from
    ``clone_gene_sums``.  Expected side: the closed forms on the used cells with their observed row sums.  ``host=True`` runs the numpy restatements
    on both sides instead; there is no silent fallback otherwise.

    Returns a dict.  ``cells``: the indices used.  Per used cell: ``stat_observed``, ``stat_mean``, ``stat_var`` and ``z_cell`` = (observed - mean) /
    sd (NaN where the variance is 0: a cell without counts or with one possible gene; ``-inf`` where the observed value is: a count on a gene with
    copy number 0).  Per (gene, clone): ``T_observed``, ``T_mean``, ``T_var``, ``T_cum3``, ``z_gene_clone`` (NaN where ``T_var`` is 0), ``exposure`` =
    ``T_mean / E`` (the exact expected count per unit of ``mu L``; NaN where ``E = 0``) and ``p_gene_clone`` = min(1, 2 min(F(T), 1 - F(T - 1))) with
    ``F = refined_normal_cdf``.  Also ``L`` (as the fit used it, after ``saturate``) and ``clone_cells`` (used cells per clone), which
    ``dosage_response`` works from.

    What the numbers are: both ``z`` are exact under the model -- mean and sd are computed, nothing is sampled, so they carry no replicate noise and
    ``p_gene_clone`` has no floor at 1 / (n_rep + 1).  What they are not: the per-cell statistic is the likelihood's LINEAR part, ``sum_g y log p``,
    not ``predictive_check``'s full ``log_prob`` (the ``lgamma`` constant has no closed-form moments), so the two ``z_cell`` differ.  ``F``'s absolute
    error against the exact distribution is about 0.03 / variance (tests/test_predictive_moments_host.py), so ``p_gene_clone`` ranks and screens and
    is no tail probability below about 1e-3.  And, as for ``predictive_check``: the clones (and ``psi``) were chosen to fit the observed cells, so the
    observed side is favoured; and real counts are overdispersed against a multinomial, so on real data these are rankings on a depth-aware scale,
    not calibrated tests."""
    Ya, _Lm, Ls, E, U, V, idx, used, rows, Uu, N, G = _predictive_inputs(fit, Y, L, x, saturate, saturation_threshold)
    C = E.shape[1]
    if host:
        ll_all = _clone_loglik_host(Ya, E, U, V, const=False)
        T_obs = np.zeros((G, C))
        dense = Ya[used].toarray() if _is_sparse(Ya) else np.asarray(Ya)[used]
        np.add.at(T_obs.T, idx[used], dense.astype(np.float64))
        mean, var, T_mean, T_var, T_cum3 = _predictive_moments_host(E, V, Uu, idx[used], rows)
    else:
        from . import engine as _engine
        opts = dict(engine_opts or {})
        eng = _engine.HipEngine(Ya, Ls, np.zeros((N, 0)), None, 0, **opts)
        try:
            ll_all = eng.clone_loglik(E, U, V, const=False)
            T_obs = np.ascontiguousarray(eng.clone_gene_sums(idx)[0])
        finally:
            eng.close()
        mean, var, T_mean, T_var, T_cum3 = _engine.predictive_moments(E, V, Uu, idx[used], rows, device=int(opts.get("device", 0)))
    obs = ll_all[used, idx[used]]
    with np.errstate(divide="ignore", invalid="ignore"):
        z_cell = np.where(var > 0, (obs - mean) / np.sqrt(np.where(var > 0, var, 1.0)), np.nan)
        z_gc = np.where(T_var > 0, (T_obs - T_mean) / np.sqrt(np.where(T_var > 0, T_var, 1.0)), np.nan)
        exposure = np.where(E > 0, T_mean / np.where(E > 0, E, 1.0), np.nan)
    p_low, p_high = refined_normal_cdf(T_obs, T_mean, T_var, T_cum3), 1.0 - refined_normal_cdf(T_obs - 1.0, T_mean, T_var, T_cum3)
    return {"cells": used, "stat_observed": obs, "stat_mean": mean, "stat_var": var, "z_cell": z_cell,
            "T_observed": T_obs, "T_mean": T_mean, "T_var": T_var, "T_cum3": T_cum3, "z_gene_clone": z_gc, "exposure": exposure,
            "p_gene_clone": np.minimum(1.0, 2.0 * np.minimum(p_low, p_high)), "L": Ls, "clone_cells": np.bincount(idx[used], minlength=C).astype(np.int64)}


def _separability_inputs_host(E, V, U, what="clone_separability"):
    """The arguments of ``ca_clone_separability`` as float64 arrays with its refusals as ValueError.  Returns ``(E, V, U, N, G, C, D)``; without factors ``N = 1``."""
    E = np.asarray(E, dtype=np.float64)
    if E.ndim != 2:
        raise ValueError(f"{what}: E is {E.shape}; expected (genes, clones)")
    G, C = E.shape
    if C < 2 or G < 1:
        raise ValueError(f"{what}: G = {G}, C = {C}: G must be >= 1 and C >= 2")
    if (U is None) != (V is None):
        raise ValueError(f"{what}: U and V go together (both, or neither)")
    N, D = 1, 0
    if U is not None:
        U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
        if U.ndim != 2 or V.ndim != 2 or V.shape[0] != G or U.shape[1] != V.shape[1]:
            raise ValueError(f"{what}: U is {U.shape} and V is {V.shape}; expected (cells, D) and ({G}, D)")
        N, D = U.shape
    if D > 8:
        raise ValueError(f"{what}: D = {D} is outside [0, 8]")
    wrong = np.argwhere(~np.isfinite(E) | (E < 0))
    if wrong.size:
        raise ValueError(f"{what}: E has a negative or non-finite entry (gene {wrong[0][0]}, clone {wrong[0][1]})")
    with np.errstate(over="ignore"):
        s = E.sum(0)
    if (s == 0).any():
        raise ValueError(f"{what}: E is zero in every gene of clone {np.flatnonzero(s == 0)[0]}: its column sums to 0")
    if not np.isfinite(s).all():
        raise ValueError(f"{what}: E sums to a non-finite value in clone {np.flatnonzero(~np.isfinite(s))[0]}")
    for name, M, row in (("V", V, "gene"), ("U", U, "cell")):
        if D > 0 and not np.isfinite(M).all():
            r, d = np.argwhere(~np.isfinite(M))[0]
            raise ValueError(f"{what}: {name} has a non-finite entry ({row} {r}, factor {d})")
    if D == 0:
        U = V = None
    return E, V, U, N, G, C, D


def _clone_separability_host(E, V, U, chunk=256, with_scale=False):
    """Numpy float64 restatement of ``ca_clone_separability`` (include/clonealign_hip.h states the outputs) from the PER-GENE sums, no expanded form:
    ``e = E / E.sum(0)``; per cell ``eta`` summed factor by factor, the shift ``m`` its maximum over every gene, ``w = exp(eta - m)``, ``Z_c = sum_g e_gc w_g``,
    ``logZ = m + log Z``; per ordered pair ``p = e_a w / Z_a``, ``excl = sum_X p``, ``d = (log e_a - log e_b) - (log Z_a - log Z_b)`` on ``S`` and
    ``m_k = sum_S p d^k``.  ``Z_a = 0`` (underflow) gives ``logZ = -inf`` and zeros in every pair entry that involves ``a``.  ``chunk`` cells at a time.
    Without factors one row (N = 1).  Returns ``(logZ [N, C], excl, m1, m2, m3 [N, C, C])``; ``with_scale=True`` appends the three scales
    ``sum_S p (|delta| + |Delta|)^k`` [N, C, C] the device's parity bars are stated in.  Refusals are the library's, as ValueError."""
    E, V, U, N, G, C, D = _separability_inputs_host(E, V, U)
    e = E / E.sum(0)
    pos = e > 0
    with np.errstate(divide="ignore"):
        le = np.where(pos, np.log(np.where(pos, e, 1.0)), 0.0)
    logZ = np.zeros((N, C))
    out = np.zeros((4, N, C, C))
    scale = np.zeros((3, N, C, C))
    for lo in range(0, N, int(chunk)):
        hi = min(N, lo + int(chunk))
        eta = np.zeros((hi - lo, G))
        for d in range(D):
            eta = eta + U[lo:hi, d:d + 1] * V[None, :, d]
        m = eta.max(1, keepdims=True)
        w = np.exp(eta - m)
        Z = np.stack([(w * e[None, :, c]).sum(1) for c in range(C)], axis=1)   # [cells, C]; a column at a time, so equal columns of e give equal bits
        with np.errstate(divide="ignore"):
            lz = np.log(Z)
        logZ[lo:hi] = m + lz
        live = Z > 0
        for a in range(C):
            pa = np.where(live[:, a:a + 1], e[None, :, a] * w / np.where(live[:, a:a + 1], Z[:, a:a + 1], 1.0), 0.0)
            for b in range(C):
                if a == b:
                    continue
                both = live[:, a] & live[:, b]
                S, X = pos[:, a] & pos[:, b], pos[:, a] & ~pos[:, b]
                delta = le[S, a] - le[S, b]
                Delta = np.where(both, lz[:, a] - np.where(both, lz[:, b], 0.0), 0.0) if both.any() else np.zeros(hi - lo)
                Delta = np.where(both, Delta, 0.0)
                dd = delta[None, :] - Delta[:, None]
                pS = pa[:, S]
                out[0, lo:hi, a, b] = np.where(both, pa[:, X].sum(1), 0.0)
                sc = np.abs(delta)[None, :] + np.abs(Delta)[:, None]
                for k in (1, 2, 3):
                    out[k, lo:hi, a, b] = np.where(both, (pS * dd ** k).sum(1), 0.0)
                    scale[k - 1, lo:hi, a, b] = np.where(both, (pS * sc ** k).sum(1), 0.0)
    res = (logZ, out[0], out[1], out[2], out[3])
    return res + (scale[0], scale[1], scale[2]) if with_scale else res


def edgeworth_normal_cdf(t, mean, var, cum3=0.0):
    """``P(T <= t)`` for a CONTINUOUS-valued sum of independent terms with the given mean, variance and third cumulant: the normal approximation with the
    first Edgeworth (skewness) term and NO continuity correction (``refined_normal_cdf`` is the form for integer-valued sums): ``F(t) = Phi(x) - gamma
    (x^2 - 1) phi(x) / 6`` with ``x = (t - mean) / sd`` and ``gamma = cum3 / sd^3``, clipped to [0, 1].  A variance of 0 is a step at ``mean``.  Arrays broadcast."""
    from scipy.special import ndtr
    t, mean, var, cum3 = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (t, mean, var, cum3)))
    ok = var > 0
    sd = np.sqrt(np.where(ok, var, 1.0))
    x = (t - mean) / sd
    F = ndtr(x) - (cum3 / sd ** 3) * (x * x - 1.0) * np.exp(-0.5 * x * x) / (6.0 * np.sqrt(2.0 * np.pi))
    return np.where(ok, np.clip(F, 0.0, 1.0), (t >= mean).astype(np.float64))


def _per_read_cumulants(excl, m1, m2, m3):
    """``(q, kappa, v, c3)`` of the log-likelihood ratio per read GIVEN that the read excludes nobody: ``q = 1 - excl``, ``kappa = m1 / q``, ``v = max(m2 / q -
    kappa^2, 0)``, ``c3 = m3 / q - 3 kappa m2 / q + 2 kappa^3``; all 0 where ``q = 0`` (every read excludes the rival)."""
    q = 1.0 - excl
    ok = q > 0
    qs = np.where(ok, q, 1.0)
    kappa, s2, s3 = np.where(ok, m1 / qs, 0.0), np.where(ok, m2 / qs, 0.0), np.where(ok, m3 / qs, 0.0)
    return q, kappa, np.maximum(s2 - kappa * kappa, 0.0), s3 - 3.0 * kappa * s2 + 2.0 * kappa ** 3


def _p_confuse(t, q, kappa, v, c3, lp_diff=0.0, concentration=None):
    """The closed form behind ``clone_separability``: the probability that ``t`` reads of a row of clone ``a`` leave ``Lambda + lp_a - lp_b <= 0``: no read
    excludes ``b`` (``q^t``) and, given that, ``Lambda`` -- mean ``t kappa``, variance ``t v``, third cumulant ``t c3`` -- falls at or below ``-(lp_a - lp_b)``
    (``edgeworth_normal_cdf``).  ``concentration`` inflates the variance by ``(t + phi) / (1 + phi)`` and drops the skewness term.  Arrays broadcast."""
    t = np.asarray(t, dtype=np.float64)
    var, cum3 = t * v, t * c3
    if concentration is not None:
        var, cum3 = var * (t + concentration) / (1.0 + concentration), 0.0
    with np.errstate(invalid="ignore"):
        return np.power(q, t) * edgeworth_normal_cdf(0.0, t * kappa + lp_diff, var, cum3)


def clone_separability(fit, L, total_counts, *, psi=None, x=None, clones=None, log_prior=None, concentration=None, per_cell=False, saturate=True,
                       saturation_threshold=6, engine_opts=None, host=False):
    """Can expression tell the clones of a fitted model apart at a given read depth -- answered BEFORE any counts are scored, in closed form, by one pass on
    the device that reads no count matrix (``engine.clone_separability`` / ``ca_clone_separability``; include/clonealign_hip.h states its five outputs).

    For a row of ``t`` reads drawn from clone ``a``, the log-likelihood ratio against clone ``b``, ``Lambda = ll_a - ll_b``, is a linear statistic of one
    multinomial.  A read on a gene where ``b`` has copy number 0 rules ``b`` out; its per-read probability is ``excl``.  Given no such read, all ``t`` reads
    fall where both clones express, and ``Lambda`` has mean ``t kappa``, variance ``t v`` and third cumulant ``t c3`` with ``q = 1 - excl``, ``kappa = m1 / q``,
    ``v = max(m2 / q - kappa^2, 0)``, ``c3 = m3 / q - 3 kappa m2 / q + 2 kappa^3``.  The probability that the cell is NOT called ``a`` over ``b`` is then
    ``p_confuse[n, a, b] = q^t clip(Phi(z) - gamma (z^2 - 1) phi(z) / 6, 0, 1)`` with ``z = -(t kappa + lp_a - lp_b) / sqrt(t v)`` and ``gamma = c3 /
    (sqrt(t) v^1.5)`` (``edgeworth_normal_cdf``: no continuity correction, ``Lambda`` is not integer-valued; ``v = 0`` gives a step at the mean).

    ``L`` [genes, clones] for the fit's retained genes, saturated as ``clone_loglik`` does.  ``total_counts``: a scalar or one read depth per cell.
    ``psi``: None means the fit's own cells (``fit["ml_params"]["psi"]``), or an array [cells, K]; ``x`` [cells, P] exactly when the fit has ``beta``.  A fit
    without factors or covariates has one row for every cell.  ``clones`` [cells]: the cells' called clones (names or indices; "unassigned" joins no row
    mean).  ``log_prior`` [clones] or [cells, clones]: default equal priors.  ``concentration=phi``: a Dirichlet-multinomial overdispersion; the variance is
    inflated by ``(t + phi) / (1 + phi)``, the Dirichlet-multinomial covariance factor, and the skewness term is dropped -- an APPROXIMATION that leaves
    ``q^t`` multinomial.  The cells go through the engine in slices, so host memory stays bounded; ``host=True`` runs the numpy restatement
    (``_clone_separability_host``) instead; there is no silent fallback otherwise.

    Returns a dict.  [C, C], row = true clone, column = rival, diagonal 0: ``kl_per_read`` (mean over the cells of ``m1``: the drift of ``Lambda`` per read),
    ``excl_per_read``, ``var_per_read`` (mean of ``v``), ``drift_per_read`` (mean of ``kappa``), ``cum3_per_read``; ``confusion``: row ``a`` is the mean of
    ``p_confuse[:, a, :]`` over the cells of clone ``a`` when ``clones`` is given (NaN for a clone without cells), over all cells otherwise.  Per cell:
    ``p_error_cell`` = min(1, sum_b p_confuse[n, clone_n, b]) and ``worst_rival`` (NaN / -1 without a called clone, so also without ``clones``), ``logZ``
    [cells, C], ``total_counts``.  Also ``clone_names`` and ``concentration``.  ``per_cell=True`` adds ``excl``, ``m1``, ``m2``, ``m3`` and ``p_confuse``
    [cells, C, C].

    What the numbers are NOT: they hold under the model.  Real counts are overdispersed against a multinomial, so without ``concentration`` the confusion
    probabilities are LOWER bounds and ``reads_needed`` an optimistic depth; the pairwise events are combined by a union bound in ``p_error_cell``; and the
    Edgeworth form is no tail probability below about 1e-3."""
    Lm, cn = _parse_cnv(L)
    G, C = Lm.shape
    names = _clone_names(fit, cn, C)
    ml = fit["ml_params"]
    K = 0 if ml.get("W") is None else int(np.asarray(ml["W"]).size // max(G, 1))
    if K > 0 and psi is None:
        psi = "fit"
    total = np.asarray(total_counts, dtype=np.float64)
    if not np.all(np.isfinite(total)) or np.any(total < 0):
        raise ValueError("total_counts must be finite and non-negative")
    sizes = {"total_counts": int(total.reshape(-1).shape[0]) if total.ndim > 0 else None,
             "psi": None if K == 0 or psi is None else int(np.asarray(ml["psi"] if isinstance(psi, str) else psi).size // K),
             "x": None if x is None else int(np.asarray(x).shape[0]),
             "clones": None if clones is None else int(np.asarray(clones, dtype=object).reshape(-1).shape[0]),
             "log_prior": None if log_prior is None or np.ndim(log_prior) < 2 else int(np.shape(log_prior)[0])}
    given = {k: v for k, v in sizes.items() if v is not None}
    if len(set(given.values())) > 1:
        raise ValueError("the arguments disagree on the number of cells: " + ", ".join(f"{k} {v}" for k, v in given.items()))
    N = next(iter(given.values())) if given else 1
    t = _fit_tables(fit, Lm, N, x, psi if K > 0 else None, saturate, saturation_threshold, what="the separability call")
    total = np.array(np.broadcast_to(total.reshape(-1) if total.ndim > 0 else total, (N,)))
    lp = np.zeros((1, C)) if log_prior is None else np.asarray(log_prior, dtype=np.float64).reshape(-1, C)
    if lp.shape[0] not in (1, N):
        raise ValueError(f"log_prior is {np.shape(log_prior)}; expected ({C},) or ({N}, {C})")
    if concentration is not None and not (np.isfinite(concentration) and concentration > 0):
        raise ValueError("concentration must be a positive number")
    idx = None
    if clones is not None:
        cl = np.asarray(clones).reshape(-1)
        if cl.dtype.kind in "iu":
            idx = cl.astype(np.int64)
        else:
            lut = {c: i for i, c in enumerate(names)}
            unknown = sorted({str(c) for c in cl if c not in lut and c != "unassigned"})
            if unknown:
                raise ValueError("clone labels that are no column of L: " + ", ".join(unknown))
            idx = np.array([lut.get(c, -1) for c in cl], dtype=np.int64)
        if idx.size and (idx.min() < -1 or idx.max() >= C):
            raise ValueError(f"clone index outside [0, {C})")
    device = int(dict(engine_opts or {}).get("device", 0))
    if not host:
        from . import engine as _engine
    step = max(1, (1 << 21) // (C * C))                              # four [cells, C, C] float64 arrays of 16 MB a slice
    sums = np.zeros((6, C, C))                                       # m1, excl, v, kappa, c3, p_confuse over the cells that count for a row
    cnt = np.zeros(C)
    logZ = np.zeros((N, C))
    p_err, rival = np.full(N, np.nan), np.full(N, -1, dtype=np.int64)
    keep = [[] for _ in range(5)] if per_cell else None
    off = ~np.eye(C, dtype=bool)
    for lo in range(0, N, step):
        hi = min(N, lo + step)
        if t.U is None:
            raw = _clone_separability_host(t.E, None, None) if host else _engine.clone_separability(t.E, None, None, device=device)
            raw = tuple(np.broadcast_to(a, (hi - lo,) + a.shape[1:]) for a in raw)
        else:
            raw = _clone_separability_host(t.E, t.V, t.U[lo:hi]) if host else _engine.clone_separability(t.E, t.V, t.U[lo:hi], device=device)
        lz, ex, a1, a2, a3 = raw
        logZ[lo:hi] = lz
        q, kappa, v, c3 = _per_read_cumulants(ex, a1, a2, a3)
        lps = lp if lp.shape[0] == 1 else lp[lo:hi]
        with np.errstate(invalid="ignore"):
            lpd = np.where(off[None], lps[:, :, None] - lps[:, None, :], 0.0)
        pc = np.where(off[None], _p_confuse(total[lo:hi, None, None], q, kappa, v, c3, lpd, concentration), 0.0)
        if idx is None:
            w = np.ones((hi - lo, C))
        else:
            w = np.zeros((hi - lo, C))
            called = np.flatnonzero(idx[lo:hi] >= 0)
            w[called, idx[lo:hi][called]] = 1.0
            row = pc[called, idx[lo:hi][called]]                     # [called, C]
            p_err[lo + called] = np.minimum(1.0, row.sum(1))
            rival[lo + called] = row.argmax(1)
        for k, a in enumerate((a1, ex, v, kappa, c3, pc)):
            sums[k] += np.einsum("na,nab->ab", w, a)
        cnt += w.sum(0)
        if per_cell:
            for k, a in enumerate((ex, a1, a2, a3, pc)):
                keep[k].append(np.array(a))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(cnt[None, :, None] > 0, sums / np.where(cnt > 0, cnt, 1.0)[None, :, None], np.nan)
    res = {"kl_per_read": mean[0], "excl_per_read": mean[1], "var_per_read": mean[2], "drift_per_read": mean[3], "cum3_per_read": mean[4], "confusion": mean[5],
           "p_error_cell": p_err, "worst_rival": rival, "logZ": logZ, "total_counts": total, "clone_names": list(names), "concentration": concentration}
    if per_cell:
        for k, name in enumerate(("excl", "m1", "m2", "m3", "p_confuse")):
            res[name] = np.concatenate(keep[k], axis=0)
    return res


def reads_needed(sep, error=0.05):
    """Reads per cell at which clone ``a`` is told from clone ``b`` with confusion at most ``error``: per ordered pair the smallest integer ``t`` with
    ``p_confuse(t) <= error``, where ``p_confuse`` is ``clone_separability``'s closed form at the cell-AVERAGED per-read quantities of ``sep`` (a result of
    ``clone_separability``: ``drift_per_read``, ``var_per_read``, ``cum3_per_read``, ``excl_per_read``, ``concentration``) and equal priors, found by doubling
    and bisection.  ``p_confuse`` need not fall monotonically -- with equal priors a cell with hardly any reads is called ``a`` by default when the rare reads
    are the ones that favour ``b`` -- so the crossing reported is the LAST one among the doubling probes 1, 2, 4, ..: from there on every probe stays at or
    below ``error``, and ``p_confuse(t) <= error < p_confuse(t - 1)``.  [C, C] float64: ``inf`` where the pair cannot be told apart at any depth (``kappa = 0`` and ``q = 1``: identical clones), 0 on the diagonal,
    NaN for a clone without cells.  As for ``clone_separability``: under the model, so without ``concentration`` an optimistic depth."""
    if not 0.0 < error < 1.0:
        raise ValueError("error must lie in (0, 1)")
    kappa, v, c3, q = sep["drift_per_read"], sep["var_per_read"], sep["cum3_per_read"], 1.0 - sep["excl_per_read"]
    C = kappa.shape[0]
    out = np.zeros((C, C))
    for a in range(C):
        for b in range(C):
            if a == b:
                continue
            if not np.isfinite(kappa[a, b]):
                out[a, b] = np.nan
                continue
            f = lambda t: float(_p_confuse(float(t), q[a, b], kappa[a, b], v[a, b], c3[a, b], 0.0, sep.get("concentration")))  # noqa: E731
            if q[a, b] >= 1.0 and kappa[a, b] <= 0.0:
                out[a, b] = np.inf
                continue
            probes = [2 ** k for k in range(41)]
            over = [k for k, tt in enumerate(probes) if f(tt) > error]
            if over and over[-1] == len(probes) - 1:
                out[a, b] = np.inf
                continue
            lo = probes[over[-1]] if over else 0                     # (f(0) = 1 > error: nothing is known without reads)
            hi = max(2 * lo, 1)
            while hi - lo > 1:                                       # f(lo) > error >= f(hi)
                mid = (lo + hi) // 2
                lo, hi = (lo, mid) if f(mid) <= error else (mid, hi)
            out[a, b] = hi
    return out


def merge_candidates(sep, threshold=0.2):
    """The unordered pairs of clones that expression cannot tell apart at the depth ``sep`` (a result of ``clone_separability``) was made for: those whose
    ``confusion`` exceeds ``threshold`` in BOTH directions.  A list of ``(name_a, name_b, confusion[a, b], confusion[b, a])``, ``a < b``, sorted by
    decreasing ``min`` of the two (ties in clone order): candidates to merge before a fit."""
    conf, names = sep["confusion"], sep["clone_names"]
    C = conf.shape[0]
    found = [(a, b) for a in range(C) for b in range(a + 1, C) if conf[a, b] > threshold and conf[b, a] > threshold]
    found.sort(key=lambda ab: (-min(conf[ab], conf[ab[::-1]]), ab))
    return [(names[a], names[b], float(conf[a, b]), float(conf[b, a])) for a, b in found]


def _dosage_fit(T, X, L, use, kappa_max=8.0, max_iter=50, tol=1e-10, max_step=2.0):
    """The per-gene fits of ``dosage_response`` from arrays [G, C]: observed totals ``T``, exposures ``X``, copy numbers ``L`` and the mask ``use`` of
    the (gene, clone) entries that take part.  Every gene runs the same safeguarded Newton iteration on its concave profile log-likelihood."""
    G, C = T.shape
    use = use & (L > 0) & np.isfinite(X) & (X > 0)
    l = np.where(use, np.log(np.where(use, L, 1.0)), 0.0)
    logX = np.where(use, np.log(np.where(use, X, 1.0)), -np.inf)
    Tm = np.where(use, T, 0.0)
    Tt, Tl = Tm.sum(1), (Tm * l).sum(1)
    n_used = use.sum(1)
    ls = np.sort(np.where(use, l, np.inf), axis=1)
    distinct = np.isfinite(ls[:, :1]).sum(1) + (np.isfinite(ls[:, 1:]) & (ls[:, 1:] != ls[:, :-1])).sum(1)
    ok = (distinct >= 2) & (Tt > 0)

    def state(k):                                                    # lp(kappa), E_pi[l], Var_pi[l], pi
        a = k[:, None] * l + logX
        top = np.where(ok, a.max(1, initial=-np.inf), 0.0)
        ex = np.where(use & ok[:, None], np.exp(a - top[:, None]), 0.0)
        s = np.where(ok, ex.sum(1), 1.0)
        pi = ex / s[:, None]
        El = (pi * l).sum(1)
        return k * Tl - Tt * (top + np.log(s)), El, (pi * (l - El[:, None]) ** 2).sum(1), pi

    k = np.ones(G)
    f, El, Vl, pi = state(k)
    f1 = f.copy()
    conv = np.zeros(G, dtype=bool)
    for _it in range(int(max_iter)):
        todo = ok & ~conv
        if not todo.any():
            break
        grad, curv = Tl - Tt * El, Tt * Vl
        with np.errstate(divide="ignore", invalid="ignore"):
            step = np.where(curv > 0, grad / np.where(curv > 0, curv, 1.0), np.sign(grad) * max_step)
        kn = np.clip(k + np.clip(step, -max_step, max_step), -kappa_max, kappa_max)
        moved = np.abs(kn - k)                                       # the Newton step inside the bounds: what convergence is judged by
        fn, Eln, Vln, pin = state(kn)
        for _h in range(40):                                         # concave in kappa: halve the step while the value falls by more than its rounding noise
            worse = todo & (fn < f - 64.0 * np.finfo(np.float64).eps * (np.abs(f) + np.abs(fn) + Tt)) & (kn != k)
            if not worse.any():
                break
            kn = np.where(worse, 0.5 * (k + kn), kn)
            fn, Eln, Vln, pin = state(kn)
        upd = todo[:, None]
        k, f, El, Vl, pi = np.where(todo, kn, k), np.where(todo, fn, f), np.where(todo, Eln, El), np.where(todo, Vln, Vl), np.where(upd, pin, pi)
        conv |= todo & (moved <= tol * np.maximum(1.0, np.abs(k)))
    f0 = state(np.zeros(G))[0]
    nan = np.full(G, np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        se = np.where(ok & (Tt * Vl > 0), 1.0 / np.sqrt(np.where(Tt * Vl > 0, Tt * Vl, 1.0)), np.where(ok, np.inf, np.nan))
        fitted = Tt[:, None] * pi
        pearson = np.where(use & (fitted > 0), (Tm - fitted) ** 2 / np.where(fitted > 0, fitted, 1.0), 0.0).sum(1)
    lrt1, lrt0 = np.maximum(0.0, 2.0 * (f - f1)), np.maximum(0.0, 2.0 * (f - f0))
    from scipy.special import erfc
    return {"kappa": np.where(ok, k, nan), "se": se, "lrt_proportional": np.where(ok, lrt1, nan), "lrt_insensitive": np.where(ok, lrt0, nan),
            "p_proportional": np.where(ok, erfc(np.sqrt(lrt1 / 2.0)), nan), "p_insensitive": np.where(ok, erfc(np.sqrt(lrt0 / 2.0)), nan),
            "n_clones_used": n_used.astype(np.int64), "total_count": Tt, "converged": ok & conv, "at_bound": ok & (np.abs(k) == kappa_max),
            "pearson": np.where(ok, pearson, nan), "df": n_used.astype(np.int64) - 2}


def dosage_response(fit, Y, L, *, moments=None, kappa_max=8.0, max_iter=50, tol=1e-10, x=None, saturate=True, saturation_threshold=6, engine_opts=None,
                    host=False):
    """Per-gene test of the model's central assumption, that expression is proportional to copy number: fits ``expression ~ mu_g L[g, c]^kappa_g`` per
    gene, where ``kappa = 1`` is the clonealign assumption and ``kappa = 0`` dosage compensation.  Works from ``predictive_moments``'s ``T_observed``
    and ``exposure`` alone, on the host, in O(genes x clones); ``moments=`` reuses a result of ``predictive_moments``, otherwise the other arguments
    go to it.

    Per gene, over the clones with used cells, ``L[g, c] > 0`` (the ``L`` the fit used, after ``saturate``) and a finite exposure ``X_c``: the Poisson
    working model, conditional on the cells' normalisers, ``T_c ~ Poisson(mu L_c^kappa X_c)``, with ``mu`` profiled out: ``lp(kappa) = kappa sum_c
    T_c l_c - T. log sum_c X_c exp(kappa l_c)``, ``l = log L``, concave; a safeguarded Newton iteration from ``kappa = 1`` (steps clipped, halved
    where the value would fall, ``|kappa| <= kappa_max``; stops at a step below ``tol``).

    Returns a dict of arrays [genes]: ``kappa``, ``se`` = 1 / sqrt(T. Var_pi[l]) (``pi_c ~ X_c L_c^kappa``), ``lrt_proportional`` = 2 (lp(kappa_hat)
    - lp(1)) and ``lrt_insensitive`` (against 0) with their chi-square(1) tail probabilities ``p_proportional`` and ``p_insensitive``,
    ``n_clones_used``, ``total_count``, ``converged``, ``at_bound`` (``|kappa| = kappa_max``: every count sits in the clones of extreme copy number),
    ``pearson`` = sum_c (T_c - fitted_c)^2 / fitted_c and ``df`` = ``n_clones_used - 2``.  A gene with fewer than two distinct copy numbers among its
    used clones, or without counts, is not identifiable: NaN, with ``n_clones_used`` as found.

    Real counts are overdispersed against the Poisson working model, which makes both likelihood-ratio tests anti-conservative: ``pearson / df`` well
    above 1 says by how much, and is what to look at before a ``p`` value.  Genes with ``kappa`` near 0 carry no information about the clone of a
    cell; they are the ones to leave out of a fit."""
    if moments is None:
        moments = predictive_moments(fit, Y, L, x=x, saturate=saturate, saturation_threshold=saturation_threshold, engine_opts=engine_opts, host=host)
    T, X, Ls = (np.asarray(moments[k], dtype=np.float64) for k in ("T_observed", "exposure", "L"))
    use = np.broadcast_to(np.asarray(moments["clone_cells"])[None, :] > 0, T.shape)
    return _dosage_fit(T, X, Ls, use, float(kappa_max), int(max_iter), float(tol))


def _profile_operands_host(mu, kappa, blocks, G, what="copy_number_profile"):
    """``mu`` [G], ``kappa`` [J] and the int labels ``blocks`` [G] (or None) of ``ca_copy_number_profile`` with its refusals as ValueError.  Returns
    ``(mu, kappa, blocks, B)``; ``B = G`` without labels."""
    mu, kappa = np.asarray(mu, dtype=np.float64).reshape(-1), np.asarray(kappa, dtype=np.float64).reshape(-1)
    if mu.shape[0] != G:
        raise ValueError(f"{what}: mu has {mu.shape[0]} entries but E has {G} rows (genes)")
    for name, v, row in (("mu", mu, "gene"), ("kappa", kappa, "candidate")):
        wrong = np.flatnonzero(~np.isfinite(v) | (v < 0))
        if wrong.size:
            raise ValueError(f"{what}: {name} has a negative or non-finite entry ({row} {wrong[0]})")
    if not 1 <= kappa.shape[0] <= 16:
        raise ValueError(f"{what}: J = {kappa.shape[0]} is outside [1, 16]")
    if blocks is None:
        return mu, kappa, None, G
    blocks = np.asarray(blocks, dtype=np.int64).reshape(-1)
    if blocks.shape[0] != G:
        raise ValueError(f"{what}: blocks has {blocks.shape[0]} labels but E has {G} rows (genes)")
    B = int(blocks.max()) + 1
    wrong = np.flatnonzero(blocks < 0)
    if wrong.size:
        raise ValueError(f"{what}: block_of_gene[{wrong[0]}] = {blocks[wrong[0]]} is outside [0, {B})")
    return mu, kappa, blocks, B


def _copy_number_profile_host(E, V, U, clone, total, mu, kappa, blocks=None, work=1 << 22):
    """Numpy float64 restatement of ``ca_copy_number_profile`` (include/clonealign_hip.h states the output): per cell ``eta``, the shift ``m``, ``w = E
    exp(eta - m)`` and ``Z`` as in ``_predictive_moments_host``; ``x = exp(eta - m) / Z`` for every gene and ``p = w / Z``.  Per-gene mode: ``a = ((mu
    kappa_j - E) / E) p`` where ``E > 0``, ``(mu kappa_j) x`` where ``E = 0``.  Block mode (``blocks``: int labels [G] in [0, B)): the shares ``A = sum_{g in
    b} mu_g x`` and ``S = sum_{g in b} p`` (1 exactly where the block holds every expressed gene of the cell's clone, at most ``1 - 2^-53`` where it does not), ``a = max(kappa_j A - S, -1)``, and 0
    by rule where every gene of the block has ``mu_g kappa_j == E[g, c]``.  ``cost[b, c, j]`` = the sum over the clone's cells with counts of ``total
    log1p(a)``.  At most ``work`` (cell, gene-or-block, candidate) terms at a time.  Refusals are the library's, as ValueError."""
    E, V, U, clone, total, N, G, C, D = _model_inputs_host(E, V, U, clone, total, "copy_number_profile")
    mu, kappa, blocks, B = _profile_operands_host(mu, kappa, blocks, G)
    J = kappa.shape[0]
    cost = np.zeros((B, C, J))
    delta = (mu[:, None] * kappa[None, :])[:, None, :] - E[:, :, None]                      # [G, C, J]: the product rounded, then the difference
    if blocks is None:
        cf = np.where(E[:, :, None] > 0, delta / np.where(E > 0, E, 1.0)[:, :, None], delta)
    else:
        onehot = np.zeros((G, B))
        onehot[np.arange(G), blocks] = 1.0
        npos = onehot.T @ (E > 0).astype(np.float64)                                         # [B, C]
        full = (npos == npos.sum(0, keepdims=True)) & (npos.sum(0, keepdims=True) > 0)
        same = (onehot.T @ (delta != 0).reshape(G, C * J).astype(np.float64)).reshape(B, C, J) == 0
    chunk = max(1, int(work) // (B * J if blocks is not None else G * J))
    live = np.flatnonzero(total > 0)
    for lo in range(0, live.size, chunk):
        rows = live[lo:lo + chunk]
        e = E[:, clone[rows]].T                                      # [cells, G]
        pos = e > 0
        eta = np.zeros(e.shape)
        for d in range(D):
            eta = eta + U[rows, d:d + 1] * V[None, :, d]
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            m = np.where(pos, eta, -np.inf).max(1, keepdims=True)
            ex = np.exp(eta - m)
            w = np.where(pos, e * ex, 0.0)
            top = w.argmax(1)[:, None]                               # the largest w (the first such gene) goes last into the sum
            rest = w.copy()
            np.put_along_axis(rest, top, 0.0, 1)
            Z = rest.sum(1, keepdims=True) + np.take_along_axis(w, top, 1)
            p, xg = w / Z, ex / Z
            t = total[rows].astype(np.float64)
            for c in np.unique(clone[rows]):
                sel = clone[rows] == c
                if blocks is None:
                    q = np.where(pos[sel], p[sel], xg[sel])[:, :, None]
                    a = np.where(cf[None, :, c, :] == 0, 0.0, cf[None, :, c, :] * q)
                else:
                    A, S = (mu[None, :] * xg[sel]) @ onehot, p[sel] @ onehot
                    S = np.where(full[None, :, c], 1.0, np.minimum(S, 1.0 - 2.0 ** -53))
                    a = np.maximum(kappa[None, None, :] * A[:, :, None] - S[:, :, None], -1.0)
                    a = np.where(same[None, :, c, :], 0.0, a)
                cost[:, c, :] += (t[sel, None, None] * np.log1p(a)).sum(0)
    return cost


def _profile_gain(T, E, mu, kappa, blocks, B):
    """The observed side of the profile: ``gain[b, c, j] = sum_{g in b} xlogy(T, mu_g kappa_j) - xlogy(T, E)`` with ``0 log 0 = 0``.  A gene whose reads are
    impossible under both weights (``T > 0``, ``E = 0`` and ``mu_g kappa_j = 0``) adds 0; otherwise an impossible candidate makes the entry ``-inf``, and
    reads on a gene with ``E = 0`` make every possible candidate ``+inf``: never NaN."""
    from scipy.special import xlogy
    with np.errstate(divide="ignore", invalid="ignore"):
        tk = xlogy(T[:, :, None], (mu[:, None] * kappa[None, :])[:, None, :])                # [G, C, J]
        te = xlogy(T, E)[:, :, None]
        term = np.where(np.isneginf(tk) & np.isneginf(te), 0.0, tk - te)
    if blocks is None:
        return term
    fin = np.isfinite(term)
    gain, neg, posi = np.zeros((B,) + term.shape[1:]), np.zeros((B,) + term.shape[1:], dtype=bool), np.zeros((B,) + term.shape[1:], dtype=bool)
    np.add.at(gain, blocks, np.where(fin, term, 0.0))
    np.logical_or.at(neg, blocks, np.isneginf(term))
    np.logical_or.at(posi, blocks, np.isposinf(term))
    return np.where(neg, -np.inf, np.where(posi, np.inf, gain))


def copy_number_profile(fit, Y, L, *, candidates=None, blocks=None, prior=None, x=None, saturate=True, saturation_threshold=6, engine_opts=None,
                        host=False):
    """Which copy number do the expression data support for this gene -- or this segment -- in this clone, and by how many nats?  The likelihood profile
    over one entry ``L[g, c]`` (or over all genes of a block at once, ``blocks``: a label per gene, chromosome arms or copy-number segments) with ``mu``,
    ``W``, ``psi``, ``beta`` and the called clones held at the fit's values: replacing the weight ``mu_g L[g, c]`` by ``mu_g kappa_j`` in clone ``c`` only
    changes the total multinomial log-likelihood by exactly ``delta_ll = gain - cost``, where ``gain`` needs the observed per-clone totals alone and
    ``cost``, the change of the cells' normalisers, is one pass on the device that reads no counts (``engine.copy_number_profile`` /
    ``ca_copy_number_profile``; include/clonealign_hip.h states it).

    Arguments, label checks and the treatment of "unassigned" cells are ``predictive_moments``'s.  ``candidates``: up to 16 copy numbers, by default the
    integers ``0 .. saturation_threshold``; ``kappa`` is ``candidates`` after ``saturate`` (candidates that coincide there, negatives and non-finite values:
    ValueError).  ``prior``: weights over the candidates (uniform by default).  Observed side, one engine with ``Y`` resident (``engine_opts`` go to its
    constructor): ``T_observed`` from ``clone_gene_sums``.  ``host=True`` runs the numpy restatement (``_copy_number_profile_host``) on both sides instead;
    there is no silent fallback otherwise.

    Returns a dict; the first axis is the genes, or with ``blocks`` the blocks in order of first appearance (``block_names``, ``block_of_gene``).
    ``candidates``, ``kappa`` [J]; ``T_observed`` [genes, clones]; ``gain``, ``cost``, ``delta_ll`` [., clones, J]; ``input_cn`` [., clones]: ``L`` as the fit
    used it (after ``saturate``), NaN for a block whose genes disagree in that clone; ``map_cn`` = ``kappa`` at the largest ``delta_ll`` (the first such);
    ``log_bf`` = ``max_j delta_ll``, the log Bayes factor of the best candidate against the matrix as given, whose ``delta_ll`` is 0 by definition;
    ``posterior`` [., clones, J] = softmax over the candidates of ``delta_ll + log prior``; ``posterior_input`` = its value at ``input_cn`` (NaN where
    ``input_cn`` is NaN or no candidate); ``clone_cells``.  Never NaN in ``delta_ll``: ``-inf`` where the candidate is 0 and the clone has reads on the gene
    (on a gene of the block), ``+inf`` for every positive candidate where the matrix as given is impossible (``E = 0`` with reads), ``-inf`` also where the candidate leaves a cell with reads no expressed gene at all (``cost = -inf``) even if none of the clone's
    reads sit on the genes in question, ``0 log 0 = 0``; a clone
    without cells has ``delta_ll = 0`` and ``posterior`` = the prior.

    What the numbers are not.  The profile is CONDITIONAL on the fitted ``mu``, ``W``, ``psi`` and clone calls: a gene whose copy number is wrong by one
    factor in ALL clones is absorbed by ``mu`` and invisible here, and the fit's ``mu`` was itself estimated under the wrong ``L`` -- so correct
    (``apply_copy_number_calls``) and refit rather than read the profile as final.  And it is MULTINOMIAL: real counts are overdispersed, so ``log_bf`` is
    anti-conservative -- a ranking on a depth-aware scale, not a calibrated Bayes factor."""
    Ya, _Lm, Ls, E, U, V, idx, used, rows, Uu, N, G = _predictive_inputs(fit, Y, L, x, saturate, saturation_threshold)
    C = E.shape[1]
    mu = np.asarray(fit["ml_params"]["mu"], dtype=np.float64).reshape(-1)
    cand = np.arange(int(saturation_threshold) + 1, dtype=np.float64) if candidates is None else np.asarray(candidates, dtype=np.float64).reshape(-1)
    if not 1 <= cand.shape[0] <= 16:
        raise ValueError(f"candidates has {cand.shape[0]} entries; between 1 and 16 are supported")
    if not np.isfinite(cand).all() or (cand < 0).any():
        raise ValueError("candidates must be finite and >= 0")
    kappa = hostprep.saturate(cand, saturation_threshold) if saturate else cand.copy()
    if np.unique(kappa).shape[0] != kappa.shape[0]:
        raise ValueError(f"candidates coincide{' after saturation at ' + str(saturation_threshold) if saturate else ''}: {kappa.tolist()}")
    J = kappa.shape[0]
    names, bg = _block_labels(blocks, G) if blocks is not None else (None, None)
    B = G if bg is None else len(names)
    pr = np.full(J, 1.0 / J) if prior is None else np.asarray(prior, dtype=np.float64).reshape(-1)
    if pr.shape[0] != J or not np.isfinite(pr).all() or (pr <= 0).any():
        raise ValueError(f"prior must hold {J} positive weights, one per candidate")
    pr = pr / pr.sum()
    if host:
        T_obs = np.zeros((G, C))
        dense = Ya[used].toarray() if _is_sparse(Ya) else np.asarray(Ya)[used]
        np.add.at(T_obs.T, idx[used], dense.astype(np.float64))
        cost = _copy_number_profile_host(E, V, Uu, idx[used], rows, mu, kappa, bg)
    else:
        from . import engine as _engine
        opts = dict(engine_opts or {})
        eng = _engine.HipEngine(Ya, Ls, np.zeros((N, 0)), None, 0, **opts)
        try:
            T_obs = np.ascontiguousarray(eng.clone_gene_sums(idx)[0])
        finally:
            eng.close()
        cost = _engine.copy_number_profile(E, V, Uu, idx[used], rows, mu, kappa, blocks=bg, device=int(opts.get("device", 0)))
    gain = _profile_gain(T_obs, E, mu, kappa, bg, B)
    with np.errstate(invalid="ignore"):
        delta = np.where(np.isinf(gain), gain, np.where(np.isneginf(cost), -np.inf, gain - cost))
    if bg is None:
        input_cn = np.array(Ls, dtype=np.float64)
    else:
        lo, hi = np.full((B, C), np.inf), np.full((B, C), -np.inf)
        np.minimum.at(lo, bg, Ls)
        np.maximum.at(hi, bg, Ls)
        input_cn = np.where(lo == hi, lo, np.nan)
    jmap = delta.argmax(2)
    best = np.take_along_axis(delta, jmap[:, :, None], 2)[:, :, 0]
    with np.errstate(invalid="ignore", over="ignore"):
        wgt = np.where(np.isposinf(best)[:, :, None], np.isposinf(delta).astype(np.float64),
                       np.exp(np.where(np.isneginf(best)[:, :, None], 0.0, delta - np.where(np.isfinite(best), best, 0.0)[:, :, None]))) * pr[None, None, :]
    post = wgt / wgt.sum(2, keepdims=True)
    hit = kappa[None, None, :] == input_cn[:, :, None]                                      # (NaN equals nothing)
    post_in = np.where(hit.any(2), (post * hit).sum(2), np.nan)
    out = {"candidates": cand, "kappa": kappa, "T_observed": T_obs, "gain": gain, "cost": cost, "delta_ll": delta, "input_cn": input_cn,
           "map_cn": kappa[jmap], "log_bf": best, "posterior": post, "posterior_input": post_in,
           "clone_cells": np.bincount(idx[used], minlength=C).astype(np.int64)}
    if bg is not None:
        out.update({"block_names": names, "block_of_gene": bg})
    return out


def suspect_copy_numbers(profile, log_bf=10.0):
    """The entries of the copy-number matrix the expression data contradict: the (gene-or-block, clone) pairs of a ``copy_number_profile`` whose best
    candidate differs from the matrix as given (``map_cn != input_cn``; a block whose genes disagree counts as different) with ``log_bf`` above the bar,
    sorted by ``log_bf``, largest first.  Returns a list of dicts: ``index`` (the row of the profile), ``block`` (its label; None in per-gene mode),
    ``clone`` (column), ``input_cn``, ``map_cn``, ``log_bf``, and the runner-up: ``runner_up_cn`` and ``runner_up_delta_ll``, the second-best candidate
    and its ``delta_ll`` (NaN with a single candidate).  ``log_bf`` is ``copy_number_profile``'s: conditional on the fit and multinomial, so a ranking on
    a depth-aware scale and anti-conservative on overdispersed counts."""
    delta, lb, mp, ic, kappa = (np.asarray(profile[k]) for k in ("delta_ll", "log_bf", "map_cn", "input_cn", "kappa"))
    rows, cols = np.nonzero((lb > float(log_bf)) & ~(mp == ic))
    order = np.argsort(-lb[rows, cols], kind="stable")
    names = profile.get("block_names")
    out = []
    for r, c in zip(rows[order].tolist(), cols[order].tolist()):
        d = delta[r, c].copy()
        d[int(d.argmax())] = -np.inf
        j2 = int(d.argmax())
        second = kappa.shape[0] > 1
        out.append({"index": r, "block": None if names is None else names[r], "clone": c, "input_cn": float(ic[r, c]), "map_cn": float(mp[r, c]),
                    "log_bf": float(lb[r, c]), "runner_up_cn": float(kappa[j2]) if second else float("nan"),
                    "runner_up_delta_ll": float(d[j2]) if second else float("nan")})
    return out


def apply_copy_number_calls(profile, L, log_bf=10.0, blocks=None):
    """A copy of ``L`` [genes, clones] (float64 array) with the entries ``suspect_copy_numbers(profile, log_bf)`` lists replaced by their ``map_cn`` --
    whole blocks in block mode (``blocks``: the labels the profile was made with; by default the profile's own).  This is the matrix to refit with: the
    profile is conditional on a ``mu`` that was estimated under the uncorrected matrix."""
    Lm = np.array(_parse_cnv(L)[0], dtype=np.float64)
    G = Lm.shape[0]
    rows = np.asarray(profile["delta_ll"]).shape[0]
    bg = profile.get("block_of_gene")
    if blocks is not None:
        if bg is None:
            raise ValueError("the profile was made per gene: blocks does not apply")
        bg = _block_labels(blocks, G)[1]
    if (G if bg is None else int(np.max(bg)) + 1) != rows or (bg is not None and len(bg) != G) or Lm.shape[1] != np.asarray(profile["log_bf"]).shape[1]:
        raise ValueError(f"L is {Lm.shape} but the profile has {rows} rows and {np.asarray(profile['log_bf']).shape[1]} clones")
    for s in suspect_copy_numbers(profile, log_bf):
        Lm[(s["index"] if bg is None else np.asarray(bg) == s["index"]), s["clone"]] = s["map_cn"]
    return Lm


def _logexpr_sums_host(Y, group_idx, n_groups, size_factors=None, chunk=4096):
    """Float64 host form of ``HipEngine.logexpr_sums`` for engines without it: Y [N, G] dense or scipy.sparse (densified ``chunk`` cells at a time),
    ``group_idx`` in [-1, n_groups) with -1 = leave the cell out.  Same return value, same refusals (ValueError)."""
    idx = np.asarray(group_idx, dtype=np.int64).reshape(-1)
    N, G = Y.shape
    Q = int(n_groups)
    if not 1 <= Q <= 64:
        raise ValueError(f"logexpr_sums: n_groups = {Q} is outside [1, 64]")
    if idx.shape[0] != N:
        raise ValueError(f"logexpr_sums: Y has {N} rows (cells) but group_idx {idx.shape[0]} entries")
    if idx.size and (idx.min() < -1 or idx.max() >= Q):
        n = int(np.flatnonzero((idx < -1) | (idx >= Q))[0])
        raise ValueError(f"logexpr_sums: group index {idx[n]} of cell {n} is outside [-1, {Q})")
    used = np.flatnonzero(idx >= 0)
    if size_factors is None:                                         # library-size factors centred at 1 over the used cells
        lib = np.asarray(Y.sum(1), dtype=np.float64).reshape(-1) if _is_sparse(Y) else np.asarray(Y).sum(1, dtype=np.float64)
        mean = lib[used].mean() if used.size else 1.0
        sf = lib / mean if mean > 0 else np.zeros(N)
    else:
        sf = np.asarray(size_factors, dtype=np.float64).reshape(-1)
        if sf.shape[0] != N:
            raise ValueError(f"logexpr_sums: Y has {N} rows (cells) but size_factors {sf.shape[0]} entries")
    wrong = used[~((sf[used] > 0) & np.isfinite(sf[used]))]
    if wrong.size:
        raise ValueError(f"logexpr_sums: cell {wrong[0]} (group {idx[wrong[0]]}) has size factor {sf[wrong[0]]}: it must be positive and finite")
    S1, S2 = np.zeros((G, Q)), np.zeros(G)
    for lo in range(0, used.size, int(chunk)):
        rows = used[lo:lo + int(chunk)]
        Yc = Y[rows]
        Yc = np.asarray(Yc.toarray() if _is_sparse(Yc) else Yc, dtype=np.float64)
        lc = np.log2(Yc / sf[rows, None] + 1.0)                      # logcounts, R/plotting.R:177
        S2 += (lc * lc).sum(0)
        for q in np.unique(idx[rows]):
            S1[:, q] += lc[idx[rows] == q].sum(0)
    return {"S1": S1, "S2": S2, "n_group": np.bincount(idx[used], minlength=Q).astype(np.int64)}


def clone_expression_profile(Y, clones, *, size_factors=None, engine=None, engine_opts=None):
    """Per-clone expression profile: the data side of plot_clonealign (R/plotting.R:177-201) from ONE sweep over the count matrix.

    ``Y`` [cells, genes]: a dense array in any dtype the engine uploads, or a scipy.sparse matrix; never densified or copied as float64 on the host.
    ``clones``: one label per cell, used as given (:181): "unassigned" is a label like any other.  The log-expression is formed from the counts,
    ``lc = log2(y / sf + 1)``, with library-size factors centred at 1 (scater's ``normalize()`` default) unless ``size_factors`` [cells] are given.
    ``engine``: a live engine whose resident matrix is ``Y``; without it a throwaway engine is built for the upload only (``K=0``; ``engine_opts`` go
    to its constructor) and closed afterwards.  An engine without ``logexpr_sums`` gets the chunked float64 host form.

    Returns a dict: ``labels`` (distinct labels in order of first appearance), ``n_cells`` per label, ``mean`` [G] and ``sd`` [G] of lc over all cells
    (sample sd, n - 1; an sd of 0 is replaced by 1, :193; a variance not above ``1e-12 * S2 / N`` counts as 0) and ``mean_z`` [G, Q], the mean z-score
    of gene g over the cells of label q, ``(S1[g][q] / n_q - mean_g) / sd_g`` (:195-200)."""
    Y = _counts_array(Y.values if hasattr(Y, "columns") and hasattr(Y, "values") else Y)
    N, G = Y.shape
    clones = np.asarray(clones, dtype=object).reshape(-1)
    if clones.shape[0] != N:
        raise ValueError(f"clones has {clones.shape[0]} labels but Y has {N} rows (cells)")
    labels = list(dict.fromkeys(clones.tolist()))
    Q = len(labels)
    if not 1 <= Q <= 64:
        raise ValueError(f"clones holds {Q} distinct labels; between 1 and 64 are supported")
    lut = {c: i for i, c in enumerate(labels)}
    idx = np.array([lut[c] for c in clones], dtype=np.int32)
    own = engine is None
    if own:
        from .engine import HipEngine
        engine = HipEngine(Y, np.ones((G, 2)), np.zeros((N, 0)), np.zeros(G), 0, **(engine_opts or {}))
    try:
        if hasattr(engine, "logexpr_sums"):
            if (engine.N, engine.G) != (N, G):
                raise ValueError(f"the engine holds a {engine.N} x {engine.G} matrix but Y is {N} x {G}")
            out = engine.logexpr_sums(idx, Q, size_factors)
        else:
            out = _logexpr_sums_host(Y, idx, Q, size_factors)
    finally:
        if own:
            engine.close()
    return _profile_from_sums(out["S1"], out["S2"], out["n_group"], labels)


def _profile_from_sums(S1, S2, n_group, labels):
    """mean, sd and per-label mean z-scores (R/plotting.R:188-200) from the sums of ``logexpr_sums``."""
    S1 = np.asarray(S1, dtype=np.float64)
    S2 = np.asarray(S2, dtype=np.float64)
    nq = np.asarray(n_group, dtype=np.float64)
    n = nq.sum()
    mean = S1.sum(1) / n
    with np.errstate(divide="ignore", invalid="ignore"):
        var = (S2 - n * mean ** 2) / (n - 1) if n > 1 else np.full(S2.shape, np.nan)           # sd(), :189
        var = np.where(var > 1e-12 * S2 / n, var, 0.0) if n > 1 else var                     # round-off must not make a constant gene vary
        sd = np.sqrt(var)
        sd[sd == 0] = 1.0                                                                     # :193
        mean_z = (S1 / nq[None, :] - mean[:, None]) / sd[:, None]                             # :195-200
    return {"labels": list(labels), "n_cells": np.asarray(n_group, dtype=np.int64), "mean": mean, "sd": sd, "mean_z": mean_z}


class ClonealignTracks(dict):
    """What plot_clonealign (R/plotting.R:70-226) draws, as numpy arrays: a dict with attribute access (``genes``, ``cnv_segments``, ``expression``,
    ``expression_segments``, each a dict of equally long columns).  ``draw()`` renders the two stacked panels."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def draw(self, ax=None):
        """The two stacked panels (:168-224): per-gene mean z-scores with the per-state segments on top, copy-number segments below.  Needs
        matplotlib; returns the figure."""
        try:
            import matplotlib.pyplot as plt
        except ImportError as e:
            raise ImportError("ClonealignTracks.draw() needs matplotlib, which is not installed; the tracks themselves (genes, cnv_segments, "
                              "expression, expression_segments) are the result") from e
        fig, (top, bottom) = plt.subplots(2, 1, sharex=True) if ax is None else (ax[0].figure, ax)
        names = list(dict.fromkeys(list(self["expression"]["clone"]) + list(self["cnv_segments"]["clone"])))
        cmap = plt.get_cmap(self["ggplot_palette"])
        colour = {c: cmap(i % max(getattr(cmap, "N", 9), 1)) for i, c in enumerate(names)}
        ex, es, cs = self["expression"], self["expression_segments"], self["cnv_segments"]
        for c in names:
            m = ex["clone"] == c
            top.scatter(ex["rank_position"][m], ex["mean_z_score"][m], color=colour[c], alpha=0.5, s=8, label=str(c))
            for i in np.flatnonzero(es["clone"] == c):
                top.plot([es["start"][i] - 1, es["end"][i] + 1], [es["per_clone_state_z_score"][i]] * 2, color=colour[c], linewidth=1.2)
            for i in np.flatnonzero(cs["clone"] == c):
                bottom.plot([cs["start"][i] - 1, cs["end"][i] + 1], [cs["copy_number"][i]] * 2, color=colour[c], linewidth=1.8)
        top.set_ylim(*self["expression_ylim"])
        top.set_ylabel("Gene expression")
        top.set_title("scRNA-seq", loc="left")
        top.legend(title="Inferred\nclone")
        bottom.set_xlabel("Genomic position")
        bottom.set_ylabel("Copy number")
        bottom.set_title("scDNA-seq", loc="left")
        return fig


def _average_rank(x):
    """R's rank() with ties.method = "average"."""
    x = np.asarray(x, dtype=np.float64)
    order = np.argsort(x, kind="stable")
    xs = x[order]
    first = np.r_[True, xs[1:] != xs[:-1]]
    run = np.cumsum(first) - 1
    lo = np.flatnonzero(first)
    hi = np.r_[lo[1:], x.size]
    out = np.empty(x.size)
    out[order] = ((lo + 1 + hi) / 2.0)[run]
    return out


def plot_clonealign(sce, clones, cnv_data, chromosome="1", chr_str="chr", start_str="start_position", end_str="end_position", jitter_cnv=True,
                    ggplot_palette="Set1", expression_ylim=(-.15, .15), cnv_dodge_sd=0.1, *, seed=None, size_factors=None, profile=None,
                    engine=None, engine_opts=None):
    """Gene expression and copy number along one chromosome, per clone: R/plotting.R:70-226, first eleven arguments as at :70-77.

    ``sce``: whatever ``clonealign()`` accepts as expression data, with the gene annotation under ``sce["rowData"]`` (a dict of columns holding
    ``chr_str``, ``start_str``, ``end_str`` and optionally ``ensembl_gene_id``); ``clones``: one label per cell; ``cnv_data``: the gene-by-clone
    copy-number DataFrame or array given to the fit.  Returns a :class:`ClonealignTracks` with the plot's data (``.draw()`` renders it):
    ``genes`` (rank_position :121, state :139-151), ``cnv_segments`` per (state, clone, copy_number) (:156-159), ``expression`` -- the mean z-score
    per (clone, gene) (:199-201) -- and ``expression_segments`` per (clone, state), joined with the segments (:203-212).

    The expression side is one device sweep over the count matrix (``clone_expression_profile``; its ``engine`` / ``engine_opts`` /
    ``size_factors`` are passed on), never a dense N x G matrix on the host; ``profile=`` takes a ``clone_expression_profile`` result so that
    several chromosomes cost one sweep.
    Differences from the reference, both stated: (1) the reference reads ``logcounts(sce)`` as the user normalised it; this forms them from the
    counts with library-size factors centred at 1, scater's ``normalize()`` default -- pass ``size_factors`` for anything else.  (2) ``jitter_cnv``
    adds ``N(0, cnv_dodge_sd)`` noise through ``numpy.random.default_rng(seed)``: the reference uses R's ``rnorm()``, whose stream cannot be
    reproduced here, so the jitter (not its distribution) differs from R's under any seed."""
    row_data = sce["rowData"] if isinstance(sce, dict) and "rowData" in sce else getattr(sce, "rowData", None)
    row_data = {} if row_data is None else row_data
    for arg, col, what in (("chr_str", chr_str, "chromosome"), ("start_str", start_str, "start position"), ("end_str", end_str, "end position")):
        if col not in row_data:                                      # :93-103
            raise ValueError(f"The column '{arg}' (currently set to '{col}') must be in rowData(sce) and refer to the {what} of each gene")
    on_chr = np.asarray([str(c) for c in np.asarray(row_data[chr_str]).reshape(-1)], dtype=object) == str(chromosome)   # :105
    if not on_chr.any():
        raise ValueError(f"No genes on chromosome {chromosome} in CNV regions")                 # :107-109
    L, cn = _parse_cnv(cnv_data)                                     # :83-85
    clone_names = cn if cn is not None else [f"clone_{string.ascii_lowercase[i]}" for i in range(L.shape[1])]
    if L.shape[0] != on_chr.shape[0]:
        raise ValueError(f"cnv_data has {L.shape[0]} rows (genes) but rowData(sce) has {on_chr.shape[0]}")
    gi = np.flatnonzero(on_chr)                                      # :111-113
    Lc = L[gi]
    ids = (np.asarray([str(v) for v in np.asarray(row_data["ensembl_gene_id"]).reshape(-1)], dtype=object)[gi] if "ensembl_gene_id" in row_data
           else np.asarray([str(i + 1) for i in range(gi.size)], dtype=object))                 # :115-117
    pos = (np.asarray(row_data[start_str], dtype=np.float64).reshape(-1)[gi] + np.asarray(row_data[end_str], dtype=np.float64).reshape(-1)[gi]) / 2
    rank = _average_rank(pos)                                        # :121
    order = np.argsort(rank, kind="stable")                          # arrange(rank_position), :135
    changed = np.r_[False, np.any(Lc[order][1:] != Lc[order][:-1], axis=1)]
    state = np.empty(gi.size, dtype=np.int64)
    state[order] = 1 + np.cumsum(changed)                            # :139-151
    n_state = int(state.max())
    # segments per (state, clone, copy_number): within a state every clone has ONE copy number, so the groups are the (state, clone) pairs (:156-159)
    seg = {k: [] for k in ("state", "clone", "copy_number", "start", "end")}
    for st in range(1, n_state + 1):
        m = state == st
        for c in sorted(range(len(clone_names)), key=lambda i: str(clone_names[i])):             # group_by() sorts its keys
            seg["state"].append(st); seg["clone"].append(clone_names[c]); seg["copy_number"].append(Lc[m, c][0])
            seg["start"].append(rank[m].min()); seg["end"].append(rank[m].max())
    seg = {"state": np.asarray(seg["state"], dtype=np.int64), "clone": np.asarray(seg["clone"], dtype=object),
           "copy_number": np.asarray(seg["copy_number"], dtype=np.float64), "start": np.asarray(seg["start"]), "end": np.asarray(seg["end"])}
    seg["length"] = seg["end"] - seg["start"]
    if jitter_cnv:                                                   # :162-164
        seg["copy_number"] = seg["copy_number"] + np.random.default_rng(seed).normal(0.0, cnv_dodge_sd, size=seg["copy_number"].shape)
    # RNA side (:177-201): the profile covers every gene of the matrix; a gene's z-scores do not depend on the other genes
    if profile is None:
        Y, _ = _parse_expression(sce)
        profile = clone_expression_profile(Y, clones, size_factors=size_factors, engine=engine, engine_opts=engine_opts)
    mz = np.asarray(profile["mean_z"])
    if mz.shape[0] != on_chr.shape[0]:
        raise ValueError(f"the expression profile covers {mz.shape[0]} genes but rowData(sce) has {on_chr.shape[0]}")
    labels = list(profile["labels"])
    Q = len(labels)
    expr = {"clone": np.repeat(np.asarray(labels, dtype=object), gi.size), "ensembl_gene_id": np.tile(ids, Q), "gene_index": np.tile(gi, Q),
            "rank_position": np.tile(rank, Q), "state": np.tile(state, Q), "mean_z_score": mz[gi].T.reshape(-1).copy()}
    per_state = np.full((Q, n_state), np.nan)                        # :203-205
    for st in range(1, n_state + 1):
        per_state[:, st - 1] = mz[gi][state == st].mean(0)
    expr["per_clone_state_z_score"] = per_state[np.repeat(np.arange(Q), gi.size), np.tile(state, Q) - 1]   # :209
    lab_of = {c: i for i, c in enumerate(labels)}
    keep = np.array([c in lab_of for c in seg["clone"]], dtype=bool)                            # inner_join(cnv_df_2, gex_per_clone_state), :212
    eseg = {k: v[keep] for k, v in seg.items()}
    eseg["per_clone_state_z_score"] = np.array([per_state[lab_of[c], st - 1] for c, st in zip(eseg["clone"], eseg["state"])], dtype=np.float64)
    return ClonealignTracks(genes={"ensembl_gene_id": ids, "gene_index": gi, "rank_position": rank, "state": state}, cnv_segments=seg, expression=expr,
                            expression_segments=eseg, clone_names=list(clone_names), labels=labels, chromosome=chromosome,
                            ggplot_palette=ggplot_palette, expression_ylim=tuple(expression_ylim), profile=profile)


def _counts_array(a):
    """The count matrix in its own dtype when the engine can upload it as it is (no float64 copy of N x G), else float64.  A
    scipy.sparse matrix stays sparse (the engine takes its compressed arrays: engine.sparse_counts)."""
    if _is_sparse(a):
        return a
    a = np.asarray(a)
    if a.dtype in (np.float64, np.float32, np.int32, np.uint16, np.uint8):
        return a
    if a.dtype.kind in "iu" and a.size and 0 <= a.min() and a.max() <= np.iinfo(np.int32).max:
        return a.astype(np.int32)            # e.g. numpy's default int64 counts: half the bytes of a float64 copy
    return a.astype(np.float64)


def _fit_mse_result(plain, with_mu):
    """``res["fit_mse"]`` of clonealign(fit_mse=True) from the two evaluations (E = L with its per-gene sums, E = mu * L)."""
    n = plain["n_cells"]
    return {"mse": plain["mse"], "mse_model_mu": with_mu["mse"],
            "mse_gene": plain["sse_gene"] / n if n else np.full(plain["sse_gene"].shape, np.nan), "n_cells": n}


def _parse_expression(gene_expression_data):
    """R/clonealign.R:207-222.  Returns (Y[cells,genes], gene_names or None)."""
    g = gene_expression_data
    if hasattr(g, "assays") or (isinstance(g, dict) and "assays" in g):        # SCE / SE stand-in
        assays = g["assays"] if isinstance(g, dict) else g.assays
        if "counts" not in assays:
            raise ValueError("counts not in assays(gene_expression_data). Available assays: "
                             + ",".join(assays))
        counts = assays["counts"]                                    # genes x cells
        names = None
        if hasattr(counts, "index"):
            names = [str(i) for i in counts.index]
        elif isinstance(g, dict) and "rownames" in g:
            names = list(g["rownames"])
        return _counts_array(counts).T, names                           # (sparse: the CSC of genes x cells is the CSR of Y, no copy)
    if hasattr(g, "columns") and hasattr(g, "values"):               # pandas DataFrame cells x genes
        return _counts_array(g.values), [str(c) for c in g.columns]
    if isinstance(g, np.ndarray) and g.ndim == 2:
        return _counts_array(g), None
    if _is_sparse(g) and g.ndim == 2:                                # the dgCMatrix branch of :207-222, kept sparse
        return _counts_array(g), None
    raise TypeError("Input gene_expression_data must be SingleCellExperiment, SummarizedExperiment, or matrix")


def _parse_cnv(copy_number_data):
    """R/clonealign.R:237-243.  Returns (L[genes,clones], clone_names or None)."""
    c = copy_number_data
    if hasattr(c, "columns") and hasattr(c, "values"):
        return np.asarray(c.values, dtype=np.float64), [str(n) for n in c.columns]
    if isinstance(c, np.ndarray) and c.ndim == 2:
        return np.asarray(c, dtype=np.float64), None
    raise TypeError("copy_number_data must be a matrix, data.frame or DataFrame. Current class: "
                    + type(c).__name__)


def _default_gene_names(G):
    # R/clonealign.R:256-258 uses ``letters`` (only 26 of them); beyond that we number.
    lt = string.ascii_lowercase
    return [f"gene_{lt[i]}" if i < 26 else f"gene_{i + 1}" for i in range(G)]


def clonealign(gene_expression_data, copy_number_data, max_iter=200, rel_tol=1e-6,
               gene_filter_threshold=0, learning_rate=0.1, x=None, clone_allele=None,
               cov=None, ref=None, fix_alpha=False, dtype="float32", saturate=True,
               saturation_threshold=6, K=None, mc_samples=1, verbose=True, initial_shrink=5,
               clone_call_probability=0.95, data_init_mu=True, *, seed=None, engine=None,
               engine_opts=None, clone_names=None, allele_ref="cov", cell_index=None, gene_index=None, devices=None, fit_mse=False,
               _reuse=None):
    """Assign scRNA-seq cells to clones.  Arguments as R/clonealign.R:184-203.

    Keyword-only extras: ``allele_ref`` -- "cov" (default) reproduces the reference, which forwards ``ref = cov`` to
    inference_tflow (R/clonealign.R:271) so that the allele-specific term sees alt = 0; "ref" forwards the caller's ``ref``
    (the evident intent: an explicit opt-in, the default stays reference-identical).  ``cell_index`` / ``gene_index``: masks or
    index arrays from ``preprocess_for_clonealign(..., return_masks=True)``; the raw matrix is then fitted on that selection
    without a filtered copy (``copy_number_data`` etc. are given for the selected genes / cells).  ``devices``: HIP ordinals -- this ONE fit
    cell-sharded over those devices of this process (forwarded untouched to ``inference_tflow``; ``run_clonealign(devices=)`` is the
    other thing: independent restarts dealt over devices).  ``fit_mse=True``: the result gains ``res["fit_mse"] = {"mse", "mse_model_mu",
    "mse_gene", "n_cells"}``, compute_ca_fit_mse() of the called clones on the retained genes (unassigned cells dropped; with ``L`` and with
    ``mu * L``; the per-gene means are those of ``L``), taken on the still-resident matrix before the engine is closed (``HipEngine.fit_mse``)."""
    if allele_ref not in ("cov", "ref"):
        raise ValueError("allele_ref must be 'cov' (reference behaviour) or 'ref'")
    Y, gene_names = _parse_expression(gene_expression_data)
    N, G = Y.shape
    sel_g = None if gene_index is None else (np.flatnonzero(np.asarray(gene_index)) if np.asarray(gene_index).dtype == bool
                                             else np.asarray(gene_index, dtype=np.int64))
    sel_c = None if cell_index is None else (np.flatnonzero(np.asarray(cell_index)) if np.asarray(cell_index).dtype == bool
                                             else np.asarray(cell_index, dtype=np.int64))
    if sel_g is not None:
        G = len(sel_g)
        if gene_names is not None:
            gene_names = [gene_names[i] for i in sel_g]
    if sel_c is not None:
        N = len(sel_c)
    if K is None:
        K = 1                                                        # :226-232 (both branches give 1)
    L, cn = _parse_cnv(copy_number_data)
    if L.shape[0] != G:
        raise ValueError("copy_number_data must have same number of genes (rows) as gene_expression_data")
    C = L.shape[1]
    if clone_names is None:
        clone_names = cn
    if clone_names is None:
        clone_names = [f"clone_{string.ascii_lowercase[i]}" for i in range(C)]   # :251-253
    if gene_names is None:
        gene_names = _default_gene_names(G)
    # NB the reference forwards ``ref = cov`` (R/clonealign.R:271); kept for drop-in behaviour
    def _post(eng, rlist, keep):
        # device-side sums for compute_correlations: no second pass over Y on the host
        if not hasattr(eng, "clone_gene_sums"):
            return None
        labels = clone_assignment(rlist["clone_probs"], clone_names, clone_call_probability)
        lut = {c: i for i, c in enumerate(clone_names)}
        idx = np.array([lut.get(c, -1) for c in labels], dtype=np.int32)
        T, Syy = eng.clone_gene_sums(idx)
        out = dict(T=T, Syy=Syy, counts=np.bincount(idx[idx >= 0], minlength=C))
        if fit_mse and hasattr(eng, "fit_mse"):                      # compute_ca_fit_mse on the resident matrix, R/clonealign.R:415-434
            Lk = L[np.asarray(keep, dtype=bool), :]
            a = eng.fit_mse(idx, Lk, per_gene=True)
            b = eng.fit_mse(idx, np.asarray(rlist["mu"], dtype=np.float64).reshape(-1, 1) * Lk)
            out["fit_mse"] = _fit_mse_result(a, b)
        return out

    res = inference_tflow(Y, L, max_iter=max_iter, rel_tol=rel_tol, learning_rate=learning_rate,
                          gene_filter_threshold=gene_filter_threshold, x=x,
                          clone_allele=clone_allele, cov=cov, ref=(cov if allele_ref == "cov" else ref), fix_alpha=fix_alpha,
                          dtype=dtype, saturate=saturate, saturation_threshold=saturation_threshold,
                          K=K, mc_samples=mc_samples, verbose=verbose, initial_shrink=initial_shrink,
                          data_init_mu=data_init_mu, gene_names=gene_names, seed=seed,
                          engine=engine, engine_opts=engine_opts, post=_post, cell_index=sel_c, gene_index=sel_g, devices=devices,
                          _reuse=_reuse)
    res = ClonealignFit(res)
    res["clone"] = clone_assignment(res["ml_params"]["clone_probs"], clone_names,
                                    clone_call_probability)          # :283
    res["clone_names"] = list(clone_names)                           # colnames(clone_probs), :286
    # the retained genes as the boolean mask inference_tflow applied (matching by NAME would mark a filtered gene that shares
    # its symbol with a retained one as kept, and L[keep] would then have more rows than the fitted matrix)
    keep = np.asarray(res.pop("retained_mask"), dtype=bool)
    post = res.pop("post", None)

    def _host_selection():                                           # (engines without device sums fit small matrices only)
        if _is_sparse(Y):
            return Y.tocsr()[np.arange(Y.shape[0]) if sel_c is None else sel_c][:, np.arange(Y.shape[1]) if sel_g is None else sel_g].toarray()
        return Y if (sel_c is None and sel_g is None) else Y[np.ix_(np.arange(Y.shape[0]) if sel_c is None else sel_c,
                                                                    np.arange(Y.shape[1]) if sel_g is None else sel_g)]
    if post is not None:
        res["correlations"] = correlations_from_sums(post["T"], post["Syy"], L[keep, :], post["counts"])   # :292-294
    else:
        res["correlations"] = compute_correlations(_host_selection()[:, keep], L[keep, :], res["clone"], clone_names)   # :292-294
    if fit_mse:
        if post is not None and "fit_mse" in post:
            res["fit_mse"] = post["fit_mse"]
        else:                                                        # an engine without fit_mse: the float64 host form
            lut = {c: i for i, c in enumerate(clone_names)}
            idx = np.array([lut.get(c, -1) for c in res["clone"]], dtype=np.int32)
            Yk, Lk = _host_selection()[:, keep], L[keep, :]
            res["fit_mse"] = _fit_mse_result(_fit_mse_host(Yk, Lk, idx, per_gene=True),
                                             _fit_mse_host(Yk, np.asarray(res["ml_params"]["mu"], dtype=np.float64).reshape(-1, 1) * Lk, idx))
    cor = res["correlations"]
    if np.any(~np.isnan(cor)):
        if np.nanquantile(cor, 0.25) < 0:                            # :296-300
            warnings.warn("Less than 75% of genes positively correlated with expression - "
                          "assignment may have failed\n")
    return res


def run_clonealign(gene_expression_data, copy_number_data, initial_shrinks=(0, 5, 10),
                   n_repeats=3, print_elbos=True, *, seed=None, devices=None, **kwargs):
    """R/clonealign.R:35-75: fit across restarts and keep the best final ELBO.

    ``devices``: list of GPU ordinals; restarts are dealt round-robin over them (one fit per
    GPU at a time, independent replicas -- SURVEY.md §8e config 5).  Default: device 0.
    """
    from .multirun import run_restarts
    jobs = []
    ss = np.random.SeedSequence(seed)
    for is_ in initial_shrinks:
        for _ in range(int(n_repeats)):
            jobs.append(dict(initial_shrink=is_))
    seeds = [int(s.generate_state(1)[0]) for s in ss.spawn(len(jobs))]
    fits = run_restarts(gene_expression_data, copy_number_data, jobs, seeds, devices, kwargs)
    final_elbos = np.array([f["convergence_info"]["final_elbo"] for f in fits])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        median_correlations = np.array([np.nanmedian(f["correlations"]) if np.any(~np.isnan(f["correlations"]))
                                        else np.nan for f in fits])
    if print_elbos:
        print("ELBOs:  " + " ".join(repr(float(e)) for e in final_elbos))       # :61-63
    best = fits[int(np.nanargmax(final_elbos))]                                   # which.max, :65
    best["multirun_info"] = {
        "clone_prevalences_at_different_shrinks": [dict(Counter(f["clone"])) for f in fits],   # :69
        "elbos": final_elbos,
        "median_correlations": median_correlations,
    }
    return best
