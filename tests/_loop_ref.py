"""Float64 reference for the WHOLE model's gradients (any K, P, S, the extra log-likelihood term, L = 0 entries, fractional L), plain numpy, no GPU:
what tests/_series_ref.py is for K = 1, P = 0, S = 1, which it reproduces there to 1e-13 (tests/test_loop_ref_host.py).

* ``ref_gradients(fc, st, eps)``: (gradient, scale) of d ELBO / d variable for all eight variables at state ``st`` and draws ``eps`` [S, G].  The scale of an
  element is the sum of the magnitudes of its summands; every comparison is ``|test - reference| <= tol * scale`` per element (``_series_ref.worst_ratio``).
* ``operand_model(fc, st, eps, family)``: the same evaluation with the roundings DESIGN.md section 3 documents for a kernel family, accumulation still in
  float64 -- what a faithful engine may differ by, computed from the reference alone.  ``family``:
    "mfma"       the matrix-core sweeps: variables, mu, coef, E and the stored gradients float32; the exponent in float32 (V' = V log2 e, FMA chain, the
                 per-cell shift); E and M each hi + lo bf16 with the lo * lo product dropped on the way forward; on the way back coef in THREE bf16 parts
                 against bf16-exact copy numbers (t = sum_c coef L exact to float32), u = E t and u mu as float32 products;
    "mfma_frac"  fractional copy numbers at C <= 8: coef in TWO parts, L as hi + lo, the c_lo * L_lo product dropped (k_bwd_mfma<.., FRAC>);
    "valu"       the vector-unit fallbacks: float32 operands and float32 products, both ways.
  A pair (way forward, way back) mixes them: ("valu", "mfma") is a plain pass whose forward sweep has no matrix-core form.
  Accumulation: the matrix-core families' sums stay float64 (their operand splits, 2^-17 per product, dominate; the bars' factor 8 covers the rest).  The VALU
  sweeps' float32 accumulators ("E, M, accumulators float32") ARE modelled, as a float32 chain in index order over the genes (forward) and
  over a slab of CHUNK cells / over the genes (way back), float64 across slabs as the engine's cross-block sums are: float32 PRODUCTS alone leave the model of
  d logits at 1.2e-9 of scale, 15 to 30 times below what a float32 sum of 70 to 95 terms is worth (sqrt(95) x 2^-25 = 2.9e-7 of ITS terms).  The engine's own
  order (lanes, tiles) is not modelled.
* the states of tests/test_gpu_loop_grad.py (``build_state``): every value float32-representable.
"""
import math

import numpy as np
from scipy.special import gammaln, logsumexp, xlogy

from tests._cases import make_case, perturbed_state
from tests._series_ref import VAR_NAMES, sigmoid, softplus, worst_ratio  # noqa: F401  (worst_ratio: re-exported for the tests)

FAMILIES = {"mfma": ("mfma", "mfma"), "mfma_frac": ("mfma", "mfma_frac"), "valu": ("valu", "valu")}     # name: (way forward, way back)
CHUNK = 512          # cells per slab of the N x G x C contraction: 512 x 3100 doubles = 12.7 MB per N x G temporary
LOG2E = math.log2(math.e)


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def bf16(a):
    """Round to nearest even at 8 significand bits (bf16), returned as float64.  Input: anything float32-representable."""
    b = np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


def acc32(a, axis):
    """The sum along ``axis`` as a float32 accumulator makes it, terms in index order (numpy's cumsum is sequential)."""
    return np.take(np.cumsum(np.asarray(a, dtype=np.float32), axis=axis, dtype=np.float32), -1, axis=axis).astype(np.float64)


def bf16_parts(a, n):
    """n bf16 parts of a float32 array: part k = bf16(a - sum of the parts before)."""
    a = f32(a)
    parts, rest = [], a
    for _ in range(n):
        p = bf16(f32(rest))
        parts.append(p)
        rest = rest - p
    return parts


def fit_constants(case):
    """Everything of a ``make_case`` problem that no variable changes: Y, L, X, extra, K, P, D, s, colsum, A = xlogy(Y, L) summed over genes, Y^T X."""
    Y = np.asarray(case["Y"], dtype=np.float64)
    L = np.asarray(case["L"], dtype=np.float64)
    N, G = Y.shape
    K = int(case["K"])
    X = None if case.get("X") is None else np.asarray(case["X"], dtype=np.float64).reshape(N, -1)
    P = 0 if X is None else X.shape[1]
    extra = None if case.get("extra_loglik") is None else np.asarray(case["extra_loglik"], dtype=np.float64)
    A = np.empty((N, L.shape[1]))
    with np.errstate(divide="ignore"):
        for b0 in range(0, N, CHUNK):
            A[b0:b0 + CHUNK] = xlogy(Y[b0:b0 + CHUNK, :, None], L[None, :, :]).sum(1)
    s = Y.sum(1)
    return {"Y": Y, "L": L, "X": X, "extra": extra, "K": K, "P": P, "D": (K + P) if K > 0 else 0, "S": int(case.get("S", 1)), "s": s, "colsum": Y.sum(0), "A": A,
            "cn": gammaln(s + 1.0) - gammaln(Y + 1.0).sum(1), "YtX": (Y.T @ X) if (P > 0 and K > 0) else np.zeros((G, 0))}


def _evaluate(fc, st, eps, family):
    """ref_gradients (family None) and operand_model (a family's roundings) are this one function: r32 is the identity for the reference."""
    exact = family is None
    fwd, bwd = (None, None) if exact else FAMILIES[family] if isinstance(family, str) else family
    assert exact or (fwd in ("mfma", "valu") and bwd in ("mfma", "mfma_frac", "valu")), family
    r32 = (lambda a: a) if exact else f32
    Y, L, s, A, colsum, K, P, D = (fc[k] for k in ("Y", "L", "s", "A", "colsum", "K", "P", "D"))
    N, G = Y.shape
    C = L.shape[1]
    eps = np.asarray(eps, dtype=np.float64).reshape(-1, G)
    S = eps.shape[0]
    loc, ls = np.asarray(st["loc"], dtype=np.float64), np.asarray(st["ls"], dtype=np.float64)
    W = np.asarray(st["W"], dtype=np.float64).reshape(G, K)
    psi = np.asarray(st["psi"], dtype=np.float64).reshape(N, K)
    beta = np.asarray(st["beta"], dtype=np.float64).reshape(G, P)
    vch = np.asarray(st["v"], dtype=np.float64).reshape(K)
    sd = np.exp(ls)
    u = loc + sd[None, :] * eps                                   # [S, G]
    mu = r32(softplus(u))
    if D > 0:
        F = np.concatenate([psi, fc["X"]], 1) if P > 0 else psi
        V = np.concatenate([W, beta], 1) if P > 0 else W
    else:
        F, V = np.zeros((N, 0)), np.zeros((G, 0))
    if not exact:
        F = f32(F)                                                 # (the covariates are held in float32; the variables are float32 already)
    gl = np.asarray(st["gamma_logits"], dtype=np.float64)
    log_gamma = gl - logsumexp(gl, 1, keepdims=True)
    gamma = np.exp(log_gamma)
    M = mu[:, :, None] * L[None, :, :]                            # [S, G, C]
    if fwd == "mfma":
        Mh, Ml = zip(*(bf16_parts(M[i], 2) for i in range(S)))
    if bwd == "mfma_frac":
        Lh, Ll = bf16_parts(L, 2)

    def exponent(sl):
        """E of a slab of cells: exact, or float32 as the sweeps make it -- V' = V log2 e, an FMA chain over d, the per-cell shift, v_exp_f32 -- and the shift."""
        n = sl.stop - sl.start
        if D == 0:
            return np.ones((n, G)), np.zeros(n)
        if exact:
            return np.exp(F[sl] @ V.T), np.zeros(n)
        Vp = f32(V * LOG2E)
        acc = np.zeros((n, G))
        for d in range(D):
            acc = f32(acc + F[sl, d:d + 1] * Vp[None, :, d])     # (an FMA rounds once per term)
        em = acc.max(1)
        return f32(np.exp2(f32(acc - em[:, None]))), em / LOG2E

    def forward(E, i):
        if fwd == "mfma":
            Eh, El = bf16_parts(E, 2)
            return Eh @ Mh[i] + Eh @ Ml[i] + El @ Mh[i]
        if fwd == "valu":
            return np.stack([acc32(f32(E * f32(M[i][None, :, c])), 1) for c in range(C)], 1)
        return E @ M[i]

    logZ = np.empty((S, N, C))
    coef = np.empty((S, N, C))
    shift = np.empty(N)
    for b0 in range(0, N, CHUNK):
        sl = slice(b0, min(N, b0 + CHUNK))
        E, shift[sl] = exponent(sl)
        for i in range(S):
            Z = forward(E, i)
            logZ[i, sl] = np.log(Z) + shift[sl, None]
            coef[i, sl] = r32(-gamma[sl] * s[sl, None] / (S * Z))  # (against the SHIFTED Z, as the backward sweep's E is the shifted one)
    dmu, dmus = np.zeros((S, G)), np.zeros((S, G))
    dV, dVs = np.zeros((G, D)), np.zeros((G, D))
    dF, dFs = np.zeros((N, D)), np.zeros((N, D))
    aL = np.abs(L)
    for b0 in range(0, N, CHUNK):
        sl = slice(b0, min(N, b0 + CHUNK))
        E, _ = exponent(sl)
        deta, detas = np.zeros_like(E), np.zeros_like(E)
        for i in range(S):
            c = coef[i, sl]
            if bwd == "mfma":                                  # three bf16 parts carry a float32 exactly to 2^-24; L is bf16-exact: the sum over c in float32
                t = f32(sum(bf16_parts(c, 3)) @ L.T)
            elif bwd == "mfma_frac":
                c1, c2 = bf16_parts(c, 2)
                t = f32(c1 @ Lh.T + c2 @ Lh.T + c1 @ Ll.T)
            elif bwd == "valu":
                t = sum(f32(c[:, k:k + 1] * f32(L[None, :, k])) for k in range(C))
            else:
                t = c @ L.T
            ta = np.abs(c) @ aL.T
            uu = r32(E * t)
            dmu[i] += acc32(uu, 0) if bwd == "valu" else uu.sum(0)
            dmus[i] += (E * ta).sum(0)
            deta += r32(uu * mu[i][None, :])
            detas += E * ta * mu[i][None, :]
        if D > 0:
            if exact:
                dF[sl], dV = deta @ V, dV + deta.T @ F[sl]
            else:
                tot = acc32 if bwd == "valu" else (lambda a, ax: a.sum(ax))
                dF[sl] = np.stack([tot(f32(deta * V[None, :, d]), 1) for d in range(D)], 1)
                dV = dV + np.stack([tot(f32(deta * F[sl, d:d + 1]), 0) for d in range(D)], 1)
            dFs[sl] = detas @ np.abs(V)
            dVs += detas.T @ np.abs(F[sl])
    g, sc = {}, {}
    # loc, ls: through mu = softplus(loc + exp(ls) eps), summed over the samples
    sig = sigmoid(u)
    logmu = np.log(mu)
    q1, q2, q3 = colsum[None, :] / (S * mu), logmu / (S * mu), (1.0 - sig) / S
    dx = (q1 + dmu - q2) * sig + q3
    dxs = (np.abs(q1) + dmus + np.abs(q2)) * sig + np.abs(q3)
    g["loc"], sc["loc"] = dx.sum(0), dxs.sum(0)
    g["ls"], sc["ls"] = (dx * eps * sd[None, :]).sum(0) + 1.0, (dxs * np.abs(eps) * sd[None, :]).sum(0) + 1.0
    if K > 0:
        chi = np.exp(vch)
        YtPsi, YW = Y.T @ psi, Y @ W
        g["W"] = YtPsi + dV[:, :K] - W * chi[None, :]
        sc["W"] = dVs[:, :K] + np.abs(YtPsi) + np.abs(W * chi[None, :])
        w2 = (W * W).sum(0)
        g["v"] = -0.5 * chi * w2 + 0.5 * G + 1.0 - chi
        sc["v"] = 0.5 * chi * w2 + 0.5 * G + 1.0 + chi
        g["psi"] = YW + dF[:, :K] - psi
        sc["psi"] = np.abs(YW) + dFs[:, :K] + np.abs(psi)
    else:
        g["W"], g["v"], g["psi"] = np.zeros((G, 0)), np.zeros(0), np.zeros((N, 0))
        sc["W"], sc["v"], sc["psi"] = np.zeros((G, 0)), np.zeros(0), np.zeros((N, 0))
    if P > 0 and K > 0:
        g["beta"], sc["beta"] = fc["YtX"] + dV[:, K:], np.abs(fc["YtX"]) + dVs[:, K:]
    else:
        g["beta"], sc["beta"] = np.zeros((G, P)), np.zeros((G, P))
    # gamma_logits
    au = np.asarray(st["alpha_unconstr"], dtype=np.float64)
    log_alpha = au - logsumexp(au)
    f = A - s[:, None] * logZ.mean(0) + log_alpha[None, :] - log_gamma
    fs = np.abs(A) + s[:, None] * np.abs(logZ).mean(0) + np.abs(log_alpha)[None, :] + np.abs(log_gamma)
    if fc["extra"] is not None:
        f, fs = f + fc["extra"], fs + np.abs(fc["extra"])
    with np.errstate(invalid="ignore"):
        # xlogy semantics: an impossible clone (A = -inf) has gamma = 0 in any state the tests build; 0 * -inf is taken as 0, as `tf$where(gamma == 0, 0, ..)`
        gf, gfs = np.where(gamma == 0.0, 0.0, gamma * f), np.where(gamma == 0.0, 0.0, gamma * fs)
        g["gamma_logits"] = np.where(gamma == 0.0, 0.0, gamma * (f - gf.sum(1, keepdims=True)))
        sc["gamma_logits"] = np.where(gamma == 0.0, 0.0, gamma * (fs + gfs.sum(1, keepdims=True)))
    # alpha_unconstr: d / d log_alpha of [sum gamma log_alpha + Dirichlet(1 / C)(alpha + 1e-3)], then through log_softmax
    alpha = np.exp(log_alpha)
    sg = gamma.sum(0)
    dir_ = (1.0 / C - 1.0) * alpha / (alpha + 1e-3)
    dla, dlas = sg + dir_, np.abs(sg) + np.abs(dir_)
    g["alpha_unconstr"] = dla - alpha * dla.sum()
    sc["alpha_unconstr"] = dlas + alpha * dlas.sum()
    if not exact:
        g = {n: f32(a) for n, a in g.items()}                     # (the update launches store float32)
    return g, sc


def ref_gradients(fc, st, eps):
    """(gradient, scale) for every variable of VAR_NAMES at state ``st`` and draws ``eps`` [S, G] (or [G]), float64 throughout."""
    return _evaluate(fc, st, eps, None)


def operand_model(fc, st, eps, family):
    """The gradients with ``family``'s documented operand roundings (module docstring) and float64 accumulation."""
    return _evaluate(fc, st, eps, family)[0]


# ------------------------------------------------------------------------------------------------------------------ the states
STATE_KINDS = ("generic", "wide", "peaked", "zero_L", "exact")


def _peak(rng, N, C):
    gl = f32(rng.normal(size=(N, C)) * 0.3)
    top = rng.integers(0, C, size=N)
    gl[np.arange(N), top] += 30.0
    gl[np.arange(N), (top + 1) % C] -= 30.0 if C > 1 else 0.0
    return f32(gl)


def var_shapes(case):
    N, G = case["Y"].shape
    C, K = case["L"].shape[1], int(case["K"])
    P = 0 if case.get("X") is None else np.asarray(case["X"]).reshape(N, -1).shape[1]
    return {"W": (G, K), "v": (K,), "psi": (N, K), "beta": (G, P), "alpha_unconstr": (C,), "loc": (G,), "ls": (G,), "gamma_logits": (N, C)}


def build_state(kind, seed, **shape):
    """(case, S0) of kind ``kind`` for ``make_case(seed=seed, **shape)``, every value float32-representable.
    generic: ``perturbed_state``.
    wide:    psi up to +-8 against loadings up to +-2: the per-cell exponent shift differs strongly between neighbouring cells of one 16-cell tile; the extreme
             cells sit first and last in the array and last in the last FULL tile (N not a multiple of 16: the last cell sits last in a partial tile).
    peaked:  gamma_logits of +-30: coef spans many orders of magnitude within a cell.
    zero_L:  a tenth of the genes have L = 0 in one clone and no counts in any cell (nothing is counted where a clone has no copy: xlogy(0, 0) = 0).
    exact:   a state whose matrix-core operands E and M = mu L carry NO split error, so that coef is the only operand left with anything to lose -- the one
             state in which coef's THIRD bf16 part (2^-17 of coef) stands against the scale alone and not beside a forward split error of its own size.
             Every gene has the same loadings (W and beta constant down their columns: eta_ng does not depend on g, the per-cell shift takes all of it and
             E = 1 exactly); loc is an integer in [40, 256 / max L] and ls = -40 (mu = softplus(loc + 4e-18 eps) = loc to the last bit of float64: exp(-40) =
             4e-18; mu L is an integer of at most eight bits, one bf16 part); Z = sum_g mu L is an integer below 2^24.  psi and the
             posteriors vary (psi generic, gamma_logits peaked as above), so d/dF, d/dV and d/dmu all carry the coef of one clone per cell, unaveraged."""
    assert kind in STATE_KINDS, kind
    case = make_case(seed=seed, **shape)
    N, G = case["Y"].shape
    C, K = case["L"].shape[1], int(case["K"])
    rng = np.random.default_rng(seed + 2000)
    if kind == "zero_L":
        L, Y = case["L"].copy(), case["Y"].copy()
        zg = rng.choice(np.arange(1, G), size=max(2, G // 10), replace=False)      # (gene 0 keeps every cell non-empty)
        Y[:, zg] = 0.0
        L[zg, rng.integers(0, C, size=zg.size)] = 0.0
        case["L"], case["Y"] = L, Y
    st = perturbed_state(var_shapes(case), seed=seed + 1000)
    if kind == "wide" and K > 0:
        psi = f32(rng.uniform(-8.0, 8.0, size=(N, K)))
        last_full = (N // 16) * 16 - 1
        for k in range(K):
            psi[0, k], psi[N - 1, k], psi[1, k] = 8.0, -8.0, -8.0
            if last_full > 1:
                psi[last_full, k] = 8.0 if k % 2 == 0 else -8.0
        W = f32(rng.uniform(-2.0, 2.0, size=(G, K)))
        W[0, :], W[G - 1, :] = 2.0, -2.0
        st["psi"], st["W"] = psi, W
    if kind in ("peaked", "exact"):
        st["gamma_logits"] = _peak(rng, N, C)
    if kind == "exact":
        top = int(256 // case["L"].max())
        assert top >= 48, top
        st["loc"] = f32(rng.integers(40, top + 1, size=G))
        st["ls"] = np.full(G, -40.0)
        P = st["beta"].shape[1]
        st["W"] = np.tile(np.array([0.75, -0.5, 0.375])[:K], (G, 1))
        st["beta"] = np.tile(np.array([0.25, -0.625])[:P], (G, 1))
    return case, st
