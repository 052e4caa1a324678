"""Float64 reference for the series form of the contraction (clonealign_amd/csrc/ca_poly.hip, ca_polymom.hip.h), plain numpy, no GPU.

Three things, for the shapes the series form takes (K = 1, P = 0, S = 1):

* ``ref_gradients``: the gradient the loop applies at a given state and draw, written directly -- no bins, no series -- and beside every gradient element
  its SCALE: the sum of the magnitudes of the summands that make it.  Every comparison against it is ``|test - reference| <= tol * scale`` element by element
  (``worst_ratio``): a max-norm over an array hides one mis-binned gene behind the largest one.
* ``series_contraction``: the algorithm as the kernels run it (bin geometry of ca_pm_B_body, forward moments B, Horner for Z and dZ/dx, backward moments Q,
  per-gene q and q'), restated in float64 with the constants read from ca_poly.h, and ``direct_contraction``, the same four sums with their scales.
* the states the host and the GPU tests share (``SPECS``, ``build_state``): one per bin count and code path of the three kernels.
"""
import math
import os
import re

import numpy as np
from scipy.special import gammaln, logsumexp, xlogy

from tests._cases import make_case, perturbed_state

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "clonealign_amd", "csrc")
VAR_NAMES = ("W", "v", "psi", "beta", "alpha_unconstr", "loc", "ls", "gamma_logits")
LOG2PI = math.log(2.0 * math.pi)


def poly_constants(header=None):
    """CA_PL_R (degree of a bin's Taylor piece), CA_PL_A (bound of |x| times half a bin's width), CA_PL_NB (most bins), CA_PL_NBL, as ca_poly.h defines them."""
    text = open(header or os.path.join(_CSRC, "ca_poly.h")).read()
    out = {}
    for name, conv in (("CA_PL_R", int), ("CA_PL_NB", int), ("CA_PL_A", float), ("CA_PL_NBL", int)):
        m = re.search(r"^\s*#\s*define\s+" + name + r"\s+([0-9.eE+-]+)", text, re.M)
        assert m, name
        out[name] = conv(m.group(1))
    return out


def genes_per_partial():
    m = re.search(r"constexpr\s+int\s+CA_PM_GPB\s*=\s*(\d+)\s*;", open(os.path.join(_CSRC, "ca_polymom.hip.h")).read())
    assert m
    return int(m.group(1))


def softplus(x):
    return np.logaddexp(0.0, x)


def sigmoid(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))


# ------------------------------------------------------------------------------------------------------------------ the direct contraction
def direct_contraction(x, v, M, coef, L, mu):
    """The four sums the series form replaces, cell by gene, and the scale of every element.  x [N], v [G], M = mu * L [G, C], coef [N, C], L [G, C], mu [G].
    Z [N, C] = sum_g M_gc E_ng;  dZ [N, C] = sum_g v_g M_gc E_ng;  dmu [G] = sum_n sum_c coef_nc L_gc E_ng;  dV [G] = mu_g sum_n sum_c coef_nc x_n L_gc E_ng."""
    E = np.exp(np.outer(x, v))
    out = {"Z": E @ M, "dZ": E @ (v[:, None] * M)}
    sc = {"Z": out["Z"].copy(), "dZ": E @ (np.abs(v)[:, None] * M)}
    t = coef @ L.T
    ta = np.abs(coef) @ np.abs(L).T
    out["dmu"] = (E * t).sum(0)
    sc["dmu"] = (E * ta).sum(0)
    out["dV"] = mu * (E * t * x[:, None]).sum(0)
    sc["dV"] = np.abs(mu) * (E * ta * np.abs(x)[:, None]).sum(0)
    return out, sc


# ------------------------------------------------------------------------------------------------------------------ the series form, restated
def bin_geometry(xmax, mn, mx, consts=None):
    """(vlo, delta, nb) as ca_pm_B_body publishes them.  The bins [vlo + b delta, vlo + (b + 1) delta) are expanded around their centres vlo + (b + 0.5) delta.
    All loadings equal (W = 0 at the start of every fit): one bin of width 1 CENTRED on the common value, so that v - v_b = 0 and the series is its first term."""
    c = consts or poly_constants()
    width = mx - mn
    nb = int(math.ceil(xmax * width / (2.0 * c["CA_PL_A"])))
    nb = min(max(nb, 1), c["CA_PL_NB"])
    if width > 0.0:
        return mn, width / nb, nb
    return mn - 0.5, 1.0, nb


def bin_of(v, vlo, delta, nb):
    return np.clip(np.floor((v - vlo) / delta).astype(np.int64), 0, nb - 1)


def series_contraction(x, v, M, coef, L, mu, consts=None, geometry=bin_geometry):
    """direct_contraction's four sums by the series algorithm, in float64, the loops in the kernels' order of ideas (not of additions)."""
    c = consts or poly_constants()
    R = c["CA_PL_R"]
    N, G, C = x.shape[0], v.shape[0], M.shape[1]
    vlo, delta, nb = geometry(float(np.abs(x).max()), float(v.min()), float(v.max()), c)
    b = bin_of(v, vlo, delta, nb)
    vb = vlo + (np.arange(nb) + 0.5) * delta
    dv = v - vb[b]
    # forward moments B[b][k][c] = sum_{g in bin b} M_gc dv^k / k!   (the 1 / k! inside the powers, as ca_pm_B_body builds them)
    pw = np.empty((G, R + 1))
    p = np.ones(G)
    for k in range(R + 1):
        pw[:, k] = p
        p = p * dv * (1.0 / (k + 1))
    B = np.zeros((nb, R + 1, C))
    for bi in range(nb):
        sel = b == bi
        B[bi] = pw[sel].T @ M[sel]
    # per cell: Z and dZ/dx by Horner over the bins (k_poly_cell)
    Z = np.zeros((N, C))
    dZ = np.zeros((N, C))
    eb = np.exp(np.outer(x, vb))                                   # [N, nb]
    for bi in range(nb):
        pz = np.tile(B[bi, R], (N, 1))
        dp = np.zeros((N, C))
        for k in range(R - 1, -1, -1):
            dp = dp * x[:, None] + pz
            pz = pz * x[:, None] + B[bi, k]
        Z += eb[:, bi, None] * pz
        dZ += eb[:, bi, None] * (vb[bi] * pz + dp)
    # backward moments Q[b][k][c] = sum_n coef_nc x_n^k exp(x_n v_b), k = 0 .. R + 1, and T_k = Q_k / k!   (k_poly_cell, k_poly_red mode 1)
    xp = np.empty((N, R + 2))
    q = np.ones(N)
    for k in range(R + 2):
        xp[:, k] = q
        q = q * x
    T = np.einsum("nc,nk,nb->bkc", coef, xp, eb)
    f = 1.0
    for k in range(R + 2):
        if k >= 2:
            f *= k
        T[:, k, :] /= f
    # per gene (k_poly_gene): q = sum_{k <= R} dv^k T_k,  q' = sum_{k <= R} dv^k (k + 1) T_{k+1}
    Tg = T[b]                                                      # [G, R + 2, C]
    qv = Tg[:, R, :].copy()
    dq = (R + 1) * Tg[:, R + 1, :]
    for k in range(R - 1, -1, -1):
        qv = qv * dv[:, None] + Tg[:, k, :]
        dq = dq * dv[:, None] + (k + 1) * Tg[:, k + 1, :]
    return {"Z": Z, "dZ": dZ, "dmu": (L * qv).sum(1), "dV": mu * (L * dq).sum(1)}, {"nb": nb, "vlo": vlo, "delta": delta, "bin": b}


# ------------------------------------------------------------------------------------------------------------------ the gradients and their scales
def fit_constants(Y, L):
    Y = np.asarray(Y, dtype=np.float64)
    L = np.asarray(L, dtype=np.float64)
    s = Y.sum(1)
    with np.errstate(divide="ignore"):
        A = xlogy(Y[:, :, None], L[None, :, :]).sum(1)
    return {"Y": Y, "L": L, "s": s, "colsum": Y.sum(0), "A": A, "cn": gammaln(s + 1.0) - gammaln(Y + 1.0).sum(1)}


def forward_parts(fc, st, eps):
    """What the contraction is made of at state ``st`` (a dict of VAR_NAMES) and draw ``eps`` [G]: x, v, mu, M, gamma, coef and the pieces the gradients share."""
    L, s = fc["L"], fc["s"]
    x = np.asarray(st["psi"], dtype=np.float64).reshape(-1)
    v = np.asarray(st["W"], dtype=np.float64).reshape(-1)
    loc, ls = np.asarray(st["loc"], dtype=np.float64), np.asarray(st["ls"], dtype=np.float64)
    e = np.asarray(eps, dtype=np.float64).reshape(-1)
    sd = np.exp(ls)
    u = loc + sd * e
    mu = softplus(u)
    M = mu[:, None] * L
    E = np.exp(np.outer(x, v))
    Z = E @ M
    gl = np.asarray(st["gamma_logits"], dtype=np.float64)
    log_gamma = gl - logsumexp(gl, 1, keepdims=True)
    gamma = np.exp(log_gamma)
    coef = -gamma * s[:, None] / Z
    return dict(x=x, v=v, loc=loc, ls=ls, eps=e, sd=sd, u=u, mu=mu, M=M, E=E, Z=Z, log_gamma=log_gamma, gamma=gamma, coef=coef)


def ref_gradients(fc, st, eps):
    """(gradient, scale) of d ELBO / d variable for every variable of VAR_NAMES at state ``st`` and draw ``eps`` (K = 1, P = 0, S = 1)."""
    Y, L, s, A, colsum = fc["Y"], fc["L"], fc["s"], fc["A"], fc["colsum"]
    p = forward_parts(fc, st, eps)
    x, v, mu, M, E, Z, gamma, log_gamma, coef = p["x"], p["v"], p["mu"], p["M"], p["E"], p["Z"], p["gamma"], p["log_gamma"], p["coef"]
    G, C = L.shape
    g, sc = {}, {}
    d, dsc = direct_contraction(x, v, M, coef, L, mu)
    # loc, ls: through mu = softplus(loc + exp(ls) eps)
    sig = sigmoid(p["u"])
    logmu = np.log(mu)
    q1, q2, q3 = colsum / mu, logmu / mu, 1.0 - sig
    dx = (q1 + d["dmu"] - q2) * sig + q3
    dxs = (np.abs(q1) + dsc["dmu"] + np.abs(q2)) * sig + np.abs(q3)
    g["loc"], sc["loc"] = dx, dxs
    g["ls"], sc["ls"] = dx * p["eps"] * p["sd"] + 1.0, dxs * np.abs(p["eps"]) * p["sd"] + 1.0
    # W
    vch = float(np.asarray(st["v"], dtype=np.float64).reshape(-1)[0])
    chi = math.exp(vch)
    YtPsi = Y.T @ x
    g["W"] = (YtPsi + d["dV"] - chi * v).reshape(G, 1)
    sc["W"] = (dsc["dV"] + np.abs(YtPsi) + np.abs(chi * v)).reshape(G, 1)
    # v (the log precision of the loadings' prior)
    w2 = float((v * v).sum())
    g["v"] = np.array([-0.5 * chi * w2 + 0.5 * G + 1.0 - chi])
    sc["v"] = np.array([0.5 * chi * w2 + 0.5 * G + 1.0 + chi])
    # psi
    YW = Y @ v
    g["psi"] = (YW + (coef * d["dZ"]).sum(1) - x).reshape(-1, 1)
    sc["psi"] = (np.abs(YW) + (np.abs(coef) * dsc["dZ"]).sum(1) + np.abs(x)).reshape(-1, 1)
    g["beta"], sc["beta"] = np.zeros((G, 0)), np.zeros((G, 0))
    # gamma_logits
    au = np.asarray(st["alpha_unconstr"], dtype=np.float64)
    log_alpha = au - logsumexp(au)
    logZ = np.log(Z)
    f = A - s[:, None] * logZ + log_alpha[None, :] - log_gamma
    fs = np.abs(A) + s[:, None] * np.abs(logZ) + np.abs(log_alpha)[None, :] + np.abs(log_gamma)
    g["gamma_logits"] = gamma * (f - (gamma * f).sum(1, keepdims=True))
    sc["gamma_logits"] = gamma * (fs + (gamma * fs).sum(1, keepdims=True))
    # alpha_unconstr: d / d log_alpha of [sum gamma log_alpha + Dirichlet(1 / C)(alpha + 1e-3)], then through log_softmax
    alpha = np.exp(log_alpha)
    sg = gamma.sum(0)
    dir_ = (1.0 / C - 1.0) * alpha / (alpha + 1e-3)
    dla, dlas = sg + dir_, np.abs(sg) + np.abs(dir_)
    g["alpha_unconstr"] = dla - alpha * dla.sum()
    sc["alpha_unconstr"] = dlas + alpha * dlas.sum()
    return g, sc


def worst_ratio(test, ref, scale):
    """max over ALL elements of |test - ref| / scale (0 for an empty array); a non-finite entry or a zero scale under a non-zero difference gives inf."""
    test, ref, scale = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (test, ref, scale))
    assert test.shape == ref.shape == scale.shape, (test.shape, ref.shape, scale.shape)
    if test.size == 0:
        return 0.0
    d = np.abs(test - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0.0, 0.0, d / scale)
    r = np.where(np.isfinite(r), r, np.inf)
    return float(r.max())


# ------------------------------------------------------------------------------------------------------------------ the shared states
# name: N, G, C (N = None: made of the device's CU count, two_pass_cells), max |psi|, (min W, max W), W on a grid of this step or None, the bin count it is named for
SPECS = {
    "one_bin":      dict(N=77, G=33, C=3, xmax=1.0, w=(-1.9, 2.0), grid=None, nb=1),
    "two_bins":     dict(N=130, G=97, C=4, xmax=4.0, w=(-1.0, 1.0), grid=None, nb=2),
    "four_bins":    dict(N=45, G=257, C=5, xmax=4.0, w=(-2.0, 2.0), grid=0.125, nb=4),
    "five_bins":    dict(N=300, G=130, C=8, xmax=4.0, w=(-2.25, 2.25), grid=None, nb=5),
    "nine_bins":    dict(N=300, G=97, C=6, xmax=4.0, w=(-4.35, 4.35), grid=None, nb=9),
    "bins_32":      dict(N=300, G=97, C=8, xmax=8.0, w=(-7.95, 7.95), grid=None, nb=32),
    "equal_0_x3":   dict(N=130, G=64, C=3, xmax=3.0, w=(0.0, 0.0), grid=None, nb=1),
    "equal_0_x8":   dict(N=130, G=64, C=3, xmax=8.0, w=(0.0, 0.0), grid=None, nb=1),
    "equal_0_x11":  dict(N=130, G=64, C=3, xmax=11.0, w=(0.0, 0.0), grid=None, nb=1),
    "equal_p_x3":   dict(N=130, G=64, C=3, xmax=3.0, w=(0.75, 0.75), grid=None, nb=1),
    "equal_p_x8":   dict(N=130, G=64, C=3, xmax=8.0, w=(0.75, 0.75), grid=None, nb=1),
    "equal_p_x11":  dict(N=130, G=64, C=3, xmax=11.0, w=(0.75, 0.75), grid=None, nb=1),
    "two_pass_c8":  dict(N=None, G=96, C=8, xmax=4.0, w=(-1.25, 1.25), grid=None, nb=3),
    "two_pass_c4":  dict(N=None, G=96, C=4, xmax=4.0, w=(-1.25, 1.25), grid=None, nb=3),
}


def two_pass_cells(n_cu, C):
    """Two cell blocks per CU, 256 / C cells per pass (C a power of two): five blocks make two full passes, one a full and a partial one, the rest one."""
    cpb = 256 // C
    return 2 * n_cu * cpb + 5 * cpb + 7


def build_state(name, n_cu=None):
    """(case, S0): the constructor arguments (tests/_cases.make_case) and the state of SPECS[name], every value float32-representable.  psi holds an exact 0,
    +max and -max; W holds its minimum and maximum (and, on a grid, every grid point: genes exactly on every interior bin boundary)."""
    sp = SPECS[name]
    seed = 101 + list(SPECS).index(name)
    G, C = sp["G"], sp["C"]
    N = sp["N"] if sp["N"] is not None else two_pass_cells(n_cu, C)
    case = make_case(seed=seed, N=N, G=G, C=C, K=1)
    shapes = {"W": (G, 1), "v": (1,), "psi": (N, 1), "beta": (G, 0), "alpha_unconstr": (C,), "loc": (G,), "ls": (G,), "gamma_logits": (N, C)}
    st = perturbed_state(shapes, seed=seed + 1000)
    rng = np.random.default_rng(seed + 2000)
    f32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)  # noqa: E731
    xm = float(np.float32(sp["xmax"]))
    psi = f32(rng.uniform(-xm, xm, size=N))
    psi[0], psi[1], psi[2] = 0.0, xm, -xm
    psi[N - 1] = -xm if N % 2 else xm               # (the last cell of the partial pass sits on the edge as well)
    lo, hi = (float(np.float32(t)) for t in sp["w"])
    if sp["grid"]:
        pts = np.arange(lo, hi + sp["grid"] / 2, sp["grid"])
        W = np.concatenate([pts, rng.choice(pts, size=G - pts.size)])
        W = rng.permutation(W)
    elif hi > lo:
        W = f32(rng.uniform(lo, hi, size=G))
        W[G // 2], W[G - 1] = lo, hi                 # (the maximum on the last gene: a second k_poly_gene block or a short last partial meets the clamp)
    else:
        W = np.full(G, lo)
    st["psi"], st["W"] = psi.reshape(N, 1), f32(W).reshape(G, 1)
    return case, st


def expected_bins(st, consts=None):
    """The bin count ca_pm_B_body takes for the arrays of ``st``: ceil(max|psi| (max W - min W) / (2 CA_PL_A)), at least one."""
    c = consts or poly_constants()
    x, w = np.abs(st["psi"]).max(), st["W"].max() - st["W"].min()
    return max(1, int(math.ceil(x * w / (2.0 * c["CA_PL_A"]))))


def poly_covers(xmax, vlo, vhi, steps, step_bound, consts=None):
    """ca_poly_covers (ca_poly.h), restated: can the series form cover a state whose ranges were these ``steps`` Adam steps ago?"""
    c = consts or poly_constants()
    x, wdt = xmax + steps * step_bound, (vhi - vlo) + 2.0 * steps * step_bound
    return x * wdt <= 2.0 * c["CA_PL_A"] * c["CA_PL_NB"]


def adam_step_bound(lr=0.1, b1=0.9, b2=0.999):
    """ca_adam_step_bound (ca_eng_state.inc), restated: the Cauchy-Schwarz bound of |m| / sqrt(v) times the supremum over t of the bias correction."""
    if not (b1 >= 0 and 0 < b2 < 1 and b1 * b1 < b2 and lr > 0):
        return -1.0
    sup, p1, p2 = 0.0, 1.0, 1.0
    for _ in range(200000):
        p1 *= b1
        p2 *= b2
        sup = max(sup, math.sqrt(1.0 - p2) / (1.0 - p1))
    return lr * sup * (1.0 - b1) / math.sqrt((1.0 - b2) * (1.0 - b1 * b1 / b2))


def step_bound_margins():
    """The factors the engine's two uses put on ca_adam_step_bound, read from the sources: (poly_step_bound's, ca_eng_loop.inc; ys_step_bound's, ca_eng_create.inc).
    Fails where either use is not written as that one function times a constant."""
    loop = open(os.path.join(_CSRC, "ca_eng_loop.inc")).read()
    create = open(os.path.join(_CSRC, "ca_eng_create.inc")).read()
    body = re.search(r"inline double poly_step_bound\(const ca_engine\* h\) \{(.*?)\n\}", loop, re.S)
    assert body, "poly_step_bound"
    mp = re.search(r"return h->adam_bound \* ([0-9.]+);", body.group(1))
    my = re.search(r"h->ys_step_bound = \(float\)\(([0-9.]+) \* h->adam_bound\)", create)
    one = re.search(r"h->adam_bound = ca_adam_step_bound\(h->opt\.learning_rate, h->opt\.beta1, h->opt\.beta2\)", create)
    assert mp and my and one, ("poly_step_bound (ca_eng_loop.inc) / ys_step_bound (ca_eng_create.inc) are no longer written as h->adam_bound times a constant, or "
                               "adam_bound no longer comes from ca_adam_step_bound: update this restatement and adam_step_bound above to the sources", bool(mp), bool(my), bool(one))
    return float(mp.group(1)), float(my.group(1))


def poly_step_bound(lr=0.1, b1=0.9, b2=0.999):
    """poly_step_bound (ca_eng_loop.inc): no Adam step moves a variable further."""
    return adam_step_bound(lr, b1, b2) * step_bound_margins()[0]


def ys_step_bound(lr=0.1, b1=0.9, b2=0.999):
    """ca_engine::ys_step_bound (ca_eng_create.inc): what the int8 stream's lagged exponents allow per step."""
    return float(np.float32(adam_step_bound(lr, b1, b2) * step_bound_margins()[1]))


def state_for(model_cls, case, st, **kw):
    """A float64 oracle holding ``st``."""
    m = model_cls(**case, dtype="float64", **kw)
    for n in VAR_NAMES:
        setattr(m, n, np.asarray(st[n], dtype=np.float64).copy())
    return m
