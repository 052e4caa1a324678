"""project_cells on the CPU: the float64 numpy restatement ``api._project_cells_host`` of ca_project_cells (per-cell MAP psi under a fit's gene-level
parameters by generalised EM with one safeguarded Newton step per round, and the clone posterior at it) and ``api.project_cells`` through an engine
without the device method.  Planted problems: clones, psi ~ N(0, 1) and multinomial counts drawn from the model itself."""
import numpy as np
import pytest

import clonealign_amd as ca
from clonealign_amd.api import _project_cells_host

CASES = {"300x200x4 K=1": (300, 200, 4, 1, 1.0, 1), "200x150x5 K=2": (200, 150, 5, 2, 0.8, 1)}


def planted(N, G, C, K, sd_w, seed, depth=400, zeros=False):
    rng = np.random.default_rng(seed)
    L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
    if zeros:
        L[rng.choice(G, 6, replace=False), rng.integers(0, C, 6)] = 0.0   # copy number 0 in one clone on a few genes
    mu = rng.lognormal(0, 1, G)
    W = rng.normal(size=(G, K)) * sd_w
    alpha = rng.dirichlet(np.full(C, 20.0))
    z = rng.choice(C, N, p=alpha)
    psi = rng.normal(size=(N, K))
    p = mu[None] * L[:, z].T * np.exp(psi @ W.T)
    p /= p.sum(1, keepdims=True)
    s = rng.integers(depth // 2, depth * 2, N)
    Y = np.stack([rng.multinomial(s[n], p[n]) for n in range(N)]).astype(np.float64)
    return dict(Y=Y, L=L, mu=mu, W=W, alpha=alpha, z=z, psi=psi, E=mu[:, None] * L, lp=np.log(alpha)[None] + np.zeros((N, C)))


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    N, G, C, K, sd, seed = CASES[request.param]
    p = planted(N, G, C, K, sd, seed, zeros=True)
    p["K"], p["name"] = K, request.param
    p["out"] = _project_cells_host(p["Y"], p["E"], p["W"], K, 0, None, p["lp"], None)
    return p


class HostOnly:                                                       # a live engine without the device methods: the CPU host forms
    def __init__(self, N, G):
        self.N, self.G = N, G


def fit_of(p, names=None):
    C = p["L"].shape[1]
    return ca.ClonealignFit(ml_params={"mu": p["mu"], "alpha": p["alpha"], "W": p["W"] if p["W"].shape[1] else None},
                            clone_names=names or [f"c{i}" for i in range(C)])


def F_of(p, psi):
    """F_n(psi) for all cells, written out directly: logsumexp_c(Multinomial log-prob + log alpha) - |psi|^2 / 2"""
    from scipy.special import gammaln, logsumexp
    Y, E = p["Y"], p["E"]
    eta = psi @ p["W"].T
    s = Y.sum(1)
    logits = np.log(np.where(E == 0, 1.0, E))[None] + eta[:, :, None]                     # [N, G, C]
    logits = np.where((E == 0)[None], -np.inf, logits)
    logp = logits - logsumexp(logits, axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        ll = np.where(Y[:, :, None] > 0, Y[:, :, None] * logp, 0.0).sum(1) + (gammaln(s + 1) - gammaln(Y + 1).sum(1))[:, None]
    return logsumexp(ll + p["lp"], axis=1) - 0.5 * (psi ** 2).sum(1)


def test_objective_never_decreases_from_round_to_round(case):
    p, K = case, case["K"]
    prev = None
    for t in range(0, 16):
        r = _project_cells_host(p["Y"], p["E"], p["W"], K, 0, None, p["lp"], None, max_iter=t)
        F = r["objective"]
        np.testing.assert_allclose(F, F_of(p, r["psi"]), rtol=1e-10)   # the objective IS F at the returned psi
        if prev is not None:
            assert (F >= prev - 1e-9 * np.abs(prev)).all(), (t, float((F - prev).min()))
        prev = F
    assert r["converged"].all() and r["rounds"].max() <= 15            # every cell had stopped moving by round 15
    assert np.array_equal(r["psi"], p["out"]["psi"])                   # a frozen cell no longer moves


def test_frozen_cells_sit_at_a_stationary_point(case):
    p, K, out = case, case["K"], case["out"]
    assert out["converged"].all()
    Y, E, W = p["Y"], p["E"], p["W"]
    s = Y.sum(1)
    psi, gamma = out["psi"], out["clone_probs"]
    w = np.exp(psi @ W.T)                                             # the analytic gradient: B - s sum_c gamma_c mean_c - psi
    mean = np.stack([((w * W[:, k]) @ E) / (w @ E) for k in range(K)], axis=2)
    grad = Y @ W - s[:, None] * np.einsum("nc,nck->nk", gamma, mean) - psi
    assert (np.abs(grad).max(1) <= 1e-6 * (1 + s)).all(), float((np.abs(grad).max(1) / (1 + s)).max())
    h = 1e-5
    for k in range(K):                                                # ... agrees with a central difference of F around a point off the optimum
        e = np.zeros(K)
        e[k] = h
        at = psi + 0.1
        fd = (F_of(p, at + e) - F_of(p, at - e)) / (2 * h)
        w = np.exp(at @ W.T)
        r0 = _project_cells_host(Y, E, W, K, 0, None, p["lp"], at, max_iter=0)
        mean = np.stack([((w * W[:, j]) @ E) / (w @ E) for j in range(K)], axis=2)
        ga = Y @ W - s[:, None] * np.einsum("nc,nck->nk", r0["clone_probs"], mean) - at
        assert np.abs(fd - ga[:, k]).max() <= 1e-5 * (1 + s.max())


def test_a_fit_without_w_equals_assign_cells_bit_for_bit():
    p = planted(120, 90, 3, 0, 0.0, 5)
    fit = fit_of(p)
    a = ca.assign_cells(fit, p["Y"], p["L"], engine=HostOnly(120, 90))
    b = ca.project_cells(fit, p["Y"], p["L"], engine=HostOnly(120, 90))
    for k in ("clone_probs", "loglik", "clone_loglik"):
        assert np.array_equal(a[k], b[k]), k
    assert list(a["clone"]) == list(b["clone"]) and b["psi"].shape == (120, 0) and not b["rounds"].any() and b["converged"].all()
    r = _project_cells_host(p["Y"], p["E"], None, 0, 0, None, p["lp"], None)   # the restatement itself at K = 0: the same numbers, zero rounds
    np.testing.assert_allclose(r["clone_probs"], a["clone_probs"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["ll"], a["clone_loglik"], rtol=1e-12)
    assert not r["rounds"].any() and r["converged"].all()


def test_no_rounds_equals_assign_cells_at_the_starting_psi(case):
    p, K = case, case["K"]
    N, G = p["Y"].shape
    start = np.random.default_rng(3).normal(size=(N, K)) * 0.5
    fit = fit_of(p)
    a = ca.assign_cells(fit, p["Y"], p["L"], psi=start, engine=HostOnly(N, G))
    b = ca.project_cells(fit, p["Y"], p["L"], psi_start=start, max_iter=0, engine=HostOnly(N, G))
    assert np.array_equal(b["psi"], start) and not b["converged"].any() and not b["rounds"].any()
    np.testing.assert_allclose(b["clone_loglik"], a["clone_loglik"], rtol=1e-12)
    np.testing.assert_allclose(b["clone_probs"], a["clone_probs"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(b["loglik"], a["loglik"], rtol=1e-12)
    assert list(a["clone"]) == list(b["clone"])
    again = ca.recompute_clone_assignment(b, 0.5)
    assert (again["clone"] != "unassigned").sum() >= (b["clone"] != "unassigned").sum()


def test_a_cell_without_a_possible_clone_keeps_its_start_and_its_neighbours_are_finite(case):
    p, K = case, case["K"]
    N, C = p["lp"].shape
    lp = p["lp"].copy()
    lp[7] = -np.inf                                                  # excluded in every clone through the prior ...
    lp[9, 1] = -np.inf                                               # ... and in one clone only
    Y = p["Y"].copy()
    g0 = np.flatnonzero((p["L"] == 0).sum(1) == 0)[0]
    E = p["E"].copy()
    E[g0] = 0.0                                                      # ... and through a positive count where every clone has copy number 0
    Y[:, g0] = 0
    Y[11, g0] = 3
    start = np.random.default_rng(4).normal(size=(N, K))
    r = _project_cells_host(Y, E, p["W"], K, 0, None, lp, start)
    for n in (7, 11):
        assert np.array_equal(r["psi"][n], start[n]) and np.isnan(r["clone_probs"][n]).all() and not r["converged"][n] and r["rounds"][n] == 0
        assert r["objective"][n] == -np.inf
    assert np.isneginf(r["ll"][11]).all() and np.isfinite(r["ll"][7]).any()
    rest = np.setdiff1d(np.arange(N), [7, 11])
    assert np.isfinite(r["psi"][rest]).all() and np.isfinite(r["clone_probs"][rest]).all() and np.isfinite(r["objective"][rest]).all()
    assert r["clone_probs"][9, 1] == 0.0 and r["converged"][rest].all()
    np.testing.assert_allclose(r["clone_probs"][rest].sum(1), 1.0, rtol=1e-12)
    keep = np.setdiff1d(np.arange(N), [7, 9, 11])                     # a cell's result depends on its own row alone
    base = _project_cells_host(Y, E, p["W"], K, 0, None, p["lp"], start)
    assert np.array_equal(r["psi"][keep], base["psi"][keep])


def test_refusals_name_the_offender():
    p = planted(40, 30, 3, 1, 0.5, 2)
    Y, E, W, lp = p["Y"], p["E"], p["W"], p["lp"]

    def refused(words, *a, **k):
        with pytest.raises(ValueError) as ex:
            _project_cells_host(*a, **k)
        assert all(w in str(ex.value) for w in words), str(ex.value)
    refused(("K = -1",), Y, E, W, -1, 0, None, lp, None)
    refused(("K + P = 9", "[0, 8]"), Y, E, np.zeros((30, 9)), 1, 8, np.zeros((40, 8)), lp, None)
    refused(("needs V",), Y, E, None, 1, 0, None, lp, None)
    refused(("needs X",), Y, E, np.zeros((30, 2)), 1, 1, None, lp, None)
    refused(("max_iter = -1",), Y, E, W, 1, 0, None, lp, None, max_iter=-1)
    for bad in (0.0, -1.0, np.inf, np.nan):
        refused(("tol",), Y, E, W, 1, 0, None, lp, None, tol=bad)
        refused(("max_step",), Y, E, W, 1, 0, None, lp, None, max_step=bad)
    Eb = E.copy()
    Eb[17, 2] = -1.0
    refused(("gene 17", "clone 2"), Y, Eb, W, 1, 0, None, lp, None)
    Eb = E.copy()
    Eb[:, 1] = 0.0
    refused(("clone 1", "sums to"), Y, Eb, W, 1, 0, None, lp, None)
    Wb = W.copy()
    Wb[5, 0] = np.nan
    refused(("V has a non-finite", "gene 5"), Y, E, Wb, 1, 0, None, lp, None)
    X = np.zeros((40, 1))
    X[3, 0] = np.inf
    refused(("X has a non-finite", "cell 3"), Y, E, np.zeros((30, 2)), 1, 1, X, lp, None)
    st = np.zeros((40, 1))
    st[8, 0] = np.nan
    refused(("psi_start has a non-finite", "cell 8"), Y, E, W, 1, 0, None, lp, st)
    for bad in (np.inf, np.nan):
        lb = lp.copy()
        lb[6, 2] = bad
        refused(("log_prior", "cell 6", "clone 2"), Y, E, W, 1, 0, None, lb, None)
    fit = fit_of(p)
    with pytest.raises(ValueError, match="x is required exactly when"):
        ca.project_cells(fit, Y, p["L"], x=np.zeros((40, 1)), engine=HostOnly(40, 30))
    with pytest.raises(ValueError, match="extra_loglik"):
        ca.project_cells(fit, Y, p["L"], extra_loglik=np.zeros((40, 2)), engine=HostOnly(40, 30))


def test_labels_are_no_worse_than_at_the_prior_mean_and_better_where_w_matters(case):
    """Chosen on the CPU: seed 1 of the 200 x 150 x 5, K = 2 problem gives 191 of 200 labels at psi = 0 and 200 with the projected psi."""
    p = case
    N, G = p["Y"].shape
    names = [f"c{i}" for i in range(p["L"].shape[1])]
    fit = fit_of(p, names)
    lut = np.asarray(names, dtype=object)
    a = ca.assign_cells(fit, p["Y"], p["L"], 0.0, saturate=False, engine=HostOnly(N, G))
    b = ca.project_cells(fit, p["Y"], p["L"], 0.0, saturate=False, engine=HostOnly(N, G))
    right0, right = int((a["clone"] == lut[p["z"]]).sum()), int((b["clone"] == lut[p["z"]]).sum())
    print(f"{p['name']}: labels right at psi = 0 {right0} / {N}, with the projected psi {right} / {N}")
    assert right >= right0
    if p["K"] == 2:
        assert right >= right0 + 5
    assert np.array_equal(b["psi"], p["out"]["psi"]) and set(b["ml_params"]) == {"psi", "clone_probs"}
    np.testing.assert_allclose(b["loglik"], b["objective"] + 0.5 * (b["psi"] ** 2).sum(1))
    assert float(np.abs(b["psi"] - p["psi"]).mean()) < 0.2           # the planted psi is recovered to within its posterior width
