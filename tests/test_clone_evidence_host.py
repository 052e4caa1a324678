"""clone_evidence on the CPU: the float64 numpy restatement ``api._clone_evidence_host`` of ca_clone_evidence -- per (cell, clone) the evidence
``log Integral Normal(psi; 0, I) Multinomial(y | c, psi) dpsi`` by a Newton mode, the Laplace value and a Gauss-Hermite rule centred at the mode -- checked
against brute-force integration, and ``clone_evidence`` / ``assign_cells_marginal`` / ``heldout_evidence`` through an engine without the device method.

Measured (printed by the tests): K = 1, 12 cells x 40 genes x 3 clones, reads 0 .. 30000: the 12-node rule is off the adaptive integral by at most
1.6e-11 (sd(W) = 0.3) and 4.3e-7 nats (sd(W) = 1.0); 4 nodes 1.1e-5 / 7.4e-4; Laplace 4.1e-4 / 2.5e-2 nats.  The bar on 12 nodes is 1e-5 nats.
K = 2, 6 cells: against a 401 x 401 trapezoid grid over +-10 Laplace standard deviations per axis (the trapezoid rule converges geometrically for this
smooth, decaying integrand; at this spacing its own error is far below 1e-10) the 7 x 7 tensor rule measured 2.0e-7 nats and Laplace 7.9e-3.  The bar is
1e-5 nats -- the K = 1 bar: a tensor rule of 7 nodes per axis on a problem of sd(W) = 0.6 should do no worse than 12 nodes at sd(W) = 1 -- and the rule
must beat Laplace.
The planted model-choice problem (200 x 150 x 3, 200 - 1500 reads, K = 1, sd(W) = 0.5, seeds 0 - 4): the true K = 1 is ahead of K = 2 with a spurious
column by 387 - 419 nats (31 - 41 paired standard errors) and of K = 0 by 1.5e4 - 3.0e4 nats."""
import numpy as np
import pytest

import clonealign_amd as ca
from clonealign_amd.api import _clone_evidence_host, _clone_loglik_host, _project_cells_host, gauss_hermite_rule
from tests.test_gpu_clone_loglik import ref_ll
from tests.test_project_cells_host import HostOnly


def small(N, G, C, K, sd_w, seed, reads):
    rng = np.random.default_rng(seed)
    L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
    mu = rng.lognormal(0, 1, G)
    W = rng.normal(size=(G, K)) * sd_w
    z = rng.integers(0, C, N)
    psi = rng.normal(size=(N, K))
    p = mu[None] * L[:, z].T * np.exp(psi @ W.T)
    p /= p.sum(1, keepdims=True)
    Y = np.stack([rng.multinomial(int(reads[n]), p[n]) for n in range(N)]).astype(np.float64)
    return Y, mu[:, None] * L, W


def f_direct(y, e, W, psi):
    """log Multinomial(y | probs ~ e exp(W psi)) - |psi|^2 / 2, written out directly"""
    from scipy.special import gammaln, logsumexp
    eta = W @ psi
    logp = np.log(e) + eta - logsumexp(np.log(e) + eta)
    return gammaln(y.sum() + 1) - gammaln(y + 1).sum() + (y * logp).sum() - 0.5 * float(psi @ psi)


def f_batch(y, e, W, psis):
    """f_direct at the rows of psis [M, K]"""
    from scipy.special import gammaln, logsumexp
    logits = np.log(e)[None] + psis @ W.T
    logp = logits - logsumexp(logits, axis=1, keepdims=True)
    return gammaln(y.sum() + 1) - gammaln(y + 1).sum() + logp @ y - 0.5 * (psis ** 2).sum(1)


READS = np.array([0, 1, 5, 20, 60, 150, 400, 1000, 3000, 8000, 15000, 30000])


@pytest.mark.parametrize("sd_w", [0.3, 1.0])
def test_k1_against_adaptive_integration(sd_w):
    from scipy.integrate import quad
    Y, E, W = small(12, 40, 3, 1, sd_w, 5, READS)
    outs = {q: _clone_evidence_host(Y, E, W, 1, 0, None, None, *gauss_hermite_rule(1, q), max_iter=100) for q in (1, 4, 12)}
    r = outs[12]
    assert r["converged"].all()
    err = {q: 0.0 for q in (0, 4, 12)}
    for n in range(12):
        for c in range(3):
            mode, h = r["psi_mode"][n, c, 0], r["psi_prec"][n, c, 0]
            f0 = f_direct(Y[n], E[:, c], W, np.array([mode]))
            half = 12.0 / np.sqrt(h)
            val, _e = quad(lambda t: np.exp(f_direct(Y[n], E[:, c], W, np.array([t])) - f0), mode - half, mode + half, epsabs=0, epsrel=1e-13, limit=400,
                           points=[mode])
            truth = f0 + np.log(val) - 0.5 * np.log(2 * np.pi)
            err[0] = max(err[0], abs(r["laplace"][n, c] - truth))
            for q in (4, 12):
                err[q] = max(err[q], abs(outs[q]["evidence"][n, c] - truth))
    print(f"clone_evidence K = 1 sd(W) = {sd_w}: off the adaptive integral by {err[12]:.2e} (12 nodes), {err[4]:.2e} (4 nodes), {err[0]:.2e} (Laplace) nats")
    assert err[12] <= 1e-5
    assert err[12] < err[4] < err[0]


def test_k2_tensor_rule_against_a_dense_grid():
    Y, E, W = small(6, 40, 3, 2, 0.6, 8, np.array([0, 10, 100, 700, 4000, 20000]))
    r = _clone_evidence_host(Y, E, W, 2, 0, None, None, *gauss_hermite_rule(2, 7), max_iter=100)
    assert r["converged"].all()
    t = np.linspace(-10.0, 10.0, 401)
    wt = np.full(401, t[1] - t[0])
    wt[[0, -1]] *= 0.5
    worst = worst_lap = 0.0
    for n in range(6):
        for c in range(3):
            mode = r["psi_mode"][n, c]
            h00, h01, h11 = r["psi_prec"][n, c]
            Lc = np.linalg.cholesky(np.array([[h00, h01], [h01, h11]]))
            f0 = f_direct(Y[n], E[:, c], W, mode)
            # psi = mode + L^-T u on a grid in u: the Jacobian is 1 / det L
            u = np.stack(np.meshgrid(t, t, indexing="ij"), axis=2).reshape(-1, 2)
            g = np.exp(f_batch(Y[n], E[:, c], W, mode[None] + np.linalg.solve(Lc.T, u.T).T) - f0).reshape(401, 401)
            truth = f0 + np.log(wt @ g @ wt) - np.log(np.diag(Lc)).sum() - np.log(2 * np.pi)
            worst = max(worst, abs(r["evidence"][n, c] - truth))
            worst_lap = max(worst_lap, abs(r["laplace"][n, c] - truth))
    print(f"clone_evidence K = 2: 7 x 7 rule off the 401 x 401 grid by {worst:.2e} nats, Laplace by {worst_lap:.2e}")
    assert worst <= 1e-5 and worst < worst_lap


def test_limits_w_zero_k_zero_one_node_and_sparse_input():
    import scipy.sparse as sps
    Y, E, W = small(40, 60, 4, 1, 0.5, 3, np.random.default_rng(1).integers(0, 3000, 40))
    E[7, 2] = 0.0
    Y[:, 7] = 0
    Y[4, 7] = 3                                                      # a positive count against a zero: that pair is impossible
    ll, scale = ref_ll(Y, E, None, None)
    for q in (1, 3, 8):                                              # W = 0: psi does not enter the likelihood, the prior integrates to 1
        r = _clone_evidence_host(Y, E, np.zeros((60, 1)), 1, 0, None, None, *gauss_hermite_rule(1, q))
        ok = np.isfinite(ll)
        assert np.array_equal(np.isneginf(r["evidence"]), ~ok) and np.isneginf(r["evidence"][4, 2]) and not np.isnan(r["evidence"]).any()
        assert (np.abs(r["evidence"][ok] - ll[ok]) <= 1e-12 * scale[ok]).all()
        assert (np.abs(r["psi_mode"]) == 0).all() and (r["psi_prec"] == 1).all()
        assert r["rounds"][4, 2] == 0 and not r["converged"][4, 2] and r["converged"][ok].all()
    r0 = _clone_evidence_host(Y, E, None, 0, 0, None, None, *gauss_hermite_rule(0, 1))
    base = _clone_loglik_host(Y, E)
    assert np.array_equal(r0["evidence"], base) and np.array_equal(r0["laplace"], base) and (r0["rounds"] == 0).all()
    assert np.array_equal(r0["converged"], np.isfinite(base))
    X = np.random.default_rng(2).normal(size=(40, 1)) * 0.5
    V = np.concatenate([W, np.random.default_rng(3).normal(size=(60, 1)) * 0.3], axis=1)
    one = _clone_evidence_host(Y, E, V, 1, 1, X, None, np.zeros((1, 1)), np.ones(1))
    assert np.array_equal(one["evidence"], one["laplace"])           # Q = 1 at z = 0: the Laplace value, bit for bit
    full = _clone_evidence_host(Y, E, V, 1, 1, X, None, *gauss_hermite_rule(1, 8))
    assert np.array_equal(full["laplace"], one["laplace"]) and np.array_equal(full["psi_mode"], one["psi_mode"])
    empty = np.flatnonzero(Y.sum(1) == 0)
    Y[0] = 0
    z = _clone_evidence_host(Y, E, V, 1, 1, X, None, *gauss_hermite_rule(1, 8))
    assert np.abs(z["evidence"][0]).max() <= 1e-12 and (z["psi_mode"][0] == 0).all(), (z["evidence"][0], empty)
    for fmt in (sps.csr_matrix, sps.csc_matrix):
        sp = _clone_evidence_host(fmt(Y), E, V, 1, 1, X, None, *gauss_hermite_rule(1, 8))
        for k in z:
            assert np.array_equal(sp[k], z[k]), (fmt.__name__, k)
    few = _clone_evidence_host(Y, E, V, 1, 1, X, None, *gauss_hermite_rule(1, 8), chunk=7)
    assert np.array_equal(few["rounds"], z["rounds"]) and np.array_equal(few["converged"], z["converged"])
    for k in ("evidence", "laplace", "psi_mode", "psi_prec"):          # (the matrix products group their sums by the chunk's rows: close, not the same bits)
        fin = np.isfinite(z[k])
        assert np.array_equal(np.isfinite(few[k]), fin) and (np.abs(few[k][fin] - z[k][fin]) <= 1e-12 * np.maximum(1.0, np.abs(z[k][fin]))).all(), ("chunk", k)


def planted_k1(seed, N=200, G=150, C=3):
    """The planted problem of the model-choice check: K = 1, sd(W) = 0.5, 200 - 1500 reads"""
    rng = np.random.default_rng(seed)
    L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
    mu = rng.lognormal(0, 1, G)
    W = rng.normal(size=(G, 1)) * 0.5
    alpha = rng.dirichlet(np.full(C, 20.0))
    z = rng.choice(C, N, p=alpha)
    psi = rng.normal(size=(N, 1))
    p = mu[None] * L[:, z].T * np.exp(psi @ W.T)
    p /= p.sum(1, keepdims=True)
    s = rng.integers(200, 1500, N)
    Y = np.stack([rng.multinomial(s[n], p[n]) for n in range(N)]).astype(np.float64)
    spurious = rng.normal(size=(G, 1)) * 0.5
    return dict(Y=Y, L=L, mu=mu, W=W, W2=np.concatenate([W, spurious], axis=1), alpha=alpha, z=z)


@pytest.mark.parametrize("seed", range(5))
def test_heldout_evidence_ranks_the_true_k_first(seed):
    p = planted_k1(seed)
    names = ["a", "b", "c"]
    fits = {k: ca.ClonealignFit(ml_params={"mu": p["mu"], "alpha": p["alpha"], "W": w}, clone_names=names)
            for k, w in (("K=0", None), ("K=1", p["W"]), ("K=2", p["W2"]))}
    host = HostOnly(*p["Y"].shape)
    res = ca.heldout_evidence(fits, p["Y"], p["L"], saturate=False, engine=host)
    d2, d0 = res["K=2"], res["K=0"]
    print(f"heldout_evidence seed {seed}: K = 1 ahead of K = 2 by {-d2['delta']:.1f} nats ({-d2['delta'] / d2['delta_se']:.1f} paired se), of K = 0 by "
          f"{-d0['delta']:.1f} nats; unconverged pairs {[res[k]['n_unconverged'] for k in fits]}")
    assert res["best"] == "K=1" and res["ranking"][0] == "K=1" and res["K=1"]["delta"] == 0.0
    assert d2["delta"] < -10 * d2["delta_se"] and d0["delta"] < d2["delta"]
    assert all(res[k]["n_unconverged"] == 0 for k in fits)
    np.testing.assert_allclose(res["K=1"]["total"], res["K=1"]["per_cell"].sum(), rtol=1e-12)
    # the value at the MAP psi is a maximum over psi: it never prefers the smaller model
    E, lp = p["mu"][:, None] * p["L"], np.log(p["alpha"])[None] + np.zeros((200, 3))
    m1 = _project_cells_host(p["Y"], E, p["W"], 1, 0, None, lp, None, max_iter=100)
    m2 = _project_cells_host(p["Y"], E, p["W2"], 2, 0, None, lp, None, max_iter=100)
    at_map = [float((m["objective"] + 0.5 * (m["psi"] ** 2).sum(1)).sum()) for m in (m1, m2)]
    assert at_map[1] >= at_map[0]
    if seed == 0:                                                    # the marginal assignment on the same cells
        out = ca.assign_cells_marginal(fits["K=1"], p["Y"], p["L"], saturate=False, engine=host)
        ev = ca.clone_evidence(fits["K=1"], p["Y"], p["L"], saturate=False, engine=host)
        assert np.array_equal(out["loglik"], res["K=1"]["per_cell"]) and np.array_equal(out["clone_evidence"], ev["evidence"])
        assert ev["psi_cov"].shape == (200, 3, 1, 1) and np.allclose(ev["psi_cov"][:, :, 0, 0] * _prec(p, ev), 1.0)
        np.testing.assert_allclose(out["clone_probs"].sum(1), 1.0, rtol=1e-12)
        assert out["psi"].shape == (200, 1) and (out["psi_sd"] > 0).all() and out["converged"].all()
        lut = np.asarray(names, dtype=object)
        assert (out["clone"] == lut[p["z"]]).mean() > 0.9
        mp = ca.project_cells(fits["K=1"], p["Y"], p["L"], saturate=False, engine=host, max_iter=100)
        print(f"assign_cells_marginal vs project_cells: max posterior change {np.abs(out['clone_probs'] - mp['clone_probs']).max():.2e}")
        assert np.array_equal(ca.recompute_clone_assignment(out, 0.5)["clone"], ca.clone_assignment(out["clone_probs"], names, 0.5))


def _prec(p, ev):
    E = p["mu"][:, None] * p["L"]
    r = _clone_evidence_host(p["Y"], E, p["W"], 1, 0, None, None, *gauss_hermite_rule(1, 8))
    assert np.array_equal(r["evidence"], ev["evidence"])
    return r["psi_prec"][:, :, 0]


def test_gauss_hermite_rule():
    z, w = gauss_hermite_rule(1, 8)
    assert z.shape == (8, 1) and abs(w.sum() - 1) <= 1e-15 and abs((w * z[:, 0] ** 2).sum() - 1) <= 1e-13 and abs((w * z[:, 0] ** 4).sum() - 3) <= 1e-12
    z, w = gauss_hermite_rule(2, 5)
    assert z.shape == (25, 2) and abs(w.sum() - 1) <= 1e-15 and abs((w * z[:, 0] * z[:, 1]).sum()) <= 1e-14 and abs((w * z[:, 1] ** 2).sum() - 1) <= 1e-13
    z, w = gauss_hermite_rule(0, 3)
    assert z.shape == (1, 0) and w.tolist() == [1.0]


def test_every_refusal_names_its_offender():
    Y, E, W = small(10, 30, 3, 1, 0.5, 1, np.full(10, 200))
    nd, wt = gauss_hermite_rule(1, 4)

    def refused(words, *a, **k):
        with pytest.raises(ValueError) as ex:
            _clone_evidence_host(*a, **k)
        assert all(w in str(ex.value) for w in words), str(ex.value)
    refused(("n_nodes = 65", "[1, 64]"), Y, E, W, 1, 0, None, None, np.zeros((65, 1)), np.full(65, 1 / 65))
    refused(("n_nodes = 0", "[1, 64]"), Y, E, W, 1, 0, None, None, np.zeros((0, 1)), np.zeros(0))
    refused(("nodes is None",), Y, E, W, 1, 0, None, None, None, wt)
    refused(("weights is None",), Y, E, W, 1, 0, None, None, nd, None)
    bad = nd.copy()
    bad[2, 0] = np.inf
    refused(("node 2", "non-finite"), Y, E, W, 1, 0, None, None, bad, wt)
    for v in (-0.1, 0.0, np.nan, np.inf):
        bw = wt.copy()
        bw[1] = v
        refused(("weight 1", "not positive and finite"), Y, E, W, 1, 0, None, None, nd, bw)
    refused(("weights sum to", "1e-12"), Y, E, W, 1, 0, None, None, nd, wt * 0.9)
    Eb = E.copy()
    Eb[17, 2] = -1.0
    refused(("gene 17", "clone 2"), Y, Eb, W, 1, 0, None, None, nd, wt)
    Eb = E.copy()
    Eb[:, 1] = 0.0
    refused(("clone 1", "sums to"), Y, Eb, W, 1, 0, None, None, nd, wt)
    Wb = W.copy()
    Wb[3, 0] = np.nan
    refused(("V has a non-finite", "gene 3"), Y, E, Wb, 1, 0, None, None, nd, wt)
    st = np.zeros((10, 1))
    st[8, 0] = np.inf
    refused(("psi_start has a non-finite", "cell 8"), Y, E, W, 1, 0, None, st, nd, wt)
    V = np.concatenate([W, W], axis=1)
    Xb = np.zeros((10, 1))
    Xb[9, 0] = np.nan
    refused(("X has a non-finite", "cell 9"), Y, E, V, 1, 1, Xb, None, nd, wt)
    refused(("P = 1", "needs X"), Y, E, V, 1, 1, None, None, nd, wt)
    refused(("needs V",), Y, E, None, 1, 0, None, None, nd, wt)
    refused(("K + P = 9", "[0, 8]"), Y, E, np.zeros((30, 9)), 1, 8, np.zeros((10, 8)), None, nd, wt)
    refused(("max_iter = -1",), Y, E, W, 1, 0, None, None, nd, wt, max_iter=-1)
    for v in (0.0, -1.0, np.inf, np.nan):
        refused(("tol",), Y, E, W, 1, 0, None, None, nd, wt, tol=v)
        refused(("max_step",), Y, E, W, 1, 0, None, None, nd, wt, max_step=v)
