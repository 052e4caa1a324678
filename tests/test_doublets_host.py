"""clone_pair_loglik / detect_doublets on the host: the float64 numpy form (``api._clone_pair_loglik_host``) and the posterior built on it, through an engine
stub without ``clone_pair_loglik`` -- no GPU.  The model: the counts of a heterotypic doublet of clones a < b are multinomial in ``w p_a + (1 - w) p_b``."""
import numpy as np
import pytest

import clonealign_amd as ca
from clonealign_amd import api


class HostOnly:                                                      # a live engine without clone_loglik / clone_pair_loglik: the CPU host forms
    def __init__(self, N, G):
        self.N, self.G = N, G


def small(N=60, G=90, C=4, D=2, seed=0):
    rng = np.random.default_rng(seed)
    L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
    mu = rng.lognormal(0.0, 1.0, G)
    E = mu[:, None] * L
    Y = rng.poisson(0.4, size=(N, G)).astype(np.float64)
    Y[0] = 0                                                         # a cell without counts
    U, V = (rng.normal(size=(N, D)) * 0.5, rng.normal(size=(G, D)) * 0.3) if D else (None, None)
    return Y, E, U, V, rng


def direct(y, pa, pb, w):
    """sum over the non-zero counts of y log(w pa + (1 - w) pb), one cell, normalised probability vectors."""
    nz = y > 0
    return float((y[nz] * np.log(w * pa[nz] + (1 - w) * pb[nz])).sum())


@pytest.mark.parametrize("D", [0, 2])
def test_formula_pair_order_and_column_mapping(D):
    Y, E, U, V, _rng = small(D=D)
    w = (0.2, 0.6)
    r = api._clone_pair_loglik_host(Y, E, U, V, weights=w, const=False, chunk=25)
    C = E.shape[1]
    want = [(a, b) for a in range(C) for b in range(a + 1, C)]
    assert r["pairs"].tolist() == [list(p) for p in want] and r["pair_ll"].shape == (Y.shape[0], len(want), 2)
    assert np.array_equal(r["ll"], api._clone_loglik_host(Y, E, U, V, const=False))
    eta = np.zeros_like(Y) if D == 0 else U @ V.T
    for n in (0, 3, 41):
        P = E * np.exp(eta[n])[:, None]
        P = P / P.sum(0)
        for p, (a, b) in enumerate(want):
            for k, wk in enumerate(w):
                ref = direct(Y[n], P[:, a], P[:, b], wk)
                assert abs(r["pair_ll"][n, p, k] - ref) <= 1e-10 * max(1.0, abs(ref)), (n, a, b, wk)
    assert np.array_equal(r["pair_ll"][0], np.zeros((len(want), 2)))             # s = 0: 0 (+ const, here off)
    # the pair (0, 2) alone, and with its clones swapped at 1 - w
    sub = api._clone_pair_loglik_host(Y, E[:, [0, 2]], U, V, weights=w, const=False)
    np.testing.assert_allclose(sub["pair_ll"][:, 0], r["pair_ll"][:, want.index((0, 2))], rtol=1e-12, atol=1e-12)
    swp = api._clone_pair_loglik_host(Y, E[:, [2, 0]], U, V, weights=(0.8, 0.4), const=False)
    np.testing.assert_allclose(swp["pair_ll"][:, 0], r["pair_ll"][:, want.index((0, 2))], rtol=1e-12, atol=1e-9)
    # the constant is clone_loglik's
    rc = api._clone_pair_loglik_host(Y, E, U, V, weights=w, const=True)
    const = api._clone_loglik_host(Y, E, U, V, const=True)[:, 0] - r["ll"][:, 0]
    np.testing.assert_allclose(rc["pair_ll"], r["pair_ll"] + const[:, None, None], rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("D", [0, 2])
def test_concavity_bound_and_identical_clones(D):
    """Jensen: log(w pa + (1 - w) pb) >= w log pa + (1 - w) log pb, so pll >= w ll_a + (1 - w) ll_b; with two identical columns the pair IS the singlet."""
    Y, E, U, V, _rng = small(D=D, seed=1)
    E[:, 3] = E[:, 1]
    w = np.array([0.1, 0.5, 0.9])
    r = api._clone_pair_loglik_host(Y, E, U, V, weights=w)
    ll, pll = r["ll"], r["pair_ll"]
    for p, (a, b) in enumerate(r["pairs"]):
        bound = w[None, :] * ll[:, a, None] + (1 - w)[None, :] * ll[:, b, None]
        scale = np.abs(ll[:, a, None]) + np.abs(ll[:, b, None]) + np.abs(pll[:, p]) + 1.0
        ok = np.isfinite(bound) & np.isfinite(pll[:, p])
        assert ok.all()
        assert (pll[:, p] >= bound - 1e-10 * scale)[ok].all(), (a, b)
    p13 = r["pairs"].tolist().index([1, 3])
    assert np.abs(pll[:, p13] - ll[:, 1, None]).max() <= 1e-10 * np.abs(ll[:, 1]).max()


def test_minus_infinity_only_where_both_clones_are_zero():
    Y, E, U, V, _rng = small(C=3, seed=2)
    E[5, :] = 0.0
    Y[:, 5] = 0                                                      # a zero count against zeros in every clone: adds nothing
    E[7, 0] = 0.0
    E[9, 0] = E[9, 1] = 0.0
    Y[:, 7] = 0
    Y[:, 9] = 0
    Y[11, 7] = 2                                                     # clone 0 alone has E = 0: -inf for the singlet, finite for its pairs
    Y[12, 9] = 1                                                     # clones 0 and 1: -inf for the pair (0, 1) only
    r = api._clone_pair_loglik_host(Y, E, U, V, weights=(0.3, 0.7))
    assert not np.isnan(r["pair_ll"]).any() and not np.isnan(r["ll"]).any()
    want = np.zeros(r["pair_ll"].shape, dtype=bool)
    want[12, r["pairs"].tolist().index([0, 1]), :] = True
    assert np.array_equal(np.isneginf(r["pair_ll"]), want)
    assert np.isneginf(r["ll"][11, 0]) and np.isneginf(r["ll"][12, :2]).all()
    assert np.isfinite(r["pair_ll"][11]).all()


def fixture(n_single=300, n_double=100, G=400, C=4, seed=3):
    """Singlets and heterotypic doublets (the sum of two multinomial rows of different clones, 800-2500 counts each) from a K = 0 model."""
    rng = np.random.default_rng(seed)
    L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
    mu = rng.lognormal(0.0, 1.0, G)
    P = mu[:, None] * L
    P = P / P.sum(0)
    names = [f"c{i}" for i in range(C)]
    rows, truth, tpair = [], [], []
    for _ in range(n_single):
        c = int(rng.integers(C))
        rows.append(rng.multinomial(int(rng.integers(800, 2501)), P[:, c]))
        truth.append(names[c])
        tpair.append(None)
    for _ in range(n_double):
        a, b = sorted(rng.choice(C, 2, replace=False).tolist())
        rows.append(rng.multinomial(int(rng.integers(800, 2501)), P[:, a]) + rng.multinomial(int(rng.integers(800, 2501)), P[:, b]))
        truth.append("doublet")
        tpair.append(f"{names[a]}+{names[b]}")
    fit = ca.ClonealignFit(ml_params={"mu": mu}, clone_names=names)
    return np.asarray(rows, dtype=np.int32), L, fit, np.asarray(truth, dtype=object), np.asarray(tpair, dtype=object)


@pytest.fixture(scope="module")
def planted():
    Y, L, fit, truth, tpair = fixture()
    res = ca.detect_doublets(fit, Y, L, doublet_rate=0.1, weights=(0.3, 0.5, 0.7), engine=HostOnly(*Y.shape))
    return Y, L, fit, truth, tpair, res


def test_recovery_of_planted_doublets(planted):
    _Y, _L, _fit, truth, tpair, res = planted
    d = truth == "doublet"
    called = res["clone"] == "doublet"
    right_pair = res["doublet_pair"][d] == tpair[d]
    print(f"doublets labelled {called[d].mean():.3f}, right pair {right_pair.mean():.3f}, singlets labelled doublet {called[~d].mean():.3f}")
    assert called[d].mean() >= 0.95
    assert right_pair.mean() >= 0.95
    assert called[~d].mean() <= 0.02
    assert (res["doublet_pair"][~called] == None).all()              # noqa: E711 (elementwise)
    w = res["doublet_weight"][d]
    assert np.isfinite(w).all() and (w > 0.3 - 1e-12).all() and (w < 0.7 + 1e-12).all()
    assert (res["log_bayes_factor"][d] > 0).mean() >= 0.95


def test_posterior_is_normalised_and_reduces_to_assign_cells(planted):
    Y, L, fit, _truth, _tpair, res = planted
    N, C = Y.shape[0], L.shape[1]
    stub = HostOnly(*Y.shape)
    assert res["pair_probs"].shape == (N, C * (C - 1) // 2) and res["clone_probs"].shape == (N, C)
    np.testing.assert_allclose(res["pair_probs"].sum(1), res["p_doublet"], atol=1e-12)
    np.testing.assert_allclose(res["clone_probs"].sum(1), 1.0, atol=1e-12)
    # over ALL hypotheses: singlets carry (1 - p_doublet) clone_probs
    np.testing.assert_allclose(((1 - res["p_doublet"])[:, None] * res["clone_probs"]).sum(1) + res["pair_probs"].sum(1), 1.0, atol=1e-12)
    assert not any(np.isnan(res[k]).any() for k in ("p_doublet", "pair_probs", "clone_probs", "loglik", "log_bayes_factor"))
    plain = ca.assign_cells(fit, Y, L, engine=stub)
    # p_doublet -> 0 with the rate: it is rho BF / (1 - rho + rho BF) with the Bayes factor the result states
    for rho in (1e-6, 1e-300):
        tiny = ca.detect_doublets(fit, Y, L, doublet_rate=rho, engine=stub)
        with np.errstate(over="ignore"):
            want = 1.0 / (1.0 + (1.0 - rho) / rho * np.exp(-res["log_bayes_factor"]))
        np.testing.assert_allclose(tiny["p_doublet"], want, rtol=1e-9, atol=1e-300)
        assert (tiny["p_doublet"] <= res["p_doublet"]).all()
    assert tiny["p_doublet"].max() <= 1e-100 and not (tiny["clone"] == "doublet").any()
    zero = ca.detect_doublets(fit, Y, L, doublet_rate=0.0, engine=stub)
    assert np.array_equal(zero["p_doublet"], np.zeros(N)) and not (zero["clone"] == "doublet").any()
    assert np.abs(zero["clone_probs"] - plain["clone_probs"]).max() <= 1e-12
    assert np.array_equal(zero["clone"], plain["clone"])
    np.testing.assert_allclose(zero["loglik"], plain["loglik"] - np.log(C), rtol=1e-12)      # (alpha: uniform here, none in assign_cells)
    assert np.array_equal(ca.recompute_clone_assignment(res, 0.5)["clone"], api.clone_assignment(res["clone_probs"], res["clone_names"], 0.5))
    # ranges of cells change nothing
    cut = ca.detect_doublets(fit, Y, L, doublet_rate=0.1, engine=stub, chunk_cells=77)
    assert np.array_equal(cut["clone"], res["clone"]) and np.array_equal(cut["pair_probs"], res["pair_probs"])


def test_extra_loglik_priors_and_impossible_cells():
    Y, L, fit, _truth, _tpair = fixture(n_single=30, n_double=10, G=120, seed=5)
    N, C = Y.shape[0], L.shape[1]
    stub = HostOnly(*Y.shape)
    fit["ml_params"]["alpha"] = np.array([0.1, 0.2, 0.3, 0.4])
    Lz = L.copy()
    Lz[3, :] = 0.0                                                   # a gene no clone expresses: a cell with a count there is impossible
    Y = Y.copy()
    Y[:, 3] = 0
    Y[4, 3] = 1
    rng = np.random.default_rng(1)
    ex = rng.normal(size=(N, C))
    res = ca.detect_doublets(fit, Y, Lz, doublet_rate=0.2, extra_loglik=ex, engine=stub, saturate=False)
    assert res["clone"][4] == "unassigned" and np.isnan(res["p_doublet"][4]) and np.isnan(res["clone_probs"][4]).all() and np.isneginf(res["loglik"][4])
    rest = np.arange(N) != 4
    for k in ("p_doublet", "pair_probs", "clone_probs", "loglik", "log_bayes_factor", "doublet_weight"):
        assert np.isfinite(res[k][rest]).all(), k
    # the posterior by hand for one cell
    r = ca.clone_pair_loglik(fit, Y, Lz, engine=stub, saturate=False)
    assert np.allclose(r["weights"], [0.3, 0.5, 0.7])
    n, al = 7, fit["ml_params"]["alpha"]
    het = 1 - (al ** 2).sum()
    hyp = list(r["ll"][n] + np.log(0.8 * al) + ex[n])
    for p, (a, b) in enumerate(r["pairs"]):
        for k in range(3):
            hyp.append(r["pair_ll"][n, p, k] + np.log(0.2 * 2 * al[a] * al[b] / het / 3) + np.logaddexp(ex[n, a], ex[n, b]) - np.log(2))
    hyp = np.asarray(hyp)
    tot = np.log(np.exp(hyp - hyp.max()).sum()) + hyp.max()
    post = np.exp(hyp - tot)
    assert abs(res["loglik"][n] - tot) <= 1e-10 * abs(tot)
    np.testing.assert_allclose(res["pair_probs"][n], post[C:].reshape(-1, 3).sum(1), atol=1e-12)
    np.testing.assert_allclose(res["p_doublet"][n], post[C:].sum(), atol=1e-12)


def test_weight_grid_is_closed_under_one_minus_w():
    assert np.allclose(api._pair_weight_grid((0.3,)), [0.3, 0.7])
    assert np.allclose(api._pair_weight_grid((0.7, 0.5, 0.3)), [0.3, 0.5, 0.7])
    g = api._pair_weight_grid((0.1, 0.25, 0.5))
    assert np.allclose(g, [0.1, 0.25, 0.5, 0.75, 0.9]) and np.allclose(np.sort(1 - g), g)
    Y, L, fit, _t, _p = fixture(n_single=8, n_double=2, G=50, seed=9)
    a = ca.clone_pair_loglik(fit, Y, L, weights=(0.3,), engine=HostOnly(*Y.shape))
    b = ca.clone_pair_loglik(fit, Y, L, weights=(0.7, 0.3), engine=HostOnly(*Y.shape))
    assert np.allclose(a["weights"], [0.3, 0.7]) and np.array_equal(a["pair_ll"], b["pair_ll"])


def test_refusals_name_the_offender():
    Y, E, U, V, _rng = small(N=12, G=30, C=3)

    def refused(words, *a, **k):
        with pytest.raises(ValueError) as ex:
            api._clone_pair_loglik_host(*a, **k)
        assert all(w in str(ex.value) for w in words), str(ex.value)
    for bad in (0.0, 1.0, -0.1, 1.5, np.nan, np.inf):
        refused(("weight 1", "(0, 1)"), Y, E, U, V, weights=(0.5, bad))
    refused(("n_weights = 0",), Y, E, U, V, weights=())
    refused(("n_weights = 9",), Y, E, U, V, weights=np.linspace(0.1, 0.9, 9))
    refused(("C = 1",), Y, E[:, :1], U, V)
    Eb = E.copy()
    Eb[17, 2] = -1.0
    refused(("gene 17", "clone 2"), Y, Eb, U, V)
    Eb = E.copy()
    Eb[:, 1] = 0.0
    refused(("clone 1", "sums to"), Y, Eb, U, V)
    Ub = U.copy()
    Ub[9, 1] = np.nan
    refused(("U has a non-finite", "cell 9"), Y, E, Ub, V)
    refused(("D = 9",), Y, E, np.zeros((12, 9)), np.zeros((30, 9)))
    refused(("U and V go together",), Y, E, U, None)
    Yf, L, fit, _t, _p = fixture(n_single=8, n_double=2, G=50, seed=9)
    with pytest.raises(ValueError, match="n_weights = 10"):
        ca.clone_pair_loglik(fit, Yf, L, weights=np.linspace(0.05, 0.45, 5), engine=HostOnly(*Yf.shape))
    with pytest.raises(ValueError, match="doublet_rate"):
        ca.detect_doublets(fit, Yf, L, doublet_rate=1.5, engine=HostOnly(*Yf.shape))
    with pytest.raises(ValueError, match="a pair needs at least 2"):
        ca.detect_doublets(ca.ClonealignFit(ml_params=fit["ml_params"]), Yf, L[:, :1], engine=HostOnly(*Yf.shape))
