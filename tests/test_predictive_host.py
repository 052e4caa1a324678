"""The numpy restatement of ca_predictive_stats (api._predictive_stats_host) against an independent statement, scipy.stats.multinomial.logpmf on the
restatement's own rows; its edge cases and refusals; predictive_check(host=True) end to end.  No GPU."""
import numpy as np
import pytest
from scipy.stats import multinomial

from clonealign_amd import api

from tests import _simulate_cases as sc


def cut(name, n=None):
    E, V, U, clone, total, seed = sc.make(name)
    if n is not None:
        V, U, clone, total = V, (None if U is None else U[:n]), clone[:n], total[:n]
    return E, V, U, clone, total, seed


@pytest.mark.parametrize("name,n", [("few_genes", None), ("ragged", 20)])
def test_restatement_equals_scipys_multinomial_on_its_own_rows(name, n):
    """ll within 1e-12 relative, T exact.  Both cases have D = 0, so p = E[:, clone] / sum(E[:, clone])."""
    E, V, U, clone, total, seed = cut(name, n)
    draw0, n_rep = 5, 3
    ll, T = api._predictive_stats_host(E, V, U, clone, total, seed, draw0=draw0, n_rep=n_rep)
    assert ll.shape == (clone.shape[0], n_rep) and T.shape == (n_rep,) + E.shape and T.dtype == np.int64
    worst = 0.0
    for r in range(n_rep):
        Y, _flagged = api._simulate_counts_host(E, V, U, clone, total, seed, draw0 + r)
        for i in range(clone.shape[0]):
            p = E[:, clone[i]] / E[:, clone[i]].sum()
            want = multinomial.logpmf(Y[i], n=int(total[i]), p=p)
            worst = max(worst, abs(ll[i, r] - want) / abs(want))
            assert abs(ll[i, r] - want) <= 1e-12 * abs(want), (name, i, r, ll[i, r], want)
        for c in range(E.shape[1]):
            assert np.array_equal(T[r][:, c], Y[clone == c].sum(0, dtype=np.int64)), (name, r, c)
    print(f"{name}: largest relative difference from scipy's logpmf {worst:.2e}")


def test_with_an_exponent_term_against_scipy():
    """D = 1 with copy number 0 in places (a 12-cell cut of `mixed`: totals 0, 1, 200 000 and 2 among them): p from a direct softmax."""
    E, V, U, clone, total, seed = cut("mixed", 12)
    ll, T = api._predictive_stats_host(E, V, U, clone, total, seed, n_rep=1)
    Y, _flagged = api._simulate_counts_host(E, V, U, clone, total, seed, 0)
    for i in range(12):
        w = E[:, clone[i]] * np.exp(U[i] @ V.T)
        want = multinomial.logpmf(Y[i], n=int(total[i]), p=w / w.sum())
        assert abs(ll[i, 0] - want) <= 1e-11 * max(abs(want), 1.0), (i, ll[i, 0], want)   # (scipy's own sum of 1234 terms against lgamma(200 001) = 2.2e6)
    assert T.sum() == total.sum()


def test_a_cell_without_counts_gives_exactly_zero():
    E, V, U, clone, total, seed = cut("ragged", 6)
    total = np.array([0, 3000, 0, 1, 0, 7], dtype=np.int64)
    ll, T = api._predictive_stats_host(E, V, U, clone, total, seed, n_rep=2)
    assert (ll[[0, 2, 4]] == 0.0).all() and not np.signbit(ll[[0, 2, 4]]).any()
    assert (ll[[1, 3, 5]] < 0.0).all() and T.sum() == 2 * total.sum()
    # ... even for a clone that cannot be drawn from at all
    E2 = np.column_stack([E[:, 0], np.zeros(E.shape[0])])
    ll, T = api._predictive_stats_host(E2, None, None, np.array([1, 1]), 0, seed, n_rep=2)
    assert (ll == 0.0).all() and (T == 0).all()


def test_splitting_cells_and_replicates_changes_nothing():
    E, V, U, clone, total, seed = cut("ragged", 12)
    ll, T = api._predictive_stats_host(E, V, U, clone, total, seed, draw0=5, n_rep=3)
    for r in range(3):
        a, Ta = api._predictive_stats_host(E, V, U, clone, total, seed, draw0=5 + r, n_rep=1)
        assert np.array_equal(a[:, 0], ll[:, r]) and np.array_equal(Ta[0], T[r])
    a, Ta = api._predictive_stats_host(E, V, U, clone[:5], total[:5], seed, draw0=5, n_rep=3)
    b, Tb = api._predictive_stats_host(E, V, U, clone[5:], total[5:], seed, draw0=5, n_rep=3, cell_offset=5)
    assert np.array_equal(np.concatenate([a, b]), ll) and np.array_equal(Ta + Tb, T)
    assert api._predictive_stats_host(E, V, U, clone, total, seed, n_rep=2, gene_totals=False)[1] is None


def test_refusals_raise_valueerror():
    E, V, U, clone, total, seed = cut("ragged", 8)
    for kw in ({"n_rep": 0}, {"n_rep": -3}, {"draw0": 2 ** 48, "n_rep": 1}, {"draw0": 2 ** 48 - 2, "n_rep": 3}, {"draw0": -1}, {"cell_offset": -1}):
        with pytest.raises(ValueError):
            api._predictive_stats_host(E, V, U, clone, total, seed, **kw)
    api._predictive_stats_host(E, V, U, clone[:1], total[:1] * 0 + 2, seed, draw0=2 ** 48 - 2, n_rep=2)       # the last two draws are allowed
    bad = np.array(E)
    bad[3, 1] = -1.0
    for args in ((bad, V, U, clone, total), (E, V, U, clone + 2, total), (E, V, U, clone, -total), (E, np.zeros((77, 1)), None, clone, total)):
        with pytest.raises(ValueError):
            api._predictive_stats_host(*args, seed)


def planted(N=60, G=40, C=3, n_bad=6, total=400, seed=5):
    """A hand-made fit and a matrix drawn from it with numpy's multinomial; in the first n_bad cells the genes are permuted."""
    rng = np.random.default_rng(seed)
    L = rng.integers(1, 5, (G, C)).astype(np.float64)
    mu = rng.lognormal(0.0, 1.0, G)
    W, psi = rng.normal(size=(G, 1)) * 0.5, rng.normal(size=(N, 1))
    z = rng.integers(0, C, N)
    names = [f"clone_{c}" for c in "abc"[:C]]
    w = (mu[:, None] * L)[:, z].T * np.exp(psi @ W.T)
    Y = np.stack([rng.multinomial(total, w[n] / w[n].sum()) for n in range(N)]).astype(np.int32)
    for n in range(n_bad):
        Y[n] = Y[n][rng.permutation(G)]
    fit = {"ml_params": {"mu": mu, "W": W, "psi": psi}, "clone_names": names, "clone": np.asarray(names, dtype=object)[z]}
    return fit, Y, L, z


def test_predictive_check_on_the_host_finds_the_planted_cells():
    fit, Y, L, z = planted()
    fit["clone"][10] = "unassigned"
    out = api.predictive_check(fit, Y, L, n_rep=12, seed=3, host=True)
    used = np.delete(np.arange(60), 10)
    assert np.array_equal(out["cells"], used)
    for k in ("ll_observed", "ll_replicate_mean", "ll_replicate_sd", "z_cell", "p_cell"):
        assert out[k].shape == (59,) and np.isfinite(out[k]).all(), k
    assert out["ll_total_replicates"].shape == (12,) and np.isfinite(out["z"])
    assert abs(out["ll_total_observed"] - out["ll_observed"].sum()) <= 1e-9 * abs(out["ll_total_observed"])
    assert (out["p_cell"][:6] == 1.0 / 13.0).all() and out["z_cell"][:6].max() < out["z_cell"][6:].min()
    assert (out["p_cell"] >= 1.0 / 13.0).all() and (out["p_cell"] <= 1.0).all()
    for k in ("T_observed", "T_replicate_mean", "T_replicate_sd", "z_gene_clone", "p_gene_clone"):
        assert out[k].shape == (40, 3), k
    assert np.array_equal(out["T_observed"].sum(0), [Y[used][z[used] == c].sum() for c in range(3)])
    assert np.allclose(out["T_replicate_mean"].sum(0), out["T_observed"].sum(0))          # a replicate keeps the row sums
    assert np.isfinite(out["z_gene_clone"][out["T_replicate_sd"] > 0]).all() and np.isnan(out["z_gene_clone"][out["T_replicate_sd"] == 0]).all()
    assert (out["p_gene_clone"] >= 2.0 / 13.0).all() and (out["p_gene_clone"] <= 1.0).all()
    assert "T_observed" not in api.predictive_check(fit, Y, L, n_rep=2, seed=3, host=True, gene_totals=False)


def test_predictive_check_refusals():
    fit, Y, L, _z = planted()
    with pytest.raises(ValueError, match="n_rep"):
        api.predictive_check(fit, Y, L, n_rep=1, host=True)
    with pytest.raises(ValueError, match="unassigned"):
        api.predictive_check(dict(fit, clone=np.full(60, "unassigned", dtype=object)), Y, L, n_rep=4, host=True)
    with pytest.raises(ValueError, match="clone labels"):
        api.predictive_check(dict(fit, clone=np.full(60, "clone_z", dtype=object)), Y, L, n_rep=4, host=True)
    with pytest.raises(ValueError, match="x is required"):
        api.predictive_check(fit, Y, L, n_rep=4, x=np.zeros((60, 1)), host=True)


def test_the_package_exports_the_new_names():
    import clonealign_amd as ca
    from clonealign_amd import engine
    assert ca.predictive_check is api.predictive_check
    assert {"ca_predictive_stats", "ca_predictive_kernel_ms"} <= set(engine.EXPORTS)
    assert callable(engine.predictive_stats) and callable(engine.predictive_kernel_ms)
