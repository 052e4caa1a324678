"""clone_loglik / assign_cells on the host: the chunked float64 form ``_clone_loglik_host`` against an xlogy restatement written here (and against
torch.distributions.Multinomial where every E > 0), the -inf / NaN rules, and the two user functions through a fake engine without ``clone_loglik``.

Bars.  The host form and the restatement add the same float64 terms in different orders (BLAS products against row sums): both stay within
G 2^-53 of the sum of the terms' magnitudes, so 1e-12 of that sum holds with room at G <= 400.  Against torch: rtol 1e-12, the figure the README holds
the oracle to (measured 5.7e-15 at 40 x 2049 x 20)."""
import numpy as np
import pytest
from scipy.special import gammaln, logsumexp

import clonealign_amd as ca
from clonealign_amd.api import _clone_loglik_host


def ref_ll(Y, E, U=None, V=None, const=True):
    """(ll, scale) [N, C]: the formula of include/clonealign_hip.h in plain numpy float64, xlogy semantics; scale = the sum of the terms' magnitudes."""
    Y = np.asarray(Y.toarray() if hasattr(Y, "toarray") else Y, dtype=np.float64)
    E = np.asarray(E, dtype=np.float64)
    N, G = Y.shape
    s = Y.sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        logE = np.log(E)
        t = np.where(Y[:, :, None] > 0, Y[:, :, None] * logE[None, :, :], 0.0)         # xlogy(y, E)
    a, scale = t.sum(1), np.abs(np.where(np.isfinite(t), t, 0.0)).sum(1)
    if U is not None and U.shape[1] > 0:
        eta = U @ V.T
        m = eta.max(1, keepdims=True)
        logz = m + np.log(np.exp(eta - m) @ E)
        a = a + (Y * eta).sum(1)[:, None]
        scale = scale + (Y * np.abs(eta)).sum(1)[:, None]
    else:
        logz = np.broadcast_to(np.log(E.sum(0))[None, :], a.shape)
    a = a - s[:, None] * logz
    scale = scale + s[:, None] * np.abs(logz)
    if const:
        a = a + (gammaln(s + 1) - gammaln(Y + 1).sum(1))[:, None]
        scale = scale + (gammaln(s + 1) + gammaln(Y + 1).sum(1))[:, None]
    return a, scale


def toy(N=60, G=257, C=5, D=3, seed=0):
    rng = np.random.default_rng(seed)
    L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
    mu = rng.lognormal(0, 1, G)
    Y = rng.poisson(0.4 * mu[None, :] * L[:, rng.integers(0, C, N)].T).astype(np.float64)
    Y[:, 0] += 1
    U = rng.normal(size=(N, D)) * 0.5
    V = rng.normal(size=(G, D)) * 0.3
    return Y, L, mu, U, V, rng


@pytest.mark.parametrize("const", [True, False])
@pytest.mark.parametrize("D", [0, 3])
@pytest.mark.parametrize("sparse", [False, True])
def test_host_form_against_the_restatement_and_torch(sparse, D, const):
    import scipy.sparse as sps
    import torch
    Y, L, mu, U, V, _ = toy(D=3)
    E = mu[:, None] * L
    Uv, Vv = (U, V) if D else (None, None)
    out = _clone_loglik_host(sps.csr_matrix(Y) if sparse else Y, E, Uv, Vv, const=const, chunk=17)
    ref, scale = ref_ll(Y, E, Uv, Vv, const=const)
    assert out.shape == ref.shape and np.isfinite(out).all()
    err = np.abs(out - ref) / scale
    print(f"host form vs restatement (sparse={sparse}, D={D}, const={const}): max |diff| / scale {err.max():.2e}")
    assert err.max() <= 1e-12
    if const:
        eta = U @ V.T if D else np.zeros_like(Y)
        for c in range(E.shape[1]):
            logits = torch.from_numpy(np.log(E[:, c])[None, :] + eta)
            for n in (0, 7, 59):
                lp = torch.distributions.Multinomial(total_count=int(Y[n].sum()), logits=logits[n]).log_prob(torch.from_numpy(Y[n])).item()
                assert abs(out[n, c] - lp) <= 1e-12 * abs(lp), (n, c, out[n, c], lp)


def test_zero_copy_number_and_extreme_exponents():
    Y, L, mu, U, V, rng = toy()
    N, G = Y.shape
    L[5, :] = 0.0
    Y[:, 5] = 0.0                                                    # zero copy number against zero counts: contributes nothing
    L[7, 3] = 0.0
    Y[:, 7] = 0.0
    Y[11, 7] = 2.0                                                   # one cell with a positive count where clone 3 has none
    E = mu[:, None] * L
    U = U.copy()
    V = V.copy()
    U[20] = 0.0
    U[20, 0] = 1.0
    V[[3, 40, 99], 0] = 800.0                                        # eta = +-800 on a few genes of cell 20
    V[[4, 41], 0] = -800.0
    for Uv, Vv in ((None, None), (U, V)):
        out = _clone_loglik_host(Y, E, Uv, Vv)
        ref, scale = ref_ll(Y, E, Uv, Vv)
        assert not np.isnan(out).any()
        assert np.array_equal(np.isneginf(out), np.isneginf(ref))
        want = np.zeros_like(out, dtype=bool)
        want[11, 3] = True
        assert np.array_equal(np.isneginf(out), want)
        ok = ~want
        assert np.isfinite(out[ok]).all()
        assert (np.abs(out[ok] - ref[ok]) / scale[ok]).max() <= 1e-12
    keep = np.arange(G) != 5                                         # gene 5 contributes nothing at all
    assert np.array_equal(np.isneginf(_clone_loglik_host(Y[:, keep], E[keep])), want)
    np.testing.assert_allclose(_clone_loglik_host(Y[:, keep], E[keep])[ok], _clone_loglik_host(Y, E)[ok], rtol=1e-13)


def test_host_form_refusals_name_the_offender():
    Y, L, mu, U, V, _ = toy()
    E = mu[:, None] * L
    for bad_value in (-1.0, np.nan, np.inf):
        Eb = E.copy()
        Eb[17, 2] = bad_value
        with pytest.raises(ValueError, match=r"gene 17, clone 2"):
            _clone_loglik_host(Y, Eb)
    Eb = E.copy()
    Eb[:, 1] = 0.0
    with pytest.raises(ValueError, match=r"clone 1 sums to"):
        _clone_loglik_host(Y, Eb)
    Ub = U.copy()
    Ub[9, 1] = np.nan
    with pytest.raises(ValueError, match=r"U has a non-finite entry \(cell 9, factor 1\)"):
        _clone_loglik_host(Y, E, Ub, V)
    Vb = V.copy()
    Vb[33, 2] = np.inf
    with pytest.raises(ValueError, match=r"V has a non-finite entry \(gene 33, factor 2\)"):
        _clone_loglik_host(Y, E, U, Vb)
    with pytest.raises(ValueError, match=r"outside \[0, 8\]"):
        _clone_loglik_host(Y, E, np.zeros((Y.shape[0], 9)), np.zeros((Y.shape[1], 9)))
    with pytest.raises(ValueError, match="go together"):
        _clone_loglik_host(Y, E, U, None)


class FakeEngine:
    """A live engine without ``clone_loglik``: the user functions fall to the host form."""

    def __init__(self, N, G):
        self.N, self.G = N, G

    def close(self):
        raise AssertionError("a given engine is not closed")


def fit_of(mu, alpha, names, W=None, psi=None, beta=None):
    ml = {"mu": mu, "alpha": alpha}
    if W is not None:
        ml.update(W=W, psi=psi)
    if beta is not None:
        ml["beta"] = beta
    return ca.ClonealignFit(ml_params=ml, clone_names=names)


def test_clone_loglik_maps_the_fit_onto_the_sweep():
    Y, L, mu, U, V, rng = toy(C=4, D=3)
    N, G = Y.shape
    L[::9] = 8.0                                                     # above the saturation threshold
    names = ["a", "b", "c", "d"]
    alpha = np.array([0.1, 0.2, 0.3, 0.4])
    eng = FakeEngine(N, G)
    Ls = np.minimum(L, 6.0)
    # K = 0, no covariates; saturate on and off
    fit = fit_of(mu, alpha, names)
    np.testing.assert_array_equal(ca.clone_loglik(fit, Y, L, engine=eng), _clone_loglik_host(Y, mu[:, None] * Ls))
    np.testing.assert_array_equal(ca.clone_loglik(fit, Y, L, saturate=False, engine=eng), _clone_loglik_host(Y, mu[:, None] * L))
    np.testing.assert_array_equal(ca.clone_loglik(fit, Y, L, saturation_threshold=3, engine=eng), _clone_loglik_host(Y, mu[:, None] * np.minimum(L, 3.0)))
    assert np.abs(ca.clone_loglik(fit, Y, L, engine=eng) - ca.clone_loglik(fit, Y, L, saturate=False, engine=eng)).max() > 1.0
    np.testing.assert_array_equal(ca.clone_loglik(fit, Y, L, const=False, engine=eng), _clone_loglik_host(Y, mu[:, None] * Ls, const=False))
    # K = 2 with one covariate: psi None (new cells: prior mean 0), "fit", an array
    W, psi, beta, x = V[:, :2], U[:, :2], V[:, 2:], U[:, 2:]
    fit = fit_of(mu, alpha, names, W=W, psi=psi, beta=beta)
    E = mu[:, None] * Ls
    np.testing.assert_array_equal(ca.clone_loglik(fit, Y, L, x=x, engine=eng), _clone_loglik_host(Y, E, x, beta))
    ref0, scale = ref_ll(Y, E, np.concatenate([np.zeros_like(psi), x], 1), V)
    assert (np.abs(ca.clone_loglik(fit, Y, L, x=x, engine=eng) - ref0) / scale).max() <= 1e-12
    np.testing.assert_array_equal(ca.clone_loglik(fit, Y, L, x=x, psi="fit", engine=eng), _clone_loglik_host(Y, E, U, V))
    other = rng.normal(size=psi.shape)
    np.testing.assert_array_equal(ca.clone_loglik(fit, Y, L, x=x[:, 0], psi=other, engine=eng),
                                  _clone_loglik_host(Y, E, np.concatenate([other, x], 1), V))
    # x is required exactly when the fit has beta; row counts; gene counts; clone names
    with pytest.raises(ValueError, match="x is required exactly when the fit has beta"):
        ca.clone_loglik(fit, Y, L, engine=eng)
    with pytest.raises(ValueError, match="x is required exactly when the fit has beta"):
        ca.clone_loglik(fit_of(mu, alpha, names), Y, L, x=x, engine=eng)
    with pytest.raises(ValueError, match="x is"):
        ca.clone_loglik(fit, Y, L, x=x[:-1], engine=eng)
    with pytest.raises(ValueError, match="psi has"):
        ca.clone_loglik(fit, Y[:-1], L, x=x[:-1], psi="fit", engine=FakeEngine(N - 1, G))
    with pytest.raises(ValueError, match="psi must be"):
        ca.clone_loglik(fit, Y, L, x=x, psi="mean", engine=eng)
    with pytest.raises(ValueError, match=r"fit\$ml_params\$mu has length 257 but L has 256 rows: evaluate on the retained genes"):
        ca.clone_loglik(fit, Y[:, :-1], L[:-1], x=x, engine=eng)
    with pytest.raises(ValueError, match=r"L has 256 rows \(genes\) but Y has 257 columns"):
        ca.clone_loglik(fit, Y, L[:-1], x=x, engine=eng)
    with pytest.raises(ValueError, match="4 clone names but L has 3 columns"):
        ca.clone_loglik(fit, Y, L[:, :3], x=x, engine=eng)
    with pytest.raises(ValueError, match="the engine holds"):
        class Wrong(FakeEngine):
            clone_loglik = None
        ca.clone_loglik(fit, Y, L, x=x, engine=Wrong(N + 1, G))


def test_assign_cells():
    Y, L, mu, U, V, rng = toy(N=80, C=4)
    N, G = Y.shape
    names = ["a", "b", "c", "d"]
    alpha = np.array([0.1, 0.2, 0.3, 0.4])
    L[7, :] = 0.0
    Y[:, 7] = 0.0
    Y[13, 7] = 1.0                                                   # cell 13: no clone is possible
    L[9, 2] = 0.0
    Y[:, 9] = 0.0
    Y[21, 9] = 3.0                                                   # cell 21: clone c is impossible
    fit = fit_of(mu, alpha, names)
    eng = FakeEngine(N, G)
    extra = rng.normal(size=(N, 4))
    for ex in (None, extra):
        res = ca.assign_cells(fit, Y, L, extra_loglik=ex, engine=eng)
        assert isinstance(res, ca.ClonealignFit) and {"clone_probs", "clone", "loglik", "clone_loglik", "clone_names"} <= set(res)
        ll = _clone_loglik_host(Y, mu[:, None] * L)
        np.testing.assert_array_equal(res["clone_loglik"], ll)
        t = ll + np.log(alpha)[None, :] + (0.0 if ex is None else ex)
        ok = np.arange(N) != 13
        np.testing.assert_allclose(res["loglik"][ok], logsumexp(t[ok], axis=1), rtol=1e-13)
        np.testing.assert_allclose(res["clone_probs"][ok], np.exp(t[ok] - logsumexp(t[ok], axis=1)[:, None]), rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(res["clone_probs"][ok].sum(1), 1.0, rtol=1e-13)
        assert np.isnan(res["clone_probs"][13]).all() and res["clone"][13] == "unassigned" and res["loglik"][13] == -np.inf
        assert res["clone_probs"][21, 2] == 0.0 and np.isfinite(res["loglik"][21])
        assert np.array_equal(res["clone"], ca.clone_assignment(res["clone_probs"], names, 0.95))
        assert res["clone_names"] == names
    strict = ca.assign_cells(fit, Y, L, 0.999999, engine=eng)
    assert (strict["clone"] == "unassigned").sum() >= (res["clone"] == "unassigned").sum()
    again = ca.recompute_clone_assignment(ca.assign_cells(fit, Y, L, engine=eng), 0.999999)
    assert np.array_equal(again["clone"], strict["clone"])
    assert "80 cells" in repr(res) and "4 clones" in repr(res) and "80 cells" in repr(again)
    with pytest.raises(ValueError, match="extra_loglik is"):
        ca.assign_cells(fit, Y, L, extra_loglik=extra[:-1], engine=eng)
