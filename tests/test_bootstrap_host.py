"""bootstrap_gene_weights / clone_loglik_reweighted / bootstrap_assignments on the host (float64 numpy only): the gene-reweighted log-likelihood, its
weights and the bootstrap support of clone calls, through an engine stub without the device method -- no GPU.

The yardstick is ``ref_ll`` of tests/test_gpu_clone_loglik.py on the RESAMPLED matrices: for integer weights ``ll_r`` must be the log-likelihood
(``const=False``) of the matrix with gene g repeated ``w_rg`` times, minus ``sum_g w_rg y_ng eta_ng`` (the same for every clone, left out by the call).
Bar: the project's float64 bar, ``1e-10 x`` the sum of the terms' magnitudes (``scale`` of ``ref_ll`` on the same resampled matrices, which counts the
subtracted term)."""
import numpy as np
import pytest

import clonealign_amd as ca
from clonealign_amd import api
from tests._cases import make_case
from tests.test_block_loglik_host import HostOnly, close, planted_fit
from tests.test_gpu_clone_loglik import ref_ll


def resampled_ref(Y, E, U, V, w):
    """(ll, scale) [N, C] of the matrix with gene g repeated w[g] times, const=False, minus sum_g w_g y_ng eta_ng."""
    idx = np.repeat(np.arange(Y.shape[1]), w.astype(np.int64))
    with np.errstate(divide="ignore", invalid="ignore"):
        ll, scale = ref_ll(Y[:, idx], E[idx], U, None if V is None else V[idx], const=False)
    if U is not None:
        ll = ll - ((Y * (U @ V.T)) @ w)[:, None]
    return ll, scale


@pytest.mark.parametrize("D", [0, 1, 3])
def test_host_form_is_the_log_likelihood_of_the_resampled_matrix(D):
    N, G, C, R = 211, 97, 4, 6
    rng = np.random.default_rng(40 + D)
    case = make_case(N=N, G=G, C=C, K=0, seed=3)
    Y, L = case["Y"].astype(np.float64), case["L"].astype(np.float64)
    L[7, 2] = 0.0                                                     # a zero of E: -inf exactly where a positive count meets it with a positive weight
    Y[:, 7] = 0
    Y[11, 7] = 3
    E = rng.lognormal(0, 0.5, G)[:, None] * L
    U, V = (None, None) if D == 0 else (rng.normal(size=(N, D)) * 0.5, rng.normal(size=(G, D)) * 0.3)
    w = api.bootstrap_gene_weights(G, R, seed=5)
    w[0, 7], w[1, 7] = 2.0, 0.0                                       # replicate 0 sees the gene, replicate 1 does not
    w[2] = 1.0                                                        # all ones: clone_loglik(const=False) minus the term
    out = api._clone_loglik_reweighted_host(Y, E, U, V, w, chunk=50, with_scale=True)
    assert out["ll"].shape == (N, R, C) and not np.isnan(out["ll"]).any()
    for r in range(R):
        ref, scale = resampled_ref(Y, E, U, V, w[r])
        close(out["ll"][:, r], ref, scale, f"D={D} replicate {r}")
        np.testing.assert_allclose(out["reads"][:, r], Y @ w[r], rtol=1e-13)
    assert np.isneginf(out["ll"][11, 0, 2]) and np.isfinite(out["ll"][11, 1, 2])
    plain = api._clone_loglik_host(Y, E, U, V, const=False)
    if D > 0:
        plain = plain - (Y * (U @ V.T)).sum(1)[:, None]
    close(out["ll"][:, 2], plain, out["scale"][:, 2] + (0 if D == 0 else (Y * np.abs(U @ V.T)).sum(1)[:, None]), f"D={D} all ones")
    # the reduced form is the reduction of ll: votes by argmax, the shares by softmax, under a prior that excludes a clone somewhere
    lp = rng.normal(size=(N, C))
    lp[5, 1] = -np.inf
    red = api._clone_loglik_reweighted_host(Y, E, U, V, w, log_prior=lp, want_ll=False, chunk=64)
    t = out["ll"] + lp[:, None, :]
    assert red["ll"] is None and np.array_equal(red["votes"], (np.argmax(t, 2)[:, :, None] == np.arange(C)).sum(1))
    p = np.exp(t - t.max(2, keepdims=True))
    p /= p.sum(2, keepdims=True)
    np.testing.assert_allclose(red["prob_sum"], p.sum(1), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(red["prob_sq"], (p * p).sum(1), rtol=1e-12, atol=1e-15)
    assert red["votes"].sum(1).tolist() == [R] * N and red["prob_sum"][5, 1] == 0.0
    part = api._clone_loglik_reweighted_host(Y, E, U, V, w[3:5], log_prior=lp, cells=(40, 90))
    assert np.array_equal(part["ll"], out["ll"][40:90, 3:5])


def test_edges_zero_reads_zero_weights_and_a_clone_without_weighted_expression():
    N, G, C = 60, 40, 3
    rng = np.random.default_rng(2)
    case = make_case(N=N, G=G, C=C, K=0, seed=9)
    Y, L = case["Y"].astype(np.float64), case["L"].astype(np.float64)
    L[:, 1] = 0.0
    L[30:, 1] = 2.0                                                   # clone 1 is expressed in the genes 30.. only
    E = rng.lognormal(0, 0.5, G)[:, None] * L
    w = np.ones((3, G))
    w[1, 30:] = 0.0                                                   # replicate 1 has no weighted gene of positive E for clone 1
    w[2, :] = 0.0
    w[2, 35] = 1.5                                                    # replicate 2 weighs one gene
    Y[4, 35] = 0                                                      # cell 4 has all its reads on zero-weight genes there
    Y[6, :30] = 0                                                     # cell 6 has no count against the zeros of clone 1
    U, V = rng.normal(size=(N, 2)), rng.normal(size=(G, 2)) * 0.2
    U[:, 0] = 0.0
    U[20] = (1.0, 0.0)
    V[[3, 12], 0], V[[4, 31], 0] = 800.0, -800.0                      # eta = +-800 on a few genes of cell 20 (factor 0 is 0 in every other cell)
    for Uv, Vv in ((None, None), (U, V)):
        out = api._clone_loglik_reweighted_host(Y, E, Uv, Vv, w)
        ll = out["ll"]
        assert not np.isnan(ll).any() and not np.isnan(out["prob_sum"]).any()
        assert (ll[4, 2] == 0.0).all() and out["reads"][4, 2] == 0.0
        has = Y[:, :30].sum(1) > 0
        assert np.isneginf(ll[has, 1, 1]).all() and np.isneginf(ll[has, 0, 1]).all()
        assert np.isfinite(ll[6, 0]).all() and not np.isnan(ll[6, 1]).any()
        # (cell 20 under replicate 2: its one weighted gene lies 800 below the cell's largest exponent, which is taken over EVERY gene as in clone_loglik,
        #  so Z underflows to 0 there and the entry is +inf -- never NaN)
        assert np.isfinite(np.delete(ll[:, :, 0], 20, axis=0)).all() and np.isfinite(ll[20, :2, 0]).all()


def test_bootstrap_gene_weights():
    G, R = 300, 50
    w = api.bootstrap_gene_weights(G, R, seed=7)
    assert w.shape == (R, G) and w.dtype == np.float64 and (w >= 0).all() and np.array_equal(w, np.round(w))
    assert np.array_equal(w.sum(1), np.full(R, float(G)))
    assert np.array_equal(w, api.bootstrap_gene_weights(G, R, seed=7))
    assert np.array_equal(w[:5], api.bootstrap_gene_weights(G, 5, seed=7))
    assert not np.array_equal(w, api.bootstrap_gene_weights(G, R, seed=8))
    assert not np.array_equal(w[0], w[1])
    # a gene's count is Binomial(G, 1/G): mean 1, variance 1 - 1/G; the mean over the replicates of any set of genes within 5 standard errors
    big = api.bootstrap_gene_weights(G, 400, seed=1)
    half = big[:, :G // 2]
    se = np.sqrt((1.0 - 1.0 / G) / half.size)
    assert abs(half.mean() - 1.0) <= 5 * se, (half.mean(), se)
    assert abs(big.var() - (1.0 - 1.0 / G)) < 0.05
    blocks = np.array(["a"] * 100 + ["b"] * 50 + [None] * 30 + ["c"] * 120, dtype=object)
    wb = api.bootstrap_gene_weights(G, R, seed=7, blocks=blocks)
    for sl in (slice(0, 100), slice(100, 150), slice(150, 180), slice(180, 300)):
        assert (wb[:, sl] == wb[:, sl.start:sl.start + 1]).all()
    assert np.array_equal(wb[:, [0, 100, 150, 180]].sum(1), np.full(R, 4.0))       # four blocks, four draws
    assert np.array_equal(wb[:3], api.bootstrap_gene_weights(G, 3, seed=7, blocks=blocks))
    with pytest.raises(ValueError, match="labels"):
        api.bootstrap_gene_weights(G, 3, blocks=blocks[:-1])


def test_zero_one_weights_are_clone_loglik_by_block_without():
    N, G, C = 300, 120, 3
    Y, L, fit, _rng = planted_fit(N, G, C, seed=17)
    blocks = np.array(["chr1"] * 30 + ["chr2"] * 15 + ["chr7"] * 50 + ["chrX"] * 25, dtype=object)
    eng = HostOnly(N, G)
    by = ca.clone_loglik_by_block(fit, Y, L, blocks, psi="fit", const=False, engine=eng)
    w = np.stack([(blocks != b).astype(np.float64) for b in by["block_names"]])
    rw = ca.clone_loglik_reweighted(fit, Y, L, w, psi="fit", engine=eng)
    eta = np.asarray(fit["ml_params"]["psi"]) @ np.asarray(fit["ml_params"]["W"]).T
    Yd = np.asarray(Y, dtype=np.float64)
    for b in range(len(by["block_names"])):
        term = (Yd * eta) @ w[b]
        scale = np.abs(by["without"][:, b]) + np.abs(term)[:, None] + (Yd * np.abs(eta)) @ w[b][:, None]
        close(rw["ll"][:, b], by["without"][:, b] - term[:, None], scale, f"without block {b}")


def test_bootstrap_assignments_on_the_host():
    N, G, C = 400, 120, 3
    Y, L, fit, rng = planted_fit(N, G, C, seed=23)
    extra = rng.normal(size=(N, C))
    eng = HostOnly(N, G)
    ref = ca.assign_cells(fit, Y, L, extra_loglik=extra, psi="fit", engine=eng)
    bs = ca.bootstrap_assignments(fit, Y, L, n_rep=40, seed=3, extra_loglik=extra, psi="fit", engine=eng)
    for k in ("clone_probs", "loglik", "clone_loglik"):
        assert np.array_equal(bs[k], ref[k]), k
    assert np.array_equal(bs["clone"], ref["clone"]) and bs["clone_names"] == ref["clone_names"]
    assert bs["n_rep"] == 40 and bs["weights_seed"] == 3
    assert bs["support"].shape == (N,) and bs["clone_support"].shape == (N, C) and bs["mean_probs"].shape == (N, C) and bs["sd_probs"].shape == (N, C)
    np.testing.assert_allclose(bs["clone_support"].sum(1), 1.0, rtol=1e-12)
    cstar = ref["clone_probs"].argmax(1)
    assert np.array_equal(bs["support"], bs["clone_support"][np.arange(N), cstar])
    low = bs["support"] < 0.95
    assert (bs["clone_bootstrap"][low] == "unassigned").all() and np.array_equal(bs["clone_bootstrap"][~low], ref["clone"][~low])
    assert bs["n_newly_unassigned"] == int((low & (ref["clone"] != "unassigned")).sum())
    again = ca.bootstrap_assignments(fit, Y, L, n_rep=40, seed=3, extra_loglik=extra, psi="fit", engine=eng)
    assert np.array_equal(again["support"], bs["support"]) and np.array_equal(again["mean_probs"], bs["mean_probs"])
    blocks = np.repeat(np.arange(12), 10)
    blk = ca.bootstrap_assignments(fit, Y, L, n_rep=10, seed=3, blocks=blocks, psi="fit", engine=eng)
    assert blk["n_rep"] == 10 and not np.array_equal(blk["support"], bs["support"])
    # all-ones weights: every replicate is the call itself
    one = ca.bootstrap_assignments(fit, Y, L, weights=np.ones((3, G)), extra_loglik=extra, psi="fit", engine=eng)
    assert one["weights_seed"] is None and one["n_rep"] == 3
    assert (one["support"] == 1.0).all() and one["n_newly_unassigned"] == 0
    np.testing.assert_allclose(one["mean_probs"], ref["clone_probs"], rtol=0, atol=1e-9)
    assert one["sd_probs"].max() <= 1e-6
    # the refusals name the offender
    bad = np.ones((3, G))
    bad[1, 17] = -0.5
    with pytest.raises(ValueError, match="replicate 1, gene 17"):
        ca.bootstrap_assignments(fit, Y, L, weights=bad, psi="fit", engine=eng)
    bad[1, 17] = np.nan
    with pytest.raises(ValueError, match="replicate 1, gene 17"):
        ca.clone_loglik_reweighted(fit, Y, L, bad, psi="fit", engine=eng)
    bad[1] = 0.0
    with pytest.raises(ValueError, match="replicate 1 are all zero"):
        ca.clone_loglik_reweighted(fit, Y, L, bad, psi="fit", engine=eng)
    with pytest.raises(ValueError, match="expected"):
        ca.clone_loglik_reweighted(fit, Y, L, np.ones((3, G - 1)), psi="fit", engine=eng)
    with pytest.raises(ValueError, match="below 1"):
        ca.bootstrap_assignments(fit, Y, L, n_rep=0, psi="fit", engine=eng)
    with pytest.raises(ValueError, match="cell range"):
        ca.clone_loglik_reweighted(fit, Y, L, np.ones((2, G)), psi="fit", cells=(10, N + 1), engine=eng)
    with pytest.raises(ValueError, match="extra_loglik"):
        ca.bootstrap_assignments(fit, Y, L, n_rep=2, extra_loglik=extra[:-1], psi="fit", engine=eng)


def test_support_withholds_the_wrong_calls_a_multinomial_posterior_makes_on_overdispersed_counts():
    """The point of it.  N = 400 cells of C = 4 clones, G = 300 genes of which 70 % have the same copy number in every clone, 2000 reads a cell drawn from a
    DIRICHLET-multinomial with concentration phi = 100 around the clone's profile (the value estimate_concentration is tested at), scored under the true mu
    with K = 0 by the multinomial of assign_cells; R = 200 replicates, one fixed seed.  The conditions are the issue's, wide against what it measured (12-27
    wrong calls with posterior >= 0.95, none of them with support >= 0.95, median support 0.45-0.52 of wrong against 0.91-0.93 of right calls)."""
    N, G, C, reads, phi, R = 400, 300, 4, 2000, 100.0, 200
    rng = np.random.default_rng(0)
    L = np.full((G, C), 2.0)
    diff = rng.choice(G, size=int(0.3 * G), replace=False)
    L[diff] = rng.integers(1, 5, size=(diff.size, C)).astype(np.float64)
    mu = rng.lognormal(0, 1, G)
    z = rng.integers(0, C, N)
    P = mu[:, None] * L
    P /= P.sum(0)
    Y = np.stack([rng.multinomial(reads, rng.dirichlet(phi * P[:, c] + 1e-12)) for c in z]).astype(np.float64)
    fit = ca.ClonealignFit(ml_params={"mu": mu, "alpha": np.full(C, 1.0 / C)}, clone_names=[f"c{i}" for i in range(C)])
    bs = ca.bootstrap_assignments(fit, Y, L, n_rep=R, seed=0, engine=HostOnly(N, G))
    call = bs["clone_probs"].argmax(1)
    wrong = call != z
    post, sup = bs["clone_probs"].max(1) >= 0.95, bs["support"] >= 0.95
    n_post, n_post_wrong, n_sup, n_sup_wrong = int(post.sum()), int((post & wrong).sum()), int(sup.sum()), int((sup & wrong).sum())
    med_wrong, med_right = float(np.median(bs["support"][wrong])), float(np.median(bs["support"][~wrong]))
    print(f"posterior >= 0.95: {n_post} calls, {n_post_wrong} wrong; support >= 0.95: {n_sup} calls, {n_sup_wrong} wrong; "
          f"median support wrong {med_wrong:.3f} / right {med_right:.3f}; newly unassigned {bs['n_newly_unassigned']}")
    assert n_post_wrong >= 5
    assert n_sup_wrong <= n_post_wrong / 4
    assert med_wrong < med_right - 0.2
