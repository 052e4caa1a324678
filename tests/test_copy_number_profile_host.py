"""api.copy_number_profile on the host (host=True: the numpy restatement on both sides), against the brute force: the multinomial log-likelihood of all
cells recomputed from scratch with api._clone_loglik_host under the modified and under the given copy-number matrix.  The cases and the planted recipe are
tests/_copy_number_profile_cases.py's, which tests/test_gpu_copy_number_profile.py runs on the device."""
import numpy as np
import pytest

from clonealign_amd import api

from tests import _copy_number_profile_cases as cc


@pytest.mark.parametrize("D", [1, 0, 3])
def test_restatement_against_brute_force(D):
    """60 x 90 x 3: fifteen random (gene, clone, candidate) and six (block, clone, candidate) triples; delta_ll equals total_ll(L modified) - total_ll(L)
    within 1e-10 of the summed magnitudes of the two totals' terms (the totals cancel: a bar relative to the difference would be wrong).  Largest ratios
    seen: 4.6e-16 (D = 1), 1.0e-15 (D = 0), 3.1e-16 (D = 3) of that sum."""
    rng = np.random.default_rng(100 + D)
    N, G, C, B = 60, 90, 3, 6
    mu = rng.lognormal(0.0, 1.0, G)
    L = rng.integers(1, 6, (G, C)).astype(np.float64)
    W, psi = (0.5 * rng.normal(size=(G, D)), rng.normal(size=(N, D))) if D else (None, None)
    z = rng.integers(0, C, N)
    w = (mu[:, None] * L)[:, z].T * (np.exp(psi @ W.T) if D else 1.0)
    Y = np.stack([rng.multinomial(1500, w[n] / w[n].sum()) for n in range(N)]).astype(np.int32)
    blocks = np.sort(rng.integers(0, B, G))
    blocks[:B] = np.arange(B)                                        # (every label occurs, in order: label = row of the profile)
    blocks = np.sort(blocks)
    fit = cc.hand_fit(mu, W, psi, z, cc.NAMES4[:C])
    base, base_mag = cc.total_ll(Y, mu, L, W, psi, z)
    worst = 0.0
    for bl, n_trip in ((None, 15), (blocks, 6)):
        prof = api.copy_number_profile(fit, Y, L, blocks=bl, host=True)
        assert not np.isnan(prof["delta_ll"]).any()
        for _ in range(n_trip):
            r, c, j = int(rng.integers(0, G if bl is None else B)), int(rng.integers(0, C)), int(rng.integers(0, 7))
            L2 = L.copy()
            L2[(r if bl is None else bl == r), c] = prof["kappa"][j]
            mod, mod_mag = cc.total_ll(Y, mu, L2, W, psi, z)
            got, want = prof["delta_ll"][r, c, j], mod - base
            if np.isinf(want):
                assert got == want, (r, c, j)
                continue
            worst = max(worst, abs(got - want) / (mod_mag + base_mag))
            assert abs(got - want) <= 1e-10 * (mod_mag + base_mag), (r, c, j, got, want)
    print(f"D = {D}: largest |delta_ll - brute force| / (sum of the terms' magnitudes) = {worst:.2e}")


def test_planted_recovery():
    """The recipe of ``planted``.  The outcome is first derived by brute force, without the code under test: for every (segment, clone) the candidate in
    1 .. 6 with the largest total log-likelihood (api._clone_loglik_host on the modified matrix) is the true copy number.  Then ``check_planted``.
    Measured (numpy restatement): block-mode log_bf of the four corrupted entries 388 .. 1398, 0 exactly on every clean entry; per gene 106 corrupted entries,
    recovered 0.934; 794 clean entries, kept 0.965 (this file's draw order; the recipe's author reports 0.967 and 0.964 with another)."""
    fit, Y, L_given, L_true, seg, bad, z = cc.planted()
    mu, W, psi = (fit["ml_params"][k] for k in ("mu", "W", "psi"))
    for b in np.unique(seg):
        for c in range(3):
            ll = []
            for k in range(1, 7):
                L2 = np.array(L_given)
                L2[seg == b, c] = k
                ll.append(cc.total_ll(Y, mu, L2, W, psi, z)[0])
            assert 1 + int(np.argmax(ll)) == L_true[seg == b, c][0], (b, c, ll)
    cc.check_planted(fit, Y, L_given, L_true, seg, bad, host=True)


def test_exact_values_of_the_restatement():
    for what, args, Lint in cc.exact_cases():
        cc.check_exact(api._copy_number_profile_host, what, args, Lint)


def test_exact_rules():
    """Copy number 0 with and without reads, an absent clone, a clone with one expressed gene, a cell without reads, "unassigned" cells dropped, colliding
    candidates refused; no NaN anywhere; blocks = arange(G) equals per-gene mode within 1e-10 of sum_n s_n (|log1p(a)| + |a| / (1 + a))."""
    fit, Y, L, z, planted_read = cc.rules_case()
    prof = api.copy_number_profile(fit, Y, L, host=True)
    cc.check_rules(prof, Y, L, z, planted_read, "host")
    # "unassigned" cells are dropped: the same bits as the call on the assigned cells alone
    used = np.setdiff1d(np.arange(40), [6, 9])
    ml = fit["ml_params"]
    sub = cc.hand_fit(ml["mu"], ml["W"], ml["psi"][used], z[used], cc.NAMES4)
    alone = api.copy_number_profile(sub, np.asarray(Y)[used], L, host=True)
    for k in ("T_observed", "cost", "delta_ll", "posterior"):
        assert np.array_equal(prof[k], alone[k]), k
    with pytest.raises(ValueError, match="coincide after saturation"):
        api.copy_number_profile(fit, Y, L, candidates=(5, 6, 7), host=True)
    for bad in ((1, -1), (1, np.nan), ()):
        with pytest.raises(ValueError, match="candidates"):
            api.copy_number_profile(fit, Y, L, candidates=bad, host=True)
    assert np.array_equal(api.copy_number_profile(fit, Y, L, candidates=(5, 6, 7), saturate=False, host=True)["kappa"], [5.0, 6.0, 7.0])
    # every gene its own block
    blk = api.copy_number_profile(fit, Y, L, blocks=np.arange(70), host=True)
    _want, scale = cc.numpy_cost(ml["mu"][:, None] * L, ml["W"], ml["psi"][used], z[used], np.asarray(Y)[used].sum(1), ml["mu"], np.arange(7.0))
    both = np.isinf(prof["delta_ll"])
    assert np.array_equal(both, np.isinf(blk["delta_ll"])) and np.array_equal(prof["delta_ll"][both], blk["delta_ll"][both])
    diff = np.abs(np.where(both, 0.0, prof["delta_ll"] - np.where(both, 0.0, blk["delta_ll"])))
    print(f"blocks = arange(G) against per-gene mode: largest |difference| / scale = {(diff[~both] / np.where(scale[~both] > 0, scale[~both], 1.0)).max():.2e}")
    assert (diff[~both] <= 1e-10 * scale[~both]).all()
    assert np.array_equal(blk["input_cn"], prof["input_cn"]) and np.array_equal(blk["map_cn"], prof["map_cn"])


def test_a_candidate_that_leaves_a_cell_with_reads_no_expressed_gene_is_minus_infinity():
    """``rules_case`` with the reads of clone_c's cells moved from gene 5, the clone's only expressed gene, to gene 6, where its copy number is 0: the counts
    are impossible under the matrix as given AND under candidate 0 on gene 5, so the observed side is finite (gene 5 has no reads) while the cells'
    normalisers vanish (cost = -inf).  delta_ll is -inf there, per gene and for a block that holds gene 5, never +inf or NaN."""
    fit, Y, L, z, _planted_read = cc.rules_case()
    Y2 = np.array(Y)
    Y2[z == 2, 6], Y2[z == 2, 5] = Y2[z == 2, 5], 0
    blocks = np.r_[np.zeros(10, dtype=np.int64), 1 + np.arange(60) // 2]
    for bl, row in ((None, 5), (blocks, 0)):
        prof = api.copy_number_profile(fit, Y2, L, blocks=bl, host=True)
        assert prof["T_observed"][5, 2] == 0.0 and prof["T_observed"][6, 2] > 0.0
        assert np.isfinite(prof["gain"][row, 2, 0])
        assert prof["cost"][row, 2, 0] == -np.inf and prof["delta_ll"][row, 2, 0] == -np.inf
        assert not np.isnan(prof["delta_ll"]).any() and not np.isnan(prof["posterior"]).any()
