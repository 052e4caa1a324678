"""The numpy restatement of ca_clone_separability (api._clone_separability_host) against a triple loop over (cell, a, b); its invariances and exact zeros;
the closed form of the confusion probability (api.clone_separability) against a host Monte Carlo; reads_needed and merge_candidates.  No GPU."""
import math

import numpy as np
import pytest

from clonealign_amd import api, engine


def test_new_symbols_are_exported():
    assert {"ca_clone_separability", "ca_clone_separability_kernel_ms"} <= set(engine.EXPORTS)
    import clonealign_amd
    for name in ("clone_separability", "reads_needed", "merge_candidates", "edgeworth_normal_cdf"):
        assert hasattr(clonealign_amd, name)


def small_case(D=2, seed=3):
    rng = np.random.default_rng(seed)
    N, G, C = 7, 11, 3
    E = rng.lognormal(0.0, 1.0, (G, 1)) * rng.integers(1, 5, (G, C)).astype(np.float64)
    E[2, 1] = E[5, 0] = E[5, 2] = E[9, 2] = 0.0
    V = rng.normal(size=(G, D)) * 0.7 if D else None
    U = rng.normal(size=(N, D)) if D else None
    return E, V, U


def triple_loop(E, V, U):
    """The header's definitions, one (cell, a, b) at a time in Python floats."""
    G, C = E.shape
    N = U.shape[0]
    e = E / E.sum(0)
    logZ, out = np.zeros((N, C)), np.zeros((4, N, C, C))
    for n in range(N):
        eta = [sum(U[n, d] * V[g, d] for d in range(U.shape[1])) for g in range(G)]
        m = max(eta)
        Z = [sum(e[g, c] * math.exp(eta[g] - m) for g in range(G)) for c in range(C)]
        for c in range(C):
            logZ[n, c] = m + math.log(Z[c])
        for a in range(C):
            for b in range(C):
                if a == b:
                    continue
                Delta = math.log(Z[a]) - math.log(Z[b])
                for g in range(G):
                    if e[g, a] <= 0:
                        continue
                    p = e[g, a] * math.exp(eta[g] - m) / Z[a]
                    if e[g, b] <= 0:
                        out[0, n, a, b] += p
                    else:
                        d = math.log(e[g, a]) - math.log(e[g, b]) - Delta
                        for k in (1, 2, 3):
                            out[k, n, a, b] += p * d ** k
    return (logZ,) + tuple(out)


def test_restatement_against_a_triple_loop():
    E, V, U = small_case()
    got, want = api._clone_separability_host(E, V, U, chunk=3), triple_loop(E, V, U)
    assert [a.shape for a in got] == [(7, 3), (7, 3, 3), (7, 3, 3), (7, 3, 3), (7, 3, 3)]
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.abs(g - w).max() <= 1e-13 * max(1.0, np.abs(w).max()), k
    assert (got[1][:, 0, 1] > 0).all() and (got[1][:, 1, 0] > 0).all() and (got[1][:, 1, 2] > 0).all()   # the planted zeros exclude


def test_invariance_to_the_scale_of_a_column():
    E, V, U = small_case()
    one = api._clone_separability_host(E, V, U, with_scale=True)
    two = api._clone_separability_host(E * np.array([1.0, 37.5, 1e-3]), V, U)
    for k in range(1, 5):
        assert (np.abs(one[k] - two[k]) <= 1e-12 * np.maximum(one[min(k, 2) + 4] if k > 1 else 1.0, 1e-300) + 1e-15).all(), k
    assert np.abs(one[0] - two[0]).max() <= 1e-12                    # logZ sees e, not E: invariant as well


def test_no_factor_equals_a_zero_factor_within_the_bars():
    E, _V, _U = small_case()
    G = E.shape[0]
    zero = api._clone_separability_host(E, np.ones((G, 1)), np.zeros((4, 1)), with_scale=True)
    none = api._clone_separability_host(E, None, None)
    assert none[0].shape == (1, 3)
    for n in range(4):
        assert np.abs(none[0][0] - zero[0][n]).max() <= 1e-10
        assert np.abs(none[1][0] - zero[1][n]).max() <= 1e-10
        for k in (1, 2, 3):
            assert (np.abs(none[1 + k][0] - zero[1 + k][n]) <= 1e-10 * zero[4 + k][n]).all(), k


def zero_case(D):
    """A duplicated clone (3 = 0), a clone that is twice another (4 = 2 x 1), zeros of E in places; clone 2 has no zero anywhere."""
    rng = np.random.default_rng(21)
    N, G = 9, 40
    E = rng.lognormal(0.0, 1.0, (G, 1)) * rng.integers(1, 5, (G, 3)).astype(np.float64)
    E[rng.random((G, 3)) < 0.15] = 0.0
    E[:, 2] = np.maximum(E[:, 2], 0.5)
    E = np.column_stack([E, E[:, 0], 2.0 * E[:, 1]])
    V, U = (rng.normal(size=(G, D)) * 0.5, rng.normal(size=(N, D))) if D else (None, None)
    return E, V, U


def check_exact_zeros(res, E, what):
    logZ, excl, m1, m2, m3 = res
    C = E.shape[1]
    assert all(np.isfinite(a).all() for a in res), what
    for a in range(C):
        assert all(x[:, a, a].tolist() == [0.0] * x.shape[0] for x in (excl, m1, m2, m3)), what
        for b in range(C):
            if a != b and not ((E[:, a] > 0) & (E[:, b] == 0)).any():
                assert (excl[:, a, b] == 0.0).all(), (what, a, b)
    for a, b in ((0, 3), (3, 0), (1, 4), (4, 1)):
        assert (m1[:, a, b] == 0.0).all() and (m2[:, a, b] == 0.0).all() and (m3[:, a, b] == 0.0).all() and (excl[:, a, b] == 0.0).all(), (what, a, b)
    assert (excl[:, 0, 1] > 0).all() and (m2[:, 0, 2] > 0).all() and (m1[:, 0, 2] > 0).all(), what


@pytest.mark.parametrize("D", (0, 1, 3))
def test_exact_zeros(D):
    E, V, U = zero_case(D)
    check_exact_zeros(api._clone_separability_host(E, V, U), E, f"D = {D}")


def test_m1_is_a_divergence():
    """m1 = sum_S p_a log(p_a / p_b) is the Kullback-Leibler divergence where neither clone excludes the other, so m1 >= -1e-12 scale there.  With exclusions
    the two restricted masses differ (q_ab = sum_S p_a, q_ba = sum_S p_b) and the log-sum inequality gives the exact bound m1 >= q_ab log(q_ab / q_ba), which
    is the same statement at q_ab = q_ba = 1; it is asserted for every ordered pair."""
    E, V, U = zero_case(2)
    res = api._clone_separability_host(E, V, U, with_scale=True)
    excl, m1, scale = res[1], res[2], res[5]
    q = 1.0 - excl
    C = E.shape[1]
    plain = 0
    for a in range(C):
        for b in range(C):
            if a == b:
                continue
            bound = q[:, a, b] * np.log(q[:, a, b] / q[:, b, a])
            assert (m1[:, a, b] >= bound - 1e-12 * scale[:, a, b]).all(), (a, b)
            if (excl[:, a, b] == 0).all() and (excl[:, b, a] == 0).all():
                plain += 1
                assert (bound == 0.0).all() and (m1[:, a, b] >= -1e-12 * scale[:, a, b]).all(), (a, b)
    assert plain >= 4


def test_refusals_of_the_restatement():
    E, V, U = small_case()
    with pytest.raises(ValueError, match=r"clone_separability: E has a negative"):
        api._clone_separability_host(-E, V, U)
    with pytest.raises(ValueError, match=r"clone_separability: E is zero in every gene of clone 1"):
        api._clone_separability_host(np.column_stack([E[:, 0], np.zeros(11)]), V, U)
    with pytest.raises(ValueError, match=r"C = 1"):
        api._clone_separability_host(E[:, :1], V, U)
    with pytest.raises(ValueError, match=r"U has a non-finite"):
        api._clone_separability_host(E, V, np.where(np.arange(14).reshape(7, 2) == 3, np.nan, U))


def monte_carlo_case():
    """The recipe of the confusion check: G = 300, C = 3, L = 2 but for 15 genes per clone at 3 / 1 / 4, one gene with copy number 0 in clone 1 where clone 0
    has 3; W ~ 0.5 N(0, 1), 40 cells with psi ~ N(0, 1)."""
    rng = np.random.default_rng(5)
    G, C, N = 300, 3, 40
    mu = rng.lognormal(0.0, 1.0, G)
    L = np.full((G, C), 2.0)
    for c, v in enumerate((3.0, 1.0, 4.0)):
        L[15 * c:15 * (c + 1), c] = v
    L[0, 0], L[0, 1] = 3.0, 0.0
    W, psi = 0.5 * rng.normal(size=(G, 1)), rng.normal(size=(N, 1))
    fit = {"ml_params": {"mu": mu, "W": W, "psi": psi}, "clone_names": ["a", "b", "c"]}
    return fit, L, rng


@pytest.fixture(scope="module")
def monte_carlo():
    """{t: (empirical confusion [3, 3], refined closed form, plain normal closed form)}, 4000 multinomial rows of t reads per (cell, clone).  Lambda is linear
    in the counts and log p_a - log p_b takes one value on all genes with the same copy-number triple, so the rows are drawn over the five triples with their
    summed probabilities: by the lumping property of the multinomial that is the distribution of the per-triple sums of a row over all 300 genes."""
    fit, L, rng = monte_carlo_case()
    ml = fit["ml_params"]
    w = (ml["mu"][:, None] * L)[None] * np.exp(ml["psi"] @ ml["W"].T)[:, :, None]            # [N, G, C]
    p = w / w.sum(1, keepdims=True)
    triples, group = np.unique(L, axis=0, return_inverse=True)
    group = group.reshape(-1)
    first = np.array([np.flatnonzero(group == k)[0] for k in range(len(triples))])
    assert len(triples) == 5
    out = {}
    for t in (50, 200, 800):
        emp = np.zeros((3, 3))
        for n in range(p.shape[0]):
            pg = np.stack([p[n, group == k].sum(0) for k in range(len(triples))])           # [groups, C]
            for a in range(3):
                y = rng.multinomial(t, pg[:, a] / pg[:, a].sum(), size=4000).astype(np.float64)
                for b in range(3):
                    if a == b:
                        continue
                    S, X = (triples[:, a] > 0) & (triples[:, b] > 0), (triples[:, a] > 0) & (triples[:, b] == 0)
                    d = np.log(p[n, first[S], a]) - np.log(p[n, first[S], b])
                    emp[a, b] += ((y[:, S] @ d <= 0) & (y[:, X].sum(1) == 0)).mean()
        sep = api.clone_separability(fit, L, t, host=True, per_cell=True)
        q, kappa, v, _c3 = api._per_read_cumulants(sep["excl"], sep["m1"], sep["m2"], sep["m3"])
        plain = api._p_confuse(float(t), q, kappa, v, 0.0).mean(0) * ~np.eye(3, dtype=bool)
        out[t] = (emp / p.shape[0], sep["confusion"], plain)
    return out


@pytest.mark.parametrize("t,bar", ((50, 0.02), (200, 0.004), (800, 0.0006)))
def test_confusion_against_monte_carlo(monte_carlo, t, bar):
    """|confusion - empirical|, largest entry, measured with numpy's multinomial at default_rng(5): 0.0068 / 0.0017 / 0.00046 at t = 50 / 200 / 800 reads;
    without the skewness term 0.024 / 0.0058 / 0.0022.  Bars: 0.02 / 0.004 / 0.0006 (2.5 x the first measurement of this recipe, 0.0079 / 0.0016 / 0.0002,
    taken with another draw; Monte Carlo standard errors are about 1e-3 at t = 50 and 2e-4 at t = 800)."""
    emp, refined, plain = monte_carlo[t]
    print(f"t = {t}: refined {np.abs(refined - emp).max():.5f}, plain normal {np.abs(plain - emp).max():.5f}")
    assert (np.diag(refined) == 0).all() and np.abs(refined - emp).max() <= bar


def test_the_skewness_term_earns_its_place(monte_carlo):
    """At 50 reads the refined form beats the plain normal: the check that m3 is wired correctly (a wrong sign or scale makes it worse, not better)."""
    emp, refined, plain = monte_carlo[50]
    assert np.abs(refined - emp).max() < 0.5 * np.abs(plain - emp).max()


def test_edgeworth_normal_cdf():
    from scipy.special import ndtr
    x = np.linspace(-3, 3, 13)
    assert np.allclose(api.edgeworth_normal_cdf(x, 0.0, 1.0), ndtr(x), rtol=0, atol=1e-15)                 # no continuity correction, no skewness: Phi itself
    assert np.array_equal(api.edgeworth_normal_cdf([-1.0, 2.0, 3.0], 2.0, 0.0), [0.0, 1.0, 1.0])          # a step at the mean
    # a gamma(shape k) variable: mean k, variance k, third cumulant 2 k
    from scipy.stats import gamma
    k = 30.0
    t = np.linspace(15, 50, 36)
    assert np.abs(api.edgeworth_normal_cdf(t, k, k, 2 * k) - gamma.cdf(t, k)).max() < 0.25 * np.abs(ndtr((t - k) / np.sqrt(k)) - gamma.cdf(t, k)).max()


def planted_merge(seed=9):
    """Four clones over 400 genes: clone 3 differs from clone 2 in ONE gene (3 against 2 copies); clones 0 and 1 differ from everything in 40 genes each."""
    rng = np.random.default_rng(seed)
    G, N = 400, 50
    mu = rng.lognormal(0.0, 1.0, G)
    L = np.full((G, 4), 2.0)
    L[:40, 0], L[40:80, 1] = 4.0, 1.0
    L[80:120, 2] = L[80:120, 3] = 3.0
    L[120, 3] = 3.0
    fit = {"ml_params": {"mu": mu, "W": 0.3 * rng.normal(size=(G, 1)), "psi": rng.normal(size=(N, 1))}, "clone_names": ["A", "B", "C", "C2"]}
    return fit, L


def test_merge_candidates_finds_the_planted_pair():
    fit, L = planted_merge()
    sep = api.clone_separability(fit, L, 3000, host=True)
    assert sep["confusion"].shape == (4, 4) and (np.diag(sep["confusion"]) == 0).all()
    found = api.merge_candidates(sep, threshold=0.2)
    assert [f[:2] for f in found] == [("C", "C2")] and found[0][2] > 0.2 and found[0][3] > 0.2
    assert api.merge_candidates(sep, threshold=0.999) == []
    assert sep["confusion"][0, 1] < 1e-6 and sep["kl_per_read"][0, 1] > 100 * sep["kl_per_read"][2, 3] > 0


def test_reads_needed_brackets_the_error():
    fit, L = planted_merge()
    L = np.column_stack([L, L[:, 0]])                                 # a fifth clone identical to the first
    fit = dict(fit, clone_names=fit["clone_names"] + ["A2"])
    sep = api.clone_separability(fit, L, 1000, host=True)
    for error in (0.05, 0.001):
        need = api.reads_needed(sep, error)
        assert need.shape == (5, 5) and (np.diag(need) == 0).all()
        assert need[0, 4] == np.inf and need[4, 0] == np.inf
        q = 1.0 - sep["excl_per_read"]
        for a in range(5):
            for b in range(5):
                if a != b and {a, b} != {0, 4}:
                    t = need[a, b]
                    f = lambda tt: float(api._p_confuse(float(tt), q[a, b], sep["drift_per_read"][a, b], sep["var_per_read"][a, b], sep["cum3_per_read"][a, b]))  # noqa: E731
                    assert np.isfinite(t) and t >= 1 and t == int(t) and f(t) <= error < f(t - 1), (a, b, t)
        assert need[2, 3] > 50 * need[0, 1]                          # one gene apart against forty


def test_python_call_on_the_host():
    fit, L = planted_merge()
    N = 50
    rng = np.random.default_rng(1)
    clones = np.array(fit["clone_names"], dtype=object)[rng.integers(0, 4, N)]
    clones[3] = "unassigned"
    total = rng.integers(100, 3000, N)
    sep = api.clone_separability(fit, L, total, clones=clones, per_cell=True, host=True)
    assert sep["p_confuse"].shape == (N, 4, 4) and sep["logZ"].shape == (N, 4) and sep["m1"].shape == (N, 4, 4)
    assert np.isnan(sep["p_error_cell"][3]) and sep["worst_rival"][3] == -1
    idx = np.array([fit["clone_names"].index(c) if c != "unassigned" else -1 for c in clones])
    for a in range(4):
        sel = idx == a
        assert np.allclose(sep["confusion"][a], sep["p_confuse"][sel, a].mean(0), rtol=1e-12, atol=0)
        assert np.allclose(sep["kl_per_read"][a], sep["m1"][sel, a].mean(0), rtol=1e-12, atol=0)
    n = 7
    assert sep["p_error_cell"][n] == min(1.0, sep["p_confuse"][n, idx[n]].sum()) and sep["worst_rival"][n] == sep["p_confuse"][n, idx[n]].argmax()
    # a prior that favours the rival raises the confusion; overdispersion raises it where it is small
    lp = np.log([0.1, 0.7, 0.1, 0.1])
    assert (api.clone_separability(fit, L, total, log_prior=lp, host=True)["confusion"][0, 1] > api.clone_separability(fit, L, total, host=True)["confusion"][0, 1])
    assert api.clone_separability(fit, L, 3000, concentration=50.0, host=True)["confusion"][0, 1] > 10 * api.clone_separability(fit, L, 3000, host=True)["confusion"][0, 1]
    # a fit without factors: one row serves every cell
    flat = {"ml_params": {"mu": fit["ml_params"]["mu"]}, "clone_names": fit["clone_names"]}
    one = api.clone_separability(flat, L, [500, 500, 2000], host=True, per_cell=True)
    assert one["p_confuse"].shape == (3, 4, 4) and np.array_equal(one["p_confuse"][0], one["p_confuse"][1]) and (one["p_confuse"][2, 0, 1] < one["p_confuse"][0, 0, 1])
    with pytest.raises(ValueError, match="disagree on the number of cells"):
        api.clone_separability(fit, L, np.ones(49), host=True)
