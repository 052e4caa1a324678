"""clone_mixture / mixture_loglik / deconvolve_clones on the host: the float64 numpy form (``api._clone_mixture_host``) of ca_clone_mixture, called directly and
through an engine stub without ``clone_mixture`` -- no GPU.  The model: the counts of a row made of several clones are multinomial in ``sum_c pi_c p_n.c``;
``mix_ll`` is concave in ``pi``, so ``bound = max_c g_c - sum_c pi_c g_c`` bounds what any other weights on the simplex could gain (a theorem: the tests check
it against brute force)."""
import numpy as np
import pytest

import clonealign_amd as ca
from clonealign_amd import api
from tests.test_doublets_host import HostOnly, small


def planted(N=240, G=300, C=4, reads=2000, D=1, seed=0, alpha=0.5, dup=False):
    """Rows drawn from planted Dirichlet(alpha) mixtures of C clones, pure and two-clone rows among them: (Y, E, U, V, PI)."""
    rng = np.random.default_rng(seed)
    L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
    if dup:
        L[:, C - 1] = L[:, 0]                                        # two clones duplicated up to scale
    mu = rng.lognormal(0.0, 1.0, G)
    E = mu[:, None] * L
    if dup:
        E[:, C - 1] *= 3.0
    U, V = (rng.normal(size=(N, D)) * 0.5, rng.normal(size=(G, D)) * 0.3) if D else (None, None)
    PI = rng.dirichlet(np.full(C, alpha), size=N)
    PI[: N // 6] = np.eye(C)[rng.integers(0, C, N // 6)]             # pure rows
    for n in range(N // 6, N // 3):                                  # two-clone rows
        a, b = rng.choice(C, 2, replace=False)
        w = rng.uniform(0.2, 0.8)
        PI[n] = 0.0
        PI[n, a], PI[n, b] = w, 1.0 - w
    eta = np.zeros((N, G)) if D == 0 else U @ V.T
    Y = np.empty((N, G))
    for n in range(N):
        P = E * np.exp(eta[n])[:, None]
        P /= P.sum(0)
        Y[n] = rng.multinomial(reads, P @ PI[n])
    return Y, E, U, V, PI


def evaluate(Y, E, U, V, pi, const=True):
    return api._clone_mixture_host(Y, E, U, V, start=pi, max_iter=0, tol=0.0, const=const)


@pytest.mark.parametrize("D", [0, 2])
def test_evaluation_at_one_hot_and_pair_starts_is_the_singlet_and_the_pair_value(D):
    Y, E, U, V, _rng = small(D=D)
    N, C = Y.shape[0], E.shape[1]
    E[5, 1] = 0.0                                                    # a zero of E in one clone: -inf for its one-hot start where the gene has a count
    ll = api._clone_loglik_host(Y, E, U, V)
    for c in range(C):
        r = evaluate(Y, E, U, V, np.eye(C)[[c] * N])
        assert np.array_equal(np.isneginf(r["mix_ll"]), np.isneginf(ll[:, c])) and not np.isnan(r["mix_ll"]).any()
        ok = np.isfinite(ll[:, c])
        assert np.abs(r["mix_ll"][ok] - ll[ok, c]).max() <= 1e-12 * np.abs(ll[ok, c]).max()
        assert np.array_equal(r["ll"], ll) and (r["rounds"] == 0).all()
    assert np.isneginf(ll[:, 1]).any()
    w = (0.3, 0.8)
    pr = api._clone_pair_loglik_host(Y, E, U, V, weights=w)
    for p, (a, b) in enumerate(pr["pairs"]):
        for k, wk in enumerate(w):
            st = np.zeros((N, C))
            st[:, a], st[:, b] = wk, 1.0 - wk
            r = evaluate(Y, E, U, V, st)
            ref = pr["pair_ll"][:, p, k]
            assert np.isfinite(ref).all()
            assert np.abs(r["mix_ll"] - ref).max() <= 1e-12 * np.abs(ref).max(), (a, b, wk)


def simplex_grid(C, steps):
    if C == 2:
        w = np.linspace(0.0, 1.0, steps + 1)
        return np.stack([w, 1.0 - w], axis=1)
    pts = [(i, j, steps - i - j) for i in range(steps + 1) for j in range(steps + 1 - i)]
    return np.asarray(pts, dtype=np.float64) / steps


@pytest.mark.parametrize("C,steps", [(2, 400), (3, 60)])
def test_no_point_of_a_fine_grid_beats_mix_ll_plus_bound(C, steps):
    Y, E, U, V, _PI = planted(N=24, G=60, C=C, reads=150, D=1, seed=C)
    N = Y.shape[0]
    grid = simplex_grid(C, steps)
    best = np.full(N, -np.inf)
    for pt in grid:
        best = np.maximum(best, evaluate(Y, E, U, V, np.broadcast_to(pt, (N, C)))["mix_ll"])
    for max_iter, tol in ((0, 0.0), (1, 0.0), (3, 0.0), (50, 1e-3)):   # the theorem holds at EVERY point, converged or not
        r = api._clone_mixture_host(Y, E, U, V, max_iter=max_iter, tol=tol)
        scale = np.abs(r["mix_ll"]) + 1.0
        assert (r["mix_ll"] + r["bound"] >= best - 1e-10 * scale).all(), (max_iter, float((best - r["mix_ll"] - r["bound"]).max()))
        assert (r["bound"] >= 0).all()
    assert r["converged"].all() and (best - r["mix_ll"] <= 1e-3 + 1e-10 * scale).all()


@pytest.mark.parametrize("C,reads,dup", [(2, 30, False), (4, 2000, False), (8, 100, True), (8, 3000, True), (20, 500, False)])
def test_bound_against_the_planted_truth_monotone_and_bookkeeping(C, reads, dup):
    Y, E, U, V, PI = planted(N=48, G=120, C=C, reads=reads, D=1, seed=C + reads, dup=dup)
    truth = evaluate(Y, E, U, V, PI)["mix_ll"]
    rng = np.random.default_rng(1)
    start = rng.dirichlet(np.ones(C), size=Y.shape[0])
    at_start = evaluate(Y, E, U, V, start)["mix_ll"]
    for max_iter, tol in ((2, 1e-3), (50, 1e-3), (50, 1e-9)):
        r = api._clone_mixture_host(Y, E, U, V, start=start, max_iter=max_iter, tol=tol)
        scale = np.abs(r["mix_ll"]) + 1.0
        assert not any(np.isnan(r[k]).any() for k in ("weights", "grad", "mix_ll", "bound"))
        assert (r["mix_ll"] + r["bound"] >= truth - 1e-10 * scale).all()
        assert (r["mix_ll"] >= at_start - 1e-10 * scale).all()
        assert (r["rounds"] <= max_iter).all() and (r["rounds"] >= 0).all()
        assert np.array_equal(r["converged"], r["bound"] <= tol)
        assert (r["weights"] >= 0).all() and np.abs(r["weights"].sum(1) - 1.0).max() <= 1e-12
        again = evaluate(Y, E, U, V, r["weights"])                   # the returned values are those of the returned weights
        assert np.abs(again["mix_ll"] - r["mix_ll"]).max() <= 1e-10 * scale.max() and np.allclose(again["bound"], r["bound"], rtol=0, atol=1e-8 * scale.max())
        if tol == 1e-3 and max_iter == 50:
            print(f"clone_mixture C={C} reads={reads} dup={dup}: converged {r['converged'].mean():.3f}, rounds median {int(np.median(r['rounds']))} max {int(r['rounds'].max())}")
            assert dup or r["converged"].all()                       # (duplicated clones make H singular: a cell may crawl by EM steps, with an honest bound)


def test_rounds_chain_bit_for_bit():
    Y, E, U, V, _PI = planted(N=40, G=100, C=5, reads=300, D=1, seed=3)
    T = 4
    one = api._clone_mixture_host(Y, E, U, V, max_iter=T, tol=0.0)
    w = None
    total = np.zeros(Y.shape[0], dtype=np.int64)
    for _ in range(T):
        r = api._clone_mixture_host(Y, E, U, V, start=w, max_iter=1, tol=0.0)
        w = r["weights"]
        total += r["rounds"]
    for k in ("weights", "grad", "mix_ll", "bound"):
        assert np.array_equal(one[k], r[k]), k
    assert np.array_equal(one["rounds"], total)


def test_a_zero_weight_revives():
    """Start on the wrong vertex of a planted pure row: EM could never leave it (0 * g = 0); a weight is free again as soon as its gamma_c > 0."""
    Y, E, U, V, PI = planted(N=36, G=200, C=4, reads=1000, D=1, seed=5)
    pure = np.flatnonzero((PI == 1.0).any(1))
    assert pure.size >= 4
    right = np.argmax(PI[pure], axis=1)
    start = np.eye(4)[(right + 1) % 4]
    r = api._clone_mixture_host(Y[pure], E, U[pure], V, start=start, max_iter=20, tol=1e-3)
    assert np.array_equal(np.argmax(r["weights"], axis=1), right)
    assert (r["weights"][np.arange(pure.size), right] > 0.9).all() and r["converged"].all()


def test_planted_recovery_at_the_issue_shape():
    Y, E, U, V, PI = planted()                                        # 240 x 300 x 4, 2000 reads, D = 1
    r = api._clone_mixture_host(Y, E, U, V, max_iter=50, tol=1e-3)
    err = float(np.abs(r["weights"] - PI).mean())
    uniform = float(np.abs(0.25 - PI).mean())
    print(f"clone_mixture planted recovery: mean |w - truth| {err:.4f} (uniform weights: {uniform:.4f}); rounds median {int(np.median(r['rounds']))} "
          f"max {int(r['rounds'].max())}")
    assert r["converged"].all() and (r["rounds"] <= 50).all()
    assert err < uniform
    lr = r["mix_ll"] - r["ll"].max(1)
    mixed = (PI > 0.2).sum(1) >= 2
    assert np.median(lr[mixed]) > 10.0 and (lr >= -1e-9 - r["bound"]).all()    # the simplex holds every vertex


def test_five_reads_and_fewer_non_zeros_than_clones_terminate_with_honest_flags():
    rng = np.random.default_rng(9)
    N, G, C = 60, 40, 5
    L = rng.integers(0, 3, size=(G, C)).astype(np.float64)          # L with zeros
    L[0] = 1.0
    E = rng.lognormal(0.0, 1.0, G)[:, None] * L
    P = E / E.sum(0)
    Y = np.stack([rng.multinomial(5, P @ rng.dirichlet(np.ones(C))) for _ in range(N)]).astype(np.float64)
    Y[3] = 0
    r = api._clone_mixture_host(Y, E, max_iter=100, tol=1e-3)
    assert ((Y > 0).sum(1) <= C).all() and ((Y > 0).sum(1) < C).sum() > N // 3      # H is singular in those cells
    for k in ("weights", "grad", "mix_ll", "bound"):
        assert not np.isnan(r[k]).any(), k
    assert (r["rounds"] <= 100).all() and np.array_equal(r["converged"], r["bound"] <= 1e-3)
    assert (r["weights"] >= 0).all() and np.abs(r["weights"].sum(1) - 1.0).max() <= 1e-12
    assert r["rounds"][3] == 0 and r["bound"][3] == 0 and np.array_equal(r["weights"][3], np.full(C, 0.2))
    best = np.full(N, -np.inf)                                        # the bound is honest where the cell did not converge, too
    for pt in rng.dirichlet(np.full(C, 0.3), size=400):
        best = np.maximum(best, api._clone_mixture_host(Y, E, start=np.broadcast_to(pt, (N, C)), max_iter=0, tol=0.0)["mix_ll"])
    fin = np.isfinite(r["mix_ll"])
    assert (r["mix_ll"] + r["bound"] >= best - 1e-9)[fin].all()


def test_unsupported_entries_zero_rows_and_the_uniform_restart():
    Y, E, U, V, _rng = small(N=30, G=50, C=3, D=0, seed=4)
    E[7] = 0.0                                                       # no clone has gene 7
    Y[:, 7] = 0
    Y[4, 7] = 2
    E[9, 0] = 0.0                                                    # clone 0 alone lacks gene 9
    Y[:, 9] = 0
    Y[6, 9] = 3
    r = api._clone_mixture_host(Y, E, max_iter=50, tol=1e-6)
    assert np.isneginf(r["mix_ll"][4]) and np.isfinite(np.delete(r["mix_ll"], 4)).all()
    Yd = Y.copy()
    Yd[4, 7] = 0
    rd = api._clone_mixture_host(Yd, E, max_iter=50, tol=1e-6)      # the weights and the bound are those of the remaining entries
    assert np.array_equal(r["weights"], rd["weights"]) and np.array_equal(r["bound"], rd["bound"])
    assert r["rounds"][0] == 0 and r["bound"][0] == 0 and r["mix_ll"][0] == 0.0   # s = 0: const_n = lgamma(1) - 0
    start = np.tile([1.0, 0.0, 0.0], (30, 1))                       # the start's zeros exclude cell 6's count on gene 9
    ev = api._clone_mixture_host(Y, E, start=start, max_iter=0, tol=0.0)
    assert np.isneginf(ev["mix_ll"][6]) and np.isposinf(ev["bound"][6]) and not np.isnan(ev["grad"]).any()
    op = api._clone_mixture_host(Y, E, start=start, max_iter=50, tol=1e-6)
    uni = api._clone_mixture_host(Y[6:7], E, max_iter=50, tol=1e-6)
    assert np.isfinite(op["mix_ll"][6]) and np.array_equal(op["weights"][6], uni["weights"][0]) and op["weights"][6, 0] < 1.0


def fit_for(E_mu, L):
    return {"ml_params": {"mu": E_mu}, "clone_names": [f"c{i}" for i in range(L.shape[1])]}


def test_api_extra_profiles_find_planted_ambient_and_prevalence():
    rng = np.random.default_rng(11)
    N, G, C = 40, 250, 3
    L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
    mu = rng.lognormal(0.0, 1.0, G)
    amb = rng.lognormal(0.0, 1.5, G)
    P = np.concatenate([mu[:, None] * L, amb[:, None]], axis=1)
    P /= P.sum(0)
    clone = rng.integers(0, C, N)
    PI = np.zeros((N, C + 1))
    PI[np.arange(N), clone] = 0.7
    PI[:, C] = 0.3                                                   # 30 % ambient in every droplet
    Y = np.stack([rng.multinomial(3000, P @ PI[n]) for n in range(N)])
    fit = fit_for(mu, L)
    eng = HostOnly(N, G)
    out = ca.deconvolve_clones(fit, Y, L, extra_profiles={"ambient": amb * 17.0}, saturate=False, engine=eng)   # (scale does not matter)
    assert out["component_names"] == ["c0", "c1", "c2", "ambient"] and out["weights"].shape == (N, C) and out["weights_extra"].shape == (N, 1)
    assert np.abs(out["weights_extra"][:, 0] - 0.3).max() < 0.08 and abs(out["prevalence"][C] - 0.3) < 0.02
    assert np.array_equal(out["dominant"], np.asarray([f"c{c}" for c in clone], dtype=object))
    assert (out["n_components"] == 2).all() and out["is_mixed"].all() and out["converged"].all()
    without = ca.clone_mixture(fit, Y, L, saturate=False, engine=eng)
    assert (out["mix_ll"] > without["mix_ll"] + 10.0).all()
    assert np.array_equal(without["log_lr_single"], without["mix_ll"] - without["ll"].max(1))
    ev = ca.mixture_loglik(fit, Y, L, out["weights_all"], extra_profiles={"ambient": amb}, saturate=False, engine=eng)
    assert (ev["rounds"] == 0).all() and np.abs(ev["mix_ll"] - out["mix_ll"]).max() <= 1e-9 * np.abs(out["mix_ll"]).max()
    bulk = ca.deconvolve_clones(fit, Y.sum(0, keepdims=True), L, extra_profiles=amb, saturate=False, engine=HostOnly(1, G))   # one row: bulk deconvolution
    want = np.append(np.bincount(clone, minlength=C) / N * 0.7, 0.3)
    assert bulk["component_names"][-1] == "extra_1" and np.abs(bulk["prevalence"] - want).max() < 0.03
    part = ca.clone_mixture(fit, Y, L, saturate=False, engine=eng, cells=(5, 9))
    assert np.array_equal(part["weights"], without["weights"][5:9])


def test_refusals_name_the_offender():
    Y, E, U, V, rng = small(N=20, G=30, C=3, D=1)
    N, C = 20, 3
    good = np.full((N, C), 1.0 / C)

    def refused(words, **kw):
        with pytest.raises(ValueError) as ex:
            api._clone_mixture_host(Y, E, U, V, **kw)
        assert all(w in str(ex.value) for w in words), str(ex.value)
    refused(("max_iter = -1", "negative"), max_iter=-1)
    for tol in (-1e-3, np.nan, np.inf):
        refused(("tol_nats",), tol=tol)
    bad = good.copy()
    bad[4, 1] = -0.1
    refused(("start has a negative or non-finite entry", "cell 4", "clone 1"), start=bad)
    bad[4, 1] = np.nan
    refused(("start has a negative or non-finite entry", "cell 4"), start=bad)
    bad = good.copy()
    bad[7] = (0.5, 0.5, 1e-8)
    refused(("the start of cell 7", "off 1 by more than 1e-9"), start=bad)
    refused(("start is",), start=good[:, :2])
    refused(("cell range",), cells=(5, N + 1))
    with pytest.raises(ValueError, match="at most 32"):
        api._clone_mixture_host(Y, np.ones((30, 33)))
    Eb = E.copy()
    Eb[3, 2] = -1.0
    with pytest.raises(ValueError, match="gene 3, clone 2"):
        api._clone_mixture_host(Y, Eb, U, V)
    L = np.ones((30, 3))
    fit = fit_for(np.ones(30), L)
    with pytest.raises(ValueError, match="extra_profiles is"):
        ca.clone_mixture(fit, Y, L, extra_profiles=np.ones((29, 1)), engine=HostOnly(N, 30))
    with pytest.raises(ValueError, match="profile ambient"):
        ca.clone_mixture(fit, Y, L, extra_profiles={"ambient": -np.ones(30)}, engine=HostOnly(N, 30))
    with pytest.raises(ValueError, match="at most 32"):
        ca.clone_mixture(fit, Y, L, extra_profiles=np.ones((30, 30)), engine=HostOnly(N, 30))
    with pytest.raises(ValueError, match="min_weight"):
        ca.deconvolve_clones(fit, Y, L, min_weight=1.5, engine=HostOnly(N, 30))

    class Holds3(HostOnly):
        C = 3

        def clone_mixture(self, *a, **k):
            raise AssertionError("not reached")
    with pytest.raises(ValueError, match="holds 3 columns.*4 components"):
        ca.clone_mixture(fit, Y, L, extra_profiles=np.ones(30), engine=Holds3(N, 30))
