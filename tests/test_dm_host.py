"""clone_loglik_dm / estimate_concentration / assign_cells_dm on the host: the float64 numpy / gammaln form (``api._clone_loglik_dm_host``) and the estimation
layer built on it, through an engine stub without ``clone_loglik_dm`` -- no GPU.  The model: the counts of a cell of clone c are Dirichlet-multinomial with
``alpha = phi p_n.c``, ``p`` the multinomial probabilities of ``clone_loglik``.

Bar of the formula checks: ``|dm - ref| <= 1e-12 * scale``, ``scale`` the sum of the magnitudes that went into the entry (``with_scale`` of the host form;
tests/test_gpu_dm_loglik.py holds the device to 1e-10 of the same scale).  Measured here: the host form against a direct
dense evaluation at most 2.6e-16 of that scale, the product form against the gamma form (two float64 formulations of the same number) 3.2e-16, a cell with
one read 1.5e-16 from ``clone_loglik``; the planted concentration 100 wins by 1.8e4 to 2.0e4 nats in seeds 0-4."""
import numpy as np
import pytest
from scipy.special import gammaln

import clonealign_amd as ca
from clonealign_amd import api
from tests.test_doublets_host import HostOnly, small

BAR = 1e-12
GRID = (10.0, 30.0, 100.0, 300.0, 1000.0, 1e4)


def direct_dm(y, p, phi, const=True):
    """DirichletMultinomial(total = sum y, alpha = phi p).log_prob(y) of one cell, dense over all genes (a gene with alpha = 0 and y = 0 adds nothing)."""
    al = phi * p
    if ((al == 0) & (y > 0)).any():
        return -np.inf
    ok = al > 0
    s = y.sum()
    r = (gammaln(phi) - gammaln(phi + s) if s > 0 else 0.0) + (gammaln(y[ok] + al[ok]) - gammaln(al[ok])).sum()
    return r + (gammaln(s + 1.0) - gammaln(y + 1.0).sum() if const else 0.0)


def planted(seed, phi=100.0, N=400, G=300, C=4, reads=2000):
    """Cells of a K = 0 model with L in 1..4: Dirichlet-multinomial rows at concentration ``phi`` (None: plain multinomial rows)."""
    rng = np.random.default_rng(seed)
    L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
    mu = rng.lognormal(0.0, 1.0, G)
    P = mu[:, None] * L
    P = P / P.sum(0)
    z = rng.integers(C, size=N)
    rows = [rng.multinomial(reads, P[:, c] if phi is None else rng.dirichlet(phi * P[:, c])) for c in z]
    names = [f"c{i}" for i in range(C)]
    fit = ca.ClonealignFit(ml_params={"mu": mu}, clone_names=names)
    return np.asarray(rows, dtype=np.int32), L, fit, np.asarray(names, dtype=object)[z]


@pytest.mark.parametrize("D", [0, 2])
@pytest.mark.parametrize("const", [True, False])
def test_formula_against_the_direct_dense_evaluation(D, const):
    Y, E, U, V, rng = small(D=D, seed=3)
    Y[5, :7] = np.arange(3, 10)                                      # counts on both sides of the device's product route
    phi = (0.5, 100.0, 1e5)
    r = api._clone_loglik_dm_host(Y, E, U, V, concentration=phi, const=const, chunk=25, with_scale=True)
    N, C = Y.shape[0], E.shape[1]
    assert r["dm_ll"].shape == (N, C, 3) and np.isfinite(r["dm_ll"]).all()
    assert np.array_equal(r["ll"], api._clone_loglik_host(Y, E, U, V, const=const))
    eta = np.zeros_like(Y) if D == 0 else U @ V.T
    worst = 0.0
    for n in range(N):
        P = E * np.exp(eta[n])[:, None]
        P = P / P.sum(0)
        for c in range(C):
            for k, f in enumerate(phi):
                worst = max(worst, abs(r["dm_ll"][n, c, k] - direct_dm(Y[n], P[:, c], f, const)) / r["scale"][n, c, k])
    print(f"dm host form against the direct dense evaluation D={D} const={const}: worst |diff| / scale {worst:.2e}")
    assert worst <= BAR
    const0 = api._clone_loglik_host(Y, E, U, V, const=const)[0, 0]   # the cell without counts: 0 + const_n (0 here: lgamma(1) - 0)
    assert np.array_equal(r["dm_ll"][0], np.full((C, 3), const0)) and const0 == 0.0
    # the same numbers whatever the chunking and the number of concentrations in a call
    one = api._clone_loglik_dm_host(Y, E, U, V, concentration=(100.0,), const=const)
    assert np.array_equal(one["dm_ll"][:, :, 0], r["dm_ll"][:, :, 1])


def test_product_form_and_gamma_form_agree():
    """lgamma(y + a) - lgamma(a) = log prod_{j < y} (a + j) for integer y: the device's route for small counts against the host's."""
    rng = np.random.default_rng(0)
    a = 10.0 ** rng.uniform(-6, 5, size=4000)
    y = rng.integers(1, 9, size=4000).astype(np.float64)
    prod = np.ones_like(a)
    for j in range(8):
        prod *= np.where(j < y, a + j, 1.0)
    gam = gammaln(y + a) - gammaln(a)
    scale = np.abs(gammaln(y + a)) + np.abs(gammaln(a)) + 1.0
    worst = float((np.abs(np.log(prod) - gam) / scale).max())
    print(f"product form against gamma form: worst |diff| / scale {worst:.2e}")
    assert worst <= BAR


@pytest.mark.parametrize("D", [0, 2])
def test_cells_with_one_read_are_multinomial_at_every_concentration(D):
    Y, E, U, V, rng = small(D=D, seed=4)
    Y[:] = 0
    Y[np.arange(Y.shape[0]), rng.integers(Y.shape[1], size=Y.shape[0])] = 1
    phi = (0.1, 10.0, 1e3, 1e6)
    r = api._clone_loglik_dm_host(Y, E, U, V, concentration=phi, with_scale=True)
    worst = float((np.abs(r["dm_ll"] - r["ll"][:, :, None]) / r["scale"]).max())
    print(f"dm, one read per cell, D={D}: worst |dm - ll| / scale {worst:.2e}")
    assert worst <= BAR


def test_a_large_concentration_gives_the_multinomial_posterior():
    Y, L, fit, _truth = planted(0, phi=None, N=120)
    host = HostOnly(*Y.shape)
    r = ca.clone_loglik_dm(fit, Y, L, concentration=[1e12], engine=host)
    assert np.array_equal(r["concentration"], [1e12])
    pm = ca.assign_cells(fit, Y, L, engine=host)["clone_probs"]
    pd = ca.assign_cells_dm(fit, Y, L, concentration=1e12, engine=host)
    assert float(np.abs(pd["clone_probs"] - pm).max()) <= 1e-6
    assert np.array_equal(pd["multinomial_clone_probs"], pm) and pd["n_calls_changed"] == 0


def test_minus_infinity_exactly_where_a_positive_count_meets_zero_expression():
    Y, E, U, V, _rng = small(C=3, seed=2)
    E[5, :] = 0.0
    Y[:, 5] = 0                                                      # a zero count against zeros in every clone: adds nothing
    E[7, 0] = 0.0
    E[9, 0] = E[9, 1] = 0.0
    Y[:, 7] = 0
    Y[:, 9] = 0
    Y[11, 7] = 2                                                     # clone 0 alone
    Y[12, 9] = 1                                                     # clones 0 and 1
    r = api._clone_loglik_dm_host(Y, E, U, V, concentration=(3.0, 300.0))
    want = np.zeros(r["dm_ll"].shape, dtype=bool)
    want[11, 0] = want[12, 0] = want[12, 1] = True
    assert not np.isnan(r["dm_ll"]).any() and np.array_equal(np.isneginf(r["dm_ll"]), want)
    assert np.array_equal(np.isneginf(r["ll"]), want[:, :, 0])


@pytest.mark.parametrize("seed", range(5))
def test_planted_overdispersion_is_recovered(seed):
    Y, L, fit, _truth = planted(seed)
    est = ca.estimate_concentration(fit, Y, L, grid=GRID, refine=0, engine=HostOnly(*Y.shape))
    M = est["marginal_loglik"]
    gap = np.sort(M)[-1] - np.sort(M)[-2]
    print(f"planted concentration 100, seed {seed}: picked {est['concentration']:g}, gap to the runner-up {gap:.3e} nats, "
          f"multinomial {est['multinomial_marginal_loglik'] - M.max():.3e} below")
    assert est["concentration"] == 100.0 and not est["at_edge"]
    assert np.array_equal(est["grid"], GRID) and M.shape == (6,) and est["n_cells_used"] == Y.shape[0]
    assert est["multinomial_marginal_loglik"] < M.max()


def test_multinomial_data_sit_at_the_upper_edge():
    Y, L, fit, _truth = planted(0, phi=None)
    est = ca.estimate_concentration(fit, Y, L, grid=GRID, refine=2, engine=HostOnly(*Y.shape))
    assert est["at_edge"] and est["concentration"] == 1e4 and est["grid"].shape == (6,)          # no refinement at an edge


def test_refinement_visits_eight_values_per_round_between_the_neighbours():
    Y, L, fit, _truth = planted(1, N=150)
    host = HostOnly(*Y.shape)
    coarse = ca.estimate_concentration(fit, Y, L, refine=0, engine=host)
    assert np.allclose(coarse["grid"], 10.0 ** np.arange(1.0, 4.75, 0.5)) and coarse["grid"].shape == (8,)
    fine = ca.estimate_concentration(fit, Y, L, refine=2, engine=host)
    assert fine["grid"].shape == (24,) and (np.diff(fine["grid"]) > 0).all()
    i = int(np.argmax(coarse["marginal_loglik"]))
    new = np.setdiff1d(fine["grid"], coarse["grid"])
    assert new.size == 16 and new.min() > coarse["grid"][i - 1] and new.max() < coarse["grid"][i + 1]
    assert fine["marginal_loglik"].max() >= coarse["marginal_loglik"].max()
    assert fine["concentration"] == fine["grid"][np.argmax(fine["marginal_loglik"])]
    assert 30.0 < fine["concentration"] < 300.0


def test_assign_cells_dm_keys_and_calibration():
    Y, L, fit, truth = planted(2)
    host = HostOnly(*Y.shape)
    plain = ca.assign_cells(fit, Y, L, engine=host)
    fixed = ca.assign_cells_dm(fit, Y, L, concentration=100.0, engine=host)
    new = {"concentration", "multinomial_clone_loglik", "multinomial_clone_probs", "multinomial_clone", "n_calls_changed", "n_newly_unassigned"}
    assert set(fixed) == set(plain) | new and fixed["concentration"] == 100.0     # a given value: no estimate is made
    assert np.array_equal(fixed["multinomial_clone"], plain["clone"]) and np.array_equal(fixed["multinomial_clone_loglik"], plain["clone_loglik"])
    assert fixed["n_calls_changed"] == int((fixed["clone"] != plain["clone"]).sum())
    assert fixed["n_newly_unassigned"] == int(((fixed["clone"] == "unassigned") & (plain["clone"] != "unassigned")).sum())
    np.testing.assert_allclose(fixed["clone_probs"].sum(1), 1.0, rtol=1e-12)
    assert np.array_equal(ca.recompute_clone_assignment(fixed, 0.95)["clone"], fixed["clone"])
    auto = ca.assign_cells_dm(fit, Y, L, concentration="auto", grid=GRID, refine=0, engine=host)
    assert set(auto) == set(fixed) | {"concentration_estimate"} and auto["concentration"] == 100.0
    assert np.array_equal(auto["clone_probs"], fixed["clone_probs"]) and np.array_equal(auto["clone"], fixed["clone"])
    wrong_dm = int(((fixed["clone"] != truth) & (fixed["clone"] != "unassigned")).sum())
    wrong_mn = int(((plain["clone"] != truth) & (plain["clone"] != "unassigned")).sum())
    print(f"planted concentration 100: wrong calls above 0.95: multinomial {wrong_mn}, Dirichlet-multinomial {wrong_dm}; "
          f"newly unassigned {fixed['n_newly_unassigned']}")
    assert wrong_dm <= wrong_mn
    ex = np.zeros((Y.shape[0], 4))
    ex[:, 1] = 50.0
    pushed = ca.assign_cells_dm(fit, Y, L, concentration=100.0, extra_loglik=ex, engine=host)
    assert (pushed["clone_probs"][:, 1] >= fixed["clone_probs"][:, 1]).all()
    with pytest.raises(ValueError, match="auto"):
        ca.assign_cells_dm(fit, Y, L, concentration="best", engine=host)


def test_refusals_name_the_offender():
    Y, L, fit, _truth = planted(0, N=20)
    host = HostOnly(*Y.shape)
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="concentration 1 is"):
            ca.clone_loglik_dm(fit, Y, L, concentration=[10.0, bad], engine=host)
        with pytest.raises(ValueError, match="concentration 0 is"):
            ca.assign_cells_dm(fit, Y, L, concentration=bad, engine=host)
        with pytest.raises(ValueError, match="concentration 1 is"):
            ca.estimate_concentration(fit, Y, L, grid=[10.0, bad], engine=host)
    with pytest.raises(ValueError, match=r"n_conc = 17 is outside \[1, 16\]"):
        ca.clone_loglik_dm(fit, Y, L, concentration=np.linspace(1, 17, 17), engine=host)
    with pytest.raises(ValueError, match=r"n_conc = 0"):
        ca.clone_loglik_dm(fit, Y, L, concentration=[], engine=host)
    with pytest.raises(ValueError, match="extra_loglik"):
        ca.estimate_concentration(fit, Y, L, grid=GRID, extra_loglik=np.zeros((3, 3)), engine=host)
    with pytest.raises(ValueError, match="genes"):
        ca.clone_loglik_dm(fit, Y[:, :-1], L, concentration=[10.0], engine=host)
