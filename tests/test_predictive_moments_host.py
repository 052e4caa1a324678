"""The numpy restatement of ca_predictive_moments (api._predictive_moments_host) against full enumeration of small multinomials and against an independent
float64 statement (``numpy_moments`` of tests/test_gpu_predictive_moments.py, the one the device is held to); refined_normal_cdf against the exact
distribution of a sum of binomials; dosage_response on closed forms and on a planted case through the host path.  No GPU."""
import itertools
import math

import numpy as np
import pytest
from scipy.special import ndtr
from scipy.stats import binom

from clonealign_amd import api, engine

from tests import _simulate_cases as sc
from tests.test_gpu_predictive_moments import RTOL, exact_zero_cases, numpy_moments


def test_exports():
    assert {"ca_predictive_moments", "ca_predictive_moments_kernel_ms"} <= set(engine.EXPORTS)


def test_enumeration_of_a_tiny_multinomial():
    """G = 3, C = 2, D = 1, totals (4, 3, 5), clones (0, 1, 1): every outcome of each cell's multinomial is enumerated.  cell_mean and cell_var are the
    mean and variance of sum_g y_g log p_g; the totals of clone 1 are the sum of two independent cells, whose cumulants add.  Bar 1e-12; measured: 9e-15
    or better."""
    rng = np.random.default_rng(3)
    E = rng.lognormal(0.0, 1.0, (3, 1)) * rng.integers(1, 5, (3, 2)).astype(np.float64)
    V, U = rng.normal(size=(3, 1)) * 0.5, rng.normal(size=(3, 1))
    clone, total = np.array([0, 1, 1]), np.array([4, 3, 5])
    got = api._predictive_moments_host(E, V, U, clone, total)
    mean, var, k1, k2, k3 = np.zeros(3), np.zeros(3), np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 3))
    for n in range(3):
        w = E[:, clone[n]] * np.exp(U[n, 0] * V[:, 0])
        p = w / w.sum()
        outcomes, prob = [], []
        for y in itertools.product(range(total[n] + 1), repeat=3):
            if sum(y) == total[n]:
                outcomes.append(y)
                prob.append(math.factorial(total[n]) / np.prod([math.factorial(v) for v in y]) * np.prod(p ** np.array(y)))
        y, prob = np.array(outcomes, dtype=np.float64), np.array(prob)
        assert abs(prob.sum() - 1.0) < 1e-13
        stat = y @ np.log(p)
        mean[n] = prob @ stat
        var[n] = prob @ (stat - mean[n]) ** 2
        k1[n] = prob @ y
        k2[n] = prob @ (y - k1[n]) ** 2
        k3[n] = prob @ (y - k1[n]) ** 3
    worst = max(np.abs(got[0] - mean).max(), np.abs(got[1] - var).max())
    for c, cells in ((0, [0]), (1, [1, 2])):
        for k, want in enumerate((k1, k2, k3)):
            worst = max(worst, np.abs(got[2 + k][:, c] - want[cells].sum(0)).max())
    print(f"largest difference from the enumeration: {worst:.1e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_restatement_agrees_with_the_independent_statement(name):
    """api._predictive_moments_host (chunked, eta factor by factor) against numpy_moments (whole arrays, eta by a matrix product) under the device's bars."""
    E, V, U, clone, total, _seed = sc.make(name)
    got = api._predictive_moments_host(E, V, U, clone, total, chunk=7)
    want, scale = numpy_moments(E, V, U, clone, total)
    for k in range(5):
        assert np.isfinite(got[k]).all()
        assert (np.abs(got[k] - want[k]) <= RTOL * scale[min(k, 2)]).all(), (name, k)


def test_exact_zeros():
    for what, args, check in exact_zero_cases():
        check(api._predictive_moments_host(*args), what)


def test_refusals_are_the_device_calls():
    E, _V, _U, clone, total, _seed = sc.make("ragged")
    with pytest.raises(ValueError, match=r"predictive_moments: E has a negative"):
        api._predictive_moments_host(-E, None, None, clone, total)
    with pytest.raises(ValueError, match=r"predictive_moments: clone\[0\] = 2 is outside"):
        api._predictive_moments_host(E, None, None, np.full(clone.shape, 2), total)
    with pytest.raises(ValueError, match=r"total\[\d+\] = 3000 but E is zero in every gene"):
        api._predictive_moments_host(np.column_stack([E[:, 0], np.zeros(E.shape[0])]), None, None, clone, total)


def test_refined_normal_cdf_without_skewness_is_the_normal():
    rng = np.random.default_rng(1)
    t, mean, var = rng.integers(0, 50, 200).astype(np.float64), rng.uniform(0, 50, 200), rng.uniform(0.1, 30, 200)
    assert np.abs(api.refined_normal_cdf(t, mean, var, 0.0) - ndtr((t + 0.5 - mean) / np.sqrt(var))).max() <= 1e-15


def test_refined_normal_cdf_is_clipped():
    t = np.arange(-5.0, 12.0)
    for cum3 in (-40.0, 40.0):
        F = api.refined_normal_cdf(t, 2.0, 1.5, cum3)
        assert (F >= 0.0).all() and (F <= 1.0).all() and (F == 0.0).any() and (F == 1.0).any()
    assert np.array_equal(api.refined_normal_cdf(np.array([1.0, 2.0, 3.0]), 2.0, 0.0, 0.0), [0.0, 1.0, 1.0])      # a point mass at the mean


def test_refined_normal_cdf_against_the_exact_distribution():
    """Sums of 40 binomials(s_i, p_i) at five levels of p: the largest |F - exact CDF| over all t is at most 0.05 / variance.  Measured: variance 1.53,
    4.70, 46.4, 411, 7055 with errors 9.4e-3, 6.0e-3, 4.8e-4, 5.0e-5, 1.4e-6 -- all within 0.028 / variance; the plain normal approximation misses the bar
    4 to 20 times over."""
    rng = np.random.default_rng(7)
    for level in (3e-5, 1e-4, 1e-3, 1e-2, 0.2):
        s = rng.integers(200, 2001, 40)
        p = level * rng.lognormal(0, 0.5, 40)
        pmf = np.ones(1)
        for si, pi in zip(s, p):
            pmf = np.convolve(pmf, binom.pmf(np.arange(si + 1), si, pi))
        mean, var, cum3 = (s * p).sum(), (s * p * (1 - p)).sum(), (s * p * (1 - p) * (1 - 2 * p)).sum()
        t = np.arange(pmf.shape[0], dtype=np.float64)
        err = np.abs(api.refined_normal_cdf(t, mean, var, cum3) - np.cumsum(pmf)).max()
        plain = np.abs(ndtr((t + 0.5 - mean) / np.sqrt(var)) - np.cumsum(pmf)).max()
        print(f"level {level:g}: variance {var:.3g}, max |F - exact| {err:.2e} ({err * var:.3f} / variance); plain normal {plain:.2e}")
        assert err <= 0.05 / var, (level, var, err)


def moments_of(T, X, L, cells=None):
    """A hand-made result of predictive_moments holding what dosage_response reads."""
    T, X, L = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (T, X, L))
    return {"T_observed": T, "exposure": X, "L": L, "clone_cells": np.ones(T.shape[1], dtype=np.int64) if cells is None else np.asarray(cells)}


def test_dosage_response_closed_forms():
    # two clones: kappa = log((T1 / X1) / (T0 / X0)) / (l1 - l0)
    out = api.dosage_response(None, None, None, moments=moments_of([40, 300], [5, 9], [1, 3]))
    want = math.log((300 / 9) / (40 / 5)) / math.log(3.0)
    assert abs(want - 1.2990172878643969) < 1e-15 and abs(out["kappa"][0] - want) <= 1e-12
    assert out["converged"][0] and not out["at_bound"][0] and out["n_clones_used"][0] == 2 and out["df"][0] == 0 and out["total_count"][0] == 340
    assert out["pearson"][0] <= 1e-12 and out["lrt_proportional"][0] >= 0 and out["lrt_insensitive"][0] > out["lrt_proportional"][0]
    assert 0 < out["p_insensitive"][0] < out["p_proportional"][0] <= 1 and np.isfinite(out["se"][0])
    # the same copy number in every used clone, no counts, a clone without cells that held the only other copy number: not identifiable
    out = api.dosage_response(None, None, None, moments=moments_of([[40, 300, 7], [0, 0, 0]], [[5, 9, 2], [5, 9, 2]], [[2, 2, 2], [1, 2, 3]]))
    assert np.isnan(out["kappa"]).all() and np.isnan(out["lrt_proportional"]).all() and np.array_equal(out["n_clones_used"], [3, 3]) and not out["converged"].any()
    out = api.dosage_response(None, None, None, moments=moments_of([40, 300, 0], [5, 9, 0], [2, 2, 3], cells=[4, 4, 0]))
    assert np.isnan(out["kappa"][0]) and out["n_clones_used"][0] == 2
    # copy number 0 and E = 0 (exposure NaN) leave a clone out
    out = api.dosage_response(None, None, None, moments=moments_of([40, 300, 0], [5, 9, np.nan], [1, 3, 0]))
    assert abs(out["kappa"][0] - want) <= 1e-12 and out["n_clones_used"][0] == 2
    # every count in the clone of largest copy number: the bound
    for kmax in (8.0, 3.0):
        out = api.dosage_response(None, None, None, moments=moments_of([0, 0, 50], [5, 9, 4], [1, 2, 4]), kappa_max=kmax)
        assert out["at_bound"][0] and out["kappa"][0] == kmax and out["lrt_proportional"][0] >= 0
    out = api.dosage_response(None, None, None, moments=moments_of([50, 0, 0], [5, 9, 4], [1, 2, 4]))
    assert out["at_bound"][0] and out["kappa"][0] == -8.0


def planted_dosage(seed=5):
    """300 cells, 150 genes, 4 clones, copy numbers 1..4, K = 1, totals 2000; the counts are drawn by the host sampler from E' = mu L^kappa_g with kappa_g
    = 0 for the first 30 genes and 1 for the rest; the "fit" is the planting's own parameters."""
    rng = np.random.default_rng(seed)
    N, G, C = 300, 150, 4
    mu = rng.lognormal(0.0, 1.0, G)
    L = rng.integers(1, 5, (G, C)).astype(np.float64)
    W, psi = rng.normal(size=(G, 1)) * 0.5, rng.normal(size=(N, 1))
    z = rng.integers(0, C, N)
    kappa = np.r_[np.zeros(30), np.ones(G - 30)]
    Y, _flagged = api._simulate_counts_host(mu[:, None] * L ** kappa[:, None], W, psi, z, 2000, seed)
    names = [f"clone_{c}" for c in "abcd"]
    fit = {"ml_params": {"mu": mu, "W": W, "psi": psi}, "clone_names": names, "clone": np.asarray(names, dtype=object)[z]}
    return fit, Y, L, kappa


def test_dosage_response_recovers_a_planted_compensation():
    fit, Y, L, kappa = planted_dosage()
    mom = api.predictive_moments(fit, Y, L, host=True)
    out = api.dosage_response(fit, Y, L, host=True)
    again = api.dosage_response(fit, Y, L, moments=mom)
    for k in out:
        assert np.array_equal(out[k], again[k], equal_nan=True), k
    ok = np.isfinite(out["kappa"])
    assert ok.sum() >= 140 and out["converged"][ok].all()
    dev = np.abs(out["kappa"] - kappa)[ok] / out["se"][ok]
    comp, prop = out["lrt_proportional"][:30][ok[:30]], out["lrt_proportional"][30:][ok[30:]]
    print(f"largest |kappa_hat - kappa| / se = {dev.max():.2f}; median lrt_proportional of the compensated genes {np.median(comp):.1f}, "
          f"95th percentile of the others {np.percentile(prop, 95):.1f}")
    assert (dev <= 5.0).all()
    assert np.median(comp) > np.percentile(prop, 95)
    assert (out["lrt_proportional"][ok] >= 0).all() and (out["lrt_insensitive"][ok] >= 0).all()
    assert np.array_equal(out["df"], out["n_clones_used"] - 2)


def test_predictive_moments_host_path():
    """The public call on the planted case: shapes, the observed side, and the z's definition."""
    fit, Y, L, _kappa = planted_dosage()
    fit = dict(fit, clone=fit["clone"].copy())
    fit["clone"][:3] = "unassigned"
    out = api.predictive_moments(fit, Y, L, host=True)
    assert np.array_equal(out["cells"], np.arange(3, 300)) and out["z_cell"].shape == (297,) and out["z_gene_clone"].shape == (150, 4)
    z = np.array([list(fit["clone_names"]).index(c) for c in fit["clone"][3:]])
    assert np.array_equal(out["T_observed"], np.stack([Y[3:][z == c].sum(0) for c in range(4)], axis=1))
    assert np.array_equal(out["clone_cells"], np.bincount(z, minlength=4))
    E = fit["ml_params"]["mu"][:, None] * L
    want, _scale = numpy_moments(E, fit["ml_params"]["W"], fit["ml_params"]["psi"][3:], z, Y[3:].sum(1))
    assert np.allclose(out["stat_mean"], want[0], rtol=1e-12) and np.allclose(out["T_var"], want[3], rtol=1e-12)
    assert np.allclose(out["z_cell"], (out["stat_observed"] - out["stat_mean"]) / np.sqrt(out["stat_var"]))
    assert np.allclose(out["exposure"] * E, out["T_mean"]) and ((out["p_gene_clone"] >= 0) & (out["p_gene_clone"] <= 1)).all()
    with pytest.raises(ValueError, match="unassigned"):
        api.predictive_moments(dict(fit, clone=np.full(300, "unassigned", dtype=object)), Y, L, host=True)
