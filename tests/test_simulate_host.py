"""The numpy restatement of ca_simulate_counts (api._simulate_counts_host) and the public simulate_counts(host=True): no GPU."""
import numpy as np
import pytest

from clonealign_amd import api
from clonealign_amd.rng import philox4x32

from tests import _simulate_cases as sc


def scalar_sampler(E, clone, total, seed, draw, cell_offset):
    """D = 0, a dozen lines of scalar Python: one Philox call per draw, an explicit loop over the draws, a linear scan for the gene."""
    N, G = len(clone), E.shape[0]
    Y = np.zeros((N, G), dtype=np.int64)
    for n in range(N):
        cum = [float(sum(E[:g + 1, clone[n]])) for g in range(G)]
        for j in range(int(total[n])):
            q = cell_offset + n
            r = philox4x32(np.array([j >> 1, q & 0xFFFFFFFF, draw & 0xFFFFFFFF, ((draw >> 32) & 0xFFFF) | ((q >> 32) << 16)], dtype=np.uint32),
                           (seed & 0xFFFFFFFF, seed >> 32))
            lo, hi = (int(r[0]), int(r[1])) if j % 2 == 0 else (int(r[2]), int(r[3]))
            t = (((hi << 21) | (lo >> 11)) + 0.5) * 2.0 ** -53 * cum[-1]
            Y[n, next(g for g in range(G) if cum[g] > t)] += 1
    return Y


def test_known_answer_against_scalar_python():
    E = np.array([[1.0, 0.5], [2.0, 0.0], [0.0, 3.0], [4.0, 1.5]])   # 4 genes x 2 clones
    clone, total = np.array([0, 1, 0]), np.array([0, 1, 5])
    for seed, draw, off in ((7, 0, 0), (2 ** 40 + 3, 2 ** 33 + 1, 2 ** 32 + 5)):
        Y, flagged = api._simulate_counts_host(E, None, None, clone, total, seed, draw, off)
        assert Y.dtype == np.int32 and Y.shape == (3, 4)
        np.testing.assert_array_equal(Y, scalar_sampler(E, clone, total, seed, draw, off))
        assert flagged.sum() == 0


def test_row_sums_and_structural_zeros():
    E, V, U, clone, total, seed = sc.make("mixed")
    Y, _ = reference("mixed")
    np.testing.assert_array_equal(Y.sum(1), total)
    assert (Y[E[:, clone].T == 0] == 0).all() and (E == 0).any()
    assert Y[0].sum() == 0 and Y[2].sum() == 200_000


def test_distribution_of_the_pooled_counts():
    """2 000 cells of one clone with one U, 5 000 draws each, 50 genes, D = 1: the pooled counts against total * p.  Deterministic (the draws' seed is 7;
    seeds 5 .. 8 all pass).  Measured: max |z| = 2.55 (bar 5), sum z^2 = 49.35 (bar: within 49.5 of 49)."""
    rng = np.random.default_rng(5)
    N, G, tot = 2000, 50, 5000
    E = rng.lognormal(0.0, 1.0, (G, 2))
    V = rng.normal(size=(G, 1)) * 0.5
    U = np.full((N, 1), 0.7)
    Y, _ = api._simulate_counts_host(E, V, U, np.ones(N, dtype=np.int32), tot, seed=7)
    w = E[:, 1] * np.exp(0.7 * V[:, 0])
    p = w / w.sum()
    exp = N * tot * p
    z = (Y.sum(0) - exp) / np.sqrt(exp * (1.0 - p))
    print(f"max |z| = {np.abs(z).max():.3f}, sum z^2 = {(z ** 2).sum():.2f}")
    assert np.abs(z).max() < 5.0
    assert abs((z ** 2).sum() - (G - 1)) < 5.0 * np.sqrt(2.0 * (G - 1))


_REF = {}


def reference(name):
    if name not in _REF:
        E, V, U, clone, total, seed = sc.make(name)
        _REF[name] = api._simulate_counts_host(E, V, U, clone, total, seed)
    return _REF[name]


def pairwise_cumsum(w):
    """Cumulative sums grouped the way a blocked scan groups them: within blocks of 64, plus the cumulative block totals."""
    G = w.shape[0]
    b = np.zeros(-(-G // 64) * 64)
    b[:G] = w
    b = b.reshape(-1, 64)
    inner = np.cumsum(b, axis=1)
    before = np.concatenate([[0.0], np.cumsum(inner[:, -1])[:-1]])
    return np.maximum.accumulate((inner + before[:, None]).reshape(-1)[:G])


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_no_draw_of_the_parity_cases_depends_on_the_grouping_of_the_sums(name):
    """The one freedom the device has: for these inputs and seeds the restatement gives the same matrix under another grouping, and flags no draw."""
    E, V, U, clone, total, seed = sc.make(name)
    Y, flagged = reference(name)
    Yp, flagged_p = api._simulate_counts_host(E, V, U, clone, total, seed, _cumsum=pairwise_cumsum)
    assert flagged.sum() == 0 and flagged_p.sum() == 0
    np.testing.assert_array_equal(Y, Yp)
    np.testing.assert_array_equal(Y.sum(1), total)


def small_fit(K=1):
    rng = np.random.default_rng(3)
    G, C = 30, 3
    L = rng.integers(1, 5, (G, C)).astype(np.float64)
    ml = {"mu": rng.lognormal(0.0, 1.0, G), "alpha": np.array([0.5, 0.3, 0.2])}
    if K:
        ml["W"] = rng.normal(size=(G, K)) * 0.5
    return {"ml_params": ml, "clone_names": ["A", "B", "C"]}, L


def test_api_defaults_are_reproducible_from_the_seed():
    fit, L = small_fit()
    a = api.simulate_counts(fit, L, n_cells=40, total_counts=200, seed=9, host=True)
    b = api.simulate_counts(fit, L, n_cells=40, total_counts=200, seed=9, host=True)
    c = api.simulate_counts(fit, L, n_cells=40, total_counts=200, seed=10, host=True)
    assert set(a) == {"counts", "clone", "clone_index", "psi", "total_counts"}
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    assert a["counts"].shape == (40, 30) and a["counts"].dtype == np.int32 and a["psi"].shape == (40, 1)
    np.testing.assert_array_equal(a["counts"].sum(1), 200)
    assert not np.array_equal(a["counts"], c["counts"]) and not np.array_equal(a["psi"], c["psi"])
    assert set(a["clone"]) <= {"A", "B", "C"} and len(set(a["clone"])) > 1
    d = api.simulate_counts(fit, L, n_cells=40, total_counts=200, seed=9, draw=1, host=True)      # another replicate of the same cells
    np.testing.assert_array_equal(d["clone_index"], a["clone_index"])
    np.testing.assert_array_equal(d["psi"], a["psi"])
    assert not np.array_equal(d["counts"], a["counts"])
    import clonealign_amd
    assert clonealign_amd.simulate_counts is api.simulate_counts and clonealign_amd.predictive_fit_mse is api.predictive_fit_mse


def test_api_takes_clones_by_name_and_by_index_and_totals_as_scalar_or_array():
    fit, L = small_fit()
    idx = np.array([0, 2, 1, 1, 0, 2])
    psi = np.linspace(-1, 1, 6).reshape(6, 1)
    tot = np.array([10, 0, 300, 7, 55, 1])
    by_idx = api.simulate_counts(fit, L, clones=idx, total_counts=tot, psi=psi, seed=4, host=True)
    by_name = api.simulate_counts(fit, L, clones=np.array(["A", "C", "B", "B", "A", "C"], dtype=object), total_counts=tot, psi=psi, seed=4, host=True)
    np.testing.assert_array_equal(by_idx["counts"], by_name["counts"])
    np.testing.assert_array_equal(by_idx["counts"].sum(1), tot)
    assert list(by_idx["clone"]) == ["A", "C", "B", "B", "A", "C"] and by_idx["psi"] is not psi
    np.testing.assert_array_equal(by_idx["psi"], psi)
    scalar = api.simulate_counts(fit, L, clones=idx, total_counts=25, psi=psi, seed=4, host=True)
    np.testing.assert_array_equal(scalar["total_counts"], np.full(6, 25))
    np.testing.assert_array_equal(scalar["counts"].sum(1), 25)
    # the tables are clone_loglik's: E = mu * saturate(L), V = W, U = psi
    from clonealign_amd import hostprep
    E = fit["ml_params"]["mu"][:, None] * hostprep.saturate(L, 6)
    ref, _ = api._simulate_counts_host(E, fit["ml_params"]["W"], psi, idx, tot, 4)
    np.testing.assert_array_equal(by_idx["counts"], ref)
    fit0, L0 = small_fit(K=0)
    out = api.simulate_counts(fit0, L0, clones=idx, total_counts=tot, seed=4, host=True)
    assert out["psi"].shape == (6, 0)
    np.testing.assert_array_equal(out["counts"].sum(1), tot)


def test_api_refusals():
    fit, L = small_fit()
    with pytest.raises(ValueError, match="unassigned"):
        api.simulate_counts(fit, L, clones=np.array(["A", "unassigned", "B"], dtype=object), total_counts=10, host=True)
    with pytest.raises(ValueError, match="no column of L"):
        api.simulate_counts(fit, L, clones=np.array(["A", "Z"], dtype=object), total_counts=10, host=True)
    with pytest.raises(ValueError, match="rows"):
        api.simulate_counts(fit, L[:-1], n_cells=4, total_counts=10, host=True)              # L has a gene fewer than the fit
    with pytest.raises(ValueError, match="clone names"):
        api.simulate_counts(fit, L[:, :2], n_cells=4, total_counts=10, host=True)
    with pytest.raises(ValueError, match="total_counts is required"):
        api.simulate_counts(fit, L, n_cells=4, host=True)
    with pytest.raises(ValueError, match="number of cells"):
        api.simulate_counts(fit, L, total_counts=10, host=True)
    with pytest.raises(ValueError, match="disagree"):
        api.simulate_counts(fit, L, clones=[0, 1], total_counts=[1, 2, 3], host=True)
    with pytest.raises(ValueError, match="x is required"):
        api.simulate_counts(fit, L, n_cells=4, total_counts=10, x=np.zeros((4, 1)), host=True)
    with pytest.raises(ValueError, match="outside"):
        api._simulate_counts_host(np.ones((3, 2)), None, None, [0, 2], 5, 1)
    with pytest.raises(ValueError, match="zero in every gene"):
        api._simulate_counts_host(np.array([[1.0, 0.0], [2.0, 0.0]]), None, None, [0, 1], 5, 1)
