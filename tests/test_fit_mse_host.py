"""compute_ca_fit_mse (R/clonealign.R:415-434): the host form, the argument checks and the exported names.  No GPU needed."""
import numpy as np
import pytest

from clonealign_amd import api, engine


# 2 cells x 3 genes x 2 clones, worked by hand:
#   cell 0 -> clone 0: rowSums = 6, colSums(L[, 0]) = 6,  a = 1:    predicted (1, 2, 3) - y (2, 1, 3)  = (-1, 1, 0)  -> 2
#   cell 1 -> clone 1: rowSums = 4, colSums(L[, 1]) = 8,  a = 0.5:  predicted (1, 2, 1) - y (0, 4, 0)  = (1, -2, 1)  -> 6
#   mse = (2 + 6) / (2 * 3) = 4 / 3;  per gene: (1 + 1, 1 + 4, 0 + 1) / 2 = (1, 2.5, 0.5)
Y_HAND = np.array([[2.0, 1.0, 3.0], [0.0, 4.0, 0.0]])
L_HAND = np.array([[1.0, 2.0], [2.0, 4.0], [3.0, 2.0]])


def hand_fit(clone=("A", "B")):
    return {"clone": np.array(clone, dtype=object), "clone_names": ["A", "B"], "ml_params": {"mu": np.array([1.0, 2.0, 0.5])}}


class HostOnlyEngine:
    """A live engine without fit_mse: compute_ca_fit_mse must take the host form."""
    N, G = 2, 3


def test_host_form_matches_the_case_worked_by_hand():
    out = api._fit_mse_host(Y_HAND, L_HAND, [0, 1], per_gene=True)
    assert out["n_cells"] == 2
    assert out["sse"] == pytest.approx(8.0, rel=1e-15)
    assert out["mse"] == pytest.approx(4.0 / 3.0, rel=1e-15)
    np.testing.assert_allclose(out["sse_gene"], [2.0, 5.0, 1.0], rtol=1e-15)
    # a skipped cell leaves the other cell's terms, and the mean is over the used cells
    out = api._fit_mse_host(Y_HAND, L_HAND, [-1, 1], per_gene=True)
    assert (out["n_cells"], out["sse"]) == (1, pytest.approx(6.0, rel=1e-15))
    assert out["mse"] == pytest.approx(2.0, rel=1e-15)
    # model_mu: E = mu * L = [[1, 2], [4, 8], [1.5, 1]]; cell 0: a = 6 / 6.5, cell 1: a = 4 / 11
    E = np.array([1.0, 2.0, 0.5])[:, None] * L_HAND
    want = ((6 / 6.5 * E[:, 0] - Y_HAND[0]) ** 2).sum() + ((4 / 11 * E[:, 1] - Y_HAND[1]) ** 2).sum()
    assert api._fit_mse_host(Y_HAND, E, [0, 1])["sse"] == pytest.approx(want, rel=1e-14)


def test_host_form_takes_a_sparse_matrix_in_chunks():
    import scipy.sparse as sps
    rng = np.random.default_rng(3)
    Y = rng.poisson(0.7, size=(57, 13)).astype(np.float64)
    L = rng.integers(1, 5, size=(13, 3)).astype(np.float64)
    idx = rng.integers(-1, 3, size=57)
    a = api._fit_mse_host(Y, L, idx, per_gene=True)
    b = api._fit_mse_host(sps.csr_matrix(Y), L, idx, per_gene=True, chunk=10)
    assert b["n_cells"] == a["n_cells"]
    np.testing.assert_allclose(b["sse_gene"], a["sse_gene"], rtol=1e-13)


def test_compute_ca_fit_mse_on_an_engine_without_the_device_pass():
    eng = HostOnlyEngine()
    assert api.compute_ca_fit_mse(hand_fit(), Y_HAND, L_HAND, engine=eng) == pytest.approx(4.0 / 3.0, rel=1e-15)
    mse, per_gene = api.compute_ca_fit_mse(hand_fit(), Y_HAND, L_HAND, per_gene=True, engine=eng)
    assert mse == pytest.approx(4.0 / 3.0, rel=1e-15)
    np.testing.assert_allclose(per_gene, [1.0, 2.5, 0.5], rtol=1e-15)
    import clonealign_amd
    assert clonealign_amd.compute_ca_fit_mse is api.compute_ca_fit_mse


def test_unassigned_cells_raise_unless_dropped():
    fit = hand_fit(("unassigned", "B"))
    with pytest.raises(ValueError, match="unassigned"):
        api.compute_ca_fit_mse(fit, Y_HAND, L_HAND, engine=HostOnlyEngine())
    assert api.compute_ca_fit_mse(fit, Y_HAND, L_HAND, drop_unassigned=True, engine=HostOnlyEngine()) == pytest.approx(2.0, rel=1e-15)


def test_model_mu_length_mismatch_names_both_lengths():
    fit = hand_fit()
    fit["ml_params"]["mu"] = np.ones(5)
    with pytest.raises(ValueError, match=r"5.*3"):
        api.compute_ca_fit_mse(fit, Y_HAND, L_HAND, model_mu=True, engine=HostOnlyEngine())


def test_shape_and_label_mismatches_raise():
    with pytest.raises(ValueError, match="genes"):
        api.compute_ca_fit_mse(hand_fit(), Y_HAND, L_HAND[:2], engine=HostOnlyEngine())
    with pytest.raises(ValueError, match="cells"):
        api.compute_ca_fit_mse(hand_fit(("A", "B", "A")), Y_HAND, L_HAND, engine=HostOnlyEngine())
    with pytest.raises(ValueError, match="no column of L"):
        api.compute_ca_fit_mse(hand_fit(("A", "Z")), Y_HAND, L_HAND, engine=HostOnlyEngine())


def test_random_clones_are_reproducible_and_draw_only_labels_present(monkeypatch):
    rng = np.random.default_rng(0)
    N, G = 400, 6
    Y = rng.poisson(3.0, size=(N, G)).astype(np.float64)
    L = rng.integers(1, 5, size=(G, 4)).astype(np.float64)
    fit = {"clone": np.array(["c1", "c3"] * (N // 2), dtype=object), "clone_names": ["c0", "c1", "c2", "c3"], "ml_params": {"mu": np.ones(G)}}
    seen = []
    real = api._fit_mse_host
    monkeypatch.setattr(api, "_fit_mse_host", lambda Y_, E_, idx, **kw: (seen.append(np.array(idx)), real(Y_, E_, idx, **kw))[1])

    class Eng:
        pass
    eng = Eng()
    eng.N, eng.G = N, G
    a = api.compute_ca_fit_mse(fit, Y, L, random_clones=True, seed=7, engine=eng)
    b = api.compute_ca_fit_mse(fit, Y, L, random_clones=True, seed=7, engine=eng)
    c = api.compute_ca_fit_mse(fit, Y, L, random_clones=True, seed=8, engine=eng)
    assert a == b and np.array_equal(seen[0], seen[1])
    assert not np.array_equal(seen[0], seen[2]) and a != c
    for idx in seen:
        assert set(np.unique(idx)) == {1, 3}          # only the labels present in fit["clone"], both of them at this size
        assert idx.shape == (N,)
    assert not np.array_equal(seen[0], np.tile([1, 3], N // 2))


def test_new_entry_points_are_exported():
    assert "ca_fit_mse" in engine.EXPORTS and "ca_group_fit_mse" in engine.EXPORTS
    assert callable(engine.HipEngine.fit_mse) and engine.HipGroupEngine.fit_mse is engine.HipEngine.fit_mse
