"""ca_simulate_counts on the device against its numpy restatement (api._simulate_counts_host), and the public simulate_counts / predictive_fit_mse."""
import ctypes

import numpy as np
import pytest

from clonealign_amd import api, engine
from clonealign_amd.engine import EngineError

from tests import _simulate_cases as sc

pytestmark = pytest.mark.gpu

_REF = {}


def reference(name):
    """(Y, flagged) of the restatement for a case: computed once, shared, never changed."""
    if name not in _REF:
        E, V, U, clone, total, seed = sc.make(name)
        Y, flagged = api._simulate_counts_host(E, V, U, clone, total, seed)
        Y.setflags(write=False)
        _REF[name] = (Y, flagged)
    return _REF[name]


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_device_equals_the_restatement(name):
    """Exact equality in every cell the restatement does not flag; a flagged cell keeps its row sum and moves at most flagged[n] draws, each to an adjacent
    gene with non-zero weight.  At most 1 % of a case's cells may be flagged (tests/test_simulate_host.py shows the restatement flags none here)."""
    E, V, U, clone, total, seed = sc.make(name)
    ref, flagged = reference(name)
    dev = engine.simulate_counts(E, V, U, clone, total, seed)
    assert dev.dtype == np.int32 and dev.shape == ref.shape
    share = float((flagged > 0).mean())
    print(f"{name}: {share:.4%} of the cells flagged, {int((dev != ref).any(1).sum())} rows differ")
    assert share <= 0.01
    np.testing.assert_array_equal(dev.sum(1), total)
    clean = flagged == 0
    assert np.array_equal(dev[clean], ref[clean])
    for n in np.flatnonzero(~clean):
        diff = dev[n].astype(np.int64) - ref[n]
        assert np.abs(diff).sum() <= 2 * flagged[n]
        live = np.flatnonzero(E[:, clone[n]] > 0)                    # a moved draw goes to the neighbouring gene among those that can be drawn
        assert (diff[E[:, clone[n]] == 0] == 0).all() and np.abs(np.cumsum(diff[live])).max() <= flagged[n]


def test_two_calls_agree_and_splitting_the_cells_changes_nothing():
    E, V, U, clone, total, seed = sc.make("mixed")
    N = clone.shape[0]
    whole = engine.simulate_counts(E, V, U, clone, total, seed)
    assert np.array_equal(whole, engine.simulate_counts(E, V, U, clone, total, seed))
    for h in (1, 37, N - 1):
        a = engine.simulate_counts(E, V, U[:h], clone[:h], total[:h], seed)
        b = engine.simulate_counts(E, V, U[h:], clone[h:], total[h:], seed, cell_offset=h)
        assert np.array_equal(whole, np.concatenate([a, b])), h
    for kw in ({"draw": 1}, {"seed": seed + 1}):
        other = engine.simulate_counts(E, V, U, clone, total, kw.get("seed", seed), draw=kw.get("draw", 0))
        assert not np.array_equal(other, whole), kw
        np.testing.assert_array_equal(other.sum(1), total)


def test_refusals_name_the_argument_and_leave_the_output_alone():
    E, V, U, clone, total, seed = (np.array(a) if isinstance(a, np.ndarray) else a for a in sc.make("ragged")[:4] + sc.make("ragged")[4:])
    N, G, C = clone.shape[0], E.shape[0], E.shape[1]
    V, U = np.zeros((G, 1)), np.zeros((N, 1))

    def refused(match, E=E, V=V, U=U, clone=clone, total=total, **kw):
        out = np.full((N, G), -7, dtype=np.int32)
        with pytest.raises(EngineError, match=match):
            engine.simulate_counts(E, V, U, clone, total, seed, out=out, **kw)
        assert (out == -7).all(), match

    def poke(a, idx, v):
        b = np.array(a, dtype=np.float64 if a.dtype.kind == "f" else a.dtype)
        b[idx] = v
        return b

    refused(r"\bE has a negative", E=poke(E, (3, 1), -1.0))
    refused(r"\bE has a negative or non-finite", E=poke(E, (3, 1), np.inf))
    refused(r"\bE has a negative or non-finite", E=poke(E, (0, 0), np.nan))
    refused(r"\bU has a non-finite", U=poke(U, (5, 0), np.nan))
    refused(r"\bV has a non-finite", V=poke(V, (76, 0), -np.inf))
    refused(r"clone\[4\] = 2 is outside", clone=poke(clone, 4, C))
    refused(r"clone\[0\] = -1 is outside", clone=poke(clone, 0, -1))
    refused(r"total\[2\] = -1 is outside", total=poke(total, 2, -1))
    refused(r"total\[32\] = 2147483648 is outside", total=poke(total, 32, 2 ** 31))
    refused(r"total\[\d+\] = 3000 but E is zero in every gene of the cell's clone 1", E=np.column_stack([E[:, 0], np.zeros(G)]))
    refused(r"D = 9 is outside", V=np.zeros((G, 9)), U=np.zeros((N, 9)))
    refused(r"cell_offset", cell_offset=-1)
    refused(r"draw", draw=2 ** 48)
    # what the binding cannot express goes to the library directly: D < 0, D > 0 without U or V, N G >= 2^62
    lib, err = engine.load_library(), ctypes.create_string_buffer(256)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    Ec, cl, tt, out = np.ascontiguousarray(E), clone.astype(np.int32), total.astype(np.int64), np.full((N, G), -7, dtype=np.int32)
    for match, args in ((b"D = -1", (N, G, C, -1, ptr(Ec), None, None)), (b"needs both U", (N, G, C, 1, ptr(Ec), ptr(V), None)),
                        (b"needs both U", (N, G, C, 1, ptr(Ec), None, ptr(U))), (b"2^62", (2 ** 40, 2 ** 22, C, 0, ptr(Ec), None, None))):
        assert lib.ca_simulate_counts(*args, ptr(cl), ptr(tt), seed, 0, 0, 0, ptr(out), err) == 1          # CA_ERR_INVALID
        assert match in err.value and (out == -7).all(), err.value
    # total = 0 everywhere is no error, even for a clone that cannot be drawn from: rows of zeros
    out = engine.simulate_counts(np.column_stack([E[:, 0], np.zeros(G)]), None, None, clone, 0, seed, out=np.full((N, G), -7, dtype=np.int32))
    assert (out == 0).all()


def planted_fit(N, G, C, seed):
    rng = np.random.default_rng(seed)
    L = rng.integers(1, 5, (G, C)).astype(np.float64)
    alpha = np.array([0.5, 0.3, 0.2])[:C]
    z = rng.choice(C, N, p=alpha)
    names = [f"clone_{c}" for c in "abc"[:C]]
    ml = {"mu": rng.lognormal(0.0, 1.0, G), "W": rng.normal(size=(G, 1)) * 0.5, "psi": rng.normal(size=(N, 1)), "alpha": alpha}
    fit = {"ml_params": ml, "clone_names": names, "clone": np.asarray(names, dtype=object)[z]}
    return fit, L, z, rng.integers(2500, 3500, N)


def test_round_trip_through_the_public_api():
    """The device and the restatement through simulate_counts(); then assign_cells() on the simulated matrix must find the planted clones again more often
    than labelling every cell with the commonest clone would."""
    fit, L, z, total = planted_fit(1200, 400, 3, seed=21)
    kw = dict(clones=fit["clone"], total_counts=total, psi=fit["ml_params"]["psi"], seed=21)
    dev, ref = api.simulate_counts(fit, L, **kw), api.simulate_counts(fit, L, host=True, **kw)
    assert np.array_equal(dev["counts"], ref["counts"])
    np.testing.assert_array_equal(dev["clone_index"], z)
    np.testing.assert_array_equal(dev["counts"].sum(1), total)
    share = [float((api.assign_cells(fit, s["counts"], L, psi=s["psi"])["clone_probs"].argmax(1) == z).mean()) for s in (dev, ref)]
    print(f"planted clones recovered: {share[0]:.4f} (device matrix), {share[1]:.4f} (restatement's); the commonest clone holds {np.bincount(z).max() / z.size:.4f}")
    assert share[0] == share[1] and share[0] > np.bincount(z).max() / z.size
    # the defaults (clones from alpha, psi from its prior) run on the device too and are the restatement's
    a, b = api.simulate_counts(fit, L, n_cells=50, total_counts=500, seed=3), api.simulate_counts(fit, L, n_cells=50, total_counts=500, seed=3, host=True)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


def test_predictive_fit_mse_tells_a_right_fit_from_a_wrong_one():
    """Data simulated from the fit itself (draw 1000) sit inside the replicates' spread; with L's clone columns permuted the observed value lies above every
    replicate.  Measured on the device: z = 0.024 for the right fit (bar |z| < 4); z = 86.4 for the permuted one (observed 743.9, replicates 628.3 .. 631.9)."""
    fit, L, z, total = planted_fit(600, 200, 3, seed=33)
    Y = api.simulate_counts(fit, L, clones=fit["clone"], total_counts=total, psi=fit["ml_params"]["psi"], seed=33, draw=1000)["counts"]
    right = api.predictive_fit_mse(fit, Y, L, n_rep=8, seed=33)
    print(f"right fit: observed {right['observed']:.5f}, replicates {np.round(right['replicates'], 5)}, z = {right['z']:.3f}")
    assert right["replicates"].shape == (8,) and np.isfinite(right["replicates"]).all() and len(set(right["replicates"].tolist())) == 8
    assert abs(right["z"]) < 4.0
    for k in ("observed_gene", "replicate_gene_mean", "replicate_gene_sd"):
        assert right[k].shape == (200,) and np.isfinite(right[k]).all()
    assert abs(right["observed_gene"].mean() - right["observed"]) <= 1e-9 * right["observed"]
    wrong = api.predictive_fit_mse(fit, Y, L[:, [1, 2, 0]], n_rep=8, seed=33)
    print(f"permuted L: observed {wrong['observed']:.5f}, replicates {np.round(wrong['replicates'], 5)}, z = {wrong['z']:.3f}")
    assert wrong["observed"] > wrong["replicates"].max()
