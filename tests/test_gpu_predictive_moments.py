"""ca_predictive_moments on the device: the moments of ca_predictive_stats's replicates in closed form.  Two oracles: a float64 numpy restatement written
here (``numpy_moments``; bars: 1e-10 of the terms' magnitudes) and verified code -- the replicates themselves, engine.predictive_stats and
engine.simulate_counts, whose sample moments must lie within their own standard errors of the closed forms."""
import ctypes

import numpy as np
import pytest

from clonealign_amd import api, engine
from clonealign_amd.engine import HipEngine

from tests import _simulate_cases as sc

pytestmark = pytest.mark.gpu
RTOL = 1e-10


def numpy_moments(E, V, U, clone, total):
    """((cell_mean, cell_var, T_mean, T_var, T_cum3), (scale of cell_mean [N], of cell_var [N], of the three tables [G, C])), float64 on whole arrays:
    p = w / sum w with w = E exp(eta - m), lp = log E + eta - m - log sum w (log1p(-(1 - p)) where p > 1/2, as include/clonealign_hip.h states); the scales are total sum_g p |lp|, total sum_g p lp^2 and sum_n total p."""
    E, clone, total = np.asarray(E, dtype=np.float64), np.asarray(clone), np.asarray(total, dtype=np.float64)
    N, (G, C) = clone.shape[0], E.shape
    e = E[:, clone].T
    pos = e > 0
    eta = np.zeros(e.shape) if U is None else U @ V.T
    live = total > 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m = np.where(pos, eta, -np.inf).max(1, keepdims=True)
        x = np.where(pos, eta - m, 0.0)
        w = np.where(pos, e * np.exp(x), 0.0)
        is_top = np.arange(G)[None, :] == w.argmax(1)[:, None]       # the largest w joins the sum last: what is left of 1 - p is then a sum of its own
        others = np.where(is_top, 0.0, w).sum(1, keepdims=True)
        Z = others + w.max(1, keepdims=True)
        p = np.where(live[:, None], w / Z, 0.0)
        lp = np.where(pos & live[:, None], np.log(np.where(pos, e, 1.0)) + x - np.log(Z), 0.0)
        lp = np.where(is_top & (w / Z > 0.5), np.log1p(-others / Z), lp)   # a gene with p > 1/2: log E + x - log Z cancels, log1p(-(the others' share)) does not
    h = (p * lp).sum(1, keepdims=True)
    t = total[:, None]
    tp = t * p
    T, sT = np.zeros((3, G, C)), np.zeros((G, C))
    for k, term in enumerate((tp, tp * (1 - p), tp * (1 - p) * (1 - 2 * p))):
        np.add.at(T[k].T, clone, term)
    np.add.at(sT.T, clone, tp)
    return (total * h[:, 0], total * (p * (lp - h) ** 2).sum(1), T[0], T[1], T[2]), (total * (p * np.abs(lp)).sum(1), total * (p * lp * lp).sum(1), sT)


def exact_zero_cases():
    """(name, arguments, check(result, name)) for the values that must be exactly 0; shared with tests/test_predictive_moments_host.py."""
    rng = np.random.default_rng(11)
    N, G, C = 40, 70, 4
    E = rng.lognormal(0.0, 1.0, (G, 1)) * rng.integers(1, 5, (G, C)).astype(np.float64)
    E[rng.random((G, C)) < 0.2] = 0.0
    E[:, 2] = 0.0
    E[5, 2] = 3.0                                                    # clone 2 has one positive gene
    clone = rng.integers(0, 3, N).astype(np.int32)                   # clone 3 has no cells
    clone[:4] = (2, 0, 2, 1)
    total = rng.integers(1, 500, N).astype(np.int64)
    total[1] = 0

    def check(res, what):
        mean, var, Tm, Tv, Tc = res
        one = clone == 2
        assert np.isfinite(np.concatenate([np.ravel(a) for a in res])).all(), what
        assert mean[1] == 0.0 and var[1] == 0.0, what                                           # total = 0
        assert (Tm[:, 3] == 0.0).all() and (Tv[:, 3] == 0.0).all() and (Tc[:, 3] == 0.0).all(), what   # an absent clone
        assert (Tm[E == 0] == 0.0).all() and (Tv[E == 0] == 0.0).all() and (Tc[E == 0] == 0.0).all(), what
        assert (var[one] == 0.0).all() and (mean[one] == 0.0).all() and (Tv[:, 2] == 0.0).all() and (Tc[:, 2] == 0.0).all(), what
        assert Tm[5, 2] == total[one].sum() and (var[~one & (total > 0)] > 0.0).all() and (Tv[:, :2][E[:, :2] > 0] > 0).all(), what

    out = []
    for D in (0, 1, 3):
        V, U = (rng.normal(size=(G, D)) * 0.5, rng.normal(size=(N, D))) if D else (None, None)
        out.append((f"D = {D}", (E, V, U, clone, total), check))
    return out


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_parity_with_the_numpy_restatement(name):
    """Every case of _simulate_cases.CASES: ragged tiles, copy number 0 with totals 0 / 1 / 200 000 (`mixed`), twenty clones and a gene past a power of
    two, 20 000 and 6000 genes (the row of w in the block's global slab / in LDS), three genes, |eta| = 700 (`steep`).  Bars: cell_mean 1e-10 total
    sum_g p |lp|, cell_var 1e-10 total sum_g p lp^2, the three tables 1e-10 sum_n total p.
    Largest ratios measured on an MI355X: cell_mean 4.9e-16 (`mixed`), cell_var 3.4e-16 (`steep`; the other cases below 2.2e-17), the tables 1.2e-15
    (`large_g`) and 1.1e-13 at `steep`.  (`steep` with lp = log E + x - log Z for every gene: cell_mean 2.4e-7 -- the case behind the log1p rule.)"""
    E, V, U, clone, total, _seed = sc.make(name)
    got = engine.predictive_moments(E, V, U, clone, total)
    want, scale = numpy_moments(E, V, U, clone, total)
    N = clone.shape[0]
    assert [a.shape for a in got] == [(N,), (N,), E.shape, E.shape, E.shape] and all(a.dtype == np.float64 for a in got)
    worst = []
    for k in range(5):
        s = scale[min(k, 2)]
        assert np.isfinite(got[k]).all(), (name, k)
        worst.append(float((np.abs(got[k] - want[k]) / np.where(s > 0, s, 1.0)).max()))
    print(f"{name}: largest |device - numpy| / scale: cell_mean {worst[0]:.2e}, cell_var {worst[1]:.2e}, T_mean {worst[2]:.2e}, T_var {worst[3]:.2e}, T_cum3 {worst[4]:.2e}")
    for k in range(5):
        assert (np.abs(got[k] - want[k]) <= RTOL * scale[min(k, 2)]).all(), (name, k, worst[k])
    assert (got[0][total == 0] == 0.0).all() and (got[1][total == 0] == 0.0).all()
    assert engine.predictive_moments_kernel_ms() > 0.0 or U is None


def test_monte_carlo_cross_check_against_the_replicates():
    """400 replicates of a 60 x 120 x 3 problem with two factors, drawn by verified code: T_rep from engine.predictive_stats, the per-cell statistic from
    the rows of engine.simulate_counts.  For every entry with positive variance: |mean_rep - T_mean| <= 6 sqrt(T_var / n_rep); |S^2 / T_var - 1| <= 6
    sqrt(2 / (n_rep - 1) + 1 / (n_rep T_var)) (the second term: the Poisson-like excess kurtosis); |mean of the statistic - cell_mean| <= 6 sqrt(cell_var
    / n_rep); its sample variance over cell_var within 1 +- 6 sqrt(2 / (n_rep - 1)).  The host sampler against the formulas gave 3.54, 3.07 and 2.98
    standard errors and a ratio in [0.818, 1.171]; the device's replicates against the device's closed forms, on an MI355X, give the same four figures."""
    rng = np.random.default_rng(2024)
    N, G, C, D = 60, 120, 3, 2
    E = rng.lognormal(0, 1, (G, 1)) * rng.integers(1, 5, (G, C))
    V = 0.5 * rng.normal(size=(G, D))
    U = rng.normal(size=(N, D))
    clone = rng.integers(0, C, N).astype(np.int32)
    total = rng.integers(200, 2001, N).astype(np.int64)
    seed, n_rep = 2024, 400
    mean, var, Tm, Tv, _Tc = engine.predictive_moments(E, V, U, clone, total)
    _ll, T_rep = engine.predictive_stats(E, V, U, clone, total, seed, draw0=0, n_rep=n_rep)
    e = E[:, clone].T
    eta = U @ V.T
    logp = np.log(e) + eta - np.log((e * np.exp(eta)).sum(1, keepdims=True))
    stat = np.stack([(engine.simulate_counts(E, V, U, clone, total, seed, draw=r) * logp).sum(1) for r in range(n_rep)], axis=1)      # [N, n_rep]
    pos = Tv > 0
    assert pos.all() and (var > 0).all()
    a = np.abs(T_rep.mean(0) - Tm) / np.sqrt(Tv / n_rep)
    b = np.abs(T_rep.var(0, ddof=1) / Tv - 1.0) / np.sqrt(2.0 / (n_rep - 1) + 1.0 / (n_rep * Tv))
    c = np.abs(stat.mean(1) - mean) / np.sqrt(var / n_rep)
    ratio = stat.var(1, ddof=1) / var
    print(f"worst standard errors: T mean {a.max():.2f}, T variance {b.max():.2f}, statistic mean {c.max():.2f}; variance ratio in [{ratio.min():.3f}, {ratio.max():.3f}]")
    assert (a <= 6.0).all() and (b <= 6.0).all() and (c <= 6.0).all()
    assert (np.abs(ratio - 1.0) <= 6.0 * np.sqrt(2.0 / (n_rep - 1))).all()


def test_determinism_and_splits():
    """`mixed`, split at 137: two calls agree bit for bit; the cell values of [0, 137) and [137, N) in two calls are the one call's bits; the two calls'
    tables add up to the one call's within 1e-12 T_mean."""
    E, V, U, clone, total, _seed = sc.make("mixed")
    h = 137
    one, again = engine.predictive_moments(E, V, U, clone, total), engine.predictive_moments(E, V, U, clone, total)
    for a, b in zip(one, again):
        assert np.array_equal(a, b)
    lo, hi = engine.predictive_moments(E, V, U[:h], clone[:h], total[:h]), engine.predictive_moments(E, V, U[h:], clone[h:], total[h:])
    for k in range(2):
        assert np.array_equal(np.concatenate([lo[k], hi[k]]), one[k]), k
    for k in range(2, 5):
        assert (np.abs(lo[k] + hi[k] - one[k]) <= 1e-12 * one[2]).all(), k
    single = engine.predictive_moments(E, V, U[7:8], clone[7:8], total[7:8])
    assert single[0][0] == one[0][7] and single[1][0] == one[1][7]


def test_batches_of_cells_change_no_bit():
    """Without many genes a batch holds 64 MB / (8 D + 56) = 1 048 576 cells at D = 1; 1 048 600 cells go as two batches.  All but 30 cells at the ends and
    around the cut have total 0 (exactly 0, listed in no strip).  The 30 cells alone give bit for bit the same cell values and, being few, tables within
    1e-12 T_mean."""
    rng = np.random.default_rng(8)
    G, C = 9, 2
    cut = (64 << 20) // (8 + 56)
    N = cut + 24
    E = rng.lognormal(0.0, 1.0, (G, 1)) * rng.integers(1, 5, (G, C)).astype(np.float64)
    V = rng.normal(size=(G, 1)) * 0.5
    U = rng.normal(size=(N, 1))
    clone = rng.integers(0, C, N).astype(np.int32)
    total = np.zeros(N, dtype=np.int64)
    cells = np.r_[0:6, cut - 6:cut + 6, N - 12:N]
    total[cells] = rng.integers(1, 300, cells.size)
    one = engine.predictive_moments(E, V, U, clone, total)
    few = engine.predictive_moments(E, V, U[cells], clone[cells], total[cells])
    assert (one[0][total == 0] == 0.0).all() and (one[1][total == 0] == 0.0).all()
    for k in range(2):
        assert np.array_equal(one[k][cells], few[k]) and (few[1] > 0).all(), k
    for k in range(2, 5):
        assert (np.abs(one[k] - few[k]) <= 1e-12 * one[2]).all(), k


def test_exact_zeros_on_the_device():
    for what, args, check in exact_zero_cases():
        check(engine.predictive_moments(*args), what)


def test_refusals_name_the_argument_and_leave_the_outputs_alone():
    E, _V, _U, clone, total, _seed = sc.make("ragged")
    N, G, C = clone.shape[0], E.shape[0], E.shape[1]
    V, U = np.zeros((G, 1)), np.zeros((N, 1))
    lib, err = engine.load_library(), ctypes.create_string_buffer(256)
    ptr = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def poke(a, idx, v):
        b = np.array(a, dtype=np.float64 if a.dtype.kind == "f" else a.dtype)
        b[idx] = v
        return b

    def refused(match, E=E, V=V, U=U, clone=clone, total=total, D=1, null=None):
        outs = [np.full(N, -7.0), np.full(N, -7.0), np.full((G, C), -7.0), np.full((G, C), -7.0), np.full((G, C), -7.0)]
        keep = [np.ascontiguousarray(a) if a is not None else None for a in (E, V, U, clone.astype(np.int32), total.astype(np.int64))]
        args = [None if i == null else ptr(o) for i, o in enumerate(outs)]
        rc = lib.ca_predictive_moments(N, G, C, D, *(ptr(a) for a in keep), 0, *args, err)
        assert rc == 1, match                                                                   # CA_ERR_INVALID
        assert err.value.startswith(b"ca_predictive_moments: ") and match in err.value, err.value
        assert all((o == -7.0).all() for o in outs), match
        assert engine.predictive_moments_kernel_ms() == 0.0

    refused(b"E has a negative", E=poke(E, (3, 1), -1.0))
    refused(b"U has a non-finite", U=poke(U, (5, 0), np.nan))
    refused(b"V has a non-finite", V=poke(V, (76, 0), np.nan))
    refused(b"clone[4] = 2 is outside", clone=poke(clone, 4, C))
    refused(b"total[2] = -1 is outside", total=poke(total, 2, -1))
    refused(b"but E is zero in every gene of the cell's clone 1", E=np.column_stack([E[:, 0], np.zeros(G)]))
    refused(b"D = 9 is outside", V=np.zeros((G, 9)), U=np.zeros((N, 9)), D=9)
    refused(b"needs both U", U=None)
    for i, name in enumerate((b"cell_mean", b"cell_var", b"T_mean", b"T_var", b"T_cum3")):
        refused(name + b" must not be NULL", null=i)
    with pytest.raises(engine.EngineError, match=r"ca_predictive_moments: E has a negative"):
        engine.predictive_moments(poke(E, (3, 1), -1.0), V, U, clone, total)
    # no cells: zeros in the tables, and total = 0 everywhere is no error even for a clone that cannot be drawn from
    empty = engine.predictive_moments(E, V, U[:0], clone[:0], total[:0])
    assert empty[0].shape == (0,) and all((a == 0.0).all() for a in empty[2:])
    zero = engine.predictive_moments(np.column_stack([E[:, 0], np.zeros(G)]), V, U, clone, 0)
    assert all((a == 0.0).all() for a in zero)


def planted(N=200, G=300, C=3, n_bad=20, total=2000, seed=77):
    """The recipe of tests/test_gpu_predictive.py: E as tests/_simulate_cases.py makes it, V ~ 0.5 N(0, 1), U ~ N(0, 1); cells 0 .. n_bad - 1 are drawn
    from their own p with the genes permuted, the others from the model.  Returned as a hand-made fit: mu and L with E = mu * L."""
    rng = np.random.default_rng(seed)
    mu = rng.lognormal(0.0, 1.0, G)
    L = rng.integers(1, 5, (G, C)).astype(np.float64)
    W, psi = rng.normal(size=(G, 1)) * 0.5, rng.normal(size=(N, 1))
    z = rng.integers(0, C, N)
    names = [f"clone_{c}" for c in "abc"[:C]]
    w = (mu[:, None] * L)[:, z].T * np.exp(psi @ W.T)
    Y = np.stack([rng.multinomial(total, w[n] / w[n].sum()) for n in range(N)]).astype(np.int32)
    for n in range(n_bad):
        Y[n] = Y[n][rng.permutation(G)]
    fit = {"ml_params": {"mu": mu, "W": W, "psi": psi}, "clone_names": names, "clone": np.asarray(names, dtype=object)[z]}
    return fit, Y, L, z


def test_python_on_the_device():
    """The planted case of tests/test_gpu_predictive.py (200 x 300 x 3; cells 0-19 have their genes permuted), dense and CSR: host=False equals host=True
    within the parity bars; the planted cells have z_cell < -20 and every other cell z_cell > -8, that file's criterion; stat_observed is
    clone_loglik(const=False)'s bits; dosage_response on the device's moments gives the host path's kappa within 1e-9.
    Measured on an MI355X: planted z_cell -73.1 .. -38.4, in-model z_cell -2.50 .. 2.48."""
    import scipy.sparse as sp
    fit, Y, L, z = planted()
    host = api.predictive_moments(fit, Y, L, host=True)
    E, V, U = fit["ml_params"]["mu"][:, None] * L, fit["ml_params"]["W"], fit["ml_params"]["psi"]
    _want, scale = numpy_moments(E, V, U, z, Y.sum(1))
    eng = HipEngine(Y, L, np.zeros((200, 0)), None, 0)
    try:
        scorer = eng.clone_loglik(E, U, V, const=False)[np.arange(200), z]
    finally:
        eng.close()
    for Yd in (Y, sp.csr_matrix(Y)):
        dev = api.predictive_moments(fit, Yd, L)
        assert np.array_equal(dev["cells"], np.arange(200)) and np.array_equal(dev["T_observed"], host["T_observed"])
        assert np.array_equal(dev["stat_observed"], scorer)
        for k, s in (("stat_mean", scale[0]), ("stat_var", scale[1]), ("T_mean", scale[2]), ("T_var", scale[2]), ("T_cum3", scale[2])):
            assert (np.abs(dev[k] - host[k]) <= RTOL * s).all(), k
        zc = dev["z_cell"]
        print(f"planted z_cell {zc[:20].min():.1f} .. {zc[:20].max():.1f}; in-model z_cell {zc[20:].min():.2f} .. {zc[20:].max():.2f}")
        assert (zc[:20] < -20.0).all() and (zc[20:] > -8.0).all()
        assert np.isfinite(dev["z_gene_clone"]).all() and ((dev["p_gene_clone"] >= 0) & (dev["p_gene_clone"] <= 1)).all()
        a, b = api.dosage_response(fit, Yd, L, moments=dev), api.dosage_response(fit, Y, L, moments=host)
        assert np.array_equal(np.isnan(a["kappa"]), np.isnan(b["kappa"])) and np.nanmax(np.abs(a["kappa"] - b["kappa"])) <= 1e-9
