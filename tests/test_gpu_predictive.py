"""ca_predictive_stats on the device: replicate rows drawn as ca_simulate_counts draws them and reduced where they are.  The oracle is verified code:
the rows of engine.simulate_counts at draw = draw0 + r with float64 numpy on top (``numpy_ll``).  Bar on ll, the one of tests/test_gpu_clone_loglik.py:
``|ll_rep - numpy| <= 1e-10 * (lgamma(total + 1) + sum_g lgamma(y + 1) + sum_g |y log p|)``; T_rep, an integer sum, is exact."""
import ctypes

import numpy as np
import pytest
from scipy.special import gammaln

from clonealign_amd import api, engine
from clonealign_amd.engine import EngineError, HipEngine

from tests import _simulate_cases as sc

pytestmark = pytest.mark.gpu
RTOL = 1e-10
DRAW0 = 5


def numpy_ll(E, V, U, clone, total, Y):
    """(ll [N], scale [N]) of the rows Y under each cell's own p, float64: log p = log E + eta - m - log sum E exp(eta - m)."""
    e = E[:, clone].T
    pos = e > 0
    eta = np.zeros(e.shape) if U is None else U @ V.T
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m = np.where(pos, eta, -np.inf).max(1, keepdims=True)
        x = np.where(pos, eta - m, 0.0)
        logp = np.where(pos, np.log(np.where(pos, e, 1.0)) + x, 0.0) - np.log(np.where(pos, e * np.exp(x), 0.0).sum(1, keepdims=True))
    y = Y.astype(np.float64)
    assert not (y[~pos] > 0).any()                                   # a gene with w = 0 is never drawn
    t = np.where(y > 0, y * np.where(y > 0, logp, 0.0), 0.0)
    lg_s, lg_y = gammaln(total + 1.0), gammaln(y + 1.0).sum(1)
    return np.where(total > 0, lg_s - lg_y + t.sum(1), 0.0), lg_s + lg_y + np.abs(t).sum(1)


def clone_sums(Y, clone, C):
    return np.stack([Y[clone == c].sum(0, dtype=np.int64) for c in range(C)], axis=1)          # [G, C]


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_parity_with_the_simulated_rows(name):
    """Every case of _simulate_cases.CASES at n_rep = 3 (large_g: 2), draw0 = 5: T_rep[r] equals the per-clone column sums of the simulated rows exactly,
    ll_rep the numpy value within the bar.  `mixed` has totals 0, 1, 2 and 200 000 and copy number 0, `steep` the shift, `two_level` and `large_g` the
    two-level table with the counters in LDS and in global memory.
    Largest |ll_rep - numpy| / scale measured on an MI355X: 3.3e-16 (mixed and pow2_plus_1; the other cases 1.1e-16 .. 2.4e-16); bar 1e-10."""
    E, V, U, clone, total, seed = sc.make(name)
    n_rep = 2 if name == "large_g" else 3
    ll, T = engine.predictive_stats(E, V, U, clone, total, seed, draw0=DRAW0, n_rep=n_rep)
    assert ll.shape == (clone.shape[0], n_rep) and ll.dtype == np.float64 and T.shape == (n_rep,) + E.shape and T.dtype == np.int64
    worst = 0.0
    for r in range(n_rep):
        Y = engine.simulate_counts(E, V, U, clone, total, seed, draw=DRAW0 + r)
        assert np.array_equal(T[r], clone_sums(Y, clone, E.shape[1])), (name, r)
        want, scale = numpy_ll(E, V, U, clone, total, Y)
        assert np.isfinite(ll[:, r]).all()
        assert (ll[total == 0, r] == 0.0).all()
        ratio = np.abs(ll[:, r] - want) / np.where(scale > 0, scale, 1.0)
        worst = max(worst, float(ratio.max()))
        assert (np.abs(ll[:, r] - want) <= RTOL * scale).all(), (name, r, float(ratio.max()))
    print(f"{name}: largest |ll_rep - numpy| / scale = {worst:.2e}")


def test_replicate_values_are_the_scorers():
    """One replicate (`mixed`, r = 1) uploaded as an engine's Y: clone_loglik(const=True) at each cell's clone agrees with ll_rep[:, 1] under the same bar,
    which is what makes observed and replicate values comparable.  Largest difference / scale measured on an MI355X: 4.2e-16."""
    E, V, U, clone, total, seed = sc.make("mixed")
    N, G = clone.shape[0], E.shape[0]
    ll, _T = engine.predictive_stats(E, V, U, clone, total, seed, draw0=DRAW0, n_rep=2, gene_totals=False)
    assert _T is None
    Y = engine.simulate_counts(E, V, U, clone, total, seed, draw=DRAW0 + 1)
    eng = HipEngine(Y, np.ones(E.shape), np.zeros((N, 0)), np.zeros(G), 0)
    try:
        scorer = eng.clone_loglik(E, U, V, const=True)[np.arange(N), clone]
    finally:
        eng.close()
    _want, scale = numpy_ll(E, V, U, clone, total, Y)
    ratio = np.abs(ll[:, 1] - scorer) / np.where(scale > 0, scale, 1.0)
    print(f"ll_rep against clone_loglik: largest difference / scale = {float(ratio.max()):.2e}")
    assert (np.abs(ll[:, 1] - scorer) <= RTOL * scale).all()


def test_independence_of_calls_replicates_cells_and_totals():
    """Bit for bit on ll_rep, exact on T_rep: two calls; n_rep = 4 against four calls of n_rep = 1; the cells split with cell_offset; T_rep = NULL."""
    E, V, U, clone, total, seed = sc.make("mixed")
    N = clone.shape[0]
    ll, T = engine.predictive_stats(E, V, U, clone, total, seed, draw0=DRAW0, n_rep=4)
    again = engine.predictive_stats(E, V, U, clone, total, seed, draw0=DRAW0, n_rep=4)
    assert np.array_equal(ll, again[0]) and np.array_equal(T, again[1])
    for r in range(4):
        a, Ta = engine.predictive_stats(E, V, U, clone, total, seed, draw0=DRAW0 + r, n_rep=1)
        assert np.array_equal(a[:, 0], ll[:, r]) and np.array_equal(Ta[0], T[r]), r
    for h in (1, 37, N - 1):
        a, Ta = engine.predictive_stats(E, V, U[:h], clone[:h], total[:h], seed, draw0=DRAW0, n_rep=4)
        b, Tb = engine.predictive_stats(E, V, U[h:], clone[h:], total[h:], seed, draw0=DRAW0, n_rep=4, cell_offset=h)
        assert np.array_equal(np.concatenate([a, b]), ll) and np.array_equal(Ta + Tb, T), h
    a, none = engine.predictive_stats(E, V, U, clone, total, seed, draw0=DRAW0, n_rep=4, gene_totals=False)
    assert none is None and np.array_equal(a, ll)
    # the caller's T buffer is overwritten, not added to
    out = (np.full(ll.shape, -7.0), np.full(T.shape, -7, dtype=np.int64))
    engine.predictive_stats(E, V, U, clone, total, seed, draw0=DRAW0, n_rep=4, out=out)
    assert np.array_equal(out[0], ll) and np.array_equal(out[1], T)
    other = engine.predictive_stats(E, V, U, clone, total, seed + 1, draw0=DRAW0, n_rep=1)[0]
    assert not np.array_equal(other[:, 0], ll[:, 0])
    assert engine.predictive_kernel_ms() > 0.0


def test_chunks_of_replicates_change_no_bit():
    """The host takes the replicates in chunks whose totals fit a 64 MB device buffer.  20 000 genes x 64 clones are 10.24 MB of int64 per replicate, so
    n_rep = 8 goes as chunks of 6 and 2: the strided copy of a chunk's ll into its columns of ll_rep, the chunk's place in T_rep and its draw index.  The
    same eight replicates from two calls of n_rep = 4 (one chunk each) are bit for bit the same ll_rep and exactly the same T_rep."""
    rng = np.random.default_rng(5)
    N, G, C = 40, 20000, 64
    E = rng.lognormal(0.0, 1.0, (G, 1)) * rng.integers(1, 5, (G, C)).astype(np.float64)
    V, U = rng.normal(size=(G, 1)) * 0.5, rng.normal(size=(N, 1))
    clone, total = rng.integers(0, C, N).astype(np.int32), rng.integers(0, 400, N).astype(np.int64)
    ll, T = engine.predictive_stats(E, V, U, clone, total, 3, draw0=DRAW0, n_rep=8, cell_offset=11)
    for lo in (0, 4):
        a, Ta = engine.predictive_stats(E, V, U, clone, total, 3, draw0=DRAW0 + lo, n_rep=4, cell_offset=11)
        assert np.array_equal(a, ll[:, lo:lo + 4]) and np.array_equal(Ta, T[lo:lo + 4]), lo
    assert (T.sum(axis=(1, 2)) == total.sum()).all() and ll[total > 1].min() < 0.0


def test_batches_of_cells_change_no_bit():
    """The host takes the cells in batches whose inputs and ll fit a 64 MB device buffer.  Without factors and at n_rep = 9 a cell takes 12 + 72 bytes, so
    800 000 cells go as batches of 798 915 and 1085; all but 24 cells at the two ends and around the cut have total 0 (nothing is drawn for them: exactly 0).
    The 24 cells alone, each called with its own cell_offset, give bit for bit the same ll_rep, and their T_rep add up to the whole call's."""
    rng = np.random.default_rng(6)
    N, G, C, n_rep = 800_000, 8, 2, 9
    cut = (64 << 20) // (12 + 8 * n_rep)
    assert 0 < cut < N
    E = rng.lognormal(0.0, 1.0, (G, 1)) * rng.integers(1, 5, (G, C)).astype(np.float64)
    clone = rng.integers(0, C, N).astype(np.int32)
    total = np.zeros(N, dtype=np.int64)
    cells = np.r_[0:6, cut - 6:cut + 6, N - 6:N]
    total[cells] = rng.integers(1, 300, cells.size)
    ll, T = engine.predictive_stats(E, None, None, clone, total, 4, draw0=DRAW0, n_rep=n_rep)
    assert (ll[total == 0] == 0.0).all()
    Tsum = np.zeros_like(T)
    for n in cells:
        a, Ta = engine.predictive_stats(E, None, None, clone[n:n + 1], total[n:n + 1], 4, draw0=DRAW0, n_rep=n_rep, cell_offset=int(n))
        assert np.array_equal(a[0], ll[n]) and (a[0] < 0.0).all(), n
        Tsum += Ta
    assert np.array_equal(Tsum, T)


def test_refusals_name_the_argument_and_leave_the_outputs_alone():
    E, _V, _U, clone, total, seed = sc.make("ragged")
    N, G, C = clone.shape[0], E.shape[0], E.shape[1]
    V, U = np.zeros((G, 1)), np.zeros((N, 1))

    def refused(match, E=E, V=V, U=U, clone=clone, total=total, n_rep=2, **kw):
        out = (np.full((N, max(n_rep, 0)), -7.0), np.full((max(n_rep, 0), G, C), -7, dtype=np.int64))
        with pytest.raises(EngineError, match=match):
            engine.predictive_stats(E, V, U, clone, total, seed, n_rep=n_rep, out=out, **kw)
        assert (out[0] == -7.0).all() and (out[1] == -7).all(), match
        assert engine.predictive_kernel_ms() == 0.0

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
    refused(r"cell_offset", cell_offset=2 ** 48 - N + 1)
    # the three of its own
    refused(r"n_rep = 0", n_rep=0)
    refused(r"n_rep = -1", n_rep=-1)
    refused(r"draw0", draw0=2 ** 48 - 1, n_rep=2)
    refused(r"draw0", draw0=2 ** 48 + 5, n_rep=1)
    lib, err = engine.load_library(), ctypes.create_string_buffer(256)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    Ec, cl, tt = np.ascontiguousarray(E), clone.astype(np.int32), total.astype(np.int64)
    ll, T = np.full((N, 2), -7.0), np.full((2, G, C), -7, dtype=np.int64)
    assert lib.ca_predictive_stats(N, G, C, 0, ptr(Ec), None, None, ptr(cl), ptr(tt), seed, 0, 2, 0, 0, None, ptr(T), err) == 1    # CA_ERR_INVALID
    assert b"ll_rep" in err.value and (T == -7).all(), err.value
    # what the binding cannot express: D < 0, D > 0 without U or V, N G >= 2^62
    for match, args in ((b"D = -1", (N, G, C, -1, ptr(Ec), None, None)), (b"needs both U", (N, G, C, 1, ptr(Ec), ptr(V), None)),
                        (b"needs both U", (N, G, C, 1, ptr(Ec), None, ptr(U))), (b"2^62", (2 ** 40, 2 ** 22, C, 0, ptr(Ec), None, None))):
        assert lib.ca_predictive_stats(*args, ptr(cl), ptr(tt), seed, 0, 2, 0, 0, ptr(ll), ptr(T), err) == 1
        assert match in err.value and err.value.startswith(b"ca_predictive_stats: ") and (ll == -7.0).all() and (T == -7).all(), err.value
    # the last two draw indices are allowed, and total = 0 everywhere is no error even for a clone that cannot be drawn from: zeros
    a, Ta = engine.predictive_stats(np.column_stack([E[:, 0], np.zeros(G)]), None, None, clone, 0, seed, draw0=2 ** 48 - 2, n_rep=2,
                                    out=(np.full((N, 2), -7.0), np.full((2, G, C), -7, dtype=np.int64)))
    assert (a == 0.0).all() and (Ta == 0).all()


def planted(N=200, G=300, C=3, n_bad=20, total=2000, seed=77):
    """The inputs of the issue's CPU experiment: E as tests/_simulate_cases.py makes it, V ~ 0.5 N(0, 1), U ~ N(0, 1); cells 0 .. n_bad - 1 are drawn from
    their own p with the genes permuted, the others from the model (numpy's multinomial).  Returned as a hand-made fit: mu and L with E = mu * L."""
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


def test_predictive_check_does_its_job():
    """200 x 300 x 3, totals 2000, n_rep = 50; cells 0-19 planted (genes permuted), 20-199 from the model.  The bars are the issue's, set from plain numpy
    multinomial draws over five seeds (planted: p_cell = 1/51 and z_cell < -150; in-model: z_cell > -5 and at most 9.4 % with p_cell <= 0.05):
    planted z_cell < -20, every other z_cell > -8, share of in-model cells with p_cell <= 0.05 at most 0.2.
    Measured on an MI355X: planted z_cell -361.1 .. -217.4, in-model z_cell >= -3.11, share 0.022."""
    fit, Y, L, z = planted()
    out = api.predictive_check(fit, Y, L, n_rep=50, seed=9)
    assert np.array_equal(out["cells"], np.arange(200))
    zc, pc = out["z_cell"], out["p_cell"]
    share = float((pc[20:] <= 0.05).mean())
    print(f"planted z_cell {zc[:20].min():.1f} .. {zc[:20].max():.1f}; in-model z_cell >= {zc[20:].min():.2f}; share of in-model cells with p_cell <= 0.05: {share:.3f}; "
          f"z = {out['z']:.2f}")
    assert (zc[:20] < -20.0).all()
    assert (zc[20:] > -8.0).all()
    assert share <= 0.2
    assert (pc[:20] == 1.0 / 51.0).all()
    assert np.isfinite(out["z_gene_clone"][out["T_replicate_sd"] > 0]).all()
    assert out["z_gene_clone"].shape == (300, 3) and out["p_gene_clone"].shape == (300, 3)
    assert np.array_equal(out["T_observed"], clone_sums(Y, z, 3))
    # host=True: the same T, the same ll within the bar (the mean over the replicates within the mean of the replicates' bars); five replicates keep the
    # numpy restatement short -- a replicate depends on (seed, r) alone, so they are the first five of the fifty
    dev, host = api.predictive_check(fit, Y, L, n_rep=5, seed=9), api.predictive_check(fit, Y, L, n_rep=5, seed=9, host=True)
    for k in ("T_observed", "T_replicate_mean", "T_replicate_sd"):
        assert np.array_equal(dev[k], host[k]), k
    assert np.array_equal(dev["T_observed"], out["T_observed"]) and np.array_equal(dev["ll_observed"], out["ll_observed"])
    E, V, U = fit["ml_params"]["mu"][:, None] * L, fit["ml_params"]["W"], fit["ml_params"]["psi"]
    total = Y.sum(1).astype(np.int64)
    _ll, scale_obs = numpy_ll(E, V, U, z, total, Y)
    assert (np.abs(dev["ll_observed"] - host["ll_observed"]) <= RTOL * scale_obs).all()
    scale_rep = np.mean([numpy_ll(E, V, U, z, total, engine.simulate_counts(E, V, U, z, total, 9, draw=r))[1] for r in range(5)], axis=0)
    assert (np.abs(dev["ll_replicate_mean"] - host["ll_replicate_mean"]) <= RTOL * scale_rep).all()
