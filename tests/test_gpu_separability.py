"""ca_clone_separability on the device: per cell and ordered pair of clones the per-read moments of the log-likelihood ratio in closed form.  Two oracles: the
float64 numpy restatement from the per-gene sums (api._clone_separability_host; bars 1e-10 of the terms' magnitudes) and verified code -- rows drawn by
engine.simulate_counts, whose sample mean and variance of the log-likelihood ratio must lie within their own standard errors of the closed forms."""
import ctypes
import functools

import numpy as np
import pytest

from clonealign_amd import api, engine

from tests import _simulate_cases as sc
from tests.test_separability_host import check_exact_zeros, zero_case

pytestmark = pytest.mark.gpu
RTOL = 1e-10
NB = 65536                                                           # cells per internal batch at most (include/clonealign_hip.h)


@functools.lru_cache(maxsize=None)
def reference(name):
    E, V, U, _clone, _total, _seed = sc.make(name)
    out = api._clone_separability_host(E, V, U, with_scale=True)
    for a in out:
        a.setflags(write=False)
    return out


def within_bars(got, want, what):
    """got: the five arrays; want: the restatement's five and its three scales.  Returns the largest ratios (logZ, excl, m1, m2, m3)."""
    bars = [RTOL * np.maximum(1.0, np.abs(want[0])), RTOL, RTOL * want[5], RTOL * want[6], RTOL * want[7]]
    worst = []
    for k in range(5):
        assert got[k].shape == want[k].shape and got[k].dtype == np.float64 and np.isfinite(got[k]).all(), (what, k)
        err = np.abs(got[k] - want[k])
        worst.append(float((err / np.where(np.asarray(bars[k]) > 0, bars[k], 1.0)).max()) * RTOL)
        assert (err <= bars[k]).all(), (what, k, worst[k])
    return worst


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_parity_with_the_numpy_restatement(name):
    """Every case of _simulate_cases.CASES (`clone` and `total` unused): N = 33, 5, 8, 16, 24, 64, 300 (ragged 16-cell tiles); G = 3, 77, 2049, 20 000 (no multiple of
    4, one past a power of two, forty gene chunks); C = 2, 3, 4, 8, 20 (10 .. 1540 columns: ragged column tiles, groups of eight tiles); E = 0 in places
    (`mixed`); |eta| = 700 (`steep`); no factors at all (`ragged`, `few_genes`: the host's row).  Bars: m_k 1e-10 sum_S p (|delta| + |Delta|)^k, excl 1e-10,
    logZ 1e-10 max(1, |logZ|).
    Largest ratios measured on an MI355X: logZ 1.3e-15 (`mixed`), excl 2.5e-16 (`mixed`), m1 4.4e-15, m2 3.3e-15, m3 5.7e-15 (`pow2_plus_1`, `mixed`); at `steep`
    m1 2.2e-13, m2 3.8e-14, m3 2.2e-14 (an ulp of eta = 700 in the exponent); the two cases without factors 8.1e-16 at most."""
    E, V, U, _clone, _total, _seed = sc.make(name)
    got = engine.clone_separability(E, V, U)
    want = reference(name)
    worst = within_bars(got, want, name)
    print(f"{name}: largest |device - numpy| / scale: logZ {worst[0]:.2e}, excl {worst[1]:.2e}, m1 {worst[2]:.2e}, m2 {worst[3]:.2e}, m3 {worst[4]:.2e}")
    C = E.shape[1]
    for k in range(1, 5):
        assert (got[k][:, np.arange(C), np.arange(C)] == 0.0).all(), k
    assert (engine.clone_separability_kernel_ms() > 0.0) == (U is not None)


def test_underflow_of_a_clone_under_the_shift():
    """U = [[800], [0]], V = +1 on genes 0-9 and -1 elsewhere, clone 1 positive on genes 10-39 only: in cell 0 every gene of clone 1 lies 1600 below the
    largest exponent, Z underflows to 0: logZ = -inf, both pair entries 0, no NaN.  Cell 1 is finite and within the bars."""
    rng = np.random.default_rng(4)
    G = 40
    E = rng.lognormal(0.0, 1.0, (G, 2))
    E[:10, 1] = 0.0
    V = np.where(np.arange(G) < 10, 1.0, -1.0)[:, None]
    U = np.array([[800.0], [0.0]])
    got = engine.clone_separability(E, V, U)
    assert not any(np.isnan(a).any() for a in got)
    assert got[0][0, 1] == -np.inf and np.isfinite(got[0][0, 0]) and np.isfinite(got[0][1]).all()
    for k in range(1, 5):
        assert (got[k][0] == 0.0).all(), k
    want = api._clone_separability_host(E, V, U, with_scale=True)
    assert want[0][0, 1] == -np.inf and all((want[k][0] == 0.0).all() for k in range(1, 5))
    within_bars([a[1:] for a in got], [a[1:] for a in want], "cell 1")
    assert got[1][1, 0, 1] > 0.0 and got[1][1, 1, 0] == 0.0


@pytest.mark.parametrize("D", (0, 1, 3))
def test_exact_zeros_on_the_device(D):
    """The diagonal; excl where no gene excludes; m1 = m2 = m3 = 0 for a duplicated clone column and for a column that is twice another."""
    E, V, U = zero_case(D)
    check_exact_zeros(engine.clone_separability(E, V, U), E, f"D = {D}")


def test_monte_carlo_cross_check_against_simulated_rows():
    """60 x 120 x 3, two factors, totals 200 .. 2000, 400 replicate rows per (cell, true clone) from engine.simulate_counts (one call per clone: the cells
    repeated 400 times, every row its own draw), Lambda = sum_g y_g (log p_a - log p_b) in numpy.  |mean - t m1| <= 6 sqrt(t v / 400) with v = m2 - m1^2, and
    the sample variance over t v within 1 +- 6 sqrt(2 / 399) = 1 +- 0.425.  The restatement against numpy's multinomial gave 3.29 standard errors and a ratio
    in [0.80, 1.24]; the device's closed forms against the device's rows, on an MI355X, 3.52 standard errors and a ratio in [0.790, 1.217]."""
    rng = np.random.default_rng(2025)
    N, G, C, D, R = 60, 120, 3, 2, 400
    E = rng.lognormal(0, 1, (G, 1)) * rng.integers(1, 5, (G, C))
    V = 0.5 * rng.normal(size=(G, D))
    U = rng.normal(size=(N, D))
    total = rng.integers(200, 2001, N).astype(np.int64)
    _logZ, excl, m1, m2, _m3 = engine.clone_separability(E, V, U)
    assert (excl == 0.0).all()
    eta = U @ V.T
    logp = np.log(E)[None] + eta[:, :, None]
    logp = logp - np.log(np.exp(logp).sum(1, keepdims=True))         # [N, G, C]
    worst_se, lo, hi = 0.0, np.inf, 0.0
    for a in range(C):
        Y = engine.simulate_counts(E, V, np.tile(U, (R, 1)), np.full(N * R, a, dtype=np.int32), np.tile(total, R), seed=77 + a).reshape(R, N, G)
        for b in range(C):
            if a == b:
                continue
            lam = np.einsum("rng,ng->rn", Y.astype(np.float64), logp[:, :, a] - logp[:, :, b])       # [R, N]
            v = m2[:, a, b] - m1[:, a, b] ** 2
            se = np.abs(lam.mean(0) - total * m1[:, a, b]) / np.sqrt(total * v / R)
            ratio = lam.var(0, ddof=1) / (total * v)
            worst_se, lo, hi = max(worst_se, se.max()), min(lo, ratio.min()), max(hi, ratio.max())
            assert (se <= 6.0).all(), (a, b, se.max())
            assert (np.abs(ratio - 1.0) <= 6.0 * np.sqrt(2.0 / (R - 1))).all(), (a, b, ratio.min(), ratio.max())
    print(f"worst standard error of the mean {worst_se:.2f}; variance ratio in [{lo:.3f}, {hi:.3f}]")


def test_determinism_and_splits():
    """`mixed`: two calls agree bit for bit; cells [0, 137) and [137, 300) in two calls are the one call's bits; one cell alone is its bits."""
    E, V, U, _clone, _total, _seed = sc.make("mixed")
    one, again = engine.clone_separability(E, V, U), engine.clone_separability(E, V, U)
    lo, hi = engine.clone_separability(E, V, U[:137]), engine.clone_separability(E, V, U[137:])
    single = engine.clone_separability(E, V, U[7:8])
    for k in range(5):
        assert np.array_equal(one[k], again[k]), k
        assert np.array_equal(np.concatenate([lo[k], hi[k]]), one[k]), k
        assert np.array_equal(single[k][0], one[k][7]), k


def test_batches_of_cells_change_no_bit():
    """With few genes and two clones a batch holds its most, 65 536 cells; 65 560 cells go as two batches.  Thirty cells at the ends and around the cut,
    called alone, give the long call's bits; every other cell is there to fill the batch."""
    rng = np.random.default_rng(8)
    G, C = 9, 2
    N = NB + 24
    E = rng.lognormal(0.0, 1.0, (G, 1)) * rng.integers(1, 5, (G, C)).astype(np.float64)
    V = rng.normal(size=(G, 1)) * 0.5
    U = rng.normal(size=(N, 1))
    cells = np.r_[0:6, NB - 6:NB + 6, N - 12:N]
    one, few = engine.clone_separability(E, V, U), engine.clone_separability(E, V, U[cells])
    for k in range(5):
        assert one[k].shape[0] == N and np.array_equal(one[k][cells], few[k]), k
    assert (few[2][:, 0, 1] > 0).all()


def test_refusals_name_the_argument_and_leave_the_outputs_alone():
    E, _V, _U, _clone, _total, _seed = sc.make("ragged")
    N, (G, C) = 5, E.shape
    V, U = np.zeros((G, 1)), np.zeros((N, 1))
    lib, err = engine.load_library(), ctypes.create_string_buffer(256)
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    engine.clone_separability(E, V, U)
    assert engine.clone_separability_kernel_ms() > 0.0

    def poke(a, idx, v):
        b = np.array(a, dtype=np.float64)
        b[idx] = v
        return b

    def refused(match, E=E, V=V, U=U, N=N, G=G, C=C, D=1, null=None):
        outs = [np.full((5, C), -7.0)] + [np.full((5, C, C), -7.0) for _ in range(4)]
        keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (E, V, U)]
        rc = lib.ca_clone_separability(N, G, C, D, *(ptr(a) for a in keep), 0, *(None if i == null else ptr(o) for i, o in enumerate(outs)), err)
        assert rc == 1, match                                                                   # CA_ERR_INVALID
        assert err.value.startswith(b"ca_clone_separability: ") and match in err.value, err.value
        assert all((o == -7.0).all() for o in outs), match
        assert engine.clone_separability_kernel_ms() == 0.0

    refused(b"C = 1", C=1)
    refused(b"G = 0", G=0)
    refused(b"N = -1", N=-1)
    refused(b"D = 9 is outside", V=np.zeros((G, 9)), U=np.zeros((N, 9)), D=9)
    refused(b"D = -1 is outside", D=-1)
    refused(b"needs both U", U=None)
    refused(b"needs both U", V=None)
    refused(b"E must not be NULL", E=None)
    refused(b"E has a negative", E=poke(E, (3, 1), -1.0))
    refused(b"E has a negative or non-finite entry (gene 4, clone 0)", E=poke(E, (4, 0), np.inf))
    refused(b"clone 1", E=np.column_stack([E[:, 0], np.zeros(G)]))
    refused(b"non-finite value in clone 0", E=poke(E, (slice(None), 0), 1e308))
    refused(b"U has a non-finite", U=poke(U, (2, 0), np.nan))
    refused(b"V has a non-finite", V=poke(V, (76, 0), np.inf))
    refused(b"2^60 or more", N=2 ** 58)
    for i, name in enumerate((b"logZ", b"excl", b"m1", b"m2", b"m3")):
        refused(name + b" must not be NULL", null=i)
    with pytest.raises(engine.EngineError, match=r"ca_clone_separability: E has a negative"):
        engine.clone_separability(poke(E, (3, 1), -1.0), V, U)
    empty = engine.clone_separability(E, V, U[:0])                    # no cells: no error
    assert [a.shape for a in empty] == [(0, C), (0, C, C), (0, C, C), (0, C, C), (0, C, C)]


def test_python_on_the_device():
    """A planted 200 x 300 x 3 fit (the recipe of tests/test_gpu_predictive_moments.py): clone_separability(fit, L, totals) equals host=True within the bars;
    confusion, reads_needed and merge_candidates agree between the two."""
    rng = np.random.default_rng(77)
    N, G, C = 200, 300, 3
    mu = rng.lognormal(0.0, 1.0, G)
    L = rng.integers(1, 5, (G, C)).astype(np.float64)
    L[:, 2] = L[:, 1]
    L[0, 2] = 5.0 - L[0, 1]                                          # clones 1 and 2 differ in one gene: a pair to merge
    L[5, 0] = 0.0
    fit = {"ml_params": {"mu": mu, "W": rng.normal(size=(G, 1)) * 0.5, "psi": rng.normal(size=(N, 1))}, "clone_names": ["clone_a", "clone_b", "clone_c"]}
    total = rng.integers(100, 1000, N)
    clones = np.asarray(fit["clone_names"], dtype=object)[rng.integers(0, C, N)]
    dev = api.clone_separability(fit, L, total, clones=clones, per_cell=True)
    host = api.clone_separability(fit, L, total, clones=clones, per_cell=True, host=True)
    want = api._clone_separability_host(mu[:, None] * L, fit["ml_params"]["W"], fit["ml_params"]["psi"], with_scale=True)
    within_bars([dev[k] for k in ("logZ", "excl", "m1", "m2", "m3")], want, "device")
    for k in ("confusion", "kl_per_read", "excl_per_read", "var_per_read", "p_error_cell", "p_confuse"):
        assert np.allclose(dev[k], host[k], rtol=1e-7, atol=1e-12), k
    assert np.array_equal(dev["worst_rival"], host["worst_rival"])
    assert np.array_equal(api.reads_needed(dev, 0.05), api.reads_needed(host, 0.05))
    a, b = api.merge_candidates(dev, 0.1), api.merge_candidates(host, 0.1)
    assert [x[:2] for x in a] == [x[:2] for x in b] == [("clone_b", "clone_c")]
    assert dev["excl_per_read"][1, 0] > 0 and dev["excl_per_read"][0, 1] == 0
