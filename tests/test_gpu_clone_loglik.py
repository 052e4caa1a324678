"""ca_clone_loglik / HipEngine.clone_loglik / clone_loglik / assign_cells: the per-cell, per-clone log-likelihood under a fitted model at its point
estimates (p_y_on_c, R/inference-tflow.R:288-296) in one float64 sweep over the resident count matrix.

The yardstick is ``ref_ll`` below, the formula restated in numpy float64 with xlogy semantics (chunked over cells).  Bar:
``|ll - ref| <= 1e-10 * scale[n][c]``, scale = sum_g y |log E| + sum_g y |eta| + s |log Z| (+ lgamma(s + 1) + sum_g lgamma(y + 1)): a float64 sum of at most
2049 terms is good to 2049 * 2^-53 = 2.3e-13 of the sum of the terms' magnitudes; 1e-10 is the margin this project gives its float64 sweeps (RTOL of
tests/test_gpu_fit_mse.py), and any float32 intermediate (6e-8) fails it."""
import numpy as np
import pytest
from scipy.special import gammaln, logsumexp

from tests._cases import eps_for, make_case
from tests.test_gpu_fit_mse import SHAPES, problem

pytestmark = pytest.mark.gpu
RTOL = 1e-10


def ref_ll(Y, E, U=None, V=None, const=True, chunk=1024):
    """(ll, scale) [N, C] for Y dense (any dtype) or scipy.sparse."""
    E = np.asarray(E, dtype=np.float64)
    N, G = Y.shape
    zero = E == 0
    logE = np.log(np.where(zero, 1.0, E))                            # xlogy: 0 * log 0 = 0 ...
    D = 0 if U is None else U.shape[1]
    ll, scale = np.empty((N, E.shape[1])), np.empty((N, E.shape[1]))
    for lo in range(0, N, chunk):
        Yc = Y[lo:lo + chunk]
        Yc = np.asarray(Yc.toarray() if hasattr(Yc, "toarray") else Yc, dtype=np.float64)
        s = Yc.sum(1)
        a, sc = Yc @ logE, Yc @ np.abs(logE)
        a[((Yc > 0).astype(np.float64) @ zero.astype(np.float64)) > 0] = -np.inf      # ... and y * log 0 = -inf for y > 0
        if D > 0:
            eta = U[lo:lo + chunk] @ V.T
            m = eta.max(1, keepdims=True)
            logz = m + np.log(np.exp(eta - m) @ E)
            a += (Yc * eta).sum(1)[:, None]
            sc += (Yc * np.abs(eta)).sum(1)[:, None]
        else:
            logz = np.broadcast_to(np.log(E.sum(0))[None, :], a.shape)
        a -= s[:, None] * logz
        sc += s[:, None] * np.abs(logz)
        if const:
            lg = gammaln(Yc + 1.0).sum(1)
            a += (gammaln(s + 1.0) - lg)[:, None]
            sc += (gammaln(s + 1.0) + lg)[:, None]
        ll[lo:lo + chunk], scale[lo:lo + chunk] = a, sc
    return ll, scale


def check(out, ref, scale, tag):
    assert out.shape == ref.shape, tag
    assert not np.isnan(out).any(), tag
    assert np.array_equal(np.isneginf(out), np.isneginf(ref)), tag
    ok = np.isfinite(ref)
    assert np.isfinite(out[ok]).all(), tag
    worst = float((np.abs(out[ok] - ref[ok]) / scale[ok]).max())
    print(f"clone_loglik {tag}: max |ll - ref| / scale {worst:.2e}")
    assert worst <= RTOL, tag
    return worst


def factors(N, G, D, rng):
    return rng.normal(size=(N, D)) * 0.5, rng.normal(size=(G, D)) * 0.3


@pytest.mark.parametrize("storage", ["u8", "u16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_with_the_float64_restatement(shape, storage):
    from clonealign_amd.engine import HipEngine
    N, G, C = shape
    Y, L, mu, _idx, rng = problem(N, G, C, storage, seed=sum(shape))
    E = mu[:, None] * L
    U, V = factors(N, G, 3, rng)
    eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, y_storage=storage)
    try:
        assert eng.info()["y_storage_name"] == storage
        for D in (0, 1, 3):
            Uv, Vv = (None, None) if D == 0 else (U[:, :D], V[:, :D])
            for const in (True, False):
                out = eng.clone_loglik(E, Uv, Vv, const=const)
                ref, scale = ref_ll(Y, E, Uv, Vv, const=const)
                check(out, ref, scale, f"{shape} {storage} D={D} const={const}")
                assert np.array_equal(eng.clone_loglik(E, Uv, Vv, const=const), out)      # two calls: identical bits
        assert np.array_equal(eng.clone_loglik(E, np.zeros((N, 0)), np.zeros((G, 0))), eng.clone_loglik(E))
    finally:
        eng.close()


@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_zero_copy_number_and_extreme_exponents(shape):
    from clonealign_amd.engine import HipEngine
    N, G, C = shape
    Y, L, mu, _idx, rng = problem(N, G, C, "u8", seed=7)
    c0 = min(3, C - 1)
    L[5, :] = 0.0
    Y[:, 5] = 0                                                      # zero copy number against zero counts: contributes nothing
    L[7, c0] = 0.0
    Y[:, 7] = 0
    Y[11, 7] = 2                                                     # one cell with a positive count where one clone has none
    E = mu[:, None] * L
    U, V = factors(N, G, 2, rng)
    U[20] = (1.0, 0.0)
    V[[3, 40, 60], 0] = 800.0                                        # eta = +-800 on a few genes of cell 20
    V[[4, 41], 0] = -800.0
    eng = HipEngine(Y, np.maximum(L, 1.0), np.zeros((N, 0)), np.zeros(G), 0)
    try:
        for Uv, Vv in ((None, None), (U, V)):
            out = eng.clone_loglik(E, Uv, Vv)
            ref, scale = ref_ll(Y, E, Uv, Vv)
            want = np.zeros((N, C), dtype=bool)
            want[11, c0] = True
            assert np.array_equal(np.isneginf(ref), want)
            check(out, ref, scale, f"{shape} zeros of E, D={0 if Uv is None else 2}")
            assert np.isfinite(out[20]).all()
    finally:
        eng.close()


@pytest.mark.parametrize("storage", ["u8", "f32"])
def test_layouts_selections_and_sparse_input(storage):
    import scipy.sparse as sps
    from clonealign_amd.engine import HipEngine
    N, G, C = 1500, 700, 5
    Y, L, mu, _idx, rng = problem(N, G, C, storage, seed=12)
    E = mu[:, None] * L
    U, V = factors(N, G, 2, rng)
    outs = {}
    for lay in ("row", "col"):
        eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, y_storage=storage, layout=lay)
        try:
            f = np.asfortranarray if lay == "col" else np.ascontiguousarray
            outs[lay] = eng.clone_loglik(f(E), f(U), f(V))
        finally:
            eng.close()
    check(outs["row"], *ref_ll(Y, E, U, V), f"layout row {storage}")
    assert np.array_equal(outs["row"], outs["col"])
    for fmt in (sps.csr_matrix, sps.csc_matrix):
        eng = HipEngine(fmt(Y), L, np.zeros((N, 0)), np.zeros(G), 0, y_storage=storage)
        try:
            assert np.array_equal(eng.clone_loglik(E, U, V), outs["row"]), fmt.__name__
        finally:
            eng.close()
    ci = np.sort(rng.choice(N, 1100, replace=False)).astype(np.int64)
    gi = np.sort(rng.choice(G, 515, replace=False)).astype(np.int32)
    sel = HipEngine(Y, L[gi], np.zeros((1100, 0)), np.zeros(515), 0, y_storage=storage, cell_index=ci, gene_index=gi)
    dense = HipEngine(np.ascontiguousarray(Y[np.ix_(ci, gi)]), L[gi], np.zeros((1100, 0)), np.zeros(515), 0, y_storage=storage)
    try:
        a, b = sel.clone_loglik(E[gi], U[ci], V[gi]), dense.clone_loglik(E[gi], U[ci], V[gi])
    finally:
        sel.close()
        dense.close()
    assert np.array_equal(a, b)
    check(a, *ref_ll(Y[np.ix_(ci, gi)], E[gi], U[ci], V[gi]), f"cell_index / gene_index {storage}")


@pytest.mark.parametrize("builtin", [True, False])
def test_the_call_changes_nothing_in_a_running_fit(builtin):
    """Five iterations, clone_loglik, five more == ten iterations straight, bit for bit: every variable and the ELBO."""
    from clonealign_amd.engine import HipEngine
    case = make_case(N=2600, G=640, C=5, K=1, seed=21)
    G = case["Y"].shape[1]
    eps = None if builtin else np.stack([eps_for(1, G, 100 + i) for i in range(20)])
    rng = np.random.default_rng(1)
    U, V = factors(2600, G, 1, rng)
    a = HipEngine(**case)
    try:
        ea = a.iterate(10, eps)
        sa = a.get_state()
    finally:
        a.close()
    b = HipEngine(**case)
    try:
        b.iterate(5, None if builtin else eps[:10])
        out = b.clone_loglik(case["L"], U, V)
        check(out, *ref_ll(case["Y"], case["L"], U, V), "mid-fit")
        eb = b.iterate(5, None if builtin else eps[10:])
        sb = b.get_state()
    finally:
        b.close()
    assert ea == eb
    for n in sa:
        assert np.array_equal(sa[n], sb[n]), n


@pytest.mark.parametrize("world", [2, 3])
def test_group_returns_the_single_handle_bits(world):
    from clonealign_amd.engine import EngineError, HipEngine, HipGroupEngine
    N, G, C = 1301, 700, 8
    Y, L, mu, _idx, rng = problem(N, G, C, "u8", seed=31)
    E = mu[:, None] * L
    U, V = factors(N, G, 1, rng)
    one = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0)
    try:
        o1 = one.clone_loglik(E, U, V)
    finally:
        one.close()
    grp = HipGroupEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, devices=[0] * world)
    try:
        og = grp.clone_loglik(E, U, V)
        bad = U.copy()
        bad[N - 1, 0] = np.nan                                       # refused on one rank's cells: refused by the group, which stays usable
        with pytest.raises(EngineError) as ex:
            grp.clone_loglik(E, bad, V)
        assert ex.value.code == 1 and "U has a non-finite entry" in ex.value.msg, ex.value.msg
        assert np.array_equal(grp.clone_loglik(E, U, V), og)
    finally:
        grp.close()
    assert np.array_equal(og, o1)


@pytest.mark.parametrize("K", [0, 1])
def test_against_the_fit_own_gamma_init(K):
    """gamma_init under an all-zero eps (mu = softplus(loc) exactly) leaves ll - logsumexp_c(ll); bar: tests/test_gpu_parity.py's for gamma_init (1e-5 of the
    largest logit; the loop's side is float32)."""
    from clonealign_amd.engine import HipEngine
    from clonealign_amd.hostprep import softplus
    case = make_case(N=900, G=500, C=4, K=K, seed=5)
    N, G = case["Y"].shape
    rng = np.random.default_rng(3)
    eng = HipEngine(**case)
    try:
        U = V = None
        if K:
            eng.set("psi", (rng.normal(size=(N, K)) * 0.5).astype(np.float32))
            eng.set("W", (rng.normal(size=(G, K)) * 0.3).astype(np.float32))
            U, V = eng.get("psi"), eng.get("W")
        eng.gamma_init(np.zeros((1, G), dtype=np.float32))
        E = softplus(eng.get("loc"))[:, None] * case["L"]
        ll = eng.clone_loglik(E, U, V)
        want = ll - logsumexp(ll, axis=1, keepdims=True)
        got = eng.get("gamma_logits")
        rel = float(np.abs(got - want).max() / np.abs(want).max())
        print(f"gamma_logits vs ll - logsumexp(ll), K={K}: {rel:.2e}")
        assert rel < 1e-5
    finally:
        eng.close()


def test_assign_cells_on_the_device():
    import clonealign_amd as ca

    class HostOnly:                                                   # a live engine without clone_loglik: the CPU host form
        def __init__(self, N, G):
            self.N, self.G = N, G
    rng = np.random.default_rng(8)
    case = make_case(N=1200, G=400, C=3, K=1, seed=17, scale=1.0)    # planted clones
    Y, L = case["Y"], case["L"]
    N, G = Y.shape
    fit = ca.ClonealignFit(ml_params={"mu": rng.lognormal(0, 1, G), "alpha": np.array([0.2, 0.3, 0.5]), "W": rng.normal(size=(G, 1)) * 0.2,
                                      "psi": rng.normal(size=(N, 1))}, clone_names=["a", "b", "c"])
    for psi in (None, "fit"):
        dev = ca.assign_cells(fit, Y, L, psi=psi)
        host = ca.assign_cells(fit, Y, L, psi=psi, engine=HostOnly(N, G))
        d = float(np.abs(dev["clone_probs"] - host["clone_probs"]).max())
        print(f"assign_cells psi={psi}: device vs host clone_probs max abs {d:.2e}")
        assert d <= 1e-9 and np.array_equal(dev["clone"], host["clone"])
        np.testing.assert_allclose(dev["loglik"], host["loglik"], rtol=1e-10)
    # after a real fit: the exact q(z) given the other parameters against the Adam-optimised one (the share is printed, not asserted)
    res = ca.clonealign(Y, L, max_iter=60, verbose=False, seed=3)
    assert len(res["retained_genes"]) == G                           # (no gene of this problem is filtered: L is the retained genes' as it is)
    again = ca.assign_cells(res, Y, L, psi="fit")
    share = float((again["clone"] == res["clone"]).mean())
    print(f"assign_cells after clonealign(): share of labels equal to the fit's own {share:.4f} "
          f"(unassigned: fit {(res['clone'] == 'unassigned').mean():.4f}, exact posterior {(again['clone'] == 'unassigned').mean():.4f})")
    assert again["clone_probs"].shape == (N, 3) and np.isfinite(again["loglik"]).all()


def test_refusals_name_the_offender_and_poll_hooks_are_refused():
    from clonealign_amd.engine import EngineError, HipEngine
    from clonealign_amd.rng import EpsStream
    case = make_case(N=700, G=300, C=4, K=1, seed=2)
    L = case["L"]
    rng = np.random.default_rng(0)
    U, V = factors(700, 300, 2, rng)
    eng = HipEngine(**case)
    try:
        def refused(words, *a, **k):
            with pytest.raises(EngineError) as ex:
                eng.clone_loglik(*a, **k)
            assert ex.value.code == 1 and all(w in ex.value.msg for w in words), ex.value.msg
        for v in (-1.0, np.inf, np.nan):
            E = L.copy()
            E[17, 2] = v
            refused(("gene 17", "clone 2"), E)
        E = L.copy()
        E[:, 1] = 0.0
        refused(("clone 1", "sums to"), E)
        Ub = U.copy()
        Ub[9, 1] = np.nan
        refused(("U has a non-finite", "cell 9"), L, Ub, V)
        Vb = V.copy()
        Vb[33, 0] = -np.inf
        refused(("V has a non-finite", "gene 33"), L, U, Vb)
        refused(("D = 9", "outside [0, 8]"), L, np.zeros((700, 9)), np.zeros((300, 9)))
        import ctypes as C
        ll = np.zeros((700, 4))
        rc = eng.lib.ca_clone_loglik(eng.h, L.ctypes.data_as(C.c_void_p), None, V.ctypes.data_as(C.c_void_p), 2, 1, ll.ctypes.data_as(C.c_void_p))
        assert rc == 1 and b"needs both U" in eng.lib.ca_last_error(eng.h)
        with pytest.raises(ValueError):
            eng.clone_loglik(L[:-1])
        with pytest.raises(ValueError):
            eng.clone_loglik(L, U[:-1], V)
        seen = {}

        def hook(i, e):
            if i == 2:
                with pytest.raises(EngineError) as ex:
                    eng.clone_loglik(L)
                seen["code"] = ex.value.code
            return False
        eng.run(EpsStream(9, 1, 300), 4, 1e-12, poll=hook)
        assert seen["code"] == 6                                     # CA_ERR_STATE
        check(eng.clone_loglik(L, U, V), *ref_ll(case["Y"], L, U, V), "after the run")
    finally:
        eng.close()
