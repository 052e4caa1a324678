"""ca_clone_pair_loglik / HipEngine.clone_pair_loglik / clone_pair_loglik / detect_doublets: the log-likelihood of the resident cells under every mixture of
two clones (a heterotypic doublet) on a weight grid, float64 on the device.

The yardstick is ``ref_pll`` below: the formula of include/clonealign_hip.h restated in numpy float64 over the non-zero counts (chunked over cells).  Bar, the
project's own for float64 sweeps (RTOL of tests/test_gpu_fit_mse.py): ``|pll - ref| <= 1e-10 * scale``, scale = sum_g y |log bracket| + sum_g y |eta| +
s |lz_ab| (+ lgamma(s + 1) + sum_g lgamma(y + 1) with the constant): a float64 sum of at most 2049 terms is good to 2049 * 2^-53 = 2.3e-13 of the sum of the
terms' magnitudes, and any float32 intermediate (6e-8) fails it.  The -inf pattern must be equal and no NaN may appear."""
import ctypes as C

import numpy as np
import pytest
from scipy.special import gammaln

from tests._cases import eps_for, make_case
from tests.test_doublets_host import HostOnly, fixture
from tests.test_gpu_clone_loglik import factors
from tests.test_gpu_fit_mse import RTOL, problem

pytestmark = pytest.mark.gpu


def pairs_of(Cn):
    return [(a, b) for a in range(Cn) for b in range(a + 1, Cn)]


def ref_pll(Y, E, U, V, weights, chunk=256):
    """(pll, scale, const, const_scale): pll [N, M, W] WITHOUT the constant, its scale, and the constant [N] with its scale [N].  Y dense or scipy.sparse."""
    E = np.asarray(E, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    N, G = Y.shape
    Cn = E.shape[1]
    D = 0 if U is None else U.shape[1]
    prs = pairs_of(Cn)
    pll, scale = np.empty((N, len(prs), w.size)), np.empty((N, len(prs), w.size))
    const, cscale = np.empty(N), np.empty(N)
    for lo in range(0, N, chunk):
        Yc = Y[lo:lo + chunk]
        Yc = np.asarray(Yc.toarray() if hasattr(Yc, "toarray") else Yc, dtype=np.float64)
        n = Yc.shape[0]
        s = Yc.sum(1)
        if D > 0:
            eta = U[lo:lo + chunk] @ V.T
            m = eta.max(1, keepdims=True)
            logz = m + np.log(np.exp(eta - m) @ E)
            base, bsc = (Yc * eta).sum(1), (Yc * np.abs(eta)).sum(1)
        else:
            logz = np.broadcast_to(np.log(E.sum(0))[None, :], (n, Cn))
            base, bsc = np.zeros(n), np.zeros(n)
        lg = gammaln(Yc + 1.0).sum(1)
        const[lo:lo + n], cscale[lo:lo + n] = gammaln(s + 1.0) - lg, gammaln(s + 1.0) + lg
        r, g = np.nonzero(Yc > 0)                                    # the non-zero counts, rows ascending and genes ascending within a row
        y = Yc[r, g]
        for p, (a, b) in enumerate(prs):
            lz = np.minimum(logz[:, a], logz[:, b])
            ca, cb = np.exp(lz - logz[:, a]), np.exp(lz - logz[:, b])
            ea, eb = E[g, a], E[g, b]
            for k, wk in enumerate(w):
                with np.errstate(divide="ignore"):
                    t = y * np.log((wk * ca)[r] * ea + ((1.0 - wk) * cb)[r] * eb)
                pll[lo:lo + n, p, k] = np.bincount(r, weights=t, minlength=n) + base - s * lz
                with np.errstate(invalid="ignore"):
                    scale[lo:lo + n, p, k] = np.bincount(r, weights=np.abs(t), minlength=n) + bsc + s * np.abs(lz)
    return pll, scale, const, cscale


def check(out, ref, scale, tag):
    assert out.shape == ref.shape, tag
    assert not np.isnan(out).any(), tag
    assert np.array_equal(np.isneginf(out), np.isneginf(ref)), tag
    ok = np.isfinite(ref)
    assert np.isfinite(out[ok]).all(), tag
    worst = float((np.abs(out[ok] - ref[ok]) / np.maximum(scale[ok], 1e-300)).max()) if ok.any() else 0.0
    print(f"clone_pair_loglik {tag}: max |pll - ref| / scale {worst:.2e}")
    assert worst <= RTOL, tag
    return worst


def engine_for(Y, L, storage=None, **kw):
    from clonealign_amd.engine import HipEngine
    N, G = Y.shape
    if storage is not None:
        kw["y_storage"] = storage
    return HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, **kw)


# (cells, genes, clones, weights): one pair, fewer cells than a block's waves and G under one segment | 84 slots: two blocks of slots per cell, rows of several
# segments | 570 slots, one column past a 2048 boundary, NC = 32 groups on the D = 0 route | 10 slots: most lanes of a wave idle
CASES = [(33, 77, 2, (0.25, 0.75)), (700, 1234, 8, (0.3, 0.5, 0.7)), (300, 2049, 20, (0.3, 0.5, 0.7)), (200, 300, 5, (0.5,))]


@pytest.mark.parametrize("storage", ["u8", "u16", "f32"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[:3])) + f"w{len(c[3])}")
def test_parity_with_the_float64_restatement(case, storage):
    N, G, Cn, w = case
    Y, L, mu, _idx, rng = problem(N, G, Cn, storage, seed=N + G + Cn)
    E = mu[:, None] * L
    U, V = factors(N, G, 3, rng)
    eng = engine_for(Y, L, storage)
    try:
        assert eng.info()["y_storage_name"] == storage
        for D in (0, 1, 3):
            Uv, Vv = (None, None) if D == 0 else (U[:, :D], V[:, :D])
            ref, scale, const, cscale = ref_pll(Y, E, Uv, Vv, w)
            for with_const in (True, False):
                r = eng.clone_pair_loglik(E, Uv, Vv, weights=w, const=with_const)
                assert r["pairs"].tolist() == [list(p) for p in pairs_of(Cn)]
                want, sc = (ref + const[:, None, None], scale + cscale[:, None, None]) if with_const else (ref, scale)
                check(r["pair_ll"], want, sc, f"{case[:3]} {storage} D={D} const={with_const}")
                assert np.array_equal(r["ll"], eng.clone_loglik(E, Uv, Vv, const=with_const))       # clone_loglik's rows, bit for bit
            again = eng.clone_pair_loglik(E, Uv, Vv, weights=w, const=False, want_ll=False)      # two calls: identical bits
            assert again["ll"] is None and np.array_equal(again["pair_ll"], r["pair_ll"])
    finally:
        eng.close()


@pytest.mark.parametrize("storage", ["u8", "f32"])
def test_the_kernel_and_the_table_route_agree(storage):
    """D = 1 with U = 0 takes k_pair_ll, D = 0 the table swept by k_clone_ll: two independent evaluations of the same numbers."""
    N, G, Cn, w = 500, 700, 6, (0.2, 0.5, 0.8)
    Y, L, mu, _idx, rng = problem(N, G, Cn, storage, seed=77)
    E = mu[:, None] * L
    eng = engine_for(Y, L, storage)
    try:
        tab = eng.clone_pair_loglik(E, weights=w)
        ker = eng.clone_pair_loglik(E, np.zeros((N, 1)), rng.normal(size=(G, 1)), weights=w)
    finally:
        eng.close()
    ref, scale, const, cscale = ref_pll(Y, E, None, None, w)
    check(ker["pair_ll"], tab["pair_ll"], scale + cscale[:, None, None], f"kernel against table {storage}")
    check(tab["pair_ll"], ref + const[:, None, None], scale + cscale[:, None, None], f"table {storage}")


@pytest.mark.parametrize("D", [0, 2])
def test_cell_ranges_return_the_full_call_bits(D):
    N, G, Cn, w = 301, 600, 4, (0.3, 0.5, 0.7)
    Y, L, mu, _idx, rng = problem(N, G, Cn, "u8", seed=5)
    E = mu[:, None] * L
    U, V = factors(N, G, D, rng) if D else (None, None)
    eng = engine_for(Y, L)
    try:
        full = eng.clone_pair_loglik(E, U, V, weights=w)
        parts = [eng.clone_pair_loglik(E, U, V, weights=w, cells=c) for c in ((0, 100), (100, 101), (101, N))]
        none = eng.clone_pair_loglik(E, U, V, weights=w, cells=(7, 7))
    finally:
        eng.close()
    assert [p["pair_ll"].shape[0] for p in parts] == [100, 1, N - 101] and none["pair_ll"].shape == (0, 6, 3)
    assert np.array_equal(np.concatenate([p["pair_ll"] for p in parts]), full["pair_ll"])
    assert np.array_equal(np.concatenate([p["ll"] for p in parts]), full["ll"])


def test_zero_copy_number_and_extreme_exponents():
    """The construction of tests/test_gpu_clone_loglik.py: eta = +-800 on a few genes of one cell, E = 0 in one clone, in two and in all of them."""
    N, G, Cn, w = 33, 77, 4, (0.3, 0.7)
    Y, L, mu, _idx, rng = problem(N, G, Cn, "u8", seed=7)
    L[5, :] = 0.0
    Y[:, 5] = 0                                                      # zero copy number against zero counts: contributes nothing
    L[7, 3] = 0.0
    Y[:, 7] = 0
    Y[11, 7] = 2                                                     # one clone without the gene: its pairs stay finite
    L[9, 1] = L[9, 3] = 0.0
    Y[:, 9] = 0
    Y[12, 9] = 1                                                     # two clones without it: -inf for the pair (1, 3) alone
    L[13, :] = 0.0
    Y[:, 13] = 0
    Y[14, 13] = 3                                                    # no clone has it: -inf for every pair of that cell
    E = mu[:, None] * L
    U, V = factors(N, G, 2, rng)
    U[20] = (1.0, 0.0)
    V[[3, 40, 60], 0] = 800.0                                        # eta = +-800 on a few genes of cell 20
    V[[4, 41], 0] = -800.0
    want = np.zeros((N, 6, 2), dtype=bool)
    want[12, pairs_of(Cn).index((1, 3))] = True
    want[14] = True
    eng = engine_for(Y, np.maximum(L, 1.0))
    try:
        for Uv, Vv in ((None, None), (U, V)):
            r = eng.clone_pair_loglik(E, Uv, Vv, weights=w)
            ref, scale, const, cscale = ref_pll(Y, E, Uv, Vv, w)
            assert np.array_equal(np.isneginf(ref), want)
            check(r["pair_ll"], ref + const[:, None, None], scale + cscale[:, None, None], f"zeros of E, D={0 if Uv is None else 2}")
            assert np.isfinite(r["pair_ll"][20]).all() and np.isfinite(r["pair_ll"][11]).all()
            assert np.array_equal(r["ll"], eng.clone_loglik(E, Uv, Vv))
    finally:
        eng.close()


@pytest.mark.parametrize("storage", ["u8", "f32"])
def test_layouts_selections_and_sparse_input(storage):
    import scipy.sparse as sps
    from clonealign_amd.engine import HipEngine
    N, G, Cn, w = 400, 700, 5, (0.3, 0.5, 0.7)
    Y, L, mu, _idx, rng = problem(N, G, Cn, storage, seed=12)
    E = mu[:, None] * L
    U, V = factors(N, G, 2, rng)
    outs = {}
    for lay in ("row", "col"):
        eng = engine_for(Y, L, storage, layout=lay)
        try:
            f = np.asfortranarray if lay == "col" else np.ascontiguousarray
            outs[lay] = [eng.clone_pair_loglik(f(E), f(U), f(V), weights=w, cells=(3, 390)), eng.clone_pair_loglik(f(E), weights=w)]
        finally:
            eng.close()
    ref, scale, const, cscale = ref_pll(Y, E, U, V, w)
    check(outs["row"][0]["pair_ll"], (ref + const[:, None, None])[3:390], (scale + cscale[:, None, None])[3:390], f"layout row {storage}")
    for i in (0, 1):
        assert np.array_equal(outs["row"][i]["pair_ll"], outs["col"][i]["pair_ll"]) and np.array_equal(outs["row"][i]["ll"], outs["col"][i]["ll"])
    for fmt in (sps.csr_matrix, sps.csc_matrix):
        eng = engine_for(fmt(Y), L, storage)
        try:
            assert np.array_equal(eng.clone_pair_loglik(E, U, V, weights=w, cells=(3, 390))["pair_ll"], outs["row"][0]["pair_ll"]), fmt.__name__
        finally:
            eng.close()
    ci = np.sort(rng.choice(N, 290, replace=False)).astype(np.int64)
    gi = np.sort(rng.choice(G, 515, replace=False)).astype(np.int32)
    sel = HipEngine(Y, L[gi], np.zeros((290, 0)), np.zeros(515), 0, y_storage=storage, cell_index=ci, gene_index=gi)
    dense = engine_for(np.ascontiguousarray(Y[np.ix_(ci, gi)]), L[gi], storage)
    try:
        a, b = sel.clone_pair_loglik(E[gi], U[ci], V[gi], weights=w), dense.clone_pair_loglik(E[gi], U[ci], V[gi], weights=w)
    finally:
        sel.close()
        dense.close()
    assert np.array_equal(a["pair_ll"], b["pair_ll"]) and np.array_equal(a["ll"], b["ll"])


@pytest.mark.parametrize("world", [2, 3])
def test_group_returns_the_single_handle_bits(world):
    from clonealign_amd.engine import EngineError, HipGroupEngine
    N, G, Cn, w = 501, 700, 8, (0.3, 0.5, 0.7)
    Y, L, mu, _idx, rng = problem(N, G, Cn, "u8", seed=31)
    E = mu[:, None] * L
    U, V = factors(N, G, 1, rng)
    one = engine_for(Y, L)
    try:
        o1 = [one.clone_pair_loglik(E, U, V, weights=w), one.clone_pair_loglik(E, weights=w), one.clone_pair_loglik(E, U, V, weights=w, cells=(100, 400))]
    finally:
        one.close()
    grp = HipGroupEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, devices=[0] * world)
    try:
        og = [grp.clone_pair_loglik(E, U, V, weights=w), grp.clone_pair_loglik(E, weights=w), grp.clone_pair_loglik(E, U, V, weights=w, cells=(100, 400))]
        bad = U.copy()
        bad[N - 1, 0] = np.nan                                       # refused on one rank's cells: refused by the group, which stays usable
        with pytest.raises(EngineError) as ex:
            grp.clone_pair_loglik(E, bad, V, weights=w)
        assert ex.value.code == 1 and "U has a non-finite entry" in ex.value.msg, ex.value.msg
        with pytest.raises(EngineError) as ex:
            grp.clone_pair_loglik(E, U, V, weights=w, cells=(400, N + 1))
        assert ex.value.code == 1 and "cell range" in ex.value.msg, ex.value.msg
        assert np.array_equal(grp.clone_pair_loglik(E, U, V, weights=w, cells=(100, 400))["pair_ll"], og[2]["pair_ll"])
    finally:
        grp.close()
    for a, b in zip(o1, og):
        assert np.array_equal(a["pair_ll"], b["pair_ll"]) and np.array_equal(a["ll"], b["ll"])


def test_the_call_changes_nothing_in_a_running_fit_and_is_refused_from_a_poll_hook():
    """Five iterations, clone_pair_loglik, five more == ten iterations straight, bit for bit: every variable and the ELBO."""
    from clonealign_amd.engine import EngineError, HipEngine
    from clonealign_amd.rng import EpsStream
    case = make_case(N=900, G=500, C=4, K=1, seed=21)
    N, G = case["Y"].shape
    eps = np.stack([eps_for(1, G, 100 + i) for i in range(20)])
    rng = np.random.default_rng(1)
    U, V = factors(N, G, 1, rng)
    w = (0.3, 0.5, 0.7)
    a = HipEngine(**case)
    try:
        ea = a.iterate(10, eps)
        sa = a.get_state()
    finally:
        a.close()
    b = HipEngine(**case)
    try:
        b.iterate(5, eps[:10])
        out = b.clone_pair_loglik(case["L"], U, V, weights=w)
        b.clone_pair_loglik(case["L"], weights=w)
        ref, scale, const, cscale = ref_pll(case["Y"], case["L"], U, V, w)
        check(out["pair_ll"], ref + const[:, None, None], scale + cscale[:, None, None], "mid-fit")
        eb = b.iterate(5, eps[10:])
        sb = b.get_state()
        seen = {}

        def hook(i, e):
            if i == 2:
                with pytest.raises(EngineError) as ex:
                    b.clone_pair_loglik(case["L"], weights=w)
                seen["code"] = ex.value.code
            return False
        b.run(EpsStream(9, 1, G), 4, 1e-12, poll=hook)
        assert seen["code"] == 6                                     # CA_ERR_STATE
    finally:
        b.close()
    assert ea == eb
    for n in sa:
        assert np.array_equal(sa[n], sb[n]), n


def test_detect_doublets_on_the_device():
    import clonealign_amd as ca
    Y, L, fit, truth, tpair = fixture(n_single=150, n_double=50, G=200, seed=4)
    N, G = Y.shape
    rng = np.random.default_rng(2)
    fit["ml_params"]["W"] = rng.normal(size=(G, 1)) * 0.05
    fit["ml_params"]["psi"] = rng.normal(size=(N, 1))
    for psi in (None, "fit"):                                        # the table route (D = 0) and the kernel (D = 1)
        dev = ca.detect_doublets(fit, Y, L, doublet_rate=0.1, psi=psi)
        host = ca.detect_doublets(fit, Y, L, doublet_rate=0.1, psi=psi, engine=HostOnly(N, G))
        cut = ca.detect_doublets(fit, Y, L, doublet_rate=0.1, psi=psi, chunk_cells=64)
        assert np.array_equal(dev["clone"], host["clone"]) and np.array_equal(dev["doublet_pair"], host["doublet_pair"])
        for k in ("p_doublet", "pair_probs", "clone_probs", "doublet_weight"):
            d = float(np.abs(dev[k] - host[k]).max())
            print(f"detect_doublets psi={psi}: device vs host {k} max abs {d:.2e}")
            assert d <= 1e-9, k
            assert np.array_equal(cut[k], dev[k]), k
        np.testing.assert_allclose(dev["loglik"], host["loglik"], rtol=1e-10)
        d = truth == "doublet"
        print(f"detect_doublets psi={psi}: doublets labelled {(dev['clone'][d] == 'doublet').mean():.3f}, right pair {(dev['doublet_pair'][d] == tpair[d]).mean():.3f}, "
              f"singlets labelled doublet {(dev['clone'][~d] == 'doublet').mean():.3f}")
    r = ca.clone_pair_loglik(fit, Y, L, psi="fit")
    assert r["pair_ll"].shape == (N, 6, 3) and np.allclose(r["weights"], [0.3, 0.5, 0.7])


def test_refusals_through_the_c_abi_name_the_offender():
    from clonealign_amd.engine import HipEngine
    N, G, Cn = 120, 90, 3
    Y, L, mu, _idx, rng = problem(N, G, Cn, "u8", seed=2)
    E = np.ascontiguousarray(mu[:, None] * L)
    U, V = factors(N, G, 2, rng)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    eng = engine_for(Y, L)
    one = HipEngine(Y, L[:, :1], np.zeros((N, 0)), np.zeros(G), 0)
    try:
        ll, pll = np.zeros((N, Cn)), np.zeros((N, 3 * 8))

        def refused(words, h=eng, E_=E, w=(0.3, 0.7), nw=None, lo=0, cnt=N, out=pll, D=0, U_=None, V_=None):
            wv = np.asarray(w, dtype=np.float64)
            rc = h.lib.ca_clone_pair_loglik(h.h, ptr(E_), ptr(U_), ptr(V_), D, 1, ptr(wv), len(wv) if nw is None else nw, lo, cnt, ptr(ll), ptr(out))
            msg = h.lib.ca_last_error(h.h).decode()
            assert rc == 1 and all(x in msg for x in words), (rc, msg)
        for bad in (0.0, 1.0, -0.5, 2.0, np.nan, np.inf):
            refused(("ca_clone_pair_loglik", "weight 1", "(0, 1)"), w=(0.5, bad))
        refused(("n_weights = 0", "[1, 8]"), nw=0)
        refused(("n_weights = 9", "[1, 8]"), w=np.linspace(0.1, 0.9, 9))
        refused(("C = 1",), h=one, E_=np.ascontiguousarray(E[:, :1]))
        refused(("cell range", f"[0, {N}]"), lo=100, cnt=21)
        refused(("cell range",), lo=-1, cnt=5)
        refused(("cell range",), lo=0, cnt=-1)
        refused(("pair_ll is NULL",), out=None)
        Eb = E.copy()
        Eb[17, 2] = -1.0
        refused(("gene 17", "clone 2"), E_=Eb)
        Ub = U.copy()
        Ub[9, 1] = np.nan
        refused(("U has a non-finite", "cell 9"), D=2, U_=Ub, V_=V)
        refused(("D = 9", "outside [0, 8]"), D=9, U_=U, V_=V)
        refused(("needs both U",), D=2, V_=V)
        with pytest.raises(ValueError):
            eng.clone_pair_loglik(E[:-1])
        r = eng.clone_pair_loglik(E, U, V, weights=(0.3, 0.7))      # still usable
        ref, scale, const, cscale = ref_pll(Y, E, U, V, (0.3, 0.7))
        check(r["pair_ll"], ref + const[:, None, None], scale + cscale[:, None, None], "after the refusals")
    finally:
        eng.close()
        one.close()
