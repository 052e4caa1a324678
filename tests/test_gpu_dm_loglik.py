"""ca_clone_loglik_dm / HipEngine.clone_loglik_dm / clone_loglik_dm / estimate_concentration / assign_cells_dm: the Dirichlet-multinomial log-likelihood of the
resident cells under every clone on a grid of concentrations, float64 on the device (k_dm_ll, clonealign_amd/csrc/ca_k_dmll.hip.h).

The yardstick is ``api._clone_loglik_dm_host``: the formula of include/clonealign_hip.h in numpy / scipy ``gammaln`` over the non-zero counts.  Bar, the project's
own for float64 sweeps (RTOL of tests/test_gpu_fit_mse.py): ``|dm - ref| <= 1e-10 * scale`` with scale = sum_{g: y > 0} (|gammaln(y + a)| + |gammaln(a)| + 1 +
|eta| + |log Z|) + |gammaln(phi)| + |gammaln(phi + s)| (+ gammaln(s + 1) + sum_g gammaln(y + 1) with the constant); the ``1 + |eta| + |log Z|`` is there because
the relative error of ``a = phi E exp(eta) / Z`` enters each term with a factor of about 1.  The -inf pattern must be equal and no NaN may appear.
Measured on an MI355X over the parity cases below: at most 2.21e-15 (MEASURED); the product route against two lgamma for the same numbers: 3.1e-17."""
import ctypes as C

import numpy as np
import pytest
from scipy.special import gammaln

from clonealign_amd import api
from tests._cases import eps_for, make_case
from tests.test_dm_host import GRID, planted
from tests.test_doublets_host import HostOnly
from tests.test_gpu_clone_loglik import factors
from tests.test_gpu_fit_mse import RTOL, problem
from tests.test_gpu_pair_loglik import engine_for

pytestmark = pytest.mark.gpu

MEASURED = "2.21e-15"                # worst |dm - ref| / scale over test_parity_with_the_float64_restatement (u8, 300 x 2049 x 20, 5 concentrations, with the constant)
Y_SMALL = 8                          # CA_DM_YSMALL: integer counts up to here take the product route, everything else two lgamma


def grid_of(K):
    return np.geomspace(1.0, 1e5, K)


def plant_counts(Y):
    """Counts on both sides of the product route's limit, the limit itself and the limit + 1, in cells 1 and 2 (exact in every storage)."""
    Y[1, :6] = (Y_SMALL, Y_SMALL + 1, 1, Y_SMALL - 1, 2 * Y_SMALL + 5, 3)
    Y[2, 1:4] = (Y_SMALL + 1, Y_SMALL, 40)
    assert (Y == Y_SMALL).any() and (Y == Y_SMALL + 1).any() and ((Y > 0) & (Y < Y_SMALL)).any() and (Y > Y_SMALL + 1).any()
    return Y


def const_of(Y):
    """(const_n, its scale) [N]: lgamma(s + 1) - sum_g lgamma(y + 1) and the sum of the two magnitudes."""
    Yd = np.asarray(Y.toarray() if hasattr(Y, "toarray") else Y, dtype=np.float64)
    lg = gammaln(Yd + 1.0).sum(1)
    return gammaln(Yd.sum(1) + 1.0) - lg, gammaln(Yd.sum(1) + 1.0) + lg


def ref_rows(N):
    """The cells the parity cases compare (the host form costs seconds per 500 000 non-zero counts): all of a small case, else the first and last 48 cells --
    whole blocks of four waves and the launch's ragged end -- and every 7th in between (every position within a block)."""
    if N <= 256:
        return np.arange(N)
    return np.unique(np.concatenate([np.arange(48), np.arange(48, N - 48, 7), np.arange(N - 48, N)]))


def reference(Y, E, U, V, phi):
    """(dm WITHOUT the constant, its scale, const [N], the constant's scale [N]) from the host form."""
    r = api._clone_loglik_dm_host(Y, E, U, V, concentration=phi, const=False, with_scale=True)
    return (r["dm_ll"], r["scale"]) + const_of(Y)


def check(out, ref, scale, tag):
    assert out.shape == ref.shape, tag
    assert not np.isnan(out).any(), tag
    assert np.array_equal(np.isneginf(out), np.isneginf(ref)), tag
    ok = np.isfinite(ref)
    assert np.isfinite(out[ok]).all(), tag
    worst = float((np.abs(out[ok] - ref[ok]) / np.maximum(scale[ok], 1e-300)).max()) if ok.any() else 0.0
    print(f"clone_loglik_dm {tag}: max |dm - ref| / scale {worst:.2e}")
    assert worst <= RTOL, tag
    return worst


# (cells, genes, clones, concentrations): fewer cells than a block's waves and a row under one segment | exactly 64 slots | 100 slots: two blocks of slots, the
# second partly idle, and one column past a 2048 boundary | the largest grid
CASES = [(33, 77, 2, 1), (700, 1234, 8, 8), (300, 2049, 20, 5), (200, 300, 5, 16)]


@pytest.mark.parametrize("storage", ["u8", "u16", "f32"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[:3])) + f"k{c[3]}")
def test_parity_with_the_float64_restatement(case, storage):
    N, G, Cn, K = case
    Y, L, mu, _idx, rng = problem(N, G, Cn, storage, seed=N + G + Cn)
    Y = plant_counts(Y)
    if storage == "f32":
        assert (Y != np.floor(Y)).any()                              # non-integer counts: two lgamma whatever their size
    if storage == "u8":
        assert (Y > 255).any() and (Y == 255).any()                  # escapes and genuine 255s
    E = mu[:, None] * L
    assert (E > 0).all()
    U, V = factors(N, G, 3, rng)
    phi = grid_of(K)
    eng = engine_for(Y, L, storage)
    try:
        assert eng.info()["y_storage_name"] == storage
        rows = ref_rows(N)
        for D in (0, 1, 3):
            Uv, Vv = (None, None) if D == 0 else (U[:, :D], V[:, :D])
            ref, scale, const, cscale = reference(Y[rows], E, None if D == 0 else Uv[rows], Vv, phi)
            assert np.isfinite(ref).all()                            # L is in 1..4: no -inf in these cases
            for with_const in (True, False):
                r = eng.clone_loglik_dm(E, Uv, Vv, concentration=phi, const=with_const)
                assert np.isfinite(r["dm_ll"]).all()                 # (every cell, compared or not)
                want, sc = (ref + const[:, None, None], scale + cscale[:, None, None]) if with_const else (ref, scale)
                check(r["dm_ll"][rows], want, sc, f"{case} {storage} D={D} const={with_const}")
                assert np.array_equal(r["ll"], eng.clone_loglik(E, Uv, Vv, const=with_const))       # clone_loglik's rows, bit for bit
            again = eng.clone_loglik_dm(E, Uv, Vv, concentration=phi, const=False, want_ll=False)    # two calls: identical bits
            assert again["ll"] is None and np.array_equal(again["dm_ll"], r["dm_ll"])
    finally:
        eng.close()


@pytest.mark.parametrize("storage,D", [("u8", 0), ("u8", 2), ("f32", 2)])
def test_cell_ranges_return_the_full_call_bits(storage, D):
    N, G, Cn, K = 301, 600, 4, 3
    Y, L, mu, _idx, rng = problem(N, G, Cn, storage, seed=5)
    E = mu[:, None] * L
    U, V = factors(N, G, D, rng) if D else (None, None)
    phi = grid_of(K)
    eng = engine_for(Y, L, storage)
    try:
        full = eng.clone_loglik_dm(E, U, V, concentration=phi)
        parts = [eng.clone_loglik_dm(E, U, V, concentration=phi, cells=c) for c in ((0, 100), (100, 101), (101, N))]
        cut = eng.clone_loglik_dm(E, U, V, concentration=phi, cells=(5, 38))          # cuts inside a block's four waves at both ends
        none = eng.clone_loglik_dm(E, U, V, concentration=phi, cells=(7, 7))
        single = eng.clone_loglik_dm(E, U, V, concentration=phi[1:2])                 # a slot's value does not depend on the other slots of the call
    finally:
        eng.close()
    assert [p["dm_ll"].shape[0] for p in parts] == [100, 1, N - 101] and none["dm_ll"].shape == (0, Cn, K)
    assert np.array_equal(np.concatenate([p["dm_ll"] for p in parts]), full["dm_ll"])
    assert np.array_equal(np.concatenate([p["ll"] for p in parts]), full["ll"])
    assert np.array_equal(cut["dm_ll"], full["dm_ll"][5:38]) and np.array_equal(cut["ll"], full["ll"][5:38])
    assert np.array_equal(single["dm_ll"][:, :, 0], full["dm_ll"][:, :, 1])


@pytest.mark.parametrize("D", [0, 2])
def test_cells_with_one_read_are_multinomial_at_every_concentration(D):
    N, G, Cn, K = 120, 300, 5, 6
    Y, L, mu, _idx, rng = problem(N, G, Cn, "u8", seed=9)
    rows = np.arange(3, 103, 10)
    Y[rows] = 0
    Y[rows, rng.integers(G, size=rows.size)] = 1                     # ten cells with a single read
    E = mu[:, None] * L
    U, V = factors(N, G, D, rng) if D else (None, None)
    phi = grid_of(K)
    eng = engine_for(Y, L)
    try:
        r = eng.clone_loglik_dm(E, U, V, concentration=phi)
        ll = eng.clone_loglik(E, U, V)
    finally:
        eng.close()
    ref, scale, const, cscale = reference(Y, E, U, V, phi)
    assert (const[rows] == 0).all()
    check(r["dm_ll"][rows], np.repeat(ll[rows][:, :, None], K, axis=2), (scale + cscale[:, None, None])[rows], f"one read per cell, D={D}")
    check(r["dm_ll"], ref + const[:, None, None], scale + cscale[:, None, None], f"single reads among others, D={D}")


def test_zero_copy_number_empty_cells_and_extreme_exponents():
    """The construction of tests/test_gpu_pair_loglik.py: E = 0 in one clone, in two and in all of them against positive counts; a cell without counts;
    eta = +-800 on a few genes of one cell (exp(eta - max) underflows there: treated like E = 0, on the device and in the host form alike)."""
    N, G, Cn, K = 33, 77, 4, 3
    Y, L, mu, _idx, rng = problem(N, G, Cn, "u8", seed=7)
    L[5, :] = 0.0
    Y[:, 5] = 0                                                      # zero copy number against zero counts: contributes nothing
    L[7, 3] = 0.0
    Y[:, 7] = 0
    Y[11, 7] = 2                                                     # one clone without the gene
    L[9, 1] = L[9, 3] = 0.0
    Y[:, 9] = 0
    Y[12, 9] = 1                                                     # two clones without it
    L[13, :] = 0.0
    Y[:, 13] = 0
    Y[14, 13] = 3                                                    # no clone has it: -inf for every clone of that cell
    Y[20] = 0                                                        # a cell without counts (dense creation accepts it)
    E = mu[:, None] * L
    U, V = factors(N, G, 2, rng)
    U[:, 0] *= 0.002                                                 # (the other cells: |eta| of a few units on those genes, nothing underflows)
    U[21] = (1.0, 0.0)
    V[[3, 40, 60], 0] = 800.0                                        # eta = +-800 on a few genes of cell 21
    V[[4, 41], 0] = -800.0
    phi = grid_of(K)
    want = np.zeros((N, Cn, K), dtype=bool)
    want[11, 3] = want[12, 1] = want[12, 3] = want[14] = True
    eng = engine_for(Y, np.maximum(L, 1.0))
    try:
        for Uv, Vv in ((None, None), (U, V)):
            r = eng.clone_loglik_dm(E, Uv, Vv, concentration=phi)
            ref, scale, const, cscale = reference(Y, E, Uv, Vv, phi)
            inf = np.isneginf(ref)
            if Uv is None:
                assert np.array_equal(inf, want)
            else:                                                    # cell 21: its counts on the genes at eta = -800 (or far below +800) underflow in every clone
                assert np.array_equal(inf[np.arange(N) != 21], want[np.arange(N) != 21]) and (inf[21].all() or not inf[21].any())
            assert inf.mean() <= 0.5
            check(r["dm_ll"], ref + const[:, None, None], scale + cscale[:, None, None], f"zeros of E, D={0 if Uv is None else 2}")
            assert np.isfinite(r["dm_ll"][11, :3]).all() and np.isfinite(r["dm_ll"][12, [0, 2]]).all()
            ll = eng.clone_loglik(E, Uv, Vv)
            assert np.array_equal(r["ll"], ll)
            assert np.array_equal(np.isneginf(r["dm_ll"][np.arange(N) != 21, :, 0]), np.isneginf(ll[np.arange(N) != 21]))
            assert np.array_equal(r["dm_ll"][20], np.zeros((Cn, K))) and const[20] == 0.0          # s = 0: 0 + const_n, exactly
    finally:
        eng.close()


def test_a_concentration_beyond_the_product_bound_takes_two_lgamma_everywhere():
    """With a concentration above 2^100 in the call no count takes the product route; the other concentrations' values are the same numbers by another formula."""
    N, G, Cn = 64, 200, 3
    Y, L, mu, _idx, rng = problem(N, G, Cn, "u8", seed=3)
    Y = plant_counts(Y)
    E = mu[:, None] * L
    U, V = factors(N, G, 1, rng)
    phi = np.array([50.0, 2e3, 1e31])
    eng = engine_for(Y, L)
    try:
        gam = eng.clone_loglik_dm(E, U, V, concentration=phi)
        prod = eng.clone_loglik_dm(E, U, V, concentration=phi[:2])
    finally:
        eng.close()
    ref, scale, const, cscale = reference(Y, E, U, V, phi)
    check(gam["dm_ll"], ref + const[:, None, None], scale + cscale[:, None, None], "two lgamma everywhere")
    check(prod["dm_ll"], gam["dm_ll"][:, :, :2], (scale + cscale[:, None, None])[:, :, :2], "product route against two lgamma")


@pytest.mark.parametrize("storage", ["u8", "f32"])
def test_layouts_and_sparse_input(storage):
    import scipy.sparse as sps
    N, G, Cn, K = 400, 700, 5, 4
    Y, L, mu, _idx, rng = problem(N, G, Cn, storage, seed=12)
    E = mu[:, None] * L
    U, V = factors(N, G, 2, rng)
    phi = grid_of(K)
    outs = {}
    for lay in ("row", "col"):
        eng = engine_for(Y, L, storage, layout=lay)
        try:
            f = np.asfortranarray if lay == "col" else np.ascontiguousarray
            outs[lay] = [eng.clone_loglik_dm(f(E), f(U), f(V), concentration=phi, cells=(3, 390)), eng.clone_loglik_dm(f(E), concentration=phi)]
        finally:
            eng.close()
    for i in (0, 1):
        assert np.array_equal(outs["row"][i]["dm_ll"], outs["col"][i]["dm_ll"]) and np.array_equal(outs["row"][i]["ll"], outs["col"][i]["ll"])
    for fmt in (sps.csr_matrix, sps.csc_matrix):
        eng = engine_for(fmt(Y), L, storage)
        try:
            assert np.array_equal(eng.clone_loglik_dm(E, U, V, concentration=phi, cells=(3, 390))["dm_ll"], outs["row"][0]["dm_ll"]), fmt.__name__
        finally:
            eng.close()


@pytest.mark.parametrize("world", [2, 3])
def test_group_returns_the_single_handle_bits(world):
    from clonealign_amd.engine import EngineError, HipGroupEngine
    N, G, Cn, K = 501, 700, 8, 4
    Y, L, mu, _idx, rng = problem(N, G, Cn, "u8", seed=31)
    E = mu[:, None] * L
    U, V = factors(N, G, 1, rng)
    phi = grid_of(K)
    one = engine_for(Y, L)
    try:
        o1 = [one.clone_loglik_dm(E, U, V, concentration=phi), one.clone_loglik_dm(E, concentration=phi), one.clone_loglik_dm(E, U, V, concentration=phi, cells=(100, 400))]
    finally:
        one.close()
    grp = HipGroupEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, devices=[0] * world)
    try:
        og = [grp.clone_loglik_dm(E, U, V, concentration=phi), grp.clone_loglik_dm(E, concentration=phi), grp.clone_loglik_dm(E, U, V, concentration=phi, cells=(100, 400))]
        bad = U.copy()
        bad[N - 1, 0] = np.nan                                       # refused on one rank's cells: refused by the group, which stays usable
        with pytest.raises(EngineError) as ex:
            grp.clone_loglik_dm(E, bad, V, concentration=phi)
        assert ex.value.code == 1 and "U has a non-finite entry" in ex.value.msg, ex.value.msg
        with pytest.raises(EngineError) as ex:
            grp.clone_loglik_dm(E, U, V, concentration=phi, cells=(400, N + 1))
        assert ex.value.code == 1 and "cell range" in ex.value.msg, ex.value.msg
        with pytest.raises(EngineError) as ex:
            grp.clone_loglik_dm(E, U, V, concentration=(10.0, -2.0))
        assert ex.value.code == 1 and "concentration 1" in ex.value.msg, ex.value.msg
        assert np.array_equal(grp.clone_loglik_dm(E, U, V, concentration=phi, cells=(100, 400))["dm_ll"], og[2]["dm_ll"])
    finally:
        grp.close()
    for a, b in zip(o1, og):
        assert np.array_equal(a["dm_ll"], b["dm_ll"]) and np.array_equal(a["ll"], b["ll"])


def test_the_call_changes_nothing_in_a_running_fit_and_is_refused_from_a_poll_hook():
    """Five iterations, clone_loglik_dm, five more == ten iterations straight, bit for bit: every variable and the ELBO."""
    from clonealign_amd.engine import EngineError, HipEngine
    from clonealign_amd.rng import EpsStream
    case = make_case(N=900, G=500, C=4, K=1, seed=21)
    N, G = case["Y"].shape
    eps = np.stack([eps_for(1, G, 100 + i) for i in range(20)])
    rng = np.random.default_rng(1)
    U, V = factors(N, G, 1, rng)
    phi = grid_of(3)
    a = HipEngine(**case)
    try:
        ea = a.iterate(10, eps)
        sa = a.get_state()
    finally:
        a.close()
    b = HipEngine(**case)
    try:
        b.iterate(5, eps[:10])
        out = b.clone_loglik_dm(case["L"], U, V, concentration=phi)
        b.clone_loglik_dm(case["L"], concentration=phi)
        ref, scale, const, cscale = reference(case["Y"], case["L"], U, V, phi)
        check(out["dm_ll"], ref + const[:, None, None], scale + cscale[:, None, None], "mid-fit")
        eb = b.iterate(5, eps[10:])
        sb = b.get_state()
        seen = {}

        def hook(i, e):
            if i == 2:
                with pytest.raises(EngineError) as ex:
                    b.clone_loglik_dm(case["L"], concentration=phi)
                seen["code"] = ex.value.code
            return False
        b.run(EpsStream(9, 1, G), 4, 1e-12, poll=hook)
        assert seen["code"] == 6                                     # CA_ERR_STATE
    finally:
        b.close()
    assert ea == eb
    for n in sa:
        assert np.array_equal(sa[n], sb[n]), n


def test_refusals_through_the_c_abi_name_the_offender():
    N, G, Cn = 120, 90, 3
    Y, L, mu, _idx, rng = problem(N, G, Cn, "u8", seed=2)
    E = np.ascontiguousarray(mu[:, None] * L)
    U, V = factors(N, G, 2, rng)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    eng = engine_for(Y, L)
    try:
        ll, dm = np.zeros((N, Cn)), np.zeros((N, Cn * 16))
        good = eng.clone_loglik_dm(E, U, V, concentration=(3.0, 300.0))

        def refused(words, E_=E, phi=(3.0, 300.0), nk=None, lo=0, cnt=N, out=dm, D=0, U_=None, V_=None, null_conc=False):
            pv = np.asarray(phi, dtype=np.float64)
            rc = eng.lib.ca_clone_loglik_dm(eng.h, ptr(E_), ptr(U_), ptr(V_), D, 1, None if null_conc else ptr(pv), len(pv) if nk is None else nk, lo, cnt, ptr(ll), ptr(out))
            msg = eng.lib.ca_last_error(eng.h).decode()
            assert rc == 1 and all(x in msg for x in words), (rc, msg)
            again = eng.clone_loglik_dm(E, U, V, concentration=(3.0, 300.0))              # after each refusal the handle still serves a valid call
            assert np.array_equal(again["dm_ll"], good["dm_ll"])
        for bad in (0.0, -1.0, np.nan, np.inf, -np.inf):
            refused(("ca_clone_loglik_dm", "concentration 1"), phi=(5.0, bad))
        refused(("concentration 0", "1e300"), phi=(1e301,))
        refused(("n_conc = 0", "[1, 16]"), nk=0)
        refused(("n_conc = 17", "[1, 16]"), phi=np.geomspace(1, 1e5, 17))
        refused(("cell range", f"[0, {N}]"), lo=100, cnt=21)
        refused(("cell range",), lo=-1, cnt=5)
        refused(("cell range",), lo=0, cnt=-1)
        refused(("dm_ll is NULL",), out=None)
        refused(("conc is NULL",), null_conc=True)
        refused(("E is NULL",), E_=None)
        Eb = E.copy()
        Eb[17, 2] = -1.0
        refused(("gene 17", "clone 2"), E_=Eb)
        Ub = U.copy()
        Ub[9, 1] = np.nan
        refused(("U has a non-finite", "cell 9"), D=2, U_=Ub, V_=V)
        refused(("D = 9", "outside [0, 8]"), D=9, U_=U, V_=V)
        refused(("needs both U",), D=2, V_=V)
        with pytest.raises(ValueError):
            eng.clone_loglik_dm(E[:-1])
        ref, scale, const, cscale = reference(Y, E, U, V, (3.0, 300.0))
        check(good["dm_ll"], ref + const[:, None, None], scale + cscale[:, None, None], "beside the refusals")
    finally:
        eng.close()


def test_assign_cells_dm_on_the_device():
    import clonealign_amd as ca
    Y, L, fit, _truth = planted(0)
    N, G = Y.shape
    dev = ca.assign_cells_dm(fit, Y, L, concentration="auto", grid=GRID, refine=0)
    host = ca.assign_cells_dm(fit, Y, L, concentration="auto", grid=GRID, refine=0, engine=HostOnly(N, G))
    assert dev["concentration"] == 100.0 and host["concentration"] == 100.0 and not dev["concentration_estimate"]["at_edge"]
    d = float(np.abs(dev["clone_probs"] - host["clone_probs"]).max())
    print(f"assign_cells_dm: device vs host clone_probs max abs {d:.2e}; marginal log-likelihoods {dev['concentration_estimate']['marginal_loglik']}")
    assert d <= 1e-9
    assert np.array_equal(dev["clone"], host["clone"]) and dev["n_calls_changed"] == host["n_calls_changed"]
    np.testing.assert_allclose(dev["concentration_estimate"]["marginal_loglik"], host["concentration_estimate"]["marginal_loglik"], rtol=1e-10)
    fit["ml_params"]["W"] = np.random.default_rng(2).normal(size=(G, 1)) * 0.05       # the route with an exponent term (D = 1), refined
    fit["ml_params"]["psi"] = np.random.default_rng(3).normal(size=(N, 1))
    dev = ca.estimate_concentration(fit, Y, L, psi="fit")
    host = ca.estimate_concentration(fit, Y, L, psi="fit", engine=HostOnly(N, G))
    assert dev["concentration"] == host["concentration"] and dev["grid"].shape == (24,)
    np.testing.assert_allclose(dev["marginal_loglik"], host["marginal_loglik"], rtol=1e-10)
    r = ca.clone_loglik_dm(fit, Y, L, concentration=[100.0, 1e3], psi="fit")
    assert r["dm_ll"].shape == (N, 4, 2) and r["ll"].shape == (N, 4)
