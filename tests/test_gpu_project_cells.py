"""ca_project_cells / HipEngine.project_cells / project_cells: per-cell MAP psi of the resident cells under a fit's gene-level parameters and the clone posterior
at it (generalised EM, one safeguarded Newton step per round; include/clonealign_hip.h states the algorithm).

The yardstick is ``api._project_cells_host``, the algorithm restated step for step in numpy float64.  Bars:
  rounds, converged: equal exactly.  A cell whose rounds differ by ONE may be left out when its deciding step sits within 1e-3 (relative) of tol -- it froze in one
    run and went one more round in the other, both to the same psi; at most 0.5 % of a case's cells, the share is printed.  The seeds are such that the
    restatement run on the genes in reversed order (another grouping of every sum) leaves out none.
  ll, objective: tests/test_gpu_clone_loglik.py's rule, |out - ref| <= 1e-10 * scale with scale the sum of the terms' magnitudes.
  psi, clone_probs: max |psi_dev - psi_ref| / max(1, |psi_ref|) was MEASURED over the cases below (every shape, storage, K in {1, 2}, P in {0, 1}): the largest
    value is PSI_MEASURED = 7.0e-11 (printed per case by the test; by shape and storage: 33 x 77 x 2 1.3e-14 / 1.8e-14 / 2.1e-14 for u8 / u16 / f32,
    3000 x 1234 x 8 3.9e-11 / 5.2e-11 / 9.4e-16, 700 x 2049 x 20 7.0e-11 / 5.4e-11 / 5.8e-16 -- the u8 / u16 problems carry escaped counts up to 70000, so
    their cells sit in the clipped rounds longest); no cell was left out in any case.  The bar is 100 x that, 7.0e-9, and never looser than 1e-8.  The margin covers the different grouping of the
    float64 sums between the device and numpy: the Newton map contracts errors near the fixed point but not in the clipped early rounds.  clone_probs is held
    to the same bar (absolute: it is a probability), after the left-out cells are removed."""
import numpy as np
import pytest

from clonealign_amd.api import _project_cells_host
from tests._cases import eps_for, make_case
from tests.test_gpu_clone_loglik import ref_ll
from tests.test_gpu_fit_mse import problem

pytestmark = pytest.mark.gpu
RTOL = 1e-10
PSI_MEASURED = 7.02e-11       # largest max |psi_dev - psi_ref| / max(1, |psi_ref|) over the parity cases (see the docstring)
PSI_TOL = min(100 * PSI_MEASURED, 1e-8)
SHAPES = [(33, 77, 2), (3000, 1234, 8), (700, 2049, 20)]
KEYS = ("psi", "ll", "clone_probs", "objective", "rounds", "converged")


def operands(N, G, C, K, P, rng):
    V = rng.normal(size=(G, K + P)) * 0.3
    X = rng.normal(size=(N, P)) * 0.5 if P else None
    lp = np.log(rng.dirichlet(np.full(C, 5.0)))[None] + rng.normal(size=(N, C)) * 0.1
    return V, X, lp


def same_bits(a, b, tag=""):
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (tag, k)


def compare(dev, ref, Y, E, V, K, X, tol, tag):
    """The bars of the docstring; returns the measured psi figure."""
    N = dev["psi"].shape[0]
    diff = dev["rounds"].astype(np.int64) - ref["rounds"]
    out = np.flatnonzero((diff != 0) | (dev["converged"] != ref["converged"]))
    print(f"project_cells {tag}: left out {out.size} of {N} cells ({out.size / N:.4%}); rounds up to {int(ref['rounds'].max())}, "
          f"converged {ref['converged'].mean():.4f}")
    assert out.size <= 0.005 * N, tag
    if out.size:                                                      # only a step within 1e-3 of tol excuses a cell: one round apart, the same psi
        assert (np.abs(diff[out]) == 1).all(), tag
        assert (np.abs(dev["psi"][out] - ref["psi"][out]).max(1) <= tol * (1 + 1e-3)).all(), tag
    keep = np.setdiff1d(np.arange(N), out)
    fig = float((np.abs(dev["psi"] - ref["psi"]) / np.maximum(1.0, np.abs(ref["psi"])))[keep].max()) if K else 0.0
    dp = float(np.abs(dev["clone_probs"] - ref["clone_probs"])[keep].max())
    U = np.concatenate([ref["psi"]] + ([X] if X is not None else []), axis=1)
    _ll, scale = ref_ll(Y, E, U if U.shape[1] else None, V if U.shape[1] else None)
    dl = float((np.abs(dev["ll"] - ref["ll"]) / scale)[keep].max())
    do = float((np.abs(dev["objective"] - ref["objective"]) / scale.max(1))[keep].max())
    print(f"project_cells {tag}: max |psi - ref| / max(1, |ref|) {fig:.2e}, clone_probs {dp:.2e}, ll / scale {dl:.2e}, objective / scale {do:.2e}")
    assert fig <= PSI_TOL and dp <= PSI_TOL, tag
    assert dl <= RTOL and do <= RTOL, tag
    return fig


@pytest.mark.parametrize("storage", ["u8", "u16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_with_the_float64_restatement(shape, storage):
    from clonealign_amd.engine import HipEngine
    N, G, C = shape
    Y, L, mu, _idx, rng = problem(N, G, C, storage, seed=sum(shape))
    E = mu[:, None] * L
    eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, y_storage=storage)
    worst = 0.0
    try:
        assert eng.info()["y_storage_name"] == storage
        for K in (1, 2):
            for P in (0, 1):
                V, X, lp = operands(N, G, C, K, P, rng)
                dev = eng.project_cells(E, V, K, X=X, log_prior=lp)
                ref = _project_cells_host(Y, E, V, K, P, X, lp, None)
                worst = max(worst, compare(dev, ref, Y, E, V, K, X, 1e-9, f"{shape} {storage} K={K} P={P}"))
                same_bits(eng.project_cells(E, V, K, X=X, log_prior=lp), dev)      # two calls: identical bits
    finally:
        eng.close()
    print(f"project_cells {shape} {storage}: largest psi figure {worst:.2e}")


def test_zero_copy_number_and_extreme_exponents():
    from clonealign_amd.engine import HipEngine
    N, G, C = 3000, 1234, 8
    Y, L, mu, _idx, rng = problem(N, G, C, "u8", seed=7)
    L[5, :] = 0.0
    Y[:, 5] = 0                                                      # zero copy number against zero counts: contributes nothing
    L[7, 3] = 0.0
    Y[:, 7] = 0
    Y[11, 7] = 2                                                     # one cell with a positive count where one clone has none
    L[9, :] = 0.0
    Y[:, 9] = 0
    Y[13, 9] = 1                                                     # ... and one where no clone has any: the cell is impossible
    E = mu[:, None] * L
    V, _X, lp = operands(N, G, C, 1, 0, rng)
    V[[3, 40, 60], 0] = 700.0                                        # eta = +-700 on a few genes of every cell that starts at psi = 1
    V[[4, 41], 0] = -700.0
    start = np.zeros((N, 1))
    start[20:30] = 1.0
    start[13] = 0.25
    lp[15, 2] = -np.inf                                              # a clone excluded through the prior
    eng = HipEngine(Y, np.maximum(L, 1.0), np.zeros((N, 0)), np.zeros(G), 0)
    try:
        dev = eng.project_cells(E, V, 1, log_prior=lp, psi_start=start, max_iter=6)
        ref = _project_cells_host(Y, E, V, 1, 0, None, lp, start, max_iter=6)
    finally:
        eng.close()
    assert np.array_equal(np.isneginf(dev["ll"]), np.isneginf(ref["ll"])) and np.isneginf(dev["ll"][11, 3]) and np.isneginf(dev["ll"][13]).all()
    assert dev["clone_probs"][11, 3] == 0.0 and dev["clone_probs"][15, 2] == 0.0
    assert np.isnan(dev["clone_probs"][13]).all() and dev["psi"][13, 0] == 0.25 and dev["rounds"][13] == 0 and not dev["converged"][13]
    rest = np.setdiff1d(np.arange(N), [13])
    assert not np.isnan(dev["ll"]).any() and np.isfinite(dev["psi"]).all()
    assert np.isfinite(dev["clone_probs"][rest]).all() and np.isfinite(dev["objective"][rest]).all()
    # clone_probs = exp(t - lse) as in assign_cells: t and lse are of the size of ll (1e5 .. 1e6 with this problem's escaped counts), so their difference
    # carries a few units of 2^-53 |ll|, and a row's sum is 1 to within that -- not to within 2^-53
    big = np.where(np.isfinite(dev["ll"]), np.abs(dev["ll"]), 0.0).max(1)[rest]
    assert (np.abs(dev["clone_probs"][rest].sum(1) - 1.0) <= 8 * 2.0 ** -53 * big + 1e-14).all()
    assert np.array_equal(dev["rounds"], ref["rounds"]) and np.array_equal(dev["converged"], ref["converged"])
    fig = float((np.abs(dev["psi"] - ref["psi"]) / np.maximum(1.0, np.abs(ref["psi"]))).max())
    print(f"project_cells zeros of E and eta = +-700: psi figure {fig:.2e}")
    assert fig <= PSI_TOL


@pytest.mark.parametrize("storage", ["u8", "f32"])
def test_layouts_selections_and_sparse_input(storage):
    import scipy.sparse as sps
    from clonealign_amd.engine import HipEngine
    N, G, C = 1500, 700, 5
    Y, L, mu, _idx, rng = problem(N, G, C, storage, seed=12)
    E = mu[:, None] * L
    V, X, lp = operands(N, G, C, 2, 1, rng)
    start = rng.normal(size=(N, 2)) * 0.3
    outs = {}
    for lay in ("row", "col"):
        eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, y_storage=storage, layout=lay)
        try:
            f = np.asfortranarray if lay == "col" else np.ascontiguousarray
            outs[lay] = eng.project_cells(f(E), f(V), 2, X=f(X), log_prior=f(lp), psi_start=f(start))
        finally:
            eng.close()
    compare(outs["row"], _project_cells_host(Y, E, V, 2, 1, X, lp, start), Y, E, V, 2, X, 1e-9, f"layout row {storage}")
    same_bits(outs["row"], outs["col"], "col")
    for fmt in (sps.csr_matrix, sps.csc_matrix):
        eng = HipEngine(fmt(Y), L, np.zeros((N, 0)), np.zeros(G), 0, y_storage=storage)
        try:
            same_bits(eng.project_cells(E, V, 2, X=X, log_prior=lp, psi_start=start), outs["row"], fmt.__name__)
        finally:
            eng.close()
    ci = np.sort(rng.choice(N, 1100, replace=False)).astype(np.int64)
    gi = np.sort(rng.choice(G, 515, replace=False)).astype(np.int32)
    sel = HipEngine(Y, L[gi], np.zeros((1100, 0)), np.zeros(515), 0, y_storage=storage, cell_index=ci, gene_index=gi)
    dense = HipEngine(np.ascontiguousarray(Y[np.ix_(ci, gi)]), L[gi], np.zeros((1100, 0)), np.zeros(515), 0, y_storage=storage)
    try:
        a = sel.project_cells(E[gi], V[gi], 2, X=X[ci], log_prior=lp[ci], psi_start=start[ci])
        b = dense.project_cells(E[gi], V[gi], 2, X=X[ci], log_prior=lp[ci], psi_start=start[ci])
    finally:
        sel.close()
        dense.close()
    same_bits(a, b, "cell_index / gene_index")


@pytest.mark.parametrize("builtin", [True, False])
def test_the_call_changes_nothing_in_a_running_fit(builtin):
    """Five iterations, project_cells, five more == ten iterations straight, bit for bit: every variable and the ELBO."""
    from clonealign_amd.engine import HipEngine
    case = make_case(N=2600, G=640, C=5, K=1, seed=21)
    G = case["Y"].shape[1]
    eps = None if builtin else np.stack([eps_for(1, G, 100 + i) for i in range(20)])
    rng = np.random.default_rng(1)
    V, _X, lp = operands(2600, G, 5, 1, 0, rng)
    a = HipEngine(**case)
    try:
        ea = a.iterate(10, eps)
        sa = a.get_state()
    finally:
        a.close()
    b = HipEngine(**case)
    try:
        b.iterate(5, None if builtin else eps[:10])
        out = b.project_cells(case["L"], V, 1, log_prior=lp)
        compare(out, _project_cells_host(case["Y"], case["L"], V, 1, 0, None, lp, None), case["Y"], case["L"], V, 1, None, 1e-9, "mid-fit")
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
    V, X, lp = operands(N, G, C, 2, 1, rng)
    start = rng.normal(size=(N, 2)) * 0.3
    one = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0)
    try:
        o1 = one.project_cells(E, V, 2, X=X, log_prior=lp, psi_start=start)
    finally:
        one.close()
    grp = HipGroupEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, devices=[0] * world)
    try:
        og = grp.project_cells(E, V, 2, X=X, log_prior=lp, psi_start=start)
        bad = X.copy()
        bad[N - 1, 0] = np.nan                                       # refused on one rank's cells: refused by the group, which stays usable
        with pytest.raises(EngineError) as ex:
            grp.project_cells(E, V, 2, X=bad, log_prior=lp, psi_start=start)
        assert ex.value.code == 1 and "X has a non-finite entry" in ex.value.msg, ex.value.msg
        same_bits(grp.project_cells(E, V, 2, X=X, log_prior=lp, psi_start=start), og, "again")
    finally:
        grp.close()
    same_bits(og, o1, f"group of {world}")


def test_two_calls_agree_and_the_host_polling_changes_nothing():
    from clonealign_amd.engine import HipEngine
    N, G, C = 3000, 1234, 8
    Y, L, mu, _idx, rng = problem(N, G, C, "u8", seed=41)
    E = mu[:, None] * L
    V, _X, lp = operands(N, G, C, 1, 0, rng)
    eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0)
    try:
        base = eng.project_cells(E, V, 1, log_prior=lp)
        same_bits(eng.project_cells(E, V, 1, log_prior=lp), base, "second call")
        for every in (1, 3, 255):                                    # after every round, every third, never
            same_bits(eng.project_cells(E, V, 1, log_prior=lp, poll_every=every), base, f"poll_every={every}")
    finally:
        eng.close()


def test_project_cells_through_the_api():
    import clonealign_amd as ca
    from tests.test_project_cells_host import HostOnly, planted
    p = planted(2400, 400, 3, 1, 1.0, 17, depth=300)
    Y, L, z = p["Y"], p["L"], p["z"]
    G = Y.shape[1]
    names = ["a", "b", "c"]
    lut = np.asarray(names, dtype=object)
    fit = ca.ClonealignFit(ml_params={"mu": p["mu"], "alpha": p["alpha"], "W": p["W"]}, clone_names=names)
    dev = ca.project_cells(fit, Y[:600], L, saturate=False)
    host = ca.project_cells(fit, Y[:600], L, saturate=False, engine=HostOnly(600, G))
    d = float(np.abs(dev["clone_probs"] - host["clone_probs"]).max())
    print(f"project_cells: device vs host clone_probs max abs {d:.2e}, psi {float(np.abs(dev['psi'] - host['psi']).max()):.2e}")
    assert d <= PSI_TOL and np.array_equal(dev["clone"], host["clone"]) and np.array_equal(dev["rounds"], host["rounds"])
    np.testing.assert_allclose(dev["loglik"], host["loglik"], rtol=1e-10)
    np.testing.assert_allclose(dev["psi"], host["psi"], rtol=0, atol=PSI_TOL)
    assert np.array_equal(ca.recompute_clone_assignment(dev, 0.5)["clone"], ca.clone_assignment(dev["clone_probs"], names, 0.5))
    with pytest.raises(ValueError, match="K <= 2"):
        ca.project_cells(ca.ClonealignFit(ml_params={"mu": p["mu"], "alpha": p["alpha"], "W": np.zeros((G, 3))}, clone_names=names), Y[:600], L)
    # after a real fit on half of the cells: the held-out half, drawn from the same model, is placed at least as well as at psi = 0
    res = ca.clonealign(Y[:1200], L, max_iter=60, verbose=False, seed=3)
    from clonealign_amd.api import _default_gene_names
    at = {g: i for i, g in enumerate(_default_gene_names(G))}
    rg = np.array([at[g] for g in res["retained_genes"]])            # (the fit's gene-level parameters belong to these genes)
    new = ca.project_cells(res, Y[1200:][:, rg], L[rg], 0.0)
    old = ca.assign_cells(res, Y[1200:][:, rg], L[rg], 0.0)
    share_new, share_old = float((new["clone"] == lut[z[1200:]]).mean()), float((old["clone"] == lut[z[1200:]]).mean())
    print(f"held-out cells after clonealign(): labels right with the projected psi {share_new:.4f}, at psi = 0 {share_old:.4f}; "
          f"converged {new['converged'].mean():.4f}, rounds up to {int(new['rounds'].max())}")
    assert share_new >= share_old


def test_refusals_name_the_offender_and_poll_hooks_are_refused():
    import ctypes as C
    from clonealign_amd.engine import EngineError, HipEngine
    from clonealign_amd.rng import EpsStream
    case = make_case(N=700, G=300, C=4, K=1, seed=2)
    L = case["L"]
    rng = np.random.default_rng(0)
    V, X, lp = operands(700, 300, 4, 1, 1, rng)
    eng = HipEngine(**case)
    try:
        def refused(words, *a, **k):
            with pytest.raises(EngineError) as ex:
                eng.project_cells(*a, **k)
            assert ex.value.code == 1 and all(w in ex.value.msg for w in words), ex.value.msg
        E = L.copy()
        E[17, 2] = -1.0
        refused(("gene 17", "clone 2"), E, V, 1, X=X)
        E = L.copy()
        E[:, 1] = 0.0
        refused(("clone 1", "sums to"), E, V, 1, X=X)
        Vb = V.copy()
        Vb[33, 0] = -np.inf
        refused(("V has a non-finite", "gene 33"), L, Vb, 1, X=X)
        Xb = X.copy()
        Xb[9, 0] = np.nan
        refused(("X has a non-finite", "cell 9"), L, V, 1, X=Xb)
        st = np.zeros((700, 1))
        st[8, 0] = np.inf
        refused(("psi_start has a non-finite", "cell 8"), L, V, 1, X=X, psi_start=st)
        for bad in (np.inf, np.nan):
            lb = lp.copy()
            lb[6, 2] = bad
            refused(("log_prior", "cell 6", "clone 2"), L, V, 1, X=X, log_prior=lb)
        refused(("K = 3", "[0, 2]"), L, np.zeros((300, 3)), 3)
        refused(("K + P = 9", "[0, 8]"), L, np.zeros((300, 9)), 1, X=np.zeros((700, 8)))
        refused(("max_iter = -1",), L, V, 1, X=X, max_iter=-1)
        for bad in (0.0, -1.0, np.inf, np.nan):
            refused(("tol",), L, V, 1, X=X, tol=bad)
            refused(("max_step",), L, V, 1, X=X, max_step=bad)
        out = [np.zeros((700, 4)) for _ in range(3)] + [np.zeros(700), np.zeros(700, dtype=np.int32), np.zeros(700, dtype=np.uint8)]
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        Lc = np.ascontiguousarray(L)
        rc = eng.lib.ca_project_cells(eng.h, ptr(Lc), None, 1, 0, None, None, None, 1, 25, 1e-9, 1.0, *[ptr(a) for a in out])
        assert rc == 1 and b"needs V" in eng.lib.ca_last_error(eng.h)
        rc = eng.lib.ca_project_cells(eng.h, ptr(Lc), ptr(V), 1, 1, None, None, None, 1, 25, 1e-9, 1.0, *[ptr(a) for a in out])
        assert rc == 1 and b"needs X" in eng.lib.ca_last_error(eng.h)
        with pytest.raises(ValueError):
            eng.project_cells(L[:-1], V, 1, X=X)
        with pytest.raises(ValueError):
            eng.project_cells(L, V, 1, X=X[:-1])
        seen = {}

        def hook(i, e):
            if i == 2:
                with pytest.raises(EngineError) as ex:
                    eng.project_cells(L, V, 1, X=X)
                seen["code"] = ex.value.code
            return False
        eng.run(EpsStream(9, 1, 300), 4, 1e-12, poll=hook)
        assert seen["code"] == 6                                     # CA_ERR_STATE
        compare(eng.project_cells(L, V, 1, X=X, log_prior=lp), _project_cells_host(case["Y"], L, V, 1, 1, X, lp, None), case["Y"], L, V, 1, X, 1e-9,
                "after the run")
    finally:
        eng.close()
