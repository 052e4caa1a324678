"""ca_clone_evidence / HipEngine.clone_evidence / clone_evidence: per (cell, clone) the evidence with psi integrated out -- a safeguarded Newton mode, the
Laplace value and a quadrature at the caller's rule (include/clonealign_hip.h states the algorithm).

The yardstick is ``api._clone_evidence_host``, the algorithm restated step for step in numpy float64.  Bars:
  rounds, converged: equal exactly.  A pair whose rounds differ by ONE may be left out when its deciding step sits within 1e-3 (relative) of tol -- it froze in
    one run and went one more round in the other, both to the same psi; at most 0.5 % of a case's pairs, the share is printed.
  evidence, laplace: tests/test_gpu_clone_loglik.py's rule, |dev - ref| <= 1e-10 * scale with scale the sum of the terms' magnitudes at the pair's mode.
  psi_mode, psi_prec: max |dev - ref| / max(1, |ref|) was MEASURED over the parity cases below (every shape, storage, K in {1, 2}, P in {0, 1}): the largest
    value is PSI_MEASURED = 9.24e-12 (printed per case by the test; by shape and storage: 33 x 77 x 2 2.3e-14 / 3.9e-12 / 1.6e-15 for u8 / u16 / f32,
    400 x 1234 x 8 9.2e-12 / 1.8e-12 / 1.8e-14, 150 x 2049 x 20 3.1e-12 / 2.0e-12 / 2.6e-14 -- the largest values are K = 2 cases of the u8 / u16 problems,
    whose escaped counts keep pairs in the clipped rounds longest); no pair was left out in any case, and evidence / laplace measured at most 4.5e-15 of
    scale.  The bar is 100 x that, 9.24e-10, and never looser than 1e-8.  The margin covers the different grouping of the
    float64 sums between the device and numpy: the Newton map contracts errors near the fixed point but not in the clipped early rounds."""
import numpy as np
import pytest

from clonealign_amd.api import _clone_evidence_host, gauss_hermite_rule
from tests.test_gpu_clone_loglik import ref_ll
from tests.test_gpu_fit_mse import problem
from tests.test_gpu_project_cells import operands

pytestmark = pytest.mark.gpu
RTOL = 1e-10
PSI_MEASURED = 9.24e-12       # largest max |dev - ref| / max(1, |ref|) of psi_mode and psi_prec over the parity cases (see the docstring)
PSI_TOL = min(100 * PSI_MEASURED, 1e-8)
SHAPES = [(33, 77, 2), (400, 1234, 8), (150, 2049, 20)]
KEYS = ("evidence", "laplace", "psi_mode", "psi_prec", "rounds", "converged")
EDGE = (400, 1234, 8)


def rule(K):
    return gauss_hermite_rule(K, 8 if K == 1 else 3)


def same_bits(a, b, tag=""):
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (tag, k)


def compare(dev, ref, Y, E, V, K, X, tol, tag):
    """The bars of the docstring; returns the measured psi figure."""
    N, C = ref["evidence"].shape
    diff = dev["rounds"].astype(np.int64) - ref["rounds"]
    out = (diff != 0) | (dev["converged"] != ref["converged"])
    print(f"clone_evidence {tag}: left out {int(out.sum())} of {N * C} pairs ({out.mean():.4%}); rounds up to {int(ref['rounds'].max())}, "
          f"converged {ref['converged'].mean():.4f}")
    assert out.sum() <= 0.005 * N * C, tag
    if out.any():                                                     # only a step within 1e-3 of tol excuses a pair: one round apart, the same psi
        assert (np.abs(diff[out]) == 1).all(), tag
        assert (np.abs(dev["psi_mode"][out] - ref["psi_mode"][out]).max(1) <= tol * (1 + 1e-3)).all(), tag
    keep = ~out
    assert np.array_equal(np.isneginf(dev["evidence"]), np.isneginf(ref["evidence"])) and np.array_equal(np.isneginf(dev["laplace"]), np.isneginf(ref["laplace"])), tag
    assert not np.isnan(dev["evidence"]).any() and not np.isnan(dev["laplace"]).any(), tag
    fig = 0.0
    for k in ("psi_mode", "psi_prec"):
        fig = max(fig, float((np.abs(dev[k] - ref[k]) / np.maximum(1.0, np.abs(ref[k])))[keep].max()))
    scale = np.empty((N, C))
    for c in range(C):                                                # the terms' magnitudes at the pair's own mode
        U = np.concatenate([ref["psi_mode"][:, c]] + ([X] if X is not None else []), axis=1)
        scale[:, c] = ref_ll(Y, E, U, V)[1][:, c]
    fin = keep & np.isfinite(ref["evidence"])
    de = float((np.abs(dev["evidence"] - ref["evidence"])[fin] / scale[fin]).max())
    dl = float((np.abs(dev["laplace"] - ref["laplace"])[fin] / scale[fin]).max())
    print(f"clone_evidence {tag}: max |psi - ref| / max(1, |ref|) {fig:.2e}, evidence / scale {de:.2e}, laplace / scale {dl:.2e}")
    assert fig <= PSI_TOL, tag
    assert de <= RTOL and dl <= RTOL, tag
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
                V, X, _lp = operands(N, G, C, K, P, rng)
                nd, wt = rule(K)
                dev = eng.clone_evidence(E, V, K, X=X, nodes=nd, weights=wt, max_iter=100)
                ref = _clone_evidence_host(Y, E, V, K, P, X, None, nd, wt, max_iter=100)
                worst = max(worst, compare(dev, ref, Y, E, V, K, X, 1e-9, f"{shape} {storage} K={K} P={P}"))
                if shape == (33, 77, 2) and storage == "u16" and K == 2 and P == 0:
                    # two pairs whose steps are clipped and whose mode is far: not converged in 100 rounds, the same flags, a finite (untrusted) value
                    assert (~ref["converged"]).sum() == 2 and np.array_equal(dev["converged"], ref["converged"])
                    assert np.isfinite(dev["evidence"][~dev["converged"]]).all() and (dev["rounds"][~dev["converged"]] == 100).all()
    finally:
        eng.close()
    print(f"clone_evidence {shape} {storage}: largest psi figure {worst:.2e}")


@pytest.fixture(scope="module")
def edge():
    """One engine on the (400, 1234, 8) u8 problem with K = 1, P = 1 operands, and its first answer."""
    from clonealign_amd.engine import HipEngine
    N, G, C = EDGE
    Y, L, mu, _idx, rng = problem(N, G, C, "u8", seed=41)
    E = mu[:, None] * L
    V, X, _lp = operands(N, G, C, 1, 1, rng)
    nd, wt = rule(1)
    eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0)
    try:
        base = eng.clone_evidence(E, V, 1, X=X, nodes=nd, weights=wt)
        yield dict(eng=eng, Y=Y, L=L, E=E, V=V, X=X, nd=nd, wt=wt, base=base, rng=rng)
    finally:
        eng.close()


def test_two_calls_agree_and_the_host_polling_changes_nothing(edge):
    e = edge
    same_bits(e["eng"].clone_evidence(e["E"], e["V"], 1, X=e["X"], nodes=e["nd"], weights=e["wt"]), e["base"], "second call")
    for every in (1, 255):                                           # after every round, never
        same_bits(e["eng"].clone_evidence(e["E"], e["V"], 1, X=e["X"], nodes=e["nd"], weights=e["wt"], poll_every=every), e["base"], f"poll_every={every}")
    one = e["eng"].clone_evidence(e["E"], e["V"], 1, X=e["X"])      # the single node 0: the Laplace value, bit for bit
    assert np.array_equal(one["evidence"], one["laplace"]) and np.array_equal(one["laplace"], e["base"]["laplace"])


def test_sparse_created_engines_return_the_dense_bits(edge):
    import scipy.sparse as sps
    from clonealign_amd.engine import HipEngine
    e = edge
    N, G, _C = EDGE
    for fmt in (sps.csr_matrix, sps.csc_matrix):
        eng = HipEngine(fmt(e["Y"]), e["L"], np.zeros((N, 0)), np.zeros(G), 0)
        try:
            same_bits(eng.clone_evidence(e["E"], e["V"], 1, X=e["X"], nodes=e["nd"], weights=e["wt"]), e["base"], fmt.__name__)
        finally:
            eng.close()


def test_group_returns_the_single_handle_bits(edge):
    from clonealign_amd.engine import EngineError, HipGroupEngine
    e = edge
    N, G, C = EDGE
    V2, _X, _lp = operands(N, G, C, 2, 1, np.random.default_rng(5))
    nd2, wt2 = rule(2)
    start = np.random.default_rng(6).normal(size=(N, 2)) * 0.3
    one = e["eng"].clone_evidence(e["E"], V2, 2, X=e["X"], psi_start=start, nodes=nd2, weights=wt2)
    grp = HipGroupEngine(e["Y"], e["L"], np.zeros((N, 0)), np.zeros(G), 0, devices=[0] * 3)
    try:
        og = grp.clone_evidence(e["E"], V2, 2, X=e["X"], psi_start=start, nodes=nd2, weights=wt2)
        bad = e["X"].copy()
        bad[N - 1, 0] = np.nan                                       # refused on one rank's cells: refused by the group, which stays usable
        with pytest.raises(EngineError) as ex:
            grp.clone_evidence(e["E"], V2, 2, X=bad, psi_start=start, nodes=nd2, weights=wt2)
        assert ex.value.code == 1 and "X has a non-finite entry" in ex.value.msg, ex.value.msg
        same_bits(grp.clone_evidence(e["E"], V2, 2, X=e["X"], psi_start=start, nodes=nd2, weights=wt2), og, "again")
        same_bits(grp.clone_evidence(e["E"], e["V"], 1, X=e["X"], nodes=e["nd"], weights=e["wt"]), e["base"], "K = 1")
    finally:
        grp.close()
    same_bits(og, one, "group of 3")


def test_edges_zero_copy_number_impossible_and_empty_cells_extreme_exponents():
    from clonealign_amd.engine import HipEngine
    N, G, C = EDGE
    Y, L, mu, _idx, rng = problem(N, G, C, "u8", seed=7)
    L[7, 3] = 0.0
    Y[:, 7] = 0
    Y[11, 7] = 2                                                     # one cell with a positive count where one clone has none
    L[9, :] = 0.0
    Y[:, 9] = 0
    Y[13, 9] = 1                                                     # ... and one where no clone has any: the cell is impossible
    Y[17] = 0                                                        # a cell with no counts
    E = mu[:, None] * L
    V, _X, _lp = operands(N, G, C, 1, 0, rng)
    V[[3, 40, 60], 0] = 700.0                                        # eta = +-700 on a few genes of every cell that starts at psi = 1
    V[[4, 41], 0] = -700.0
    start = np.zeros((N, 1))
    start[20:30] = 1.0
    start[13] = 0.25
    nd, wt = rule(1)
    eng = HipEngine(Y, np.maximum(L, 1.0), np.zeros((N, 0)), np.zeros(G), 0)
    try:
        dev = eng.clone_evidence(E, V, 1, psi_start=start, nodes=nd, weights=wt, max_iter=6)
        ref = _clone_evidence_host(Y, E, V, 1, 0, None, start, nd, wt, max_iter=6)
    finally:
        eng.close()
    dead = np.zeros((N, C), dtype=bool)
    dead[11, 3] = True
    dead[13] = True
    for k in ("evidence", "laplace"):
        assert np.array_equal(np.isneginf(dev[k]), dead), k           # -inf in that clone only / in all clones of the impossible cell
        assert np.isfinite(dev[k][~dead]).all(), k
    for k in KEYS:
        assert not np.isnan(dev[k].astype(np.float64)).any(), k
    assert (dev["rounds"][dead] == 0).all() and not dev["converged"][dead].any()
    assert (dev["psi_mode"][13] == 0.25).all() and dev["psi_mode"][11, 3, 0] == 0.0 and (dev["psi_prec"][dead] == 1.0).all()
    assert np.abs(dev["evidence"][17]).max() <= 1e-12 and np.abs(dev["laplace"][17]).max() <= 1e-12 and (dev["psi_mode"][17] == 0.0).all()
    assert np.array_equal(dev["rounds"], ref["rounds"]) and np.array_equal(dev["converged"], ref["converged"])
    fig = float((np.abs(dev["psi_mode"] - ref["psi_mode"]) / np.maximum(1.0, np.abs(ref["psi_mode"]))).max())
    big = np.where(np.isfinite(ref["evidence"]), np.abs(ref["evidence"]), 1.0)
    de = float((np.abs(dev["evidence"][~dead] - ref["evidence"][~dead]) / np.maximum(big[~dead], 1.0)).max())
    # (evidence is printed, not held to a bar here: where a gene at eta = 700 carries all the weight, cov = Z2 / Z0 - mean^2 is a difference of two numbers of
    # size 490000 that is 0 in exact arithmetic, so s * cov -- and with it log det H -- is rounding noise of relative size 1e-5; measured 1.8e-5)
    print(f"clone_evidence zeros of E and eta = +-700: psi figure {fig:.2e}, evidence relative {de:.2e}")
    assert fig <= PSI_TOL


def test_k_zero_returns_clone_loglik_bits(edge):
    e = edge
    beta = e["V"][:, 1:]
    r = e["eng"].clone_evidence(e["E"], beta, 0, X=e["X"])
    ll = e["eng"].clone_loglik(e["E"], e["X"], beta)
    assert np.array_equal(r["evidence"], ll) and np.array_equal(r["laplace"], ll) and (r["rounds"] == 0).all() and r["converged"].all()
    assert r["psi_mode"].shape == (EDGE[0], EDGE[2], 0)
    r = e["eng"].clone_evidence(e["E"])
    assert np.array_equal(r["evidence"], e["eng"].clone_loglik(e["E"]))


def test_through_the_api_the_device_equals_the_host_form():
    import clonealign_amd as ca
    from tests.test_clone_evidence_host import planted_k1
    from tests.test_project_cells_host import HostOnly
    p = planted_k1(0)
    names = ["a", "b", "c"]
    fits = {k: ca.ClonealignFit(ml_params={"mu": p["mu"], "alpha": p["alpha"], "W": w}, clone_names=names)
            for k, w in (("K=0", None), ("K=1", p["W"]), ("K=2", p["W2"]))}
    host = HostOnly(*p["Y"].shape)
    dev = ca.assign_cells_marginal(fits["K=1"], p["Y"], p["L"], saturate=False)
    ref = ca.assign_cells_marginal(fits["K=1"], p["Y"], p["L"], saturate=False, engine=host)
    assert np.array_equal(dev["clone"], ref["clone"]) and np.array_equal(dev["rounds"], ref["rounds"]) and np.array_equal(dev["converged"], ref["converged"])
    np.testing.assert_allclose(dev["loglik"], ref["loglik"], rtol=1e-10)
    np.testing.assert_allclose(dev["clone_probs"], ref["clone_probs"], rtol=0, atol=PSI_TOL)
    np.testing.assert_allclose(dev["psi"], ref["psi"], rtol=0, atol=PSI_TOL)
    np.testing.assert_allclose(dev["psi_sd"], ref["psi_sd"], rtol=0, atol=PSI_TOL)
    hd = ca.heldout_evidence(fits, p["Y"], p["L"], saturate=False)
    hr = ca.heldout_evidence(fits, p["Y"], p["L"], saturate=False, engine=host)
    assert hd["ranking"] == hr["ranking"] == ["K=1", "K=2", "K=0"]
    for k in fits:
        np.testing.assert_allclose(hd[k]["per_cell"], hr[k]["per_cell"], rtol=1e-10)
        assert hd[k]["n_unconverged"] == hr[k]["n_unconverged"]
        assert abs(hd[k]["delta"] - hr[k]["delta"]) <= 1e-8 * abs(hr["K=1"]["total"])
    with pytest.raises(ValueError, match="K <= 2"):
        ca.clone_evidence(ca.ClonealignFit(ml_params={"mu": p["mu"], "alpha": p["alpha"], "W": np.zeros((150, 3))}, clone_names=names), p["Y"], p["L"])


def test_refusals_name_the_offender_and_poll_hooks_are_refused():
    import ctypes as C
    from clonealign_amd.engine import EngineError, HipEngine
    from clonealign_amd.rng import EpsStream
    from tests._cases import make_case
    case = make_case(N=700, G=300, C=4, K=1, seed=2)
    L = case["L"]
    rng = np.random.default_rng(0)
    V, X, _lp = operands(700, 300, 4, 1, 1, rng)
    nd, wt = rule(1)
    eng = HipEngine(**case)
    try:
        def refused(words, *a, **k):
            with pytest.raises(EngineError) as ex:
                eng.clone_evidence(*a, **k)
            assert ex.value.code == 1 and all(w in ex.value.msg for w in words), ex.value.msg
        refused(("n_nodes = 0", "[1, 64]"), L, V, 1, X=X, nodes=np.zeros((0, 1)), weights=np.zeros(0))
        refused(("n_nodes = 65", "[1, 64]"), L, V, 1, X=X, nodes=np.zeros((65, 1)), weights=np.full(65, 1 / 65))
        bw = wt.copy()
        bw[3] = -bw[3]
        refused(("weight 3", "not positive"), L, V, 1, X=X, nodes=nd, weights=bw)
        refused(("weights sum to", "1e-12"), L, V, 1, X=X, nodes=nd, weights=wt * 0.9)
        bn = nd.copy()
        bn[5, 0] = np.nan
        refused(("node 5", "non-finite"), L, V, 1, X=X, nodes=bn, weights=wt)
        refused(("K = 3", "[0, 2]"), L, np.zeros((300, 3)), 3, nodes=np.zeros((1, 3)), weights=np.ones(1))
        Xb = X.copy()
        Xb[9, 0] = np.nan
        refused(("X has a non-finite", "cell 9"), L, V, 1, X=Xb, nodes=nd, weights=wt)
        E = L.copy()
        E[17, 2] = -1.0
        refused(("gene 17", "clone 2"), E, V, 1, X=X, nodes=nd, weights=wt)
        refused(("max_iter = -1",), L, V, 1, X=X, nodes=nd, weights=wt, max_iter=-1)
        refused(("tol",), L, V, 1, X=X, nodes=nd, weights=wt, tol=0.0)
        out = [np.zeros((700, 4)) for _ in range(4)] + [np.zeros((700, 4), dtype=np.int32), np.zeros((700, 4), dtype=np.uint8)]
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        Lc, Vc, Xc = np.ascontiguousarray(L), np.ascontiguousarray(V), np.ascontiguousarray(X)
        rc = eng.lib.ca_clone_evidence(eng.h, ptr(Lc), ptr(Vc), 1, 1, ptr(Xc), None, 1, 8, None, ptr(wt), 25, 1e-9, 1.0, *[ptr(a) for a in out])
        assert rc == 1 and b"nodes is NULL" in eng.lib.ca_last_error(eng.h)
        rc = eng.lib.ca_clone_evidence(eng.h, ptr(Lc), ptr(Vc), 1, 1, ptr(Xc), None, 1, 8, ptr(nd), None, 25, 1e-9, 1.0, *[ptr(a) for a in out])
        assert rc == 1 and b"weights is NULL" in eng.lib.ca_last_error(eng.h)
        with pytest.raises(ValueError):
            eng.clone_evidence(L[:-1], V, 1, X=X)
        with pytest.raises(ValueError):
            eng.clone_evidence(L, V, 1, X=X, nodes=nd)
        seen = {}

        def hook(i, e):
            if i == 2:
                with pytest.raises(EngineError) as ex:
                    eng.clone_evidence(L, V, 1, X=X, nodes=nd, weights=wt)
                seen["code"] = ex.value.code
            return False
        eng.run(EpsStream(9, 1, 300), 4, 1e-12, poll=hook)
        assert seen["code"] == 6                                     # CA_ERR_STATE
        compare(eng.clone_evidence(L, V, 1, X=X, nodes=nd, weights=wt), _clone_evidence_host(case["Y"], L, V, 1, 1, X, None, nd, wt), case["Y"], L, V, 1, X,
                1e-9, "after the run")
    finally:
        eng.close()
