"""ca_fit_mse / HipEngine.fit_mse / compute_ca_fit_mse / clonealign(fit_mse=True): the squared error of a fit (R/clonealign.R:415-434) in one
float64 sweep over the resident count matrix.

The yardstick is ``ref_mse`` below, the reference's formula restated in plain numpy float64 (chunked over cells).  Bar: relative 1e-10 on the
total, on every gene's sum and on every cell's sum.  Both sides add non-negative float64 terms by pairwise / tree sums, so they differ by about
log2(N G) 2^-53 < 1e-14; the margin covers the order of the additions, and any float32 intermediate (6e-8) fails it."""
import numpy as np
import pytest

from tests._cases import make_case

pytestmark = pytest.mark.gpu
RTOL = 1e-10


def ref_mse(Y, E, idx, chunk=8192):
    """(total, sse_gene[G], sse_cell[N]) of R/clonealign.R:423-432 for the cells with idx >= 0; Y dense (any dtype) or scipy.sparse."""
    E = np.asarray(E, dtype=np.float64)
    idx = np.asarray(idx)
    N, G = Y.shape
    col = E.sum(0)                                                   # colSums(predicted_expression), per clone
    sse_gene, sse_cell = np.zeros(G), np.zeros(N)
    for lo in range(0, N, chunk):
        rows = lo + np.flatnonzero(idx[lo:lo + chunk] >= 0)
        if rows.size == 0:
            continue
        Yc = Y[rows]
        Yc = np.asarray(Yc.toarray() if hasattr(Yc, "toarray") else Yc, dtype=np.float64)
        normalizer = Yc.sum(1) / col[idx[rows]]                      # :429
        predicted = E[:, idx[rows]].T * normalizer[:, None]          # :430
        sq = (predicted - Yc) ** 2                                   # :432
        sse_gene += sq.sum(0)
        sse_cell[rows] = sq.sum(1)
    return float(sse_gene.sum()), sse_gene, sse_cell


def check(out, Y, E, idx, tag=""):
    tot, sg, sc = ref_mse(Y, E, idx)
    used = int((np.asarray(idx) >= 0).sum())
    print(f"fit_mse {tag}: total rel {abs(out['sse'] - tot) / tot:.2e}, gene max rel {np.abs(out['sse_gene'] / sg - 1).max():.2e}, "
          f"cell max rel {np.abs(out['sse_cell'][sc > 0] / sc[sc > 0] - 1).max():.2e}")
    assert out["n_cells"] == used
    assert abs(out["sse"] - tot) <= RTOL * tot, tag
    np.testing.assert_allclose(out["sse_gene"], sg, rtol=RTOL, atol=0, err_msg=tag)
    np.testing.assert_allclose(out["sse_cell"], sc, rtol=RTOL, atol=0, err_msg=tag)
    assert np.all(out["sse_cell"][np.asarray(idx) < 0] == 0.0)
    assert abs(out["mse"] - tot / (used * Y.shape[1])) <= RTOL * out["mse"]


def problem(N, G, C, storage, seed):
    """Counts for one storage width: u8 with several counts above 255 (the overflow list), u16 up to 60000, f32 with non-integer values."""
    rng = np.random.default_rng(seed)
    case = make_case(N=N, G=G, C=C, K=0, seed=seed)
    Y = case["Y"]
    if storage == "u8":
        hot = rng.choice(N * G, size=max(7, N * G // 500), replace=False)
        Y.reshape(-1)[hot] = rng.integers(256, 70000, size=hot.size)
        Y.reshape(-1)[hot[:3]] = 255                               # genuine 255s beside the escapes
    elif storage == "u16":
        hot = rng.choice(N * G, size=max(7, N * G // 50), replace=False)
        Y.reshape(-1)[hot] = rng.integers(256, 60001, size=hot.size)
    else:
        Y = (Y + rng.random(Y.shape) * (Y > 0)).astype(np.float32)   # what the f32 storage holds exactly
    mu = rng.lognormal(0, 0.5, G)
    idx = rng.integers(0, C, N).astype(np.int32)
    return Y, case["L"], mu, idx, rng


SHAPES = [(33, 77, 2), (3000, 1234, 8), (5000, 2049, 20)]


@pytest.mark.parametrize("storage", ["u8", "u16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_with_the_float64_restatement(shape, storage):
    from clonealign_amd.engine import HipEngine
    N, G, C = shape
    Y, L, mu, idx, rng = problem(N, G, C, storage, seed=sum(shape))
    skip = idx.copy()
    skip[rng.choice(N, N // 10, replace=False)] = -1                # a tenth of the cells skipped
    eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, y_storage=storage)
    try:
        assert eng.info()["y_storage_name"] == storage
        for name, E in (("L", L), ("mu*L", mu[:, None] * L)):
            for lab, ii in (("all", idx), ("tenth skipped", skip)):
                out = eng.fit_mse(ii, E, per_gene=True, per_cell=True)
                check(out, Y, E, ii, f"{shape} {storage} E={name} {lab}")
                again = eng.fit_mse(ii, E, per_gene=True, per_cell=True)      # two calls: identical bits
                assert again["sse"] == out["sse"] and np.array_equal(again["sse_gene"], out["sse_gene"])
                assert np.array_equal(again["sse_cell"], out["sse_cell"])
        lean = eng.fit_mse(idx, L)                                   # no per-gene / per-cell output asked for
        assert set(lean) == {"sse", "n_cells", "mse"} and lean["sse"] == eng.fit_mse(idx, L, per_gene=True)["sse"]
    finally:
        eng.close()


@pytest.mark.parametrize("storage", ["u8", "f32"])
def test_both_layouts_and_selections_of_the_raw_matrix(storage):
    from clonealign_amd.engine import HipEngine
    N, G, C = 1500, 700, 5
    Y, L, mu, idx, rng = problem(N, G, C, storage, seed=12)
    E = mu[:, None] * L
    idx[::7] = -1
    outs = {}
    for lay in ("row", "col"):
        eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, y_storage=storage, layout=lay)
        try:
            outs[lay] = eng.fit_mse(idx, np.asfortranarray(E) if lay == "col" else E, per_gene=True, per_cell=True)
        finally:
            eng.close()
        check(outs[lay], Y, E, idx, f"layout {lay} {storage}")
    assert outs["row"]["sse"] == outs["col"]["sse"] and np.array_equal(outs["row"]["sse_cell"], outs["col"]["sse_cell"])
    ci = np.sort(rng.choice(N, 1100, replace=False)).astype(np.int64)
    gi = np.sort(rng.choice(G, 515, replace=False)).astype(np.int32)
    eng = HipEngine(Y, L[gi], np.zeros((1100, 0)), np.zeros(515), 0, y_storage=storage, cell_index=ci, gene_index=gi)
    try:
        out = eng.fit_mse(idx[ci], E[gi], per_gene=True, per_cell=True)
    finally:
        eng.close()
    check(out, Y[np.ix_(ci, gi)], E[gi], idx[ci], f"cell_index / gene_index {storage}")


@pytest.mark.parametrize("fmt", ["csr", "csc"])
def test_from_sparse_input(fmt):
    import scipy.sparse as sps
    from clonealign_amd.engine import HipEngine
    N, G, C = 2500, 900, 6
    rng = np.random.default_rng(5)
    L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
    z = rng.integers(0, C, N)
    Y = rng.poisson(0.15 * L[:, z].T).astype(np.float64)
    Y[:, 0] += 1
    hot = rng.choice(N * G, 40, replace=False)
    Y.reshape(-1)[hot] = rng.integers(256, 9000, size=40)
    Ys = sps.csr_matrix(Y) if fmt == "csr" else sps.csc_matrix(Y)
    idx = rng.integers(-1, C, N).astype(np.int32)
    eng = HipEngine(Ys, L, np.zeros((N, 0)), np.zeros(G), 0)
    try:
        assert eng.info()["y_storage_name"] == "u8"
        out = eng.fit_mse(idx, L, per_gene=True, per_cell=True)
    finally:
        eng.close()
    check(out, Ys.tocsr(), L, idx, f"sparse {fmt}")


@pytest.mark.parametrize("builtin", [True, False])
def test_the_call_changes_nothing_in_a_running_fit(builtin):
    """Five iterations, fit_mse, five more == ten iterations straight, bit for bit: every variable and the ELBO."""
    from clonealign_amd.engine import HipEngine
    from tests._cases import eps_for
    case = make_case(N=2600, G=640, C=5, K=1, seed=21)
    G = case["Y"].shape[1]
    eps = None if builtin else np.stack([eps_for(1, G, 100 + i) for i in range(20)])
    idx = np.random.default_rng(1).integers(-1, 5, 2600).astype(np.int32)
    a = HipEngine(**case)
    try:
        ea = a.iterate(10, eps)
        sa = a.get_state()
    finally:
        a.close()
    b = HipEngine(**case)
    try:
        b.iterate(5, None if builtin else eps[:10])
        out = b.fit_mse(idx, case["L"], per_gene=True, per_cell=True)
        check(out, case["Y"], case["L"], idx, "mid-fit")
        eb = b.iterate(5, None if builtin else eps[10:])
        sb = b.get_state()
    finally:
        b.close()
    assert ea == eb
    for n in sa:
        assert np.array_equal(sa[n], sb[n]), n


@pytest.mark.parametrize("world", [2, 3])
def test_group_returns_the_single_handle_result(world):
    from clonealign_amd.engine import HipEngine, HipGroupEngine
    N, G, C = 1301, 700, 8
    Y, L, mu, idx, rng = problem(N, G, C, "u8", seed=31)
    idx[rng.choice(N, 130, replace=False)] = -1
    E = mu[:, None] * L
    one = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0)
    try:
        o1 = one.fit_mse(idx, E, per_gene=True, per_cell=True)
    finally:
        one.close()
    grp = HipGroupEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, devices=[0] * world)
    try:
        og = grp.fit_mse(idx, E, per_gene=True, per_cell=True)
        with pytest.raises(Exception) as ex:                         # refused on one rank's cells: refused by the group, which stays usable
            bad = idx.copy()
            bad[N - 1] = C
            grp.fit_mse(bad, E)
        assert ex.value.code == 1
        assert grp.fit_mse(idx, E)["sse"] == og["sse"]
    finally:
        grp.close()
    check(og, Y, E, idx, f"group of {world}")
    assert og["n_cells"] == o1["n_cells"]
    assert np.array_equal(og["sse_cell"], o1["sse_cell"])            # per cell: the same bits
    assert abs(og["sse"] - o1["sse"]) <= 1e-12 * o1["sse"]           # totals: only the grouping of the fp64 rank sums differs
    np.testing.assert_allclose(og["sse_gene"], o1["sse_gene"], rtol=1e-12, atol=0)


def test_clonealign_with_fit_mse():
    import clonealign_amd as ca
    from clonealign_amd.engine import HipEngine
    case = make_case(N=1200, G=400, C=3, K=1, seed=17, scale=1.0)   # planted clones
    Y, L = case["Y"].copy(), case["L"]
    Y[:, [5, 77]] = 0                                                # two genes the gene filter removes
    kw = dict(max_iter=40, verbose=False, seed=3)
    res = ca.clonealign(Y, L, fit_mse=True, **kw)
    plain = ca.clonealign(Y, L, **kw)
    assert "fit_mse" not in plain
    assert set(res) - {"fit_mse"} == set(plain)
    for k in plain["ml_params"]:
        assert np.array_equal(plain["ml_params"][k], res["ml_params"][k]), k
    assert np.array_equal(plain["convergence_info"]["elbo"], res["convergence_info"]["elbo"])
    assert plain["convergence_info"]["final_elbo"] == res["convergence_info"]["final_elbo"]
    assert np.array_equal(plain["clone"], res["clone"]) and np.array_equal(plain["correlations"], res["correlations"], equal_nan=True)

    keep = np.ones(400, dtype=bool)
    keep[[5, 77]] = False
    assert len(res["retained_genes"]) == 398
    Yk, Lk = Y[:, keep], L[keep]
    lut = {c: i for i, c in enumerate(res["clone_names"])}
    idx = np.array([lut.get(c, -1) for c in res["clone"]], dtype=np.int32)
    fm = res["fit_mse"]
    assert set(fm) == {"mse", "mse_model_mu", "mse_gene", "n_cells"} and fm["n_cells"] == int((idx >= 0).sum()) > 0
    tot, sg, _ = ref_mse(Yk, Lk, idx)
    assert abs(fm["mse"] - tot / (fm["n_cells"] * 398)) <= RTOL * fm["mse"]
    np.testing.assert_allclose(fm["mse_gene"], sg / fm["n_cells"], rtol=RTOL, atol=0)
    tot_mu, _, _ = ref_mse(Yk, res["ml_params"]["mu"][:, None] * Lk, idx)
    assert abs(fm["mse_model_mu"] - tot_mu / (fm["n_cells"] * 398)) <= RTOL * fm["mse_model_mu"]
    # the stand-alone function, on a throwaway engine and on a live one
    alone = ca.compute_ca_fit_mse(res, Yk, Lk, drop_unassigned=True)
    assert abs(alone - fm["mse"]) <= 1e-12 * fm["mse"]
    assert abs(ca.compute_ca_fit_mse(res, Yk, Lk, model_mu=True, drop_unassigned=True) - fm["mse_model_mu"]) <= 1e-12 * fm["mse_model_mu"]
    eng = HipEngine(Yk, Lk, np.zeros((1200, 0)), None, 0)
    try:
        mse, per_gene = ca.compute_ca_fit_mse(res, Yk, Lk, drop_unassigned=True, per_gene=True, engine=eng)
        assert mse == alone and np.array_equal(per_gene, fm["mse_gene"])
        for seed in range(5):                                        # the check the reference's authors use it for
            rnd = ca.compute_ca_fit_mse(res, Yk, Lk, random_clones=True, seed=seed, drop_unassigned=True, engine=eng)
            print(f"fit_mse: fitted labels {mse:.6f}, random labels (seed {seed}) {rnd:.6f}")
            assert mse < rnd, seed
    finally:
        eng.close()


def test_invalid_input_and_calls_from_a_poll_hook_are_refused():
    from clonealign_amd.engine import EngineError, HipEngine
    from clonealign_amd.rng import EpsStream
    case = make_case(N=700, G=300, C=4, K=1, seed=2)
    L = case["L"]
    idx = np.random.default_rng(0).integers(0, 3, 700).astype(np.int32)     # clone 3 is not in use
    eng = HipEngine(**case)
    try:
        for bad_value in (4, -2):
            bad = idx.copy()
            bad[11] = bad_value
            with pytest.raises(EngineError) as ex:
                eng.fit_mse(bad, L)
            assert ex.value.code == 1 and "clone index" in ex.value.msg and "cell 11" in ex.value.msg, ex.value.msg
        E = L.copy()
        E[:, 1] = 0.0
        with pytest.raises(EngineError) as ex:
            eng.fit_mse(idx, E)
        assert ex.value.code == 1 and "clone 1" in ex.value.msg and "sums to" in ex.value.msg, ex.value.msg
        E = L.copy()
        E[:, 3] = 0.0                                                # a zero column of a clone nobody has: fine
        assert eng.fit_mse(idx, E)["sse"] == eng.fit_mse(idx, L)["sse"]
        E = L.copy()
        E[17, 2] = np.inf
        with pytest.raises(EngineError) as ex:
            eng.fit_mse(idx, E)
        assert ex.value.code == 1 and "non-finite" in ex.value.msg, ex.value.msg
        seen = {}

        def hook(i, e):
            if i == 2:
                with pytest.raises(EngineError) as ex:
                    eng.fit_mse(idx, L)
                seen["code"] = ex.value.code
            return False
        eng.run(EpsStream(9, 1, 300), 4, 1e-12, poll=hook)
        assert seen["code"] == 6                                     # CA_ERR_STATE
        check(eng.fit_mse(idx, L, per_gene=True, per_cell=True), case["Y"], L, idx, "after the run")
    finally:
        eng.close()


def test_at_size_100k_cells():
    """100k x 5k x 8 in u8 storage with an overflow list; also guards 64-bit indexing (N * Gp = 5.1e8 bytes, list x segment offsets)."""
    from clonealign_amd.engine import HipEngine
    N, G, C = 100_000, 5000, 8
    rng = np.random.default_rng(99)
    L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
    mu = rng.lognormal(0, 1, G)
    z = rng.integers(0, C, N)
    Y = np.empty((N, G), dtype=np.int32)
    for lo in range(0, N, 10_000):
        Y[lo:lo + 10_000] = rng.poisson(mu[None, :] * L[:, z[lo:lo + 10_000]].T * 0.5)
    Y[:, 0] += 1
    hot = rng.choice(N * G, 5000, replace=False)
    Y.reshape(-1)[hot] = rng.integers(256, 100000, size=hot.size)
    idx = z.astype(np.int32)
    flip = rng.choice(N, N // 5, replace=False)
    idx[flip] = rng.integers(0, C, flip.size)
    idx[rng.choice(N, N // 10, replace=False)] = -1
    E = mu[:, None] * L
    eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0)
    try:
        assert eng.info()["y_storage_name"] == "u8"
        out = eng.fit_mse(idx, E, per_gene=True, per_cell=True)
    finally:
        eng.close()
    check(out, Y, E, idx, "100k x 5k x 8")
