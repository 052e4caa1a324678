"""The device-side fit helpers on every count storage and route, against float64 / int64 numpy (tests/_device_helper_cases.py):
the resident image read back cell by cell, ca_clone_gene_sums (T exact, Syy to float64), ca_init_psi_pca against the float64 SVD, the
loc0 = NULL mu guess of ca_create, ca_preprocess.  Every figure a test bounds is printed first on a line starting with "r23|"
(profiles/r23_device_helpers.txt is those lines of one run)."""
import numpy as np
import pytest
import scipy.sparse as sps

from tests import _device_helper_cases as dc

pytestmark = pytest.mark.gpu

C = 4
PCA_BAR = 2e-4          # the project's bar of the device PCA against prcomp + scale
PCA_MODEL_FACTOR = 16   # beside it: this many times the error of the float32 model of the final projection (dc.pca_model_error)
MU_BAR = 2e-6           # the project's bar of the device mu guess, of the largest magnitude
T_SHAPES = [(700, 300), (257, 1030)]


def _rec(*parts):
    print("r23|" + "|".join(str(p) for p in parts))


def _engine(Y, K=1, loc0=1.0, cls=None, L=None, **kw):
    from clonealign_amd.engine import HipEngine
    N, G = kw.pop("shape_fit", None) or Y.shape
    L = dc.copy_numbers(G, C) if L is None else L
    return (cls or HipEngine)(Y, L, np.zeros((N, K)), None if loc0 is None else np.full(G, loc0), K, **kw)


def _sparse(Y, fmt, vdtype=np.float64, ib=4, device=False):
    """Y as a scipy / torch sparse matrix: format, value dtype, index width, host or device arrays."""
    m = (sps.csr_matrix if fmt == "csr" else sps.csc_matrix)(np.asarray(Y).astype(vdtype))
    if ib == 8:
        m.indptr, m.indices = m.indptr.astype(np.int64), m.indices.astype(np.int64)
    if not device:
        return m
    import torch
    t = torch.device("cuda:0")
    mk = torch.sparse_csr_tensor if fmt == "csr" else torch.sparse_csc_tensor
    idx_dt = torch.int64 if ib == 8 else torch.int32
    return mk(torch.tensor(m.indptr, dtype=idx_dt, device=t), torch.tensor(m.indices, dtype=idx_dt, device=t),
              torch.tensor(m.data, device=t), size=Y.shape)


def _check_store(eng, Y, store, ovf=None):
    """The storage the engine picked, and whether it keeps a u8 overflow list (ca_info does not count the list's entries: u8 storage of a
    matrix with counts above 255 has one, there is no other place for them -- and the read-back below finds their values in it)."""
    info = eng.info()
    assert info["y_storage_name"] == store, (info["y_storage_name"], store)
    n_ovf = int((np.asarray(Y) > 255).sum()) if store == "u8" else 0
    if ovf is not None:
        assert (n_ovf > 0) == ovf, n_ovf
    return info


# ------------------------------------------------------------------ 1. the resident image, read back
def _read_back(eng, Y, store, n_ovf=None):
    """The engine's resident matrix is Y [N, G] (float64, the selection applied): 2 C cells through T of one-cell clones, s for all cells."""
    N, G = Y.shape
    assert (eng.N, eng.G) == (N, G)
    _check_store(eng, Y, store, n_ovf)
    for cells in dc.readback_cells(Y, C):
        if not cells:
            continue
        T, _ = eng.clone_gene_sums(dc.one_cell_labels(N, cells))
        want = np.zeros((G, C))
        want[:, :len(cells)] = Y[cells].T
        assert np.array_equal(np.asarray(T), want), (cells, np.argwhere(np.asarray(T) != want)[:5])
    assert np.array_equal(eng.get("s"), Y.sum(1))


DENSE = [("float64", "f32frac"), ("float32", "f32int"), ("int32", "u8ovf"), ("uint16", "u16"), ("uint8", "u8")]


@pytest.mark.parametrize("layout", ["row", "col"])
@pytest.mark.parametrize("dtype,kind", DENSE, ids=[d for d, _ in DENSE])
def test_read_back_host_dense(dtype, kind, layout):
    Y = dc.variant(kind, 700, 300)
    eng = _engine(Y.astype(dtype), layout=layout)
    try:
        _read_back(eng, Y, dc.STORAGE[kind], n_ovf=kind == "u8ovf")
    finally:
        eng.close()


@pytest.mark.parametrize("kind", ["u8ovf", "u16"])
def test_read_back_device_pointer_and_selections(kind):
    import torch
    Y = dc.variant(kind, 700, 300)
    Yd = torch.tensor(Y.astype(np.int32), device="cuda:0")
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    ci = np.sort(rng.choice(700, size=523, replace=False))
    gi = np.sort(rng.choice(300, size=201, replace=False))
    dev = dict(y_device_ptr=Yd.data_ptr(), y_device_dtype=np.int32, shape=(700, 300))
    for sel, want in ((dict(), Y), (dict(cell_index=ci, gene_index=gi), Y[ci][:, gi]), (dict(cell_index=ci), Y[ci]), (dict(gene_index=gi), Y[:, gi])):
        store = dc.auto_storage(want)[0]
        for eng in (_engine(None, shape_fit=want.shape, **dev, **sel), _engine(Y, shape_fit=want.shape, **sel),
                    _engine(Y, shape_fit=want.shape, layout="col", **sel)):
            try:
                _read_back(eng, want, store)
            finally:
                eng.close()


SPARSE = [(f, ib, dev) for f in ("csr", "csc") for ib in (4, 8) for dev in (False, True)]


@pytest.mark.parametrize("fmt,ib,device", SPARSE, ids=[f"{f}-i{b * 8}-{'dev' if d else 'host'}" for f, b, d in SPARSE])
def test_read_back_sparse(fmt, ib, device):
    for kind, vdt in (("u8", np.uint8), ("u8ovf", np.int32), ("u16", np.float64), ("f32int", np.float32), ("f32frac", np.float64)):
        Y = dc.variant(kind, 333, 95)
        eng = _engine(_sparse(Y, fmt, vdt, ib, device))
        try:
            _read_back(eng, Y, dc.STORAGE[kind], n_ovf=kind == "u8ovf")
        finally:
            eng.close()


def _wide(store):
    """Counts whose rows are wider than one 32 KiB segment of the sparse densify: f32 24 x 8300, u16 16 x 16500."""
    N, G = (24, 8300) if store == "f32" else (16, 16500)
    rng = np.random.default_rng([7, G])
    Y = rng.poisson(0.6, size=(N, G)).astype(np.float64)
    Y[:, 0] += 1
    Y[0, :] += 1
    flat = rng.choice(Y.size, Y.size // 30, replace=False)
    Y.flat[flat] = rng.integers(256, 60000, size=flat.size)
    if store == "f32":
        Y[3, 5] = 2.5
        Y[N - 1, G - 1] = 70000.0
    drop = np.setdiff1d(rng.choice(G, 40, replace=False), [0, 5, G - 1])
    return Y, np.setdiff1d(np.arange(G), drop)


@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("store", ["f32", "u16"])
def test_read_back_through_the_multi_segment_densify(store, fmt):
    Y, gi = _wide(store)
    seg = 32768 // (4 if store == "f32" else 2)
    assert Y.shape[1] > seg and gi.size > seg        # more than one segment's worth, with and without the selection
    for sel, want in ((dict(), Y), (dict(gene_index=gi), Y[:, gi])):
        eng = _engine(_sparse(Y, fmt), shape_fit=want.shape, **sel)
        try:
            _read_back(eng, want, store)
        finally:
            eng.close()


@pytest.mark.parametrize("N", [1, 1023, 1024, 1025, 2049])
def test_read_back_csc_at_the_scan_slice_boundaries(N):
    Y = np.minimum(dc.planted(N, 70, seed=N), 255).astype(np.float64)
    Y.flat[::211] += 300.0
    for ib in (4, 8):
        eng = _engine(_sparse(Y, "csc", np.float64, ib))
        try:
            _read_back(eng, Y, "u8", n_ovf=True)
        finally:
            eng.close()


def test_read_back_engine_without_latent_factors():
    """The throwaway engine of api.predictive_check: K = 0, loc0 = NULL."""
    for kind in ("u8ovf", "f32int"):
        Y = dc.variant(kind, 333, 95)
        eng = _engine(Y, K=0, loc0=None)
        try:
            _read_back(eng, Y, dc.STORAGE[kind])
        finally:
            eng.close()


# ------------------------------------------------------------------ 2. T exact, Syy accurate
T_CASES = [(k, s, "uniform") for s in T_SHAPES for k in dc.VARIANTS] + [("large-" + k, dc.LARGE_SHAPE[:2], lab) for k in dc.LARGE for lab in dc.LABELS]


@pytest.mark.parametrize("kind,shape,labels", T_CASES, ids=[f"{k}-{s[0]}x{s[1]}-{lab}" for k, s, lab in T_CASES])
def test_clone_sums_exact_and_correlations_match_the_host_formula(kind, shape, labels):
    from clonealign_amd.api import correlations_from_sums
    from clonealign_amd.engine import HipGroupEngine
    N, G = shape
    large = kind.startswith("large-")
    base = kind[6:] if large else kind
    Y = dc.large_counts(base) if large else dc.variant(base, N, G)
    kw = dict(y_storage=dc.storage_arg(base, Y))
    if large and dc.large_tune(base):
        kw["tune"] = dc.large_tune(base)
    idx = dc.clone_labels(N, C, skew=labels == "skew")
    L = dc.copy_numbers(G, C).copy()
    L[G // 2] = 2.0                                  # a gene whose copy number does not vary: NaN on both sides
    Tref, Sref = dc.clone_sums_ref(Y, idx, C)
    host = dc.host_correlations(Y, L, idx)
    counts = np.bincount(idx[idx >= 0], minlength=C)
    assert np.isnan(host[G // 2]) and np.isfinite(np.delete(host, G // 2)).all()
    one = _engine(Y, L=L, **kw)
    grp = _engine(Y, L=L, cls=HipGroupEngine, devices=[0, 0], transport="host", **kw)
    try:
        info = _check_store(one, Y, dc.STORAGE[base], base == "u8ovf")
        (T, Syy), (Tg, Sg) = one.clone_gene_sums(idx), grp.clone_gene_sums(idx)
        t_err = float(np.abs(T - Tref).max() / np.abs(Tref).max())
        s_err = float((np.abs(Syy - Sref) / Sref).max())
        r = correlations_from_sums(T, Syy, L, counts)
        r_err = float(np.nanmax(np.abs(r - host)))
        _rec("sums", kind, f"{N}x{G}", labels, info["y_storage_name"], f"T exact {bool(np.array_equal(T, Tref))} (max rel {t_err:.2e})",
             f"Syy max rel {s_err:.2e}", f"r max abs {r_err:.2e}", f"group T equal {bool(np.array_equal(Tg, T))}",
             f"genes with mean >= 1e4: {int((Y[idx >= 0].mean(0) >= 1e4).sum())}")
        if base == "f32frac":
            np.testing.assert_allclose(T, Tref, rtol=1e-12, atol=0)
            np.testing.assert_allclose(Tg, Tref, rtol=1e-12, atol=0)
        else:
            assert np.array_equal(T, Tref), np.argwhere(T != Tref)[:5]
            assert np.array_equal(Tg, Tref)
        assert np.array_equal(Tg, T)
        # float64 sums of at most N terms each exact in float64 (y < 2^24): N half-ulps at the very most
        assert s_err <= N * 2.0 ** -53 and float((np.abs(Sg - Sref) / Sref).max()) <= N * 2.0 ** -53
        for rr in (r, correlations_from_sums(Tg, Sg, L, counts)):
            assert np.array_equal(np.isnan(rr), np.isnan(host))
            np.testing.assert_allclose(rr, host, rtol=1e-9, atol=1e-12, equal_nan=True)
    finally:
        one.close(); grp.close()


# ------------------------------------------------------------------ 3. PCA
_PCA_REF = {}


def _pca_ref(kind, shape, K):
    """(float64 scores of hostprep.pca_init, float32-model error per column, conditions) -- computed once per input, never changed."""
    key = (kind, shape, K)
    if key not in _PCA_REF:
        from clonealign_amd import hostprep
        Y = dc.variant(kind, *shape)
        ref = hostprep.pca_init(Y, K, None)
        ref.setflags(write=False)
        _PCA_REF[key] = (ref, dc.pca_model_error(Y, K), dc.pca_conditions(Y, 2))
    return _PCA_REF[key]


def _check_pca(eng, kind, shape, K, route, layout):
    N = shape[0]
    ref, model, (gap, sd) = _pca_ref(kind, shape, K)
    assert gap >= dc.GAP_MIN and sd > dc.SD_MIN, (gap, sd)
    dev = np.asarray(eng.pca_init(None, n_iter=60, seed=1))
    err = dc.sign_error(dev, ref)
    _rec("pca", kind, f"{shape[0]}x{shape[1]}", f"K={K}", route, eng.info()["y_storage_name"], "model " + " ".join(f"{m:.2e}" for m in model),
         "measured " + " ".join(f"{e:.2e}" for e in err), f"gap {gap:.2f}", f"min sd {sd:.2f}")
    assert (err < PCA_BAR).all(), (err, PCA_BAR)
    assert (err <= PCA_MODEL_FACTOR * model).all(), (err, model)
    np.testing.assert_allclose(dev.std(0, ddof=1), 1.0, rtol=1e-6)
    np.testing.assert_allclose(eng.get("psi"), dev, rtol=0, atol=1e-6)
    # noise goes in where the layout says: element (n, k) of the caller's matrix onto element (n, k) of the scores
    noise = np.random.default_rng([N, K]).normal(0, 0.05, size=(N, K))
    with_noise = np.asarray(eng.pca_init(np.asarray(noise, order="F" if layout == "col" else "C"), n_iter=60, seed=1))
    np.testing.assert_allclose(with_noise - dev, noise, rtol=0, atol=1e-12)
    np.testing.assert_allclose(eng.get("psi"), with_noise, rtol=0, atol=1e-6)


@pytest.mark.parametrize("shape", dc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", dc.VARIANTS)
def test_pca_init_matches_the_float64_svd(kind, shape):
    Y = dc.variant(kind, *shape)
    layout = "col" if (dc.VARIANTS.index(kind) + dc.SHAPES.index(shape)) % 2 else "row"
    for K in (1, 2):
        eng = _engine(Y, K=K, layout=layout, y_storage=dc.storage_arg(kind, Y))
        try:
            _check_store(eng, Y, dc.STORAGE[kind], kind == "u8ovf")
            _check_pca(eng, kind, shape, K, "dense-" + layout, layout)
        finally:
            eng.close()


@pytest.mark.parametrize("route", ["csr", "selection"])
def test_pca_init_on_sparse_created_and_selection_created_engines(route):
    kind, shape = ("u8ovf", (700, 300)) if route == "csr" else ("u16", (257, 1030))
    Y = dc.variant(kind, *shape)
    for K in (1, 2):
        if route == "csr":
            eng = _engine(_sparse(Y, "csr", np.int32), K=K)
        else:   # the variant's matrix cut out of a larger raw one at upload
            rng = np.random.default_rng(4)
            N, G = shape
            raw = rng.poisson(3.0, size=(N + 60, G + 45)).astype(np.float64)
            ci, gi = np.sort(rng.choice(N + 60, N, replace=False)), np.sort(rng.choice(G + 45, G, replace=False))
            raw[np.ix_(ci, gi)] = Y
            eng = _engine(raw, K=K, shape_fit=shape, cell_index=ci, gene_index=gi)
        try:
            assert eng.info()["y_storage_name"] == dc.STORAGE[kind]
            _check_pca(eng, kind, shape, K, route, "row")
        finally:
            eng.close()


def test_pca_init_refuses_a_constant_gene():
    from clonealign_amd.engine import EngineError
    for kind in ("u8", "u16", "f32frac"):
        Y = dc.variant(kind, 333, 95).copy()
        Y[:, 9] = 3.0
        eng = _engine(Y, y_storage=dc.STORAGE[kind])
        try:
            with pytest.raises(EngineError, match="constant/zero column"):
                eng.pca_init(None)
        finally:
            eng.close()


# ------------------------------------------------------------------ 4. mu guess
def _check_mu(eng, Y, tag):
    from clonealign_amd import hostprep
    want = hostprep.safe_inverse_softplus(hostprep.mu_guess(np.asarray(Y, dtype=np.float64), True))
    got = eng.get("loc")
    err = float(np.abs(got - want).max() / np.abs(want).max())
    _rec("mu", *tag, eng.info()["y_storage_name"], f"measured {err:.2e}")
    assert err <= MU_BAR, err


@pytest.mark.parametrize("shape", T_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", dc.VARIANTS)
def test_mu_guess_matches_the_host_formula(kind, shape):
    Y = dc.variant(kind, *shape)
    eng = _engine(Y, loc0=None, y_storage=dc.storage_arg(kind, Y))
    try:
        _check_store(eng, Y, dc.STORAGE[kind], kind == "u8ovf")
        _check_mu(eng, Y, (kind, f"{shape[0]}x{shape[1]}", "dense"))
    finally:
        eng.close()


@pytest.mark.parametrize("route", ["csr", "selection"])
def test_mu_guess_on_sparse_created_and_selection_created_engines(route):
    kind, shape = ("u8ovf", (700, 300)) if route == "csr" else ("f32int", (257, 1030))
    Y = dc.variant(kind, *shape)
    if route == "csr":
        eng = _engine(_sparse(Y, "csr", np.int32), loc0=None)
    else:
        rng = np.random.default_rng(4)
        N, G = shape
        raw = rng.poisson(3.0, size=(N + 60, G + 45)).astype(np.float64)
        ci, gi = np.sort(rng.choice(N + 60, N, replace=False)), np.sort(rng.choice(G + 45, G, replace=False))
        raw[np.ix_(ci, gi)] = Y
        eng = _engine(raw, loc0=None, shape_fit=shape, cell_index=ci, gene_index=gi)
    try:
        assert eng.info()["y_storage_name"] == dc.STORAGE[kind]
        _check_mu(eng, Y, (kind, f"{shape[0]}x{shape[1]}", route))
    finally:
        eng.close()


# ------------------------------------------------------------------ 5. ca_preprocess
@pytest.mark.parametrize("layout", ["row", "col"])
@pytest.mark.parametrize("dtype", ["float32", "uint8"])
def test_preprocess_sums_are_exact_and_masks_are_the_host_mirrors(dtype, layout):
    """2500 cells: three row blocks of the column-sum kernel, the last one ragged; float32 with counts up to 2^24 - 1, uint8 clipped at 255."""
    from clonealign_amd.engine import preprocess_masks
    from clonealign_amd.preprocess import preprocess_for_clonealign
    Yi, L = dc.preprocess_case()
    if dtype == "uint8":
        Yi = np.minimum(Yi, 255)
    Y = Yi.astype(dtype)
    assert np.array_equal(Y.astype(np.int64), Yi)
    N, G = Yi.shape
    for kw in (dict(min_counts_per_gene=20, min_counts_per_cell=25, nmads=10), dict(min_counts_per_gene=20, min_counts_per_cell=25, remove_outlying_genes=False)):
        kg, kc, gs, cs = preprocess_masks(Y, L, layout=layout, **kw)
        host = preprocess_for_clonealign(Yi.astype(np.float64), L, on="host", **kw)
        assert np.array_equal(np.flatnonzero(kg), host["retained_genes"]) and np.array_equal(np.flatnonzero(kc), host["retained_cells"])
        assert 0 < kg.sum() < G and 0 < kc.sum() < N
        assert np.array_equal(gs, Yi.sum(0).astype(np.float64))
        assert np.array_equal(cs, Yi[:, kg].sum(1).astype(np.float64))
        if dtype == "float32" and not kw.get("remove_outlying_genes", True):
            assert gs.max() > 2 ** 24 and cs.max() > 2 ** 24     # sums that a float32 accumulator would have rounded
