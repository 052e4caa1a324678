"""Sparse (CSR / CSC) count matrices on the MI355X (ca_create_sparse / ca_group_create_sparse): the device ingest builds exactly the
resident matrix, storage pick and u8 overflow list the dense ca_create builds, so every fit on sparse input is the dense fit bit for bit.
That is the oracle of every test here: the same problem through both entry points, compared with np.array_equal."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sps

from tests._cases import make_case

pytestmark = pytest.mark.gpu


def _drive(eng, G, S, n_iter=6):
    from clonealign_amd.rng import EpsStream
    tr = eng.run(EpsStream(77, S, G), n_iter, 1e-12)
    fin = eng.final_elbo(EpsStream(78, S, G), 3)
    return np.asarray(tr), np.asarray(fin), eng.get_params()


def _same_fit(dense, sparse, G, S):
    i1, i2 = dense.info(), sparse.info()
    assert i1 == i2
    t1, f1, p1 = _drive(dense, G, S)
    t2, f2, p2 = _drive(sparse, G, S)
    assert np.array_equal(t1, t2) and np.array_equal(f1, f2)
    assert p1.keys() == p2.keys()
    for k in p1:
        assert np.array_equal(p1[k], p2[k]), k
    return i1


def _values(kind, shape, seed):
    """Counts whose storage pick is `kind` (C = 4 clones, K = 1): u8, u8 with overflow entries, u16 (more than 1/64 above 255), f32."""
    rng = np.random.default_rng(seed)
    Y = rng.poisson(0.6, size=shape).astype(np.float64)
    Y[:, 0] += 1
    Y[0, :] += 1
    n = Y.size
    if kind == "u8ovf":
        flat = rng.choice(n, n // 200, replace=False)
        Y.flat[flat] = rng.integers(256, 5000, size=flat.size)
    elif kind == "u16":
        flat = rng.choice(n, n // 30, replace=False)
        Y.flat[flat] = rng.integers(256, 60000, size=flat.size)
    elif kind == "f32":
        Y[3, 5] = 2.5
    return Y


def _as(Y, fmt, vdtype, ib, device):
    """Y as a scipy / torch sparse matrix: format, value dtype, index width, host or device arrays."""
    m = (sps.csr_matrix if fmt == "csr" else sps.csc_matrix)(Y.astype(vdtype))
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


FORMS = [("csr", np.float64, 4, False), ("csc", np.float64, 4, False), ("csr", np.int32, 8, False), ("csc", np.float32, 8, False),
         ("csr", np.float32, 8, True), ("csc", np.float64, 4, True)]
STORE = {"u8": "u8", "u8ovf": "u8", "u16": "u16", "f32": "f32"}


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f"{f[0]}-{np.dtype(f[1]).name}-i{f[2]}-{'dev' if f[3] else 'host'}")
@pytest.mark.parametrize("kind", list(STORE))
def test_sparse_create_is_bit_identical_to_dense(kind, form):
    from clonealign_amd.engine import HipEngine
    fmt, vdt, ib, dev = form
    if kind == "f32" and vdt == np.int32:
        pytest.skip("non-integral counts have no int32 form")
    case = make_case(N=300, G=150, C=4, K=1, seed=11)
    Y = _values(kind, (300, 150), 5)
    dense = HipEngine(**{**case, "Y": Y})
    sparse = HipEngine(**{**case, "Y": _as(Y, fmt, vdt, ib, dev)})
    try:
        info = _same_fit(dense, sparse, 150, 1)
        assert info["y_storage_name"] == STORE[kind]
    finally:
        dense.close(); sparse.close()


@pytest.mark.parametrize("fmt", ["csr", "csc"])
def test_sparse_selection_equals_the_dense_selection_and_the_pick_follows_it(fmt):
    from clonealign_amd.engine import HipEngine
    rng = np.random.default_rng(3)
    N, G = 400, 260
    case = make_case(N=N, G=G, C=4, K=1, seed=12)
    Y = _values("u8", (N, G), 6)
    Y[17, 40] = 0.5                         # the only non-integral count: its cell is not selected
    Y[:, 100:105] = rng.integers(300, 900, (N, 5))   # every count above 255 (more than 1/64 of all) lies in five genes: not selected
    ci = np.flatnonzero((rng.random(N) < 0.8) & (np.arange(N) != 17))
    gi = np.flatnonzero((rng.random(G) < 0.7) & ((np.arange(G) < 100) | (np.arange(G) >= 105))).astype(np.int32)
    sel = dict(L=case["L"][gi], psi0=case["psi0"][ci], loc0=case["loc0"][gi], K=1, S=1, cell_index=ci, gene_index=gi)
    dense = HipEngine(Y, **sel)
    sparse = HipEngine(_as(Y, fmt, np.float64, 4, False), **sel)
    try:
        assert _same_fit(dense, sparse, len(gi), 1)["y_storage_name"] == "u8"
    finally:
        dense.close(); sparse.close()
    # gene selection only, keeping the overflow genes: u16 on both (more than 1/64 of the selected counts above 255)
    gi2 = np.arange(0, 120, dtype=np.int32)
    sel2 = dict(L=case["L"][gi2], psi0=case["psi0"], loc0=case["loc0"][gi2], K=1, S=1, gene_index=gi2)
    Y2 = Y.copy(); Y2[17, 40] = 1.0
    dense = HipEngine(Y2, **sel2)
    sparse = HipEngine(_as(Y2, fmt, np.float64, 8, False), **sel2)
    try:
        assert _same_fit(dense, sparse, len(gi2), 1)["y_storage_name"] == "u16"
    finally:
        dense.close(); sparse.close()


def test_sparse_edge_cases_all_zero_gene_and_explicit_zero_are_accepted():
    from clonealign_amd.engine import HipEngine
    case = make_case(N=200, G=90, C=3, K=1, seed=13)
    Y = _values("u8", (200, 90), 7)
    Y[:, 7] = 0.0                            # an all-zero gene
    Y[5, 8] = 3.0
    m2 = sps.csr_matrix(Y)
    k = m2.indptr[5] + int(np.flatnonzero(m2.indices[m2.indptr[5]:m2.indptr[6]] == 8)[0])
    m2.data[k] = 0.0                         # ... and an explicit stored zero in a run
    Y[5, 8] = 0.0
    dense = HipEngine(**{**case, "Y": Y})
    sparse = HipEngine(**{**case, "Y": m2})
    try:
        _same_fit(dense, sparse, 90, 1)
    finally:
        dense.close(); sparse.close()


def test_sparse_all_zero_cell_is_refused_as_on_the_dense_path():
    import clonealign_amd as ca
    rng = np.random.default_rng(2)
    N, G = 2100, 2000
    Y = sps.random(N, G, density=0.02, format="csr", random_state=3, data_rvs=lambda n: rng.integers(1, 5, n).astype(np.float64))
    Y = sps.csr_matrix(Y.toarray() * (np.arange(N) != 9)[:, None])   # cell 9 has no counts
    L = rng.integers(1, 4, size=(G, 3)).astype(np.float64)
    with pytest.raises(ValueError, match="Some cells have no counts mapping"):
        ca.clonealign(Y, L, verbose=False, max_iter=2, seed=1)


def _malformed():
    rng = np.random.default_rng(4)
    Y = rng.poisson(1.0, size=(30, 20)).astype(np.float64)
    Y[:, 0] += 1
    out = {}

    def mk(edit, msg):
        m = sps.csr_matrix(Y)
        edit(m)
        m.has_canonical_format = True      # hand the arrays over exactly as edited
        return m, msg
    out["negative"] = mk(lambda m: m.data.__setitem__(3, -1.0), "negative or NaN")
    out["nan"] = mk(lambda m: m.data.__setitem__(4, np.nan), "negative or NaN")
    out["index_out_of_range"] = mk(lambda m: m.indices.__setitem__(m.indptr[2], 25), "out of range")
    out["unsorted"] = mk(lambda m: m.indices.__setitem__(slice(m.indptr[3], m.indptr[3] + 2), m.indices[m.indptr[3]:m.indptr[3] + 2][::-1].copy()),
                         "strictly increasing")
    out["duplicate"] = mk(lambda m: m.indices.__setitem__(m.indptr[4] + 1, m.indices[m.indptr[4]]), "strictly increasing")
    out["decreasing_ptr"] = mk(lambda m: m.indptr.__setitem__(5, m.indptr[4] - 1), "ptr must")
    out["ptr_last_not_nnz"] = mk(lambda m: m.indptr.__setitem__(-1, m.indptr[-1] - 1), "ptr must")
    return Y, out


@pytest.mark.parametrize("name", ["negative", "nan", "index_out_of_range", "unsorted", "duplicate", "decreasing_ptr", "ptr_last_not_nnz"])
def test_sparse_malformed_input_is_refused_with_a_message(name):
    from clonealign_amd.engine import EngineError, HipEngine
    Y, cases = _malformed()
    m, msg = cases[name]
    case = make_case(N=30, G=20, C=3, K=1, seed=1)
    with pytest.raises(EngineError, match=msg) as e:
        HipEngine(**{**case, "Y": m})
    assert e.value.code == 1
    if name == "negative":                   # the dense path says the same
        with pytest.raises(EngineError, match=msg):
            HipEngine(**{**case, "Y": m.toarray()})
    # the device is fine afterwards
    eng = HipEngine(**{**case, "Y": sps.csr_matrix(Y)})
    eng.close()


def test_sparse_entry_point_refuses_a_dense_y_beside_it():
    import ctypes as C
    from clonealign_amd import engine as E
    case = make_case(N=30, G=20, C=3, K=1, seed=1)
    eng = E.HipEngine.__new__(E.HipEngine)
    prob, opt = eng._prepare(sps.csr_matrix(case["Y"]), case["L"], case["psi0"], case["loc0"], 1, 1, None, None, 0.1, 0, "auto", 1, 0, 1,
                             False, None, None, None, "row", None, None, (), (), None, False, 0, 0)
    prob.Y = C.c_void_p(case["Y"].ctypes.data)
    h = C.c_void_p()
    assert eng.lib.ca_create_sparse(C.byref(prob), C.byref(eng._sparse), C.byref(opt), C.byref(h)) == 1
    assert b"must be NULL" in eng.lib.ca_last_error(None)
    assert not h.value


def _info_of_fits(monkeypatch):
    """Record ca_info of every HipEngine as it closes (clonealign() closes its engine itself)."""
    from clonealign_amd import engine as E
    seen = []
    orig = E.HipEngine.close

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            seen.append(self.info())
        orig(self)
    monkeypatch.setattr(E.HipEngine, "close", close)
    return seen


def test_cfg3_sparse_clonealign_is_the_dense_fit_and_makes_no_host_matrix(monkeypatch):
    import tracemalloc

    import clonealign_amd as ca
    import synth_data as synth
    N, G, C = 100_000, 5_000, 8                          # BASELINE cfg-3
    prob = synth.make_problem(N, G, C, seed=20240)
    Yd, L = prob["Y"], prob["L"]
    csr = sps.csr_matrix(Yd)
    seen = _info_of_fits(monkeypatch)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dense = ca.clonealign(Yd, L, seed=7, max_iter=50, verbose=False)
        reuse = {}
        tracemalloc.start()
        try:
            sparse = ca.clonealign(csr, L, seed=7, max_iter=50, verbose=False, _reuse=reuse)
            _cur, peak = tracemalloc.get_traced_memory()
        finally:
            tracemalloc.stop()
    try:
        assert sps.issparse(reuse["prep"]["Y_dat"])             # the prepared matrix stayed sparse ...
        assert peak < N * G // 8, peak                          # ... and no N x G array was made on the host (not even 1 byte per count)
        seen.append(reuse["eng"].info())
    finally:
        reuse["eng"].close()
    assert np.array_equal(dense["convergence_info"]["elbo"], sparse["convergence_info"]["elbo"])
    assert dense["convergence_info"]["final_elbo"] == sparse["convergence_info"]["final_elbo"]
    for k in dense["ml_params"]:
        assert np.array_equal(dense["ml_params"][k], sparse["ml_params"][k]), k
    assert list(dense["clone"]) == list(sparse["clone"])
    assert np.array_equal(dense["correlations"], sparse["correlations"], equal_nan=True)
    a, b = seen[0], seen[-1]
    assert (a["fwd_series"], a["series_passes"], a["y_storage_name"]) == (b["fwd_series"], b["series_passes"], b["y_storage_name"])


def _mid_problem(seed=21):
    """Above the 4e6-count threshold, so sparse input takes the device path (4400 x 1000)."""
    case = make_case(N=4400, G=1000, C=4, K=1, seed=seed, scale=0.3)
    return case["Y"].astype(np.int32), case["L"]


def test_sharded_sparse_inference_equals_the_dense_one():
    from clonealign_amd.inference import inference_tflow
    Y, L = _mid_problem()
    kw = dict(max_iter=15, verbose=False, seed=4, devices=[0, 0])
    a = inference_tflow(sps.csc_matrix(Y), L, **kw)
    b = inference_tflow(Y, L, **kw)
    assert np.array_equal(a["convergence_info"]["elbo"], b["convergence_info"]["elbo"])
    assert a["convergence_info"]["final_elbo"] == b["convergence_info"]["final_elbo"]
    for k in b["ml_params"]:
        assert np.array_equal(a["ml_params"][k], b["ml_params"][k]), k


def test_run_clonealign_restarts_on_sparse_input_equal_the_dense_restarts():
    import clonealign_amd as ca
    Y, L = _mid_problem(seed=22)
    kw = dict(initial_shrinks=(0, 5), n_repeats=2, seed=9, max_iter=15, verbose=False, print_elbos=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = ca.run_clonealign(sps.csr_matrix(Y), L, **kw)
        b = ca.run_clonealign(Y, L, **kw)
    assert np.array_equal(a["multirun_info"]["elbos"], b["multirun_info"]["elbos"])
    assert np.array_equal(a["convergence_info"]["elbo"], b["convergence_info"]["elbo"])
    for k in b["ml_params"]:
        assert np.array_equal(a["ml_params"][k], b["ml_params"][k]), k
    assert list(a["clone"]) == list(b["clone"])
