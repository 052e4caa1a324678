"""Sparse (CSR / CSC) count matrices on the host side (no GPU): the C ABI's ca_sparse against its ctypes mirror, and the Python layers
(api / inference / preprocess) giving on sparse input exactly what they give on the same matrix dense."""
import ctypes
import os
import subprocess
import warnings

import numpy as np
import pytest
import scipy.sparse as sps

import clonealign_amd as ca
from clonealign_amd import hostprep
from oracle.fused_numpy import FusedModel
from tests import _golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = dict(engine=FusedModel, engine_opts=dict(dtype="float32"))

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "clonealign_hip.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("ca_sparse %zu\n", sizeof(ca_sparse));
  F(ca_sparse, kind); F(ca_sparse, val_dtype); F(ca_sparse, index_bytes); F(ca_sparse, on_device); F(ca_sparse, nnz); F(ca_sparse, ptr);
  F(ca_sparse, idx); F(ca_sparse, val);
  printf("csr %d\ncsc %d\n", (int)CA_SPARSE_CSR, (int)CA_SPARSE_CSC);
  return 0;
}
"""


@pytest.fixture(scope="module")
def example():
    return _golden.example()


def test_ca_sparse_matches_the_header_as_the_c_compiler_lays_it_out(tmp_path):
    from clonealign_amd import engine
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).strip().splitlines())
    assert int(got["ca_sparse"]) == ctypes.sizeof(engine.CaSparse) == 48
    for name, _t in engine.CaSparse._fields_:
        assert int(got[f"ca_sparse.{name}"]) == getattr(engine.CaSparse, name).offset, name
    assert (int(got["csr"]), int(got["csc"])) == (engine.CA_SPARSE_CSR, engine.CA_SPARSE_CSC)


def test_sparse_entry_points_are_exported():
    from clonealign_amd import engine
    lib = engine.load_library()
    for s in ("ca_create_sparse", "ca_group_create_sparse"):
        assert s in engine.EXPORTS and hasattr(lib, s)


def test_sparse_counts_hands_over_the_arrays_without_a_dense_copy():
    from clonealign_amd.engine import CA_F64, CA_I32, CA_U8, CA_U16, CA_SPARSE_CSC, CA_SPARSE_CSR, sparse_counts
    rng = np.random.default_rng(1)
    Y = rng.poisson(0.5, size=(40, 30)).astype(np.float64)
    csr = sps.csr_matrix(Y)
    sp, keep = sparse_counts(csr)
    assert sp.kind == CA_SPARSE_CSR and sp.val_dtype == CA_F64 and sp.index_bytes == 4 and sp.nnz == csr.nnz
    assert keep[2] is csr.data and keep[0] is csr.indptr          # the caller's arrays themselves
    csc = sps.csc_matrix(Y.astype(np.int64))
    sp, keep = sparse_counts(csc)
    assert sp.kind == CA_SPARSE_CSC and sp.val_dtype == CA_U8 and keep[2].dtype == np.uint8   # narrowest exact dtype
    big = sps.csr_matrix(Y.astype(np.int64) * 300)
    assert sparse_counts(big)[0].val_dtype == CA_U16
    assert sparse_counts(sps.csr_matrix(Y.astype(np.int64) * 70000))[0].val_dtype == CA_I32
    wide = sps.csr_matrix(Y)
    wide.indptr, wide.indices = wide.indptr.astype(np.int64), wide.indices.astype(np.int64)
    assert sparse_counts(wide)[0].index_bytes == 8
    # duplicates / unsorted indices: canonicalised on a copy, the caller's matrix untouched
    dup = sps.csr_matrix((np.array([1.0, 2.0, 3.0]), np.array([2, 0, 2]), np.array([0, 3, 3])), shape=(2, 4))
    assert not dup.has_canonical_format
    sp, keep = sparse_counts(dup)
    assert list(keep[1]) == [0, 2] and list(keep[2]) == [2.0, 4.0] and sp.nnz == 2
    assert list(dup.indices) == [2, 0, 2]


def _fits_equal(a, b):
    assert np.array_equal(a["convergence_info"]["elbo"], b["convergence_info"]["elbo"])
    assert a["convergence_info"]["final_elbo"] == b["convergence_info"]["final_elbo"]
    assert a["ml_params"].keys() == b["ml_params"].keys()
    for k in a["ml_params"]:
        assert np.array_equal(a["ml_params"][k], b["ml_params"][k]), k
    assert list(a["clone"]) == list(b["clone"])
    assert np.array_equal(a["correlations"], b["correlations"], equal_nan=True)
    assert list(a["retained_genes"]) == list(b["retained_genes"])


def _cal(data, L, clones, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return ca.clonealign(data, L, clone_names=clones, verbose=False, max_iter=6, **ORACLE, **kw)


@pytest.mark.parametrize("form", ["csr", "csc", "coo", "sce", "csr_array"])
def test_clonealign_on_sparse_input_equals_the_dense_call(example, form):
    Y, L, clones, genes, cells = example
    dense = _cal(Y, L, clones, seed=3)
    if form == "sce":                                   # SCE stand-in whose counts assay is a dgCMatrix: genes x cells CSC
        data = {"assays": {"counts": sps.csc_matrix(Y.T)}}
    elif form == "csr_array":
        data = sps.csr_array(Y)
    else:
        data = getattr(sps, f"{form}_matrix")(Y)
    sparse = _cal(data, L, clones, seed=3)
    _fits_equal(sparse, dense)


def test_clonealign_on_a_non_canonical_sparse_matrix_equals_its_canonical_form(example):
    Y, L, clones, genes, cells = example
    coo = sps.coo_matrix(Y)
    # split every entry into two halves in reversed order: duplicates and unsorted indices within each row
    r, c, v = coo.row, coo.col, coo.data.astype(np.float64)
    half = np.floor(v / 2)
    raw = sps.csr_matrix((np.concatenate([v - half, half])[::-1], (np.concatenate([r, r])[::-1], np.concatenate([c, c])[::-1])),
                         shape=Y.shape)
    raw.has_canonical_format = False
    assert np.array_equal(raw.toarray(), Y)
    _fits_equal(_cal(raw, L, clones, seed=5), _cal(sps.csr_matrix(Y), L, clones, seed=5))


def test_clonealign_selection_on_sparse_input_equals_the_dense_selection(example):
    Y, L, clones, genes, cells = example
    rng = np.random.default_rng(8)
    kc = rng.random(Y.shape[0]) < 0.8
    kg = rng.random(Y.shape[1]) < 0.7
    a = _cal(sps.csc_matrix(Y), L[kg], clones, seed=2, cell_index=kc, gene_index=kg)
    b = _cal(Y, L[kg], clones, seed=2, cell_index=kc, gene_index=kg)
    _fits_equal(a, b)


def test_parse_expression_keeps_sparse_input_sparse(example):
    from clonealign_amd.api import _parse_expression
    Y = example[0]
    csr = sps.csr_matrix(Y)
    got, names = _parse_expression(csr)
    assert got is csr and names is None
    got, _ = _parse_expression({"assays": {"counts": sps.csc_matrix(Y.T)}})
    assert sps.issparse(got) and got.format == "csr" and np.array_equal(got.toarray(), Y)


def test_selected_sums_of_a_sparse_matrix_equal_the_dense_sums(example):
    Y = example[0]
    rng = np.random.default_rng(4)
    rows = np.flatnonzero(rng.random(Y.shape[0]) < 0.6)
    cols = np.flatnonzero(rng.random(Y.shape[1]) < 0.6)
    for S in (sps.csr_matrix(Y), sps.csc_matrix(Y)):
        for r, c in ((None, None), (rows, None), (None, cols), (rows, cols)):
            for axis in (0, 1):
                assert np.array_equal(hostprep.selected_sums(S, r, c, axis), hostprep.selected_sums(Y, r, c, axis))


@pytest.mark.parametrize("fmt", ["csr", "csc"])
def test_preprocess_on_sparse_input_equals_the_dense_result(example, fmt):
    Y, L, clones, genes, cells = example
    S = getattr(sps, f"{fmt}_matrix")(Y)
    kw = dict(min_counts_per_gene=20, min_counts_per_cell=100)
    d = ca.preprocess_for_clonealign(Y, L, **kw)
    s = ca.preprocess_for_clonealign(S, L, **kw)
    assert sps.issparse(s["gene_expression_data"]) and s["gene_expression_data"].format == "csr"
    assert np.array_equal(s["gene_expression_data"].toarray(), d["gene_expression_data"])
    assert np.array_equal(s["copy_number_data"], d["copy_number_data"])
    assert list(s["retained_cells"]) == list(d["retained_cells"]) and list(s["retained_genes"]) == list(d["retained_genes"])
    m = ca.preprocess_for_clonealign(S, L, return_masks=True, **kw)
    assert list(m["retained_cells"]) == list(d["retained_cells"]) and list(m["retained_genes"]) == list(d["retained_genes"])
    assert m["keep_genes"].sum() == len(d["retained_genes"]) and m["keep_cells"].sum() == len(d["retained_cells"])
    assert np.array_equal(Y[np.ix_(m["keep_cells"], m["keep_genes"])], d["gene_expression_data"])
    assert np.array_equal(m["copy_number_data"], d["copy_number_data"])
    with pytest.raises(ValueError, match="dense"):
        ca.preprocess_for_clonealign(S, L, on="device", **kw)


def test_inference_keeps_a_big_sparse_matrix_sparse_and_refuses_what_needs_the_host_matrix():
    from clonealign_amd.inference import _sparse_input
    Y = sps.random(3000, 2000, density=0.01, format="csr", random_state=1)
    assert _sparse_input(Y, None, None, None, None, "auto", 1) is Y          # above 4e6 counts: stays sparse
    assert _sparse_input(Y.tocsc(), None, None, None, None, "auto", 1).format == "csc"
    small = _sparse_input(Y, np.arange(100), None, None, None, "auto", 1)   # the selection is small: densified
    assert isinstance(small, np.ndarray) and np.array_equal(small, Y.toarray())
    assert isinstance(_sparse_input(Y, None, None, FusedModel, None, "auto", 1), np.ndarray)   # engine= other than the HIP engine
    with pytest.raises(ValueError, match="devices="):
        _sparse_input(Y, None, None, None, dict(rank=0, world=2), "auto", 1)
    with pytest.raises(ValueError, match="devices="):
        _sparse_input(Y, None, None, None, None, "host", 1)
    assert _sparse_input(Y, None, None, None, None, "host", 0) is Y         # K = 0: no PCA, nothing needs the host matrix
