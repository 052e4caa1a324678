"""ca_clone_loglik_by_block / HipEngine.clone_loglik_by_block / clone_loglik_by_block / assignment_support: the four sufficient statistics of the
log-likelihood per (cell, block of genes) from one float64 sweep over the resident count matrix.

The yardstick is ``ref_ll`` of tests/test_gpu_clone_loglik.py on the RESTRICTED matrices: from the device's four arrays, ``within[:, b]`` and
``without[:, b]`` -- composed by the public function's own arithmetic, ``api._by_block_terms`` -- must be the log-likelihood of block b's columns alone
and of the matrix with block b's columns deleted.  Bar: ``1e-10 x scale`` with ``ref_ll``'s scale on the same restricted matrix (the sum of the terms'
magnitudes; tests/test_gpu_clone_loglik.py has the reasoning); ``s`` is exact (integer counts, and float32 values over 21 binades, add exactly in
float64) and ``lg`` is good to 1e-10 relative (a sum of non-negative terms).  The device call always covers every cell; on the two larger shapes the
float64 restatement is taken on a subset of the rows (both ends of the cell axis, where the partial waves and blocks are, and every 11th cell between):
a cell's values depend on its row alone, which the bit tests below pin down."""
import numpy as np
import pytest
from scipy.special import gammaln

from clonealign_amd import api
from tests._cases import make_case
from tests.test_block_loglik_host import HostOnly, contiguous_labels, interleaved_labels, planted_fit
from tests.test_gpu_clone_loglik import factors, ref_ll
from tests.test_gpu_fit_mse import SHAPES, problem

pytestmark = pytest.mark.gpu
RTOL = 1e-10
LABELLINGS = {"contiguous": contiguous_labels, "mod5of7": interleaved_labels, "one": lambda G: (np.zeros(G, dtype=np.int32), 1)}
CASES = [(SHAPES[0], "u8"), (SHAPES[1], "u8"), (SHAPES[2], "u8"), (SHAPES[1], "u16"), (SHAPES[1], "f32")]


def engine_for(Y, L, storage="u8", **kw):
    from clonealign_amd.engine import HipEngine
    N, G = Y.shape
    return HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, y_storage=storage, **kw)


def ref_rows(N):
    if N <= 1024:
        return np.arange(N)
    return np.unique(np.concatenate([np.arange(192), np.arange(192, N - 192, 11), np.arange(N - 192, N)]))


def same(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]) for k in ("A", "logZ", "s", "lg"))


def rows_of(st, lo, hi):
    return {k: (None if v is None else v[lo:hi]) for k, v in st.items()}


def stacked(parts):
    return {k: (None if parts[0][k] is None else np.concatenate([p[k] for p in parts])) for k in ("A", "logZ", "s", "lg")}


def close(out, ref, scale, tag):
    assert out.shape == ref.shape, tag
    assert not np.isnan(out).any(), tag
    assert np.array_equal(np.isneginf(out), np.isneginf(ref)), tag
    ok = np.isfinite(ref)
    assert np.isfinite(out[ok]).all(), tag
    worst = float((np.abs(out[ok] - ref[ok]) / np.maximum(scale[ok], 1e-300)).max()) if ok.any() else 0.0
    assert (np.abs(out[ok] - ref[ok]) <= RTOL * scale[ok]).all(), (tag, worst)
    return worst


def check_against_restricted(st, Y, E, U, V, bg, B, const, rows, tag):
    """within / without of the device's arrays against ref_ll on the restricted matrices, s and lg against their definitions, on the cells ``rows``."""
    sub = {k: (None if v is None else v[rows]) for k, v in st.items()}
    terms = api._by_block_terms(sub["A"], sub["logZ"], sub["s"], sub["lg"])
    Yr = np.asarray(Y[rows], dtype=np.float64)
    Ur = None if U is None else U[rows]
    worst = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in range(B):
            inb, out = np.flatnonzero(bg == b), np.flatnonzero(bg != b)
            assert np.array_equal(sub["s"][:, b], Yr[:, inb].sum(1)), f"{tag} s {b}"
            if const:
                np.testing.assert_allclose(sub["lg"][:, b], gammaln(Yr[:, inb] + 1.0).sum(1), rtol=RTOL, atol=0, err_msg=f"{tag} lg {b}")
            for name, keep in (("within", inb), ("without", out)):
                if keep.size == 0:
                    assert (terms[name][:, b] == 0).all(), f"{tag} {name} {b}"
                    continue
                ref, scale = ref_ll(Yr[:, keep], E[keep], Ur, None if V is None else V[keep], const=const)
                worst = max(worst, close(terms[name][:, b], ref, scale, f"{tag} {name} {b}"))
    print(f"clone_loglik_by_block {tag}: max |term - ref| / scale {worst:.2e}")
    return terms


@pytest.mark.parametrize("labelling", sorted(LABELLINGS))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[0])) + "-" + c[1])
def test_parity_with_the_float64_restatement_on_the_restricted_matrices(case, labelling):
    (N, G, C), storage = case
    Y, L, mu, _idx, rng = problem(N, G, C, storage, seed=sum(case[0]))
    E = mu[:, None] * L
    U, V = factors(N, G, 3, rng)
    bg, B = LABELLINGS[labelling](G)
    rows = ref_rows(N)
    eng = engine_for(Y, L, storage)
    try:
        assert eng.info()["y_storage_name"] == storage
        for D in (0, 1, 3):
            Uv, Vv = (None, None) if D == 0 else (U[:, :D], V[:, :D])
            for const in (True, False):
                st = eng.clone_loglik_by_block(E, Uv, Vv, bg, B, const=const)
                assert st["A"].shape == st["logZ"].shape == (N, B, C) and st["s"].shape == (N, B) and (st["lg"] is None) == (not const)
                check_against_restricted(st, Y, E, Uv, Vv, bg, B, const, rows, f"{case} {labelling} D={D} const={const}")
                assert same(eng.clone_loglik_by_block(E, Uv, Vv, bg, B, const=const), st)       # two calls: identical bits
            for b in range(B):                                       # an empty block: 0, 0, 0 and -inf
                if not (bg == b).any():
                    assert (st["A"][:, b] == 0).all() and (st["s"][:, b] == 0).all() and np.isneginf(st["logZ"][:, b]).all()
    finally:
        eng.close()


@pytest.mark.parametrize("case", [(SHAPES[1], "contiguous"), (SHAPES[1], "mod5of7"), (SHAPES[2], "mod5of7")], ids=lambda c: "x".join(map(str, c[0])) + "-" + c[1])
def test_a_cell_does_not_depend_on_its_range_its_batch_or_the_block_numbering(case):
    """(5000, 2049, 20) with ``g % 5``: every gene is a run, and 2049 runs of 20 + 2 columns are 361 kB of slab per cell (707 kB with the chunks of Z at
    D = 2), so the budget of 1 GiB takes the cells 2816 (1280) at a time -- more than one internal batch -- and the ranged calls are cut into batches at
    other cells."""
    (N, G, C), labelling = case
    Y, L, mu, _idx, rng = problem(N, G, C, "u8", seed=sum(case[0]) + 1)
    E = mu[:, None] * L
    U, V = factors(N, G, 2, rng)
    bg, B = LABELLINGS[labelling](G)
    eng = engine_for(Y, L)
    try:
        for Uv, Vv in ((None, None), (U, V)):
            whole = eng.clone_loglik_by_block(E, Uv, Vv, bg, B)
            parts = [eng.clone_loglik_by_block(E, Uv, Vv, bg, B, cells=r) for r in ((0, 100), (100, N - 100), (N - 100, N))]
            assert same(stacked(parts), whole)
            assert eng.clone_loglik_by_block(E, Uv, Vv, bg, B, cells=(70, 70))["A"].shape == (0, B, C)
            perm = np.random.default_rng(3).permutation(B).astype(np.int32)
            moved = eng.clone_loglik_by_block(E, Uv, Vv, perm[bg], B, cells=(0, 700))
            for k in ("A", "logZ", "s", "lg"):
                assert np.array_equal(moved[k][:, perm], whole[k][:700]), k
    finally:
        eng.close()


def test_group_returns_the_single_handle_bits():
    from clonealign_amd.engine import EngineError, HipGroupEngine
    N, G, C = SHAPES[1]
    Y, L, mu, _idx, rng = problem(N, G, C, "u8", seed=31)
    E = mu[:, None] * L
    U, V = factors(N, G, 1, rng)
    bg, B = contiguous_labels(G)
    one = engine_for(Y, L)
    try:
        o1 = one.clone_loglik_by_block(E, U, V, bg, B)
        o0 = one.clone_loglik_by_block(E, None, None, bg, B, const=False, cells=(1400, 1700))
    finally:
        one.close()
    grp = HipGroupEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, devices=[0, 0])
    try:
        assert same(grp.clone_loglik_by_block(E, U, V, bg, B), o1)
        assert same(grp.clone_loglik_by_block(E, None, None, bg, B, const=False, cells=(1400, 1700)), o0)      # a range across the two shards
        bad = U.copy()
        bad[N - 1, 0] = np.nan                                       # refused on one rank's cells: refused by the group, which stays usable
        with pytest.raises(EngineError) as ex:
            grp.clone_loglik_by_block(E, bad, V, bg, B)
        assert ex.value.code == 1 and "U has a non-finite entry" in ex.value.msg, ex.value.msg
        assert same(grp.clone_loglik_by_block(E, U, V, bg, B), o1)
    finally:
        grp.close()


@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_zero_copy_number_and_extreme_exponents(shape):
    """The construction of the test of this name in tests/test_gpu_clone_loglik.py, by block."""
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
    bg, B = contiguous_labels(G)
    eng = engine_for(Y, np.maximum(L, 1.0))
    try:
        for Uv, Vv in ((None, None), (U, V)):
            st = eng.clone_loglik_by_block(E, Uv, Vv, bg, B)
            for k in ("A", "logZ", "s", "lg"):
                assert not np.isnan(st[k]).any(), k
            assert not np.isposinf(st["logZ"]).any() and np.isfinite(st["logZ"]).all()       # (every block has a gene with E > 0 in every clone)
            want = np.zeros((N, B, C), dtype=bool)
            want[11, bg[7], c0] = True
            assert np.array_equal(np.isneginf(st["A"]), want)
            terms = check_against_restricted(st, Y, E, Uv, Vv, bg, B, True, np.arange(N), f"{shape} zeros of E, D={0 if Uv is None else 2}")
            assert np.isfinite(terms["within"][20]).all() and np.isfinite(terms["without"][20]).all()
            assert np.isneginf(terms["without"][11, :, c0]).sum() == B - 1 and np.isfinite(terms["without"][11, bg[7], c0])
    finally:
        eng.close()


def test_sparse_upload_gives_the_dense_engine_bits():
    import scipy.sparse as sps
    N, G, C = SHAPES[1]
    Y, L, mu, _idx, rng = problem(N, G, C, "u8", seed=12)
    E = mu[:, None] * L
    U, V = factors(N, G, 2, rng)
    bg, B = contiguous_labels(G)
    outs = []
    for M in (Y, sps.csr_matrix(Y)):
        eng = engine_for(M, L)
        try:
            outs.append(eng.clone_loglik_by_block(E, U, V, bg, B))
        finally:
            eng.close()
    assert same(outs[0], outs[1])


def test_layouts_agree():
    from clonealign_amd.engine import HipEngine
    N, G, C = 1500, 700, 5
    Y, L, mu, _idx, rng = problem(N, G, C, "u8", seed=13)
    E = mu[:, None] * L
    U, V = factors(N, G, 2, rng)
    bg, B = interleaved_labels(G)
    outs = {}
    for lay in ("row", "col"):
        eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, layout=lay)
        try:
            f = np.asfortranarray if lay == "col" else np.ascontiguousarray
            outs[lay] = eng.clone_loglik_by_block(f(E), f(U), f(V), bg, B, cells=(3, 1400))
        finally:
            eng.close()
    assert same(outs["row"], outs["col"])


def test_refusals_name_the_offender_and_poll_hooks_are_refused():
    from clonealign_amd.engine import EngineError, HipEngine
    from clonealign_amd.rng import EpsStream
    case = make_case(N=700, G=300, C=4, K=1, seed=2)
    L = case["L"]
    rng = np.random.default_rng(0)
    U, V = factors(700, 300, 2, rng)
    bg, B = interleaved_labels(300)
    eng = HipEngine(**case)
    try:
        def refused(words, *a, **k):
            with pytest.raises(EngineError) as ex:
                eng.clone_loglik_by_block(*a, **k)
            assert ex.value.code == 1 and all(w in ex.value.msg for w in words), ex.value.msg
        hi = bg.copy()
        hi[123] = 7
        refused(("block_of_gene[123] = 7", "outside [0, 7)"), L, U, V, hi, B)
        lo = bg.copy()
        lo[4] = -1
        refused(("block_of_gene[4] = -1",), L, U, V, lo, B)
        refused(("n_blocks = 0",), L, U, V, np.zeros(300, dtype=np.int32), 0)
        refused(("cell range", "outside [0, 700]"), L, U, V, bg, B, cells=(650, 701))
        refused(("cell range", "outside [0, 700]"), L, U, V, bg, B, cells=(-1, 10))
        Ub = U.copy()
        Ub[9, 1] = np.nan
        refused(("U has a non-finite", "cell 9"), L, Ub, V, bg, B)
        E = L.copy()
        E[17, 2] = -1.0
        refused(("gene 17", "clone 2"), E, U, V, bg, B)
        refused(("D = 9", "outside [0, 8]"), L, np.zeros((700, 9)), np.zeros((300, 9)), bg, B)
        with pytest.raises(ValueError):
            eng.clone_loglik_by_block(L, U, V, bg[:-1], B)
        with pytest.raises(ValueError):
            eng.clone_loglik_by_block(L, U, V, bg.astype(np.float64), B)
        import ctypes as C
        out = [np.zeros((700, B * 4)), np.zeros((700, B * 4)), np.zeros((700, B))]
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        rc = eng.lib.ca_clone_loglik_by_block(eng.h, p(L), None, None, 0, 1, p(bg), B, 0, 700, p(out[0]), p(out[1]), p(out[2]), None)
        assert rc == 1 and b"lg" in eng.lib.ca_last_error(eng.h) and b"NULL" in eng.lib.ca_last_error(eng.h)
        seen = {}

        def hook(i, e):
            if i == 2:
                with pytest.raises(EngineError) as ex:
                    eng.clone_loglik_by_block(L, None, None, bg, B)
                seen["code"] = ex.value.code
            return False
        eng.run(EpsStream(9, 1, 300), 4, 1e-12, poll=hook)
        assert seen["code"] == 6                                     # CA_ERR_STATE
        st = eng.clone_loglik_by_block(L, U, V, bg, B)
        check_against_restricted(st, case["Y"], L, U, V, bg, B, True, np.arange(700), "after the run")
    finally:
        eng.close()


def test_assignment_support_through_a_live_fit_engine():
    import clonealign_amd as ca
    from clonealign_amd.engine import HipEngine
    N, G, C = 1200, 400, 3
    Y, L, fit, rng = planted_fit(N, G, C, seed=17)
    blocks = np.array(["1p"] * 90 + ["1q"] * 130 + ["7"] * 1 + ["X"] * 179, dtype=object)
    extra = rng.normal(size=(N, C))
    case = make_case(N=N, G=G, C=C, K=1, seed=17, scale=1.0)
    eng = HipEngine(**case)                                          # the engine of a fit: its resident matrix is Y
    try:
        assert np.array_equal(case["Y"], Y)
        eng.iterate(2, None)
        dev = ca.assignment_support(fit, Y, L, blocks, extra_loglik=extra, psi="fit", engine=eng)
        again = ca.assign_cells(fit, Y, L, extra_loglik=extra, psi="fit", engine=eng)
    finally:
        eng.close()
    host = ca.assignment_support(fit, Y, L, blocks, extra_loglik=extra, psi="fit", engine=HostOnly(N, G))
    for k in ("clone_probs", "loglik", "clone_loglik"):
        assert np.array_equal(dev[k], again[k]), k                   # everything assign_cells returns, identically
    assert np.array_equal(dev["clone"], again["clone"]) and np.array_equal(dev["clone"], host["clone"])
    assert np.array_equal(dev["clone_without"], host["clone_without"]) and np.array_equal(dev["n_flips"], host["n_flips"])
    assert list(dev["block_names"]) == ["1p", "1q", "7", "X"] and np.array_equal(dev["counts"], host["counts"])
    E = fit["ml_params"]["mu"][:, None] * L
    U, V = fit["ml_params"]["psi"], fit["ml_params"]["W"]
    for b, name in enumerate(dev["block_names"]):
        for key, keep in (("within", np.flatnonzero(blocks == name)), ("without", np.flatnonzero(blocks != name))):
            _ref, scale = ref_ll(Y[:, keep], E[keep], U, V[keep])
            close(dev[key][:, b], host[key][:, b], scale, f"assignment_support {key} {name}")
    d = float(np.abs(dev["probs_without"] - host["probs_without"]).max())
    print(f"assignment_support: device vs host probs_without max abs {d:.2e}; flips per block {dev['n_flips']}")
    assert d <= 1e-9
    np.testing.assert_allclose(dev["margin_without"], host["margin_without"], rtol=1e-9, atol=1e-8)
    np.testing.assert_allclose(dev["margin"], host["margin"], rtol=1e-9, atol=1e-8)
