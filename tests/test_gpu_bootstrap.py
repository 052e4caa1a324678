"""ca_clone_loglik_reweighted / HipEngine.clone_loglik_reweighted / clone_loglik_reweighted / bootstrap_assignments: the gene-reweighted log-likelihood of
every replicate of a bootstrap in two float64 products on the matrix cores, reduced to votes and shares on the device.

The yardstick is ``api._clone_loglik_reweighted_host`` (chunked numpy float64; tests/test_bootstrap_host.py ties it to ``ref_ll`` on the resampled
matrices).  Bar, the family's: the same -inf pattern, no NaN, finite ``ll`` within ``1e-10 x scale`` with scale = sum_g w y |log E| + s |log Z| (a float64
sum of at most 2049 terms is good to 2.3e-13 of the sum of the terms' magnitudes; any float32 intermediate, 6e-8, fails it).  ``reads`` is a sum of
non-negative terms: 1e-10 of itself.  The shares: softmax has |dp_c| <= 2 p_c (1 - p_c) max_j |dt_j| <= max_j |dt_j| / 2 to first order, so a replicate's share is
good to max_c (1e-10 scale) (twice the first-order bound), its square to twice that; the sums over R replicates to the sum of those.  ``votes`` are integers: they
must be EQUAL, after the test has shown that no replicate of the host reference has its two best clones closer than 1e-6 of the terms' magnitude (10^4
bars apart: the device cannot turn such an argmax).

Where the big shape is used the host reference covers three ranges of its cells (the first, the ones around the cut between the two internal batches, the
last); the device computes every cell, and its ranges are compared bit for bit among themselves."""
import ctypes as C

import numpy as np
import pytest

import clonealign_amd as ca
from clonealign_amd import api
from clonealign_amd.engine import CA_BOOT_RCHUNK, reweighted_cells_per_batch
from tests._cases import make_case
from tests.test_block_loglik_host import HostOnly, close, planted_fit
from tests.test_gpu_clone_loglik import factors
from tests.test_gpu_fit_mse import SHAPES, problem

pytestmark = pytest.mark.gpu
RTOL = 1e-10
KEYS = ("votes", "prob_sum", "prob_sq", "reads", "ll")


def weights_for(G, R, seed, fractional):
    """Integer bootstrap weights, or those times a positive factor per (replicate, gene) with some genes left at 0."""
    w = api.bootstrap_gene_weights(G, R, seed=seed)
    if fractional:
        w = w * np.random.default_rng(seed).uniform(0.25, 1.75, size=w.shape)
    return w


def against_host(out, Y, E, U, V, w, lp, cells, tag, vote_cells=None):
    """One device result against the host form on the same cells; returns the worst ll error in units of the bar.  ``vote_cells``: the first so many cells of
    the range are the ones whose seeds were picked so that the host reference has no near tie (None: all of them)."""
    lo, hi = cells
    ref = api._clone_loglik_reweighted_host(Y, E, U, V, w, log_prior=lp, cells=cells, with_scale=True)
    ll, scale = out["ll"][lo:hi], ref["scale"]
    close(ll, ref["ll"], scale, tag + " ll")
    ok = np.isfinite(ref["ll"])
    worst = float((np.abs(ll[ok] - ref["ll"][ok]) / np.maximum(scale[ok], 1e-300)).max()) if ok.any() else 0.0
    np.testing.assert_allclose(out["reads"][lo:hi], ref["reads"], rtol=RTOL, atol=0, err_msg=tag)
    tol = (RTOL * np.where(ok, scale, 0.0).max(2)).sum(1)[:, None] + 1e-14 * w.shape[0]
    for k, f in (("prob_sum", 1.0), ("prob_sq", 2.0)):
        err = np.abs(out[k][lo:hi] - ref[k])
        assert not np.isnan(out[k]).any() and (err <= f * tol).all(), (tag, k, float((err / tol).max()))
    # votes: first the host reference's own margins, then equality
    t = ref["ll"] if lp is None else ref["ll"] + lp[lo:hi, None, :]
    top = np.sort(np.where(np.isnan(t), -np.inf, t), axis=2)
    with np.errstate(invalid="ignore"):
        margin = top[:, :, -1] - top[:, :, -2]
    margin = np.where(np.isnan(margin), np.inf, margin)               # (-inf against -inf: no rival)
    need = 1e-6 * np.where(ok, scale, 0.0).max(2)
    nv = hi - lo if vote_cells is None else min(vote_cells, hi - lo)
    near = margin < need
    assert not near[:nv].any(), (tag, "the host reference has a near tie: pick another seed", int(near[:nv].sum()), int(near.sum()))
    assert np.array_equal(out["votes"][lo:lo + nv], ref["votes"][:nv]), tag
    clear = ~near.any(1)                                               # past the seeded cells: every cell whose replicates are all clear of a tie as well
    assert np.array_equal(out["votes"][lo:hi][clear], ref["votes"][clear]), tag
    print(f"clone_loglik_reweighted {tag}: max |ll - ref| / scale {worst:.2e}; smallest margin / scale {float((margin / np.maximum(need * 1e6, 1e-300)).min()):.2e}")
    return worst


def same(a, b, tag, rows=slice(None)):
    for k in KEYS:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (tag, k)
        else:
            assert np.array_equal(a[k][rows], b[k], equal_nan=True), (tag, k)


@pytest.mark.parametrize("storage", ["u8", "u16", "f32"])
def test_parity_small_shape_every_storage_every_D_every_R(storage):
    from clonealign_amd.engine import HipEngine
    N, G, Cn = SHAPES[0]
    Y, L, mu, _idx, rng = problem(N, G, Cn, storage, seed=sum(SHAPES[0]))
    E = mu[:, None] * L
    U, V = factors(N, G, 3, rng)
    lp = rng.normal(size=(N, Cn))
    eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, y_storage=storage)
    try:
        assert eng.info()["y_storage_name"] == storage
        for D in (0, 1, 3):
            Uv, Vv = (None, None) if D == 0 else (U[:, :D], V[:, :D])
            for R in (1, 5, 37):
                for frac in (False, True):
                    w = weights_for(G, R, seed=R + D, fractional=frac)
                    out = eng.clone_loglik_reweighted(E, Uv, Vv, w, log_prior=lp, want_ll=True)
                    against_host(out, Y, E, Uv, Vv, w, lp, (0, N), f"{SHAPES[0]} {storage} D={D} R={R} frac={frac}")
                    same(eng.clone_loglik_reweighted(E, Uv, Vv, w, log_prior=lp, want_ll=True), out, "second call")
    finally:
        eng.close()


@pytest.mark.parametrize("storage,D,R,frac", [("u8", 1, 5, False), ("u16", 0, 37, True), ("f32", 3, 1, True)])
def test_parity_middle_shape(storage, D, R, frac):
    from clonealign_amd.engine import HipEngine
    N, G, Cn = SHAPES[1]
    Y, L, mu, _idx, rng = problem(N, G, Cn, storage, seed=sum(SHAPES[1]))
    E = mu[:, None] * L
    U, V = factors(N, G, 3, rng)
    Uv, Vv = (None, None) if D == 0 else (U[:, :D], V[:, :D])
    w = weights_for(G, R, seed=11, fractional=frac)
    eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, y_storage=storage)
    try:
        out = eng.clone_loglik_reweighted(E, Uv, Vv, w, want_ll=True)
        for cells in ((0, 600), (2400, N)):
            against_host(out, Y, E, Uv, Vv, w, None, cells, f"{SHAPES[1]} {storage} D={D} R={R} cells {cells}", vote_cells=60)
    finally:
        eng.close()


def test_parity_big_shape_two_replicate_chunks_two_cell_batches():
    """5000 x 2049 x 20, u8 with escapes, D = 3, R = 37: 37 replicates are two chunks of CA_BOOT_RCHUNK, and the slabs of a chunk put 4352 cells in a batch."""
    from clonealign_amd.engine import HipEngine
    N, G, Cn = SHAPES[2]
    D, R = 3, 37
    NB = reweighted_cells_per_batch(N, G, Cn, D, R)
    assert R > CA_BOOT_RCHUNK and 0 < NB < N, (CA_BOOT_RCHUNK, NB)
    Y, L, mu, _idx, rng = problem(N, G, Cn, "u8", seed=sum(SHAPES[2]))
    E = mu[:, None] * L
    U, V = factors(N, G, D, rng)
    w = weights_for(G, R, seed=6, fractional=False)                  # (a seed under which the 40 vote cells of each range have no near tie: checked on the CPU)
    eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, y_storage="u8")
    try:
        assert eng.info()["y_storage_name"] == "u8"
        out = eng.clone_loglik_reweighted(E, U, V, w, want_ll=True)
        for cells in ((0, 200), (NB - 100, NB + 100), (N - 200, N)):
            against_host(out, Y, E, U, V, w, None, cells, f"{SHAPES[2]} u8 D={D} R={R} cells {cells}", vote_cells=40)
        # a range that the full call cuts between its two batches is one batch of its own call; the chunks' cut falls elsewhere with fewer replicates
        lo, hi = NB - 300, NB + 300
        same(out, eng.clone_loglik_reweighted(E, U, V, w, cells=(lo, hi), want_ll=True), "across the batch cut", slice(lo, hi))
        tail = eng.clone_loglik_reweighted(E, U, V, w[30:], cells=(lo, hi), want_ll=True)
        assert np.array_equal(tail["ll"], out["ll"][lo:hi, 30:]) and np.array_equal(tail["reads"], out["reads"][lo:hi, 30:])
    finally:
        eng.close()


def test_a_cell_does_not_depend_on_its_range_its_batch_or_the_replicates_beside_it():
    from clonealign_amd.engine import HipEngine
    N, G, Cn = SHAPES[1]
    R = 37
    Y, L, mu, _idx, rng = problem(N, G, Cn, "u8", seed=77)
    E = mu[:, None] * L
    U, V = factors(N, G, 1, rng)
    lp = rng.normal(size=(N, Cn))
    w = weights_for(G, R, seed=8, fractional=True)
    eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0)
    try:
        for Uv, Vv in ((U, V), (None, None)):
            full = eng.clone_loglik_reweighted(E, Uv, Vv, w, log_prior=lp, want_ll=True)
            same(eng.clone_loglik_reweighted(E, Uv, Vv, w, log_prior=lp, want_ll=True), full, "second call")
            off = eng.clone_loglik_reweighted(E, Uv, Vv, w, log_prior=lp)
            assert off["ll"] is None and all(np.array_equal(off[k], full[k]) for k in KEYS[:4])
            for cells in ((0, 100), (100, 101), (101, N), (5, 38)):      # (the last cuts inside a tile of 16 cells at both ends)
                same(full, eng.clone_loglik_reweighted(E, Uv, Vv, w, log_prior=lp, cells=cells, want_ll=True), f"cells {cells}", slice(*cells))
            none = eng.clone_loglik_reweighted(E, Uv, Vv, w, log_prior=lp, cells=(7, 7), want_ll=True)
            assert none["ll"].shape == (0, R, Cn) and none["votes"].shape == (0, Cn)
            # R calls with one replicate each: the same ll and reads; votes and shares add up in replicate order to the same bits
            votes, ps, pq = np.zeros((N, Cn), dtype=np.int32), np.zeros((N, Cn)), np.zeros((N, Cn))
            for r in range(R):
                one = eng.clone_loglik_reweighted(E, Uv, Vv, w[r:r + 1], log_prior=lp, want_ll=True)
                assert np.array_equal(one["ll"][:, 0], full["ll"][:, r]) and np.array_equal(one["reads"][:, 0], full["reads"][:, r]), r
                votes += one["votes"]
                ps = ps + one["prob_sum"]
                pq = pq + one["prob_sq"]
            assert np.array_equal(votes, full["votes"]) and np.array_equal(ps, full["prob_sum"]) and np.array_equal(pq, full["prob_sq"])
    finally:
        eng.close()


@pytest.mark.parametrize("world", [2, 3])
def test_group_returns_the_single_handle_bits(world):
    from clonealign_amd.engine import EngineError, HipEngine, HipGroupEngine
    N, G, Cn = 1301, 700, 8
    R = 35
    Y, L, mu, _idx, rng = problem(N, G, Cn, "u8", seed=31)
    E = mu[:, None] * L
    U, V = factors(N, G, 1, rng)
    lp = rng.normal(size=(N, Cn))
    w = weights_for(G, R, seed=2, fractional=False)
    one = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0)
    try:
        o1 = [one.clone_loglik_reweighted(E, U, V, w, log_prior=lp, want_ll=True), one.clone_loglik_reweighted(E, None, None, w),
              one.clone_loglik_reweighted(E, U, V, w, log_prior=lp, cells=(100, 1000), want_ll=True)]
    finally:
        one.close()
    grp = HipGroupEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, devices=[0] * world)
    try:
        og = [grp.clone_loglik_reweighted(E, U, V, w, log_prior=lp, want_ll=True), grp.clone_loglik_reweighted(E, None, None, w),
              grp.clone_loglik_reweighted(E, U, V, w, log_prior=lp, cells=(100, 1000), want_ll=True)]
        bad = U.copy()
        bad[N - 1, 0] = np.nan                                       # refused on one rank's cells: refused by the group, which stays usable
        with pytest.raises(EngineError) as ex:
            grp.clone_loglik_reweighted(E, bad, V, w)
        assert ex.value.code == 1 and "U has a non-finite entry" in ex.value.msg, ex.value.msg
        wb = w.copy()
        wb[3, 5] = -1.0
        with pytest.raises(EngineError) as ex:
            grp.clone_loglik_reweighted(E, U, V, wb)
        assert ex.value.code == 1 and "replicate 3, gene 5" in ex.value.msg, ex.value.msg
        with pytest.raises(EngineError) as ex:
            grp.clone_loglik_reweighted(E, U, V, w, cells=(400, N + 1))
        assert ex.value.code == 1 and "cell range" in ex.value.msg, ex.value.msg
        same(grp.clone_loglik_reweighted(E, U, V, w, log_prior=lp, cells=(100, 1000), want_ll=True), og[2], "after the refusals")
    finally:
        grp.close()
    for a, b in zip(og, o1):
        same(a, b, f"group of {world}")


@pytest.mark.parametrize("storage", ["u8", "f32"])
def test_layouts_and_sparse_input(storage):
    import scipy.sparse as sps
    from clonealign_amd.engine import HipEngine
    N, G, Cn = 1500, 700, 5
    R = 6
    Y, L, mu, _idx, rng = problem(N, G, Cn, storage, seed=12)
    E = mu[:, None] * L
    U, V = factors(N, G, 2, rng)
    lp = rng.normal(size=(N, Cn))
    w = weights_for(G, R, seed=5, fractional=True)
    outs = {}
    for lay in ("row", "col"):
        eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, y_storage=storage, layout=lay)
        try:
            f = np.asfortranarray if lay == "col" else np.ascontiguousarray
            outs[lay] = eng.clone_loglik_reweighted(f(E), f(U), f(V), w, log_prior=f(lp), cells=(3, 1390), want_ll=True)
        finally:
            eng.close()
    ref =api._clone_loglik_reweighted_host(Y, E, U, V, w, log_prior=lp, cells=(3, 1390), with_scale=True)
    close(outs["row"]["ll"], ref["ll"], ref["scale"], f"layout row {storage}")
    same(outs["col"], outs["row"], "column-major handle")
    for fmt in (sps.csr_matrix, sps.csc_matrix):
        eng = HipEngine(fmt(Y), L, np.zeros((N, 0)), np.zeros(G), 0, y_storage=storage)
        try:
            same(eng.clone_loglik_reweighted(E, U, V, w, log_prior=lp, cells=(3, 1390), want_ll=True), outs["row"], fmt.__name__)
        finally:
            eng.close()


def test_edges_zero_copy_number_zero_weights_zero_reads_and_extreme_exponents():
    from clonealign_amd.engine import HipEngine
    N, G, Cn = SHAPES[1]
    Y, L, mu, _idx, rng = problem(N, G, Cn, "u8", seed=7)
    L[5, :] = 0.0
    Y[:, 5] = 0                                                      # zero copy number against zero counts: contributes nothing
    L[7, 3] = 0.0
    Y[:, 7] = 0
    Y[11, 7] = 2                                                     # a positive count where clone 3 has none ...
    L[9, 2] = 0.0
    Y[:, 9] = 0
    Y[12, 9] = 400                                                   # ... and an escaped one where clone 2 has none
    L[:600, 6] = 0.0                                                 # clone 6 is expressed in the genes 600.. only
    E = mu[:, None] * L
    w = np.ones((4, G))
    w[1, 7] = 0.0                                                    # replicate 1 does not see gene 7, replicate 0 does
    w[1, 9] = 0.5
    w[2, 600:] = 0.0                                                 # replicate 2 has no weighted gene of positive E for clone 6
    w[3] = 0.0
    w[3, 1000:1010] = 2.0                                            # replicate 3 weighs ten genes
    Y[40, 1000:1010] = 0                                             # cell 40 has all its reads on zero-weight genes there
    U, V = factors(N, G, 2, rng)
    U[:, 0] = 0.0
    U[20] = (1.0, 0.0)
    V[[3, 40, 60], 0] = 800.0                                        # eta = +-800 on a few genes of cell 20
    V[[4, 41], 0] = -800.0
    eng = HipEngine(Y, np.maximum(L, 1.0), np.zeros((N, 0)), np.zeros(G), 0)
    try:
        for Uv, Vv in ((None, None), (U, V)):
            out = eng.clone_loglik_reweighted(E, Uv, Vv, w, want_ll=True)
            ref = api._clone_loglik_reweighted_host(Y, E, Uv, Vv, w, with_scale=True)
            for k in KEYS:
                assert not np.isnan(out[k]).any(), k
            ll = out["ll"]
            assert np.isneginf(ll[11, 0, 3]) and np.isfinite(ll[11, 1, 3]) and np.isneginf(ll[12, :3, 2]).all() and np.isfinite(ll[12, 3, 2])
            assert (ll[40, 3] == 0.0).all() and out["reads"][40, 3] == 0.0
            has = Y[:, :600].sum(1) > 0
            assert np.isneginf(ll[has][:, :3, 6]).all()               # -inf by the mask, never -inf - s (-inf)
            finite = np.isfinite(ref["ll"])
            assert np.array_equal(np.isneginf(ll), np.isneginf(ref["ll"])) and np.array_equal(np.isfinite(ll), finite)
            err = np.abs(ll[finite] - ref["ll"][finite])
            assert (err <= RTOL * ref["scale"][finite]).all(), float((err / np.maximum(ref["scale"][finite], 1e-300)).max())
            assert np.isfinite(ll[20, :3]).sum() >= 3 * (Cn - 3)
    finally:
        eng.close()


def test_refusals_name_the_offender():
    from clonealign_amd.engine import EngineError, HipEngine
    case = make_case(N=700, G=300, C=4, K=1, seed=2)
    L = case["L"]
    rng = np.random.default_rng(0)
    U, V = factors(700, 300, 2, rng)
    w = np.ones((3, 300))
    eng = HipEngine(**case)
    try:
        good = eng.clone_loglik_reweighted(L, U, V, w, want_ll=True)

        def refused(words, *a, **k):
            with pytest.raises(EngineError) as ex:
                eng.clone_loglik_reweighted(*a, **k)
            assert ex.value.code == 1 and all(x in ex.value.msg for x in words), ex.value.msg
            same(eng.clone_loglik_reweighted(L, U, V, w, want_ll=True), good, "after a refusal")   # the handle still serves a valid call
        refused(("ca_clone_loglik_reweighted", "R = 0", "below 1"), L, U, V, np.ones((0, 300)))
        for v in (-1.0, np.nan, np.inf):
            wb = w.copy()
            wb[2, 17] = v
            refused(("replicate 2", "gene 17"), L, U, V, wb)
        wb = w.copy()
        wb[1] = 0.0
        refused(("replicate 1", "all zero"), L, U, V, wb)
        refused(("cell range", "outside [0, 700]"), L, U, V, w, cells=(10, 701))
        refused(("cell range",), L, U, V, w, cells=(-1, 5))
        E = L.copy()
        E[17, 2] = -1.0
        refused(("gene 17", "clone 2"), E, U, V, w)
        lp = np.zeros((700, 4))
        lp[9, 1] = np.nan
        refused(("log_prior", "cell 9", "clone 1"), L, U, V, w, log_prior=lp)
        Ub = U.copy()
        Ub[9, 1] = np.nan
        refused(("U has a non-finite", "cell 9"), L, Ub, V, w)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)                 # noqa: E731
        votes, ps, pq = np.zeros((700, 4), dtype=np.int32), np.zeros((700, 4)), np.zeros((700, 4))
        rc = eng.lib.ca_clone_loglik_reweighted(eng.h, ptr(L), None, ptr(V), 2, ptr(w), 3, None, 0, 700, None, ptr(votes), ptr(ps), ptr(pq), None)
        assert rc == 1 and b"needs both U" in eng.lib.ca_last_error(eng.h)
        rc = eng.lib.ca_clone_loglik_reweighted(eng.h, ptr(L), None, None, 0, ptr(w), 3, None, 0, 700, None, None, ptr(ps), ptr(pq), None)
        assert rc == 1 and b"votes is NULL" in eng.lib.ca_last_error(eng.h)
        with pytest.raises(ValueError):
            eng.clone_loglik_reweighted(L, U, V, w[:, :-1])
        with pytest.raises(ValueError):
            eng.clone_loglik_reweighted(L, U, V, w, log_prior=lp[:-1])
    finally:
        eng.close()


def test_bootstrap_assignments_through_a_live_fit_engine():
    from clonealign_amd.engine import HipEngine, reweighted_kernel_ms
    N, G, Cn, R = 1200, 400, 3, 40
    Y, L, fit, rng = planted_fit(N, G, Cn, seed=17)
    extra = rng.normal(size=(N, Cn))
    host = ca.bootstrap_assignments(fit, Y, L, n_rep=R, seed=5, extra_loglik=extra, psi="fit", engine=HostOnly(N, G))
    case = make_case(N=N, G=G, C=Cn, K=1, seed=17, scale=1.0)
    eng = HipEngine(**case)
    try:
        eng.iterate(3, None)                                         # a fit in progress: the call changes nothing in it and does not need it finished
        dev = ca.bootstrap_assignments(fit, Y, L, n_rep=R, seed=5, extra_loglik=extra, psi="fit", engine=eng)
        assert reweighted_kernel_ms() > 0.0
    finally:
        eng.close()
    # the host reference's margins first (its ll through the same public call), then the votes must be equal
    w = ca.bootstrap_gene_weights(G, R, seed=5)
    ft = api._fit_tables(fit, np.asarray(L, dtype=np.float64), N, None, "fit", True, 6)
    prior = np.log(fit["ml_params"]["alpha"])[None, :] + extra
    ref = api._clone_loglik_reweighted_host(Y, ft.E, ft.U, ft.V, w, log_prior=prior, with_scale=True)
    t = np.sort(ref["ll"] + prior[:, None, :], axis=2)
    assert ((t[:, :, -1] - t[:, :, -2]) >= 1e-6 * ref["scale"].max(2)).all()
    assert np.array_equal(ref["votes"] / float(R), host["clone_support"])
    assert np.array_equal(dev["clone_support"], host["clone_support"]) and np.array_equal(dev["support"], host["support"])
    assert np.array_equal(dev["clone"], host["clone"]) and np.array_equal(dev["clone_bootstrap"], host["clone_bootstrap"])
    assert dev["n_newly_unassigned"] == host["n_newly_unassigned"] and dev["n_rep"] == R and dev["weights_seed"] == 5
    # a share is good to 1e-10 x the terms' magnitude (the module docstring), the mean of R of them too; the standard deviation is the root of a
    # difference of two such means, so near sd = 0 it is good to the root of that
    tol = 1e-10 * float(ref["scale"].max())
    np.testing.assert_allclose(dev["clone_probs"], host["clone_probs"], rtol=0, atol=tol)
    np.testing.assert_allclose(dev["mean_probs"], host["mean_probs"], rtol=0, atol=tol)
    np.testing.assert_allclose(dev["sd_probs"], host["sd_probs"], rtol=0, atol=np.sqrt(4 * tol))
