"""ca_clone_mixture / HipEngine.clone_mixture / clone_mixture / deconvolve_clones: the maximum-likelihood mixture of all clones per resident cell -- simplex
weights by projected Newton with a certified bound -- float64 on the device.

The yardstick of an EVALUATION is ``ref_eval`` below: the formulas of include/clonealign_hip.h restated in numpy float64 over the non-zero counts.  Bars, the
project's own for float64 sweeps (RTOL of tests/test_gpu_fit_mse.py): ``|mix_ll - ref| <= 1e-10 * scale``, scale = sum_g y |log m| + sum_g y |eta| + s |lz|
(+ lgamma(s + 1) + sum_g lgamma(y + 1) with the constant); ``grad`` relative to itself (its terms are positive); ``bound`` = max_c g_c - sum_c pi_c g_c within
1e-10 of the two sums' magnitudes.  The -inf pattern must be equal and no NaN may appear.  An OPTIMISATION is not compared round by round with anything: the
host recomputes mix_ll, grad and bound at the weights the device returns (the same bars), and the theorem is checked against the host form's optimum:
``mix_ll_device + bound_device >= mix_ll(any other weights) - 1e-10 * scale`` for every cell, converged or not."""
import ctypes as C

import numpy as np
import pytest
from scipy.special import gammaln

from clonealign_amd import api
from tests._cases import eps_for, make_case
from tests.test_doublets_host import HostOnly
from tests.test_gpu_clone_loglik import factors
from tests.test_gpu_fit_mse import RTOL, problem
from tests.test_gpu_pair_loglik import engine_for, pairs_of

pytestmark = pytest.mark.gpu

KEYS = ("weights", "grad", "mix_ll", "bound", "rounds", "ll")


def ref_eval(Y, E, U, V, pi, const=True, chunk=256):
    """mix_ll, grad, bound at the weights ``pi`` [N, C] with their bars' scales: {"mix_ll", "scale", "grad", "bound", "btol"}.  Y dense (any dtype)."""
    E = np.asarray(E, dtype=np.float64)
    N, G = Y.shape
    Cn = E.shape[1]
    D = 0 if U is None else U.shape[1]
    out = {"mix_ll": np.empty(N), "scale": np.empty(N), "grad": np.empty((N, Cn)), "bound": np.empty(N), "btol": np.empty(N)}
    for lo in range(0, N, chunk):
        Yc = np.asarray(Y[lo:lo + chunk], dtype=np.float64)
        n = Yc.shape[0]
        s = Yc.sum(1)
        if D > 0:
            eta = U[lo:lo + chunk] @ V.T
            mx = eta.max(1, keepdims=True)
            logz = mx + np.log(np.exp(eta - mx) @ E)
            base, bsc = (Yc * eta).sum(1), (Yc * np.abs(eta)).sum(1)
        else:
            logz = np.broadcast_to(np.log(E.sum(0))[None, :], (n, Cn))
            base, bsc = np.zeros(n), np.zeros(n)
        if const:
            lg = gammaln(Yc + 1.0).sum(1)
            base, bsc = base + gammaln(s + 1.0) - lg, bsc + gammaln(s + 1.0) + lg
        lz = logz.min(1)
        a = np.exp(lz[:, None] - logz)
        r, g = np.nonzero(Yc > 0)                                    # rows ascending, genes ascending within a row
        y = Yc[r, g]
        q = E[g] * a[r]
        usable = q.sum(1) > 0
        m = (q * pi[lo + r]).sum(1)
        good = usable & (m > 0)
        ms = np.where(good, m, 1.0)
        cnt = lambda w: np.bincount(r, weights=w, minlength=n)       # noqa: E731
        ninf, bad = cnt(~usable) > 0, cnt(usable & ~good) > 0
        t = np.where(good, y * np.log(ms), 0.0)
        seff = cnt(np.where(usable, y, 0.0))
        gs = np.stack([cnt(np.where(good, y / ms, 0.0) * q[:, c]) for c in range(Cn)], axis=1)
        sg = (pi[lo:lo + n] * gs).sum(1)
        gap = np.maximum(gs.max(1) - sg, 0.0)
        sl = slice(lo, lo + n)
        out["bound"][sl] = np.where(seff > 0, np.where(bad, np.inf, gap), 0.0)
        out["btol"][sl] = RTOL * (gs.max(1) + sg)
        out["mix_ll"][sl] = np.where(ninf | bad, -np.inf, cnt(t) + base - np.where(s > 0, s * lz, 0.0))
        out["scale"][sl] = cnt(np.abs(t)) + bsc + s * np.abs(lz)
        out["grad"][sl] = np.where(seff[:, None] > 0, gs / np.where(seff > 0, seff, 1.0)[:, None], 0.0)
    return out


def check_eval(dev, ref, tag, rows=slice(None)):
    """The device's mix_ll, grad and bound against an evaluation at the same weights, at the bars of the docstring."""
    for k in ("weights", "grad", "mix_ll", "bound"):
        assert not np.isnan(dev[k]).any(), (tag, k)
    mll, bnd, grad = dev["mix_ll"][rows], dev["bound"][rows], dev["grad"][rows]
    assert np.array_equal(np.isneginf(mll), np.isneginf(ref["mix_ll"])) and not np.isposinf(mll).any(), tag
    ok = np.isfinite(ref["mix_ll"])
    worst = float((np.abs(mll[ok] - ref["mix_ll"][ok]) / np.maximum(ref["scale"][ok], 1e-300)).max()) if ok.any() else 0.0
    gerr = float((np.abs(grad - ref["grad"]) / np.maximum(ref["grad"], 1e-300))[ref["grad"] > 0].max()) if (ref["grad"] > 0).any() else 0.0
    assert np.array_equal(grad == 0, ref["grad"] == 0), tag
    assert np.array_equal(np.isposinf(bnd), np.isposinf(ref["bound"])), tag
    fb = np.isfinite(ref["bound"])
    berr = float((np.abs(bnd[fb] - ref["bound"][fb]) / np.maximum(ref["btol"][fb], 1e-300)).max()) if fb.any() else 0.0
    print(f"clone_mixture {tag}: max |mix_ll - ref| / scale {worst:.2e}, grad rel {gerr:.2e}, bound err / its bar {berr:.2e}")
    assert worst <= RTOL and gerr <= RTOL and berr <= 1.0, tag


def same_bits(a, b, tag="", rows=slice(None)):
    for k in KEYS:
        assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k][rows]), (tag, k)


def planted_problem(N, G, Cn, storage, seed):
    """``problem`` of the neighbours with the rows and genes every mixture test wants: row 0 without counts, row 1 with one non-zero, row 2 with fewer
    non-zeros than clones, row 3 with EVERY column non-zero (at G = 2049 a list longer than any segment and no multiple of 64) and, in u8, an escape beside a
    genuine 255; genes where E = 0 in one clone, in all but the last, and in all of them -- the last against a positive count of row 4 alone."""
    Y, L, mu, _idx, rng = problem(N, G, Cn, storage, seed=seed)
    ga, gb, gc = 5, 9, 13
    Y[0] = 0
    Y[1] = 0
    Y[1, 20] = 4
    Y[2] = 0
    Y[2, 21:21 + max(Cn - 1, 1)] = 1
    Y[3] = np.maximum(Y[3], 1)
    Y[3, 30], Y[3, 31] = 255, 300
    Y[:, gc] = 0
    Y[4, gc] = 2
    Y[3, gc] = 0                                                      # (row 3 keeps every OTHER column: its mix_ll stays finite)
    Y[5, ga] = Y[6, gb] = 3
    E = mu[:, None] * L
    E[ga, 0] = 0.0
    E[gb, :Cn - 1] = 0.0
    E[gc, :] = 0.0
    return Y, np.maximum(L, 1.0), E, rng


def starts_with_zeros(rng, N, Cn):
    st = rng.dirichlet(np.ones(Cn), size=N)
    st[rng.random((N, Cn)) < 0.3] = 0.0
    st[st.sum(1) == 0, 0] = 1.0
    return st / st.sum(1, keepdims=True)


# (cells, genes, clones): fewer cells than a block's waves, G under one segment, 5 slots | 44 slots, rows of several segments | 230 slots: four sweeps of the
# slot pass, one column past a 2048 boundary | 20 slots: most lanes of the slot pass idle
SHAPES = [(33, 77, 2), (700, 1234, 8), (300, 2049, 20), (200, 300, 5)]


@pytest.mark.parametrize("storage", ["u8", "u16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_evaluation_parity_with_the_float64_restatement(shape, storage):
    N, G, Cn = shape
    Y, L, E, rng = planted_problem(N, G, Cn, storage, seed=sum(shape))
    U, V = factors(N, G, 3, rng)
    st = starts_with_zeros(rng, N, Cn)
    st[3] = 1.0 / Cn                                                 # (row 3 has a count on every gene, the ones a single clone supports included)
    eng = engine_for(Y, L, storage)
    try:
        assert eng.info()["y_storage_name"] == storage
        for D in (0, 3):
            Uv, Vv = (None, None) if D == 0 else (U, V)
            for const in (True, False):
                r = eng.clone_mixture(E, Uv, Vv, start=st, max_iter=0, const=const)
                tag = f"{shape} {storage} D={D} const={const}"
                check_eval(r, ref_eval(Y, E, Uv, Vv, st, const), tag)
                assert np.array_equal(r["weights"], st) and (r["rounds"] == 0).all()
                assert np.isneginf(r["mix_ll"][4]) and np.isfinite(r["mix_ll"][3]) and r["bound"][0] == 0
                assert np.array_equal(r["ll"], eng.clone_loglik(E, Uv, Vv, const=const)[:N])          # clone_loglik's bits
            again = eng.clone_mixture(E, Uv, Vv, start=st, max_iter=0, const=False, want_ll=False)
            assert again["ll"] is None
            same_bits({k: (None if k == "ll" else r[k]) for k in KEYS}, again, "two calls")
            # one-hot and pair starts: clone_loglik's and clone_pair_loglik's values, at the same bar
            ll = eng.clone_loglik(E, Uv, Vv)
            for c in sorted({0, Cn - 1}):
                hot = np.zeros((N, Cn))
                hot[:, c] = 1.0
                ev = eng.clone_mixture(E, Uv, Vv, start=hot, max_iter=0)
                sc = ref_eval(Y, E, Uv, Vv, hot)["scale"]
                assert np.array_equal(np.isneginf(ev["mix_ll"]), np.isneginf(ll[:, c])) and not np.isnan(ev["mix_ll"]).any()
                ok = np.isfinite(ll[:, c])
                assert (np.abs(ev["mix_ll"][ok] - ll[ok, c]) <= RTOL * sc[ok]).all(), (tag, "one-hot", c)
            w = (0.3, 0.8)
            pr = eng.clone_pair_loglik(E, Uv, Vv, weights=w, want_ll=False)["pair_ll"]
            prs = pairs_of(Cn)
            for p in sorted({0, len(prs) - 1}):
                for k, wk in enumerate(w):
                    two = np.zeros((N, Cn))
                    two[:, prs[p][0]], two[:, prs[p][1]] = wk, 1.0 - wk
                    ev = eng.clone_mixture(E, Uv, Vv, start=two, max_iter=0)
                    sc = ref_eval(Y, E, Uv, Vv, two)["scale"]
                    assert np.array_equal(np.isneginf(ev["mix_ll"]), np.isneginf(pr[:, p, k]))
                    ok = np.isfinite(pr[:, p, k])
                    assert (np.abs(ev["mix_ll"][ok] - pr[ok, p, k]) <= RTOL * sc[ok]).all(), (tag, "pair", p, wk)
    finally:
        eng.close()


@pytest.mark.parametrize("storage", ["u8", "u16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_optimisation_is_certified_by_the_host(shape, storage):
    N, G, Cn = shape
    Y, L, E, rng = planted_problem(N, G, Cn, storage, seed=sum(shape) + 1)
    U, V = factors(N, G, 3, rng)
    st = starts_with_zeros(rng, N, Cn)
    head = min(N, 64)                                                # the cells whose optimum the host form computes too (the planted rows among them)
    eng = engine_for(Y, L, storage)
    try:
        for D in (0, 3):
            Uv, Vv = (None, None) if D == 0 else (U, V)
            at_start = ref_eval(Y, E, Uv, Vv, st)
            tol = 1e-3
            host = api._clone_mixture_host(Y[:head], E, None if Uv is None else Uv[:head], Vv, max_iter=60, tol=1e-6)
            for start, max_iter in ((None, 50), (st, 50), (st, 2)):
                r = eng.clone_mixture(E, Uv, Vv, start=start, max_iter=max_iter, tol=tol)
                tag = f"{shape} {storage} D={D} start={'uniform' if start is None else 'zeros'} max_iter={max_iter}"
                ref = ref_eval(Y, E, Uv, Vv, r["weights"])          # at the weights the device returned
                check_eval(r, ref, tag)
                assert (r["rounds"] >= 0).all() and (r["rounds"] <= max_iter).all() and np.array_equal(r["converged"], r["bound"] <= tol), tag
                assert (r["weights"] >= 0).all() and np.abs(r["weights"].sum(1) - 1.0).max() <= 1e-12, tag
                assert r["rounds"][0] == 0 and r["bound"][0] == 0 and np.isneginf(r["mix_ll"][4]) and np.isfinite(np.delete(r["mix_ll"], 4)).all(), tag
                print(f"clone_mixture {tag}: converged {r['converged'].mean():.3f}, rounds median {int(np.median(r['rounds']))} max {int(r['rounds'].max())}")
                if start is not None:                                # monotone, against the start the device really took (the uniform one where the start's zeros exclude the data)
                    took = np.where(np.isposinf(at_start["bound"])[:, None], 1.0 / Cn, st)
                    was = ref_eval(Y, E, Uv, Vv, took)
                    fin = np.isfinite(was["mix_ll"])
                    assert (r["mix_ll"][fin] >= was["mix_ll"][fin] - RTOL * was["scale"][fin]).all(), tag
                # the theorem, against the host form's optimum (any weights would do: it is a theorem)
                fin = np.isfinite(host["mix_ll"])
                assert np.array_equal(fin, np.isfinite(r["mix_ll"][:head])), tag
                lhs = r["mix_ll"][:head] + r["bound"][:head]
                assert (lhs[fin] >= host["mix_ll"][fin] - RTOL * ref["scale"][:head][fin]).all(), (tag, float((host["mix_ll"][fin] - lhs[fin]).max()))
    finally:
        eng.close()


@pytest.mark.parametrize("D", [0, 2])
def test_ranges_chains_and_layouts_return_the_same_bits(D):
    N, G, Cn = 301, 600, 4
    Y, L, E, rng = planted_problem(N, G, Cn, "u8", seed=5)
    U, V = factors(N, G, D, rng) if D else (None, None)
    st = starts_with_zeros(rng, N, Cn)
    outs = {}
    for lay in ("row", "col"):
        f = np.asfortranarray if lay == "col" else np.ascontiguousarray
        fo = lambda a: None if a is None else f(a)                  # noqa: E731
        eng = engine_for(Y, L, layout=lay)
        try:
            full = eng.clone_mixture(fo(E), fo(U), fo(V), start=fo(st), max_iter=50, tol=1e-3)
            outs[lay] = full
            same_bits(full, eng.clone_mixture(fo(E), fo(U), fo(V), start=fo(st), max_iter=50, tol=1e-3), "two calls")
            for lo, hi in ((0, 100), (100, 101), (101, N)):
                same_bits(eng.clone_mixture(fo(E), fo(U), fo(V), start=fo(st[lo:hi]), max_iter=50, tol=1e-3, cells=(lo, hi)), full, (lay, lo, hi), slice(lo, hi))
            none = eng.clone_mixture(fo(E), fo(U), fo(V), max_iter=50, cells=(7, 7))
            assert none["weights"].shape == (0, Cn) and none["mix_ll"].shape == (0,) and none["rounds"].shape == (0,)
            # T rounds in one call are T calls of one round each, started from the previous weights
            T = 4
            one = eng.clone_mixture(fo(E), fo(U), fo(V), start=fo(st), max_iter=T, tol=0.0)
            w, total = st, np.zeros(N, dtype=np.int64)
            for _ in range(T):
                step = eng.clone_mixture(fo(E), fo(U), fo(V), start=fo(w), max_iter=1, tol=0.0)
                # (a start whose zeros exclude the data is replaced by the uniform one in the first call only: afterwards the weights are the device's own)
                w, total = step["weights"], total + step["rounds"]
            for k in ("weights", "grad", "mix_ll", "bound", "ll"):
                assert np.array_equal(one[k], step[k]), (lay, k)
            assert np.array_equal(one["rounds"], total)
        finally:
            eng.close()
    same_bits(outs["row"], outs["col"], "row-major against column-major")


def test_many_cells_in_two_batches_equal_one_batch():
    """3400 x 2049 x 3 in u8, D = 1: the list slab takes 3072 padded columns x 28 bytes a cell, so the quarter-gigabyte budget holds 3072 cells -- the full call
    runs two batches, and a range across the cut is one batch of its own call."""
    N, G, Cn = 3400, 2049, 3
    Y, L, E, rng = planted_problem(N, G, Cn, "u8", seed=8)
    U, V = factors(N, G, 1, rng)
    eng = engine_for(Y, L)
    try:
        full = eng.clone_mixture(E, U, V, max_iter=20, tol=1e-3)
        for lo, hi in ((2900, 3300), (3072, N), (0, 64)):
            same_bits(eng.clone_mixture(E, U, V, max_iter=20, tol=1e-3, cells=(lo, hi)), full, (lo, hi), slice(lo, hi))
    finally:
        eng.close()
    rows = np.r_[0:8, 3068:3080, N - 4:N]
    ref = ref_eval(Y[rows], E, U[rows], V, full["weights"][rows])
    check_eval({k: full[k][rows] for k in ("weights", "grad", "mix_ll", "bound")}, ref, "around the batch cut")
    print(f"clone_mixture 3400 x 2049 x 3: converged {full['converged'].mean():.3f} within 20 rounds")


def test_group_returns_the_single_handle_bits():
    from clonealign_amd.engine import EngineError, HipGroupEngine
    N, G, Cn = 501, 700, 8
    Y, L, E, rng = planted_problem(N, G, Cn, "u8", seed=31)
    U, V = factors(N, G, 1, rng)
    st = starts_with_zeros(rng, N, Cn)
    calls = [dict(U=U, V=V, start=st), dict(), dict(U=U, V=V, start=st[100:400], cells=(100, 400)), dict(U=U, V=V, start=st, max_iter=0)]
    one = engine_for(Y, L)
    try:
        o1 = [one.clone_mixture(E, **{"max_iter": 30, **kw}) for kw in calls]
    finally:
        one.close()
    grp = HipGroupEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, devices=[0, 0])
    try:
        og = [grp.clone_mixture(E, **{"max_iter": 30, **kw}) for kw in calls]
        bad = st.copy()
        bad[N - 1] = 0.5                                             # refused on one rank's cells: refused by the group, which stays usable
        with pytest.raises(EngineError) as ex:
            grp.clone_mixture(E, U, V, start=bad)
        assert ex.value.code == 1 and "the start of cell" in ex.value.msg and "off 1" in ex.value.msg, ex.value.msg
        with pytest.raises(EngineError) as ex:
            grp.clone_mixture(E, U, V, cells=(400, N + 1))
        assert ex.value.code == 1 and "cell range" in ex.value.msg, ex.value.msg
        same_bits(grp.clone_mixture(E, U, V, start=st[100:400], max_iter=30, cells=(100, 400)), og[2], "after the refusals")
    finally:
        grp.close()
    for a, b in zip(o1, og):
        same_bits(a, b, "group against one handle")


def test_the_call_changes_nothing_in_a_running_fit_and_is_refused_from_a_poll_hook():
    """Five iterations, clone_mixture, five more == ten iterations straight, bit for bit: every variable and the ELBO."""
    from clonealign_amd.engine import EngineError, HipEngine
    from clonealign_amd.rng import EpsStream
    case = make_case(N=900, G=500, C=4, K=1, seed=21)
    N, G = case["Y"].shape
    eps = np.stack([eps_for(1, G, 100 + i) for i in range(20)])
    U, V = factors(N, G, 1, np.random.default_rng(1))
    a = HipEngine(**case)
    try:
        ea = a.iterate(10, eps)
        sa = a.get_state()
    finally:
        a.close()
    b = HipEngine(**case)
    try:
        b.iterate(5, eps[:10])
        out = b.clone_mixture(case["L"], U, V)
        b.clone_mixture(case["L"], max_iter=0)
        check_eval(out, ref_eval(case["Y"], case["L"], U, V, out["weights"]), "mid-fit")
        eb = b.iterate(5, eps[10:])
        sb = b.get_state()
        seen = {}

        def hook(i, e):
            if i == 2:
                with pytest.raises(EngineError) as ex:
                    b.clone_mixture(case["L"])
                seen["code"] = ex.value.code
            return False
        b.run(EpsStream(9, 1, G), 4, 1e-12, poll=hook)
        assert seen["code"] == 6                                     # CA_ERR_STATE
    finally:
        b.close()
    assert ea == eb
    for n in sa:
        assert np.array_equal(sa[n], sb[n]), n


def test_deconvolve_clones_on_the_device_finds_planted_ambient():
    import clonealign_amd as ca
    rng = np.random.default_rng(11)
    N, G, Cn = 120, 400, 3
    L = rng.integers(1, 5, size=(G, Cn)).astype(np.float64)
    mu = rng.lognormal(0.0, 1.0, G)
    amb = rng.lognormal(0.0, 1.5, G)
    W = rng.normal(size=(G, 1)) * 0.05
    psi = rng.normal(size=(N, 1))
    clone = rng.integers(0, Cn, N)
    PI = np.zeros((N, Cn + 1))
    PI[np.arange(N), clone] = 0.7
    PI[:, Cn] = 0.3
    Y = np.empty((N, G), dtype=np.int32)
    for n in range(N):
        P = np.concatenate([mu[:, None] * L, amb[:, None]], axis=1) * np.exp(W[:, 0] * psi[n, 0])[:, None]
        Y[n] = rng.multinomial(3000, (P / P.sum(0)) @ PI[n])
    fit = {"ml_params": {"mu": mu, "W": W, "psi": psi}, "clone_names": ["a", "b", "c"]}
    for ps in (None, "fit"):                                         # D = 0 and D = 1
        dev = ca.deconvolve_clones(fit, Y, L, extra_profiles={"ambient": amb}, psi=ps, saturate=False)
        host = ca.deconvolve_clones(fit, Y, L, extra_profiles={"ambient": amb}, psi=ps, saturate=False, engine=HostOnly(N, G))
        assert dev["component_names"] == ["a", "b", "c", "ambient"] and dev["weights_extra"].shape == (N, 1) and dev["converged"].all()
        assert np.abs(dev["weights_extra"][:, 0] - 0.3).max() < 0.08 and np.array_equal(dev["dominant"], np.asarray(fit["clone_names"], dtype=object)[clone])
        d = float(np.abs(dev["mix_ll"] - host["mix_ll"]).max())
        print(f"deconvolve_clones psi={ps}: device vs host mix_ll max abs {d:.2e} nats, weights max abs {np.abs(dev['weights_all'] - host['weights_all']).max():.2e}")
        assert d <= 2e-3 + 1e-9                                      # both within tol = 1e-3 nats of the same maximum
        ev = ca.mixture_loglik(fit, Y, L, dev["weights_all"], extra_profiles={"ambient": amb}, psi=ps, saturate=False)
        assert np.array_equal(ev["mix_ll"], dev["mix_ll"]) and (ev["rounds"] == 0).all()
    from clonealign_amd.engine import HipEngine
    three = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0)
    try:
        with pytest.raises(ValueError, match="holds 3 columns"):
            ca.clone_mixture(fit, Y, L, extra_profiles=amb, saturate=False, engine=three)
        r = ca.clone_mixture(fit, Y, L, saturate=False, engine=three)
        assert r["weights"].shape == (N, Cn) and (r["log_lr_single"] >= -r["bound"] - 1e-9).all()
    finally:
        three.close()


def test_refusals_through_the_c_abi_name_the_offender():
    from clonealign_amd.engine import HipEngine
    N, G, Cn = 120, 90, 3
    Y, L, mu, _idx, rng = problem(N, G, Cn, "u8", seed=2)
    E = np.ascontiguousarray(mu[:, None] * L)
    U, V = factors(N, G, 2, rng)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    eng = engine_for(Y, L)
    wide = HipEngine(Y, np.ones((G, 33)), np.zeros((N, 0)), np.zeros(G), 0)
    try:
        w, g, m, b, rd = np.zeros((N, Cn)), np.zeros((N, Cn)), np.zeros(N), np.zeros(N), np.zeros(N, dtype=np.int32)
        good = np.full((N, Cn), 1.0 / Cn)

        def refused(words, h=eng, E_=E, st=None, it=10, tol=1e-3, lo=0, cnt=N, D=0, U_=None, V_=None, outs=None):
            o = dict(w=w, m=m, b=b, rd=rd) | (outs or {})
            rc = h.lib.ca_clone_mixture(h.h, ptr(E_), ptr(U_), ptr(V_), D, 1, ptr(st), it, tol, lo, cnt, None, ptr(o["w"]), ptr(g), ptr(o["m"]), ptr(o["b"]), ptr(o["rd"]))
            msg = h.lib.ca_last_error(h.h).decode()
            assert rc == 1 and all(x in msg for x in words), (rc, msg)
        refused(("ca_clone_mixture", "max_iter = -1", "negative"), it=-1)
        for tol in (-1e-3, np.nan, np.inf):
            refused(("tol_nats",), tol=tol)
        bad = good.copy()
        bad[4, 1] = -0.1
        refused(("start has a negative or non-finite entry", "cell 4", "clone 1"), st=bad)
        bad[4, 1] = np.nan
        refused(("start has a negative or non-finite entry", "cell 4"), st=bad)
        bad = good.copy()
        bad[7] = (0.5, 0.5, 1e-8)
        refused(("the start of cell 7", "off 1 by more than 1e-9"), st=bad)
        refused(("C = 33", "at most 32"), h=wide, E_=np.ones((G, 33)))
        refused(("cell range", f"[0, {N}]"), lo=100, cnt=21)
        refused(("cell range",), lo=-1, cnt=5)
        for name, key in (("weights", "w"), ("mix_ll", "m"), ("bound_nats", "b"), ("rounds", "rd")):
            refused((f"{name} is NULL",), outs={key: None})
        Eb = E.copy()
        Eb[17, 2] = -1.0
        refused(("gene 17", "clone 2"), E_=Eb)
        Ub = U.copy()
        Ub[9, 1] = np.nan
        refused(("U has a non-finite", "cell 9"), D=2, U_=Ub, V_=V)
        refused(("D = 9", "outside [0, 8]"), D=9, U_=U, V_=V)
        with pytest.raises(ValueError):
            eng.clone_mixture(E, start=good[:, :2])
        r = eng.clone_mixture(E, U, V)                               # still usable
        check_eval(r, ref_eval(Y, E, U, V, r["weights"]), "after the refusals")
    finally:
        eng.close()
        wide.close()
