"""ca_logexpr_sums / HipEngine.logexpr_sums / clone_expression_profile / plot_clonealign: the data side of plot_clonealign (R/plotting.R:177-205) in one
float64 sweep over the resident count matrix.

The yardstick is ``ref_profile`` below: ``lc = log2(Y / sf[:, None] + 1)`` restated in plain numpy float64, chunked over cells, in two passes (mean
first, then centred squares for the sd).

Bars.  Raw sums: relative 1e-10 on every entry of S1 and S2, n_group exact -- ca_fit_mse's bar with its derivation: both sides add non-negative
float64 terms in tree order (about log2(N G) 2^-53), the device's log2 differs from numpy's by a few ulp per term, and any float32 intermediate
(6e-8) fails.  Derived z-scores: for EVERY gene ``|mean_z - ref| <= 2e-10 (1 + kappa_g) (1 + |ref|)`` with ``kappa_g = S2_g / ((N - 1) var_g)`` from
the restatement: what a relative 1e-10 on S1 and S2 can do to ``(S1 / n - m) / sd`` through the cancellation ``S2 - N m^2`` in the variance."""
import threading

import numpy as np
import pytest

from tests._cases import make_case

pytestmark = pytest.mark.gpu
RTOL = 1e-10
SHAPES = [(33, 77, 2), (3000, 1234, 8), (5000, 2049, 20)]          # the shapes and storages of tests/test_gpu_fit_mse.py


def problem(N, G, C, storage, seed):
    """Counts for one storage width: u8 with several counts above 255 (the overflow list) and genuine 255s, u16 up to 60000, f32 with non-integer
    values (the construction of tests/test_gpu_fit_mse.py)."""
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


def ref_profile(Y, gidx, Q, sf=None, chunk=4096):
    """Two passes in numpy float64 over the cells with gidx >= 0; Y dense (any dtype) or scipy.sparse.  Returns S1 [G, Q], S2 [G], n_group [Q], mean,
    var (centred, n - 1), sd (0 -> 1), mean_z [G, Q] and kappa [G]."""
    gidx = np.asarray(gidx)
    N, G = Y.shape
    used = np.flatnonzero(gidx >= 0)

    def rows_of(lo):
        rows = used[lo:lo + chunk]
        Yc = Y[rows]
        return rows, np.asarray(Yc.toarray() if hasattr(Yc, "toarray") else Yc, dtype=np.float64)
    if sf is None:
        lib = np.zeros(N)
        for lo in range(0, used.size, chunk):
            rows, Yc = rows_of(lo)
            lib[rows] = Yc.sum(1)
        sf = lib / lib[used].mean()
    sf = np.asarray(sf, dtype=np.float64)
    S1, S2 = np.zeros((G, Q)), np.zeros(G)
    for lo in range(0, used.size, chunk):
        rows, Yc = rows_of(lo)
        lc = np.log2(Yc / sf[rows, None] + 1)
        S2 += (lc * lc).sum(0)
        for q in np.unique(gidx[rows]):
            S1[:, q] += lc[gidx[rows] == q].sum(0)
    n_group = np.bincount(gidx[used], minlength=Q)
    n = used.size
    mean = S1.sum(1) / n
    css = np.zeros(G)
    for lo in range(0, used.size, chunk):
        rows, Yc = rows_of(lo)
        css += ((np.log2(Yc / sf[rows, None] + 1) - mean) ** 2).sum(0)
    var = css / (n - 1)
    flat = var <= 1e-24 * S2 / n                                     # a gene that is constant over the used cells (all zero, or the two-pass
    var[flat] = 0.0                                                  # form's rounding of a constant): sd 0 -> 1 and z = 0 (R/plotting.R:193),
    sd = np.sqrt(var)                                                # held to the bound with kappa = 0, i.e. |z| <= 2e-10
    sd[sd == 0] = 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_z = (S1 / n_group[None, :] - mean[:, None]) / sd[:, None]
        mean_z[flat] = 0.0
        kappa = np.where(flat, 0.0, S2 / ((n - 1) * np.where(flat, 1.0, var)))
    return dict(S1=S1, S2=S2, n_group=n_group, mean=mean, var=var, sd=sd, mean_z=mean_z, kappa=kappa)


def check_sums(out, ref, tag=""):
    with np.errstate(divide="ignore", invalid="ignore"):
        e1 = np.nanmax(np.where(ref["S1"] > 0, np.abs(out["S1"] / ref["S1"] - 1), np.abs(out["S1"])))
        e2 = np.nanmax(np.where(ref["S2"] > 0, np.abs(out["S2"] / ref["S2"] - 1), np.abs(out["S2"])))
    print(f"logexpr_sums {tag}: S1 max rel {e1:.2e}, S2 max rel {e2:.2e}")
    assert np.array_equal(out["n_group"], ref["n_group"]), tag
    np.testing.assert_allclose(out["S1"], ref["S1"], rtol=RTOL, atol=0, err_msg=tag)
    np.testing.assert_allclose(out["S2"], ref["S2"], rtol=RTOL, atol=0, err_msg=tag)


def check_z(mean_z, ref, tag=""):
    """every gene, every group that has cells"""
    have = ref["n_group"] > 0
    bound = 2e-10 * (1 + ref["kappa"])[:, None] * (1 + np.abs(ref["mean_z"][:, have]))
    err = np.abs(np.asarray(mean_z)[:, have] - ref["mean_z"][:, have])
    print(f"mean_z {tag}: largest error / bound {np.max(err / bound):.3e} over {err.shape[0]} genes x {err.shape[1]} groups (max kappa {ref['kappa'].max():.3g})")
    assert np.all(np.isfinite(err)) and err.shape[0] == ref["S2"].shape[0]
    assert np.all(err <= bound), tag


def groups_for(N, C, rng):
    """clone labels 0..C-1 plus one extra group C for "unassigned"; a second copy with a tenth of the cells left out (-1)"""
    gidx = rng.integers(0, C + 1, N).astype(np.int32)
    skip = gidx.copy()
    skip[rng.choice(N, N // 10, replace=False)] = -1
    return gidx, skip


def bounded(fn, seconds=120):
    """fn() on a thread: (result or exception); fails instead of hanging when a collective is left waiting"""
    box = {}

    def run():
        try:
            box["value"] = fn()
        except Exception as e:                                      # noqa: BLE001
            box["error"] = e
    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(seconds)
    assert not t.is_alive(), f"the call did not return within {seconds} s"
    return box


@pytest.mark.parametrize("storage", ["u8", "u16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_with_the_float64_restatement(shape, storage):
    from clonealign_amd import api
    from clonealign_amd.engine import HipEngine
    N, G, C = shape
    Y, L, mu, _, rng = problem(N, G, C, storage, seed=sum(shape))
    gidx, skip = groups_for(N, C, rng)
    sf_own = rng.lognormal(0, 0.4, N)
    eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, y_storage=storage)
    try:
        assert eng.info()["y_storage_name"] == storage
        for lab, gi in (("all", gidx), ("tenth left out", skip)):
            for sfn, sf in (("library", None), ("given", sf_own)):
                tag = f"{shape} {storage} {lab} sf={sfn}"
                out = eng.logexpr_sums(gi, C + 1, sf)
                ref = ref_profile(Y, gi, C + 1, sf)
                check_sums(out, ref, tag)
                check_z(api._profile_from_sums(out["S1"], out["S2"], out["n_group"], range(C + 1))["mean_z"], ref, tag)
                again = eng.logexpr_sums(gi, C + 1, sf)                # two calls: identical bits
                assert np.array_equal(again["S1"], out["S1"]) and np.array_equal(again["S2"], out["S2"]) and np.array_equal(again["n_group"], out["n_group"])
        one = eng.logexpr_sums(np.zeros(N, dtype=np.int32), 1)        # one group, and an empty one beside it
        two = eng.logexpr_sums(np.zeros(N, dtype=np.int32), 2)
        assert np.array_equal(one["S1"][:, 0], two["S1"][:, 0]) and np.all(two["S1"][:, 1] == 0) and two["n_group"].tolist() == [N, 0]
    finally:
        eng.close()


def test_column_major_layout():
    from clonealign_amd.engine import HipEngine
    N, G, C = 1500, 700, 5
    Y, L, mu, _, rng = problem(N, G, C, "u8", seed=12)
    gidx, skip = groups_for(N, C, rng)
    outs = {}
    for lay in ("row", "col"):
        eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, layout=lay)
        try:
            outs[lay] = eng.logexpr_sums(skip, C + 1)
        finally:
            eng.close()
    check_sums(outs["col"], ref_profile(Y, skip, C + 1), "layout col")
    assert np.array_equal(outs["row"]["S1"], outs["col"]["S1"]) and np.array_equal(outs["row"]["S2"], outs["col"]["S2"])


@pytest.mark.parametrize("fmt", ["csr", "csc"])
def test_sparse_input_equals_the_dense_engine_bit_for_bit(fmt):
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
    gidx, skip = groups_for(N, C, rng)
    outs = []
    for mat in (Y, Ys):
        eng = HipEngine(mat, L, np.zeros((N, 0)), np.zeros(G), 0)
        try:
            assert eng.info()["y_storage_name"] == "u8"
            outs.append(eng.logexpr_sums(skip, C + 1))
        finally:
            eng.close()
    check_sums(outs[1], ref_profile(Ys.tocsr(), skip, C + 1), f"sparse {fmt}")
    for k in ("S1", "S2", "n_group"):
        assert np.array_equal(outs[0][k], outs[1][k]), k


@pytest.mark.parametrize("world", [2, 3])
def test_group_agrees_with_the_single_handle(world):
    from clonealign_amd.engine import HipEngine, HipGroupEngine
    N, G, C = 1301, 700, 8
    Y, L, mu, _, rng = problem(N, G, C, "u8", seed=31)
    gidx, skip = groups_for(N, C, rng)
    skip[N - 2] = 0                                                  # (a used cell of the last rank, for the refusals below)
    sf_own = rng.lognormal(0, 0.4, N)
    one = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0)
    try:
        o1 = {name: one.logexpr_sums(skip, C + 1, sf) for name, sf in (("library", None), ("given", sf_own))}
    finally:
        one.close()
    grp = HipGroupEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, devices=[0] * world)
    try:
        for name, sf in (("library", None), ("given", sf_own)):
            og = bounded(lambda: grp.logexpr_sums(skip, C + 1, sf))["value"]
            check_sums(og, ref_profile(Y, skip, C + 1, sf), f"group of {world}, sf={name}")
            assert np.array_equal(og["n_group"], o1[name]["n_group"])
            np.testing.assert_allclose(og["S1"], o1[name]["S1"], rtol=RTOL, atol=0)
            np.testing.assert_allclose(og["S2"], o1[name]["S2"], rtol=RTOL, atol=0)
        # refused on the LAST rank's cells only: every rank returns the code (the group stays alive and usable), nothing hangs
        bad = skip.copy()
        bad[N - 1] = C + 1
        box = bounded(lambda: grp.logexpr_sums(bad, C + 1))
        assert box["error"].code == 1 and box["error"].msg, box
        box = bounded(lambda: grp.logexpr_sums(skip, 65))
        assert box["error"].code == 1 and "65" in box["error"].msg
        box = bounded(lambda: grp.logexpr_sums(skip, C + 1, np.where(np.arange(N) == N - 2, 0.0, sf_own)))
        assert box["error"].code == 1 and "size factor" in box["error"].msg, box
        again = bounded(lambda: grp.logexpr_sums(skip, C + 1))["value"]
        assert np.array_equal(again["n_group"], o1["library"]["n_group"])
        np.testing.assert_allclose(again["S1"], o1["library"]["S1"], rtol=RTOL, atol=0)
    finally:
        grp.close()


@pytest.mark.parametrize("world", [1, 2])
def test_refusals(world):
    """A zero-library used cell, a group index equal to n_groups and n_groups = 65: CA_ERR_INVALID with a message, on a handle and on a group."""
    from clonealign_amd.engine import EngineError, HipEngine, HipGroupEngine
    case = make_case(N=700, G=300, C=4, K=0, seed=2)
    Y, L = case["Y"].copy(), case["L"]
    Y[650] = 0                                                       # an empty cell, in the last rank's shard
    N = 700
    gidx = np.random.default_rng(0).integers(0, 5, N).astype(np.int32)
    gidx[650] = 3
    eng = (HipEngine(Y, L, np.zeros((N, 0)), np.zeros(300), 0) if world == 1 else
           HipGroupEngine(Y, L, np.zeros((N, 0)), np.zeros(300), 0, devices=[0] * world))
    try:
        box = bounded(lambda: eng.logexpr_sums(gidx, 5))
        assert isinstance(box["error"], EngineError) and box["error"].code == 1, box
        assert "size factor" in box["error"].msg and ("cell 650" in box["error"].msg or world > 1), box["error"].msg
        left_out = gidx.copy()
        left_out[650] = -1                                           # the same cell left out: fine
        ok = bounded(lambda: eng.logexpr_sums(left_out, 5))["value"]
        check_sums(ok, ref_profile(Y, left_out, 5), f"empty cell left out, world {world}")
        for value in (5, -2):
            bad = left_out.copy()
            bad[11] = value
            box = bounded(lambda: eng.logexpr_sums(bad, 5))
            assert box["error"].code == 1 and "group index" in box["error"].msg and "cell 11" in box["error"].msg, box["error"].msg
        for q in (65, 0):
            box = bounded(lambda: eng.logexpr_sums(left_out, q))
            assert box["error"].code == 1 and "n_groups" in box["error"].msg, box["error"].msg
        for value in (0.0, -1.0, np.inf, np.nan):
            sf = np.ones(N)
            sf[20] = value
            box = bounded(lambda: eng.logexpr_sums(left_out, 5, sf))
            assert box["error"].code == 1 and "size factor" in box["error"].msg and "cell 20" in box["error"].msg, box["error"].msg
        sf = np.ones(N)
        sf[650] = 0.0                                                # a bad size factor of a cell that is left out: fine
        assert np.array_equal(bounded(lambda: eng.logexpr_sums(left_out, 5, sf))["value"]["n_group"], ok["n_group"])
    finally:
        eng.close()


def test_read_only_and_refused_from_a_poll_hook():
    """Five iterations, logexpr_sums, five more == ten iterations straight, bit for bit; from a poll hook the call is CA_ERR_STATE."""
    from clonealign_amd.engine import EngineError, HipEngine
    from clonealign_amd.rng import EpsStream
    case = make_case(N=2600, G=640, C=5, K=1, seed=21)
    gidx = np.random.default_rng(1).integers(-1, 6, 2600).astype(np.int32)
    a = HipEngine(**case)
    try:
        ea = a.iterate(10, None)
        sa = a.get_state()
    finally:
        a.close()
    b = HipEngine(**case)
    try:
        b.iterate(5, None)
        check_sums(b.logexpr_sums(gidx, 6), ref_profile(case["Y"], gidx, 6), "mid-fit")
        eb = b.iterate(5, None)
        sb = b.get_state()
        seen = {}

        def hook(i, e):
            if i == 2:
                with pytest.raises(EngineError) as ex:
                    b.logexpr_sums(gidx, 6)
                seen["code"] = ex.value.code
            return False
        b.run(EpsStream(9, 1, 640), 4, 1e-12, poll=hook)
        assert seen["code"] == 6                                     # CA_ERR_STATE
    finally:
        b.close()
    assert ea == eb
    for n in sa:
        assert np.array_equal(sa[n], sb[n]), n


def test_plot_clonealign_on_the_live_engine_of_a_fit(monkeypatch):
    import clonealign_amd as ca
    from clonealign_amd import api, engine as eng_mod
    N, G, C = 600, 300, 4
    case = make_case(N=N, G=G, C=C, K=1, seed=17, scale=1.0)
    Y, L = case["Y"].astype(np.int32), case["L"]
    rng = np.random.default_rng(3)
    row = {"chr": np.where(np.arange(G) % 3 == 0, "2", "1"), "start_position": rng.integers(1, 10 ** 6, G), "end_position": rng.integers(1, 10 ** 6, G)}
    sce = {"assays": {"counts": np.ascontiguousarray(Y.T)}, "rowData": row}
    fit = ca.clonealign(sce, L, max_iter=30, verbose=False, seed=3)
    assert len(fit["clone"]) == N
    live = eng_mod.HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0)   # a live engine whose resident matrix is the counts of sce
    try:
        dev = ca.plot_clonealign(sce, fit["clone"], L, chromosome="1", jitter_cnv=False, engine=live)
        assert live.info()["y_storage_name"] in ("u8", "u16", "f32")   # still open: the caller's engine is not closed
    finally:
        live.close()

    class HostOnly:
        pass
    stub = HostOnly()
    stub.N, stub.G = N, G
    host = ca.plot_clonealign(sce, fit["clone"], L, chromosome="1", jitter_cnv=False, engine=stub)
    labels = dev.labels
    assert labels == host.labels == list(dict.fromkeys(fit["clone"].tolist()))
    lut = {c: i for i, c in enumerate(labels)}
    ref = ref_profile(Y, np.array([lut[c] for c in fit["clone"]]), len(labels))
    check_z(dev.profile["mean_z"], ref, "plot_clonealign, live engine")
    check_z(host.profile["mean_z"], ref, "plot_clonealign, host form")
    gi = dev.genes["gene_index"]
    assert np.array_equal(gi, np.flatnonzero(row["chr"] == "1")) and np.array_equal(gi, host.genes["gene_index"])
    bound = 2e-10 * (1 + ref["kappa"][gi])[None, :] * (1 + np.abs(ref["mean_z"][gi].T))               # [label, gene on the chromosome]
    d = np.abs(dev.expression["mean_z_score"].reshape(len(labels), gi.size) - host.expression["mean_z_score"].reshape(len(labels), gi.size))
    print(f"plot_clonealign: device vs host form, largest difference / bound {np.max(d / bound):.3e}")
    assert np.all(d <= bound)
    for k in ("state", "start", "end", "length", "copy_number"):
        assert np.array_equal(dev.cnv_segments[k], host.cnv_segments[k]), k
    assert np.array_equal(dev.expression_segments["clone"], host.expression_segments["clone"])
    # a (clone, state) value is the mean of its genes' values: held to the mean of those genes' bounds
    es, state = dev.expression_segments, dev.genes["state"]
    seg_bound = np.array([bound[lut[c]][state == st].mean() for c, st in zip(es["clone"], es["state"])])
    seg_d = np.abs(es["per_clone_state_z_score"] - host.expression_segments["per_clone_state_z_score"])
    print(f"plot_clonealign: per (clone, state), largest difference / bound {np.max(seg_d / seg_bound):.3e} over {seg_d.size} segments")
    assert seg_d.size > 0 and np.all(seg_d <= seg_bound)
    # engine=None: clone_expression_profile builds its own engine and closes it
    made = []
    real = eng_mod.HipEngine

    class Spy(real):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    monkeypatch.setattr(eng_mod, "HipEngine", Spy)
    prof = api.clone_expression_profile(Y, fit["clone"])
    assert len(made) == 1 and not made[0].h                         # closed
    check_z(prof["mean_z"], ref, "clone_expression_profile, own engine")
    assert np.array_equal(prof["mean_z"], dev.profile["mean_z"])


def test_at_size_100k_cells():
    """100k x 5k x 8 in u8 storage with an overflow list; also guards 64-bit indexing (N * Gp = 5.1e8 bytes)."""
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
    gidx, skip = groups_for(N, C, rng)
    eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0)
    try:
        assert eng.info()["y_storage_name"] == "u8"
        out = eng.logexpr_sums(skip, C + 1)
    finally:
        eng.close()
    check_sums(out, ref_profile(Y, skip, C + 1), "100k x 5k x 8")
