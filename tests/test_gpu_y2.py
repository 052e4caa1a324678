"""The series form's 2-bit / 4-bit loop image (CA_VAR_Y2): within each 512-gene segment the genes are ordered by how often they reach 3, the first N2 64-gene
blocks of a segment hold min(y, 3) in 2 bits and every count from 3 up in an escape list, the other blocks keep 4 bits.  Integer sums are order-free, so every
gradient, ELBO and parameter is the 4-bit image's and the 1-byte image's bit for bit: the oracle of every test here is the same engine with
variant_off=("y2",) and with ("y2", "y4"), compared with np.array_equal.  The default picks the image only from a size far above these shapes; they force it
(variant_on "y2", N2 = 6)."""
import numpy as np
import pytest
import scipy.sparse as sps

from tests._cases import eps_for, make_case
from tests._y2_ref import plan_np, stored_u8

pytestmark = pytest.mark.gpu

ON = ("series", "y2")


def _skewed(N, G, seed, frac_hi=0.15):
    """Gene means drawn log-normally (the sort is not the identity), a few counts from 15 up and a few above 255."""
    rng = np.random.default_rng(seed)
    mu = rng.lognormal(-1.5, 1.6, G)
    mu[rng.random(G) < frac_hi] *= 8.0
    Y = rng.poisson(np.minimum(mu, 40.0)[None, :], size=(N, G)).astype(np.float64)
    flat = rng.choice(Y.size, max(Y.size // 3000, 4), replace=False)
    Y.flat[flat] = rng.integers(200, 400, size=flat.size)
    Y[:, 0] += 1
    Y[0, :] += 1
    return Y


def _case(Y, C=4, seed=3):
    N, G = Y.shape
    c = make_case(N=8, G=G, C=C, K=1, seed=seed)
    rng = np.random.default_rng(seed)
    return dict(Y=Y, L=c["L"], psi0=rng.normal(size=(N, 1)), loc0=c["loc0"], K=1, S=1)


def _drive(eng, G, n_iter=3):
    out = []
    if hasattr(eng, "gradients"):
        g, e = eng.gradients(eps_for(1, G, 5))
        out.append(np.asarray([e]))
        out.extend(np.asarray(g[k]) for k in sorted(g))
    eps = np.stack([eps_for(1, G, 20 + i)[0] for i in range(2 * n_iter)])[:, None, :]
    out.append(np.asarray([eng.iterate(n_iter, eps)]))
    return out


def _trio(make, G, drive=_drive, n2=6, check=None):
    """The forced image against the 4-bit image and the 1-byte image: bit-equal traces and states.  Returns the forced engine's info."""
    res = []
    for off, want_n2, want_bits in (((), n2, 4), (("y2",), 0, 4), (("y2", "y4"), 0, 8)):
        eng = make(off)
        try:
            i0 = eng.rank_info(0) if hasattr(eng, "rank_info") else eng.info()
            assert i0["fwd_series"] == 1, i0
            assert (i0["y_stream_n2"], i0["y_stream_bits"]) == (want_n2, want_bits), (off, i0["y_stream_n2"], i0["y_stream_bits"])
            traces = drive(eng, G)
            st = eng.get_state() if hasattr(eng, "get_state") else eng.get_params()
            i1 = eng.rank_info(0) if hasattr(eng, "rank_info") else eng.info()
            res.append((traces, st, i0, i1))
        finally:
            eng.close()
    ta, sa, ia, ja = res[0]
    for tb, sb, _, jb in res[1:]:
        assert len(ta) == len(tb)
        for x, y in zip(ta, tb):
            assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (x, y)
        assert set(sa) == set(sb)
        for k in sb:
            assert np.array_equal(sa[k], sb[k], equal_nan=True), k
        assert (ja["series_passes"], ja["series_fallbacks"]) == (jb["series_passes"], jb["series_fallbacks"]), (ja, jb)
    if check:
        check(ia, ja)
    return ia


def _host(case, variant_on=ON, **kw):
    from clonealign_amd.engine import HipEngine
    return lambda off: HipEngine(**case, variant_on=variant_on, variant_off=off, **kw)


def _matches_plan(info, Y, force=6):
    n2, n_esc, _, _ = plan_np(stored_u8(Y), force)
    assert (info["y_stream_n2"], info["y_stream_esc"]) == (n2, n_esc), (info["y_stream_n2"], info["y_stream_esc"], n2, n_esc)


@pytest.mark.parametrize("N,G", [(4133, 1030), (1000, 333)])
def test_y2_ragged(N, G):
    """No size a multiple of a tile; at 333 genes the only segment is mostly padding and ties decide the order."""
    Y = _skewed(N, G, N)
    info = _trio(_host(_case(Y)), G)
    _matches_plan(info, Y)
    _, _, perm, _ = plan_np(stored_u8(Y), 6)
    assert not np.array_equal(perm[:512], np.arange(512))          # the sort moved genes


def test_y2_boundary_counts():
    """2, 3, 4, 14, 15, 16, 255 and 300 planted in genes that are otherwise all zero (narrow blocks) and in genes that are mostly >= 3 (wide blocks)."""
    N, G = 3000, 1100
    rng = np.random.default_rng(9)
    Y = np.zeros((N, G))
    hot = rng.choice(G, G // 5, replace=False)                     # 220 of 1100: past the 2 x 64 wide positions of each segment some stay narrow, so plant by the plan
    Y[:, hot] = rng.poisson(6.0, size=(N, hot.size))
    Y[:, 0] += 1
    Y[0, :] += 1
    u8 = stored_u8(Y)
    _, _, _, pos = plan_np(u8, 6)
    narrow = np.flatnonzero((pos < 384)[:G] & (u8.sum(0) <= 2))    # all-zero genes (but for the first row) in narrow blocks
    wide = np.flatnonzero((pos >= 384)[:G])
    assert narrow.size >= 40 and wide.size >= 40
    for i, v in enumerate((2, 3, 4, 14, 15, 16, 255, 300)):
        rows = slice(10 + 30 * i, 40 + 30 * i)
        Y[rows, rng.choice(narrow, 20, replace=False)[:, None]] = v
        Y[rows, rng.choice(wide, 20, replace=False)[:, None]] = v
    u8 = stored_u8(Y)
    _, _, _, pos2 = plan_np(u8, 6)
    assert (pos2[narrow] < 384).mean() > 0.9 and (pos2[wide] >= 384).mean() > 0.5   # the planted genes stayed where they were meant to be
    info = _trio(_host(_case(Y)), G)
    _matches_plan(info, Y)


def test_y2_identity_order():
    """Every gene has the same histogram (each column a rotation of one column): the order is the identity by the tie rule."""
    N, G = 2048, 512
    rng = np.random.default_rng(4)
    col = rng.poisson(1.2, size=N).astype(np.float64)
    col[:3] = (17, 3, 260)
    Y = np.stack([np.roll(col, 5 * g) for g in range(G)], axis=1)
    _, _, perm, _ = plan_np(stored_u8(Y), 6)
    assert np.array_equal(perm[:512], np.arange(512))
    info = _trio(_host(_case(Y)), G)
    _matches_plan(info, Y)


def test_y2_many_escapes_in_a_step():
    """One 64-cell step of one segment with about 150 and one with about 300 entries from narrow-block genes: past the 128 prefetched ones, and past 256."""
    N, G = 640, 512
    rng = np.random.default_rng(6)
    Y = rng.poisson(0.05, size=(N, G)).astype(np.float64)
    Y[:, 448:] = rng.poisson(7.0, size=(N, 64))                    # the wide blocks' genes
    Y[:, 0] += 1
    Y[0, :] += 1
    for r0, n in ((64, 150), (256, 300)):
        idx = rng.choice(64 * 384, n, replace=False)
        Y[r0 + idx // 384, idx % 384] = rng.integers(3, 40, size=n)
    u8 = stored_u8(Y)
    _, _, _, pos = plan_np(u8, 6)
    nar = pos[:G] < 384
    per_step = [(u8[s:s + 64][:, nar] >= 3).sum() + (u8[s:s + 64][:, ~nar] >= 15).sum() for s in range(0, N, 64)]
    assert max(per_step) > 256 and sorted(per_step)[-2] > 128, per_step
    info = _trio(_host(_case(Y)), G)
    _matches_plan(info, Y)


def test_y2_csr_ingest():
    Y = _skewed(5000, 1500, 6)
    case = _case(Y)
    sp = dict(case, Y=sps.csr_matrix(Y))
    info = _trio(_host(sp), 1500)
    _matches_plan(info, Y)


def test_y2_two_ranks_on_one_device():
    """Each rank builds its image from its own cells; the group's trace and state are the same group's with the image off, bit for bit, whatever image the
    ranks read (a sharded fit is not bit-equal to the one-handle fit with any image: the ranks' partial sums meet in another order, tests/test_gpu_group.py)."""
    from clonealign_amd.engine import HipGroupEngine
    case = make_case(seed=31, N=2400, G=640, C=5, K=1)

    def drive(eng, G):
        from clonealign_amd.rng import EpsStream
        eps = np.stack([eps_for(1, G, 40 + i) for i in range(9)])
        return [np.asarray(eng.run(EpsStream(7, 1, G), 5, 1e-12)), np.asarray([eng.iterate(4, eps)])]

    _trio(lambda off: HipGroupEngine(**case, variant_on=ON, variant_off=off, devices=[0, 0], transport="host"), 640, drive=drive)


def test_y2_passes_handed_to_the_sweeps_and_back():
    """W blown up by hand: those passes go to the sweeps, whose riding stream reads the 4-bit image; W back: the 2-bit / 4-bit image again, inside one fit."""
    case = make_case(seed=35, N=900, G=300, C=5, K=1)
    eps = np.stack([eps_for(1, 300, 70 + i) for i in range(9)])

    def drive(eng, G):
        eng.gamma_init(eps_for(1, G, 0))
        out = [np.asarray([eng.iterate(4, eps)])]
        W = eng.get("W")
        eng.set("W", W * 60.0 + 3.0 * np.sign(W))
        out.append(np.asarray([eng.iterate(4, eps)]))
        eng.set("W", W)
        out.append(np.asarray([eng.iterate(4, eps)]))
        return out

    def check(i0, i1):
        assert i1["series_fallbacks"] > 0 and i1["series_passes"] >= 8, i1

    _trio(_host(case), 300, drive=drive, check=check)


@pytest.fixture(scope="module")
def long_strips():
    """26 700 x 4 700 drawn on the device: strips of 128 cells, so a wave crosses a step boundary and its last loads lie past the strip."""
    import torch
    import synth_data as synth
    from clonealign_amd.hostprep import safe_inverse_softplus
    N, G, C = 26700, 4700, 8
    Yd, aux = synth.make_problem_torch(N, G, C, seed=20251, device="cuda:0")
    rm = Yd.sum(1, keepdim=True).to(torch.float64) / G
    col = (Yd.to(torch.float64) / rm).sum(0)
    loc0 = safe_inverse_softplus(np.maximum(col.cpu().numpy() / N, 1e-6))
    psi0 = np.random.default_rng(20252).normal(size=(N, 1))
    torch.cuda.synchronize()

    def make(off, variant_on=ON):
        from clonealign_amd.engine import HipEngine
        return HipEngine(None, aux["L"], psi0, loc0, 1, 1, y_device_ptr=Yd.data_ptr(), y_device_dtype=np.int32, shape=(N, G), device=0, profile=0, variant_on=variant_on, variant_off=off)
    yield dict(make=make, G=G, Y=Yd)
    del Yd


def test_y2_strips_longer_than_a_step(long_strips):
    info = _trio(long_strips["make"], long_strips["G"], drive=lambda e, G: _drive(e, G, n_iter=2))
    _matches_plan(info, long_strips["Y"].cpu().numpy())


def test_y2_pick(long_strips):
    """Below the size floor the default keeps the 4-bit image alone; forced, N2 = 6 and the list the rule's restatement counts."""
    eng = long_strips["make"]((), variant_on=())
    try:
        i = eng.info()
        assert (i["fwd_series"], i["y_stream_bits"], i["y_stream_n2"]) == (1, 4, 0), i
        assert i["y_stream_bytes"] == 26752 * 5120 // 2 + 4 * i["y_stream_esc"]
    finally:
        eng.close()
    eng = long_strips["make"](())
    try:
        j = eng.info()
        assert j["y_stream_n2"] == 6
        assert j["y_stream_bytes"] == (26752 // 64) * 10 * (6 * 1024 + 2 * 2048) + 4 * j["y_stream_esc"]
        assert j["y_device_bytes"] > i["y_device_bytes"] + j["y_stream_bytes"] - 1
    finally:
        eng.close()
