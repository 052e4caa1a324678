"""The moment role BEHIND the stream's blocks (CA_VAR_MOM_LAST / CA_VARX_MOM_LAST, clonealign_amd/csrc/ca_polymom.hip.h): the same launch of the count-matrix stream
with the series form's forward moments riding (tests/test_gpu_mom_ride.py), its blocks in another order -- the stream's blocks first, so that all of them are
resident from the start, the moment blocks and their reducers in the slots the stream leaves free, the overflow list's blocks last.  Scheduling only: the stream's
body gets the block index it got, the moment role the same group and reducer numbers, no sum a new operand or a new order.  So a fit with the order forced on and one
with the switch off (the role in front, block for block the launch as it was) must agree to the last bit: ELBO traces, every state array, the pass counts.
(The reducers' bounded wait has no test that provokes it; its path is unchanged and is read in the code.)"""
import numpy as np
import pytest

from tests._cases import eps_for, make_case
from tests.test_gpu_mom_ride import _drive_default, _wide

pytestmark = pytest.mark.gpu

# ---- the rule (ca_mom_last_pick, clonealign_amd/csrc/ca_eng_create.inc) with the constants recorded in profiles/r14_mom_last_ab.txt, restated here on purpose -----------
ML_STREAM_FIXED_US = 6.6            # the stream's launch alone: fixed part ...
ML_STREAM_BYTES_PER_US = 5.62e6     # ... and stored image bytes per microsecond (fit of 17.66 / 29.42 / 52.20 us at 25k / 50k / 100k cells x 5k genes)
ML_MIN_STREAM_US = 45.0             # the shortest stream behind which the role's one-round chain is taken to pay (it does at 52.2 us, it does not at 29.4 us)
ML_MAX_PER = 4                      # the most gene groups per moment block that was measured
MOM_NRED = 21


def _expected_pick(info):
    """What the rule gives for this engine, from what ca_get_info reports: shape, compute units, bits per stored count and the free slots the rule saw."""
    N, G, n_cu = int(info["N"]), int(info["G"]), int(info["n_cu"])
    Gp = (G + 1023) // 1024 * 1024
    nseg = Gp // 1024
    cdiv = lambda a, b: (a + b - 1) // b    # noqa: E731
    RS = 64
    while RS < 512 and cdiv(N, 4 * RS) * nseg > 4 * n_cu:
        RS *= 2
    nb_stream = cdiv(N, 4 * RS) * nseg
    free = int(info["mom_free_slots"])
    slots = nb_stream + free
    ngrp = cdiv(G, 32)
    xcd = max(n_cu // 32, 1)
    if nb_stream + ngrp + MOM_NRED <= slots:       # nothing would be displaced
        return 0
    free_x = slots // xcd - cdiv(nb_stream, xcd)  # the XCD with the most stream blocks
    if free_x < 1:
        return 0
    per = max(1, cdiv(ngrp, free_x * xcd))        # gene groups per moment block for one round of the free slots
    if per > ML_MAX_PER:
        return 0
    image = (N + 63) // 64 * 64 * Gp * int(info["y_stream_bits"]) // 8
    return int(ML_STREAM_FIXED_US + image / ML_STREAM_BYTES_PER_US >= ML_MIN_STREAM_US)


def _pair(make, drive, G, variant_on=("series",), variant_off=(), bits=None, ranks=0):
    """The same fit with the moment role behind the stream's blocks (forced) and with the switch off: bit-equal traces and states, equal pass counts."""
    res = []
    for last in (True, False):
        eng = make(variant_on=tuple(variant_on) + (("mom_last",) if last else ()), variant_off=tuple(variant_off) + (() if last else ("mom_last",)))
        try:
            i0 = eng.rank_info(0) if ranks else eng.info()
            assert i0["fwd_series"] == 1 and i0["mom_ride"] == 1, i0
            assert i0["mom_last"] == int(last), (last, i0["mom_last"])
            if bits is not None:
                assert i0["y_stream_bits"] == bits, i0["y_stream_bits"]
            traces = drive(eng, G)
            infos = [eng.rank_info(r) for r in range(ranks)] if ranks else [eng.info()]
            res.append((traces, eng.get_state(), infos))
        finally:
            eng.close()
    (ta, sa, ia), (tb, sb, ib) = res
    assert len(ta) == len(tb)
    for x, y in zip(ta, tb):
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (x, y)
    assert set(sa) == set(sb)
    for n in sb:
        assert np.array_equal(sa[n], sb[n], equal_nan=True), n
    for x, y in zip(ia, ib):
        assert (x["series_passes"], x["series_fallbacks"]) == (y["series_passes"], y["series_fallbacks"]), (x, y)
        assert x["series_passes"] > 0
    return ia[0]


def _host(case, group=None):
    from clonealign_amd.engine import HipEngine, HipGroupEngine
    if group:
        return lambda **kw: HipGroupEngine(**case, **group, **kw)
    return lambda **kw: HipEngine(**case, **kw)


@pytest.fixture(scope="module")
def big():
    """25 000 x 5 000 x 8, generated on the device once and handed over by pointer: 980 stream blocks at the 64-cell strip and 157 + 21 blocks of the moment role."""
    import torch
    import synth_data as synth
    from clonealign_amd.hostprep import safe_inverse_softplus
    N, G, C = 25_000, 5_000, 8
    Yd, aux = synth.make_problem_torch(N, G, C, seed=20251, device="cuda:0")
    rm = Yd.sum(1, keepdim=True).to(torch.float64) / G
    col = (Yd.to(torch.float64) / rm).sum(0)
    loc0 = safe_inverse_softplus(np.maximum(col.cpu().numpy() / N, 1e-6))
    psi0 = np.random.default_rng(20252).normal(size=(N, 1))
    eps = np.stack([eps_for(1, G, 500 + i) for i in range(9)])
    torch.cuda.synchronize()

    def make(**kw):
        from clonealign_amd.engine import HipEngine
        return HipEngine(None, aux["L"], psi0, loc0, 1, 1, y_device_ptr=Yd.data_ptr(), y_device_dtype=np.int32, shape=(N, G), device=0, profile=0, **kw)
    yield dict(make=make, G=G, eps=eps)
    del Yd
    torch.cuda.empty_cache()


def _drive_iterate(eps):
    def drive(eng, G):
        eng.gamma_init(eps_for(1, G, 0))
        return [np.asarray([eng.iterate(4, eps)])]
    return drive


def test_everything_resident():
    """A few stream blocks and a few of the moment role, all resident at once: only the indices swap."""
    case = make_case(seed=41, N=1301, G=700, C=8, K=1)
    i = _pair(_host(case), _drive_default, 700, variant_on=("series", "y4"), bits=4)
    assert i["series_fallbacks"] == 0


def test_moment_blocks_queue_behind_the_streams_blocks(big):
    """The case the order exists for: 980 + 178 blocks on 1024 slots -- the moment blocks wait for the few slots the stream leaves free."""
    i = _pair(big["make"], _drive_iterate(big["eps"]), big["G"], variant_on=())
    assert i["mom_last"] == 1 and i["series_passes"] >= 4, i


def test_several_bins():
    """Wide loadings: the reducers read nb > 1 from the header a moment block behind the stream's blocks wrote."""
    case = make_case(seed=42, N=900, G=300, C=5, K=1)
    W = _wide(case, 0.45)      # max|psi| ~ 3.3, W range ~ 2.5: product ~ 8 -> two or three bins
    i = _pair(_host(case), lambda e, G: _drive_default(e, G, W), 300, variant_on=("series", "y4"), bits=4)
    assert i["series_fallbacks"] == 0


def test_one_byte_image_with_overflow_blocks():
    """The 1-byte stream and counts above 255: k_ys_mfma_ovf_mom<false>, the overflow list's blocks behind the moment role."""
    case = make_case(seed=41, N=1301, G=700, C=8, K=1)
    rng = np.random.default_rng(5)
    Y = case["Y"].copy()
    idx = rng.choice(Y.size, 300, replace=False)
    Y.flat[idx] = rng.integers(256, 900, size=idx.size)
    case["Y"] = Y
    assert (Y > 255).sum() >= 300
    _pair(_host(case), _drive_default, 700, variant_off=("y4",), bits=8)


def test_two_ranks_on_one_device_over_the_host_reduction():
    """Cell-sharded: max |psi| of all ranks from the slots the fit's collective carries (nglob), read by moment blocks that start late; replicas bit-identical."""
    case = make_case(seed=31, N=2400, G=640, C=5, K=1)
    _pair(_host(case, group=dict(devices=[0, 0], transport="host")), _drive_default, 640, ranks=2)


def test_rule_keeps_the_order_where_nothing_is_displaced():
    from clonealign_amd.engine import HipEngine
    eng = HipEngine(**make_case(seed=41, N=1301, G=700, C=8, K=1), variant_on=("series", "y4"))
    try:
        i = eng.info()
        assert i["mom_ride"] == 1 and i["mom_last"] == 0, i
        assert _expected_pick(i) == 0, i
    finally:
        eng.close()


def test_rule_at_the_size_where_blocks_are_displaced(big):
    eng = big["make"]()
    try:
        i = eng.info()
        assert i["fwd_series"] == 1 and i["mom_ride"] == 1 and i["y_stream_bits"] == 4, i
        print("mom_last", i["mom_last"], "free slots", i["mom_free_slots"], "expected", _expected_pick(i))
        assert 0 < i["mom_free_slots"] < 157 + 21, i      # 980 stream blocks (98 strips x 10 gene segments) leave a few slots, fewer than the role has blocks
        assert i["mom_last"] == _expected_pick(i), i
    finally:
        eng.close()
