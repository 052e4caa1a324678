"""The series form's forward moments as the MOMENT ROLE of its count-matrix stream's launch (CA_VAR_MOM_RIDE, clonealign_amd/csrc/ca_polymom.hip.h): the first
blocks of k_ys_mfma_mom / k_ys_mfma_ovf_mom make the bin geometry, the per-group partials and their fixed-order sums that k_poly_B + k_poly_red make as two launches
in front of the stream when the switch is off.  Scheduling only: both orders call the same bodies, every sum keeps its operands and its order, so a fit with the
switch on and one with it off must agree to the last bit -- ELBO traces, every state array, and the passes each gave to the series form and to the sweeps.
(The reducers' bounded wait has no test that provokes it; its error path -- sticky word, block leaves, comm_check reports CA_ERR_STATE -- is read in the code.)"""
import numpy as np
import pytest

from tests._cases import eps_for, make_case

pytestmark = pytest.mark.gpu


def _wide(case, sigma, seed=2):
    """Loadings spread so that max|psi| (max W - min W) needs several bins."""
    G = case["Y"].shape[1]
    return np.random.default_rng(seed).normal(0, sigma, size=(G, 1)).astype(np.float32).astype(np.float64)


def _drive_default(eng, G, W=None):
    from clonealign_amd.rng import EpsStream
    eps = np.stack([eps_for(1, G, 40 + i) for i in range(9)])
    out = []
    if W is not None:
        eng.gamma_init(eps_for(1, G, 0))
        eng.set("W", W)
    else:
        out.append(np.asarray(eng.run(EpsStream(7, 1, G), 5, 1e-12)))
    out.append(np.asarray([eng.iterate(4, eps)]))
    out.append(np.asarray(eng.run(EpsStream(9, 1, G), 3, 1e-12)))
    return out


def _on_off(case, drive, variant_on=("series",), variant_off=(), bits=None, group=None):
    """The same fit with the moments riding and with their own launches: bit-equal traces and states, equal pass counts; returns the riding engine's info."""
    from clonealign_amd.engine import HipEngine, HipGroupEngine
    G = case["Y"].shape[1]
    res = []
    for off in ((), ("mom_ride",)):
        if group:
            eng = HipGroupEngine(**case, variant_on=variant_on, variant_off=tuple(variant_off) + off, **group)
        else:
            eng = HipEngine(**case, variant_on=variant_on, variant_off=tuple(variant_off) + off)
        try:
            i0 = eng.info()
            assert i0["fwd_series"] == 1, i0
            assert i0["mom_ride"] == (0 if off else 1), (off, i0["mom_ride"])
            if bits is not None:
                assert i0["y_stream_bits"] == bits, i0["y_stream_bits"]
            traces = drive(eng, G)
            infos = [eng.rank_info(r) for r in range(len(group["devices"]))] if group else [eng.info()]
            res.append((traces, eng.get_state(), infos))      # (a group's get_state also checks that the ranks' replicas are bit-identical)
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


def test_one_bin():
    """A fresh fit: W starts at zero and stays small -- one bin."""
    i = _on_off(make_case(seed=41, N=1301, G=700, C=8, K=1), _drive_default, variant_on=("series", "y4"), bits=4)
    assert i["series_fallbacks"] == 0


def test_two_or_three_bins():
    case = make_case(seed=42, N=900, G=300, C=5, K=1)
    W = _wide(case, 0.45)      # max|psi| ~ 3.3, W range ~ 2.5: product ~ 8 -> two or three bins
    i = _on_off(case, lambda e, G: _drive_default(e, G, W), variant_on=("series", "y4"), bits=4)
    assert i["series_fallbacks"] == 0


def test_wide_exponent_range_takes_the_slab_path():
    """Thirteen or so bins: past the four a thread keeps in registers (NBR) and the four whose tables sit in LDS (NBL)."""
    case = make_case(seed=33, N=600, G=200, C=4, K=1)
    W = _wide(case, 2.5)       # max|psi| ~ 3.2, W range ~ 14: product ~ 45 -> a dozen bins
    i = _on_off(case, lambda e, G: _drive_default(e, G, W), variant_on=("series", "y4"), bits=4)
    assert i["series_fallbacks"] == 0


def test_a_pass_handed_to_the_sweeps_and_back():
    """W blown up by hand: the guard gives those passes to the sweeps (the moments' role is not launched, the ranges keep their own launches); W back: the series
    form, and the riding moments, take over again."""
    case = make_case(seed=35, N=900, G=300, C=5, K=1)
    eps = np.stack([eps_for(1, 300, 70 + i) for i in range(9)])
    seen = []

    def drive(eng, G):
        eng.gamma_init(eps_for(1, G, 0))
        out = [np.asarray([eng.iterate(4, eps)])]
        p0 = eng.info()
        W = eng.get("W")
        eng.set("W", W * 60.0 + 3.0 * np.sign(W))
        out.append(np.asarray([eng.iterate(4, eps)]))
        p1 = eng.info()
        eng.set("W", W)
        out.append(np.asarray([eng.iterate(4, eps)]))
        p2 = eng.info()
        seen.append((p0, p1, p2))
        return out

    _on_off(case, drive)
    for p0, p1, p2 in seen:
        assert p0["series_fallbacks"] == 0 and p0["series_passes"] >= 4, p0
        assert p1["series_fallbacks"] > 0, p1
        assert p2["series_passes"] > p1["series_passes"], (p1, p2)


def test_one_byte_image():
    """The 1-byte loop image (what the configurations with many counts from 15 up keep): k_ys_mfma_mom<false>."""
    _on_off(make_case(seed=43, N=1301, G=700, C=8, K=1), _drive_default, variant_off=("y4",), bits=8)


@pytest.mark.parametrize("bits", [4, 8])
def test_counts_above_255_run_the_overflow_kernel(bits):
    """Entries above 255 put the overflow list's blocks behind the stream's: k_ys_mfma_ovf_mom, three kinds of block in one launch."""
    case = make_case(seed=44, N=1100, G=520, C=6, K=1)
    rng = np.random.default_rng(5)
    Y = case["Y"].copy()
    idx = rng.choice(Y.size, 300, replace=False)
    Y.flat[idx] = rng.integers(256, 900, size=idx.size)
    case["Y"] = Y
    assert (Y > 255).sum() >= 300
    if bits == 4:
        _on_off(case, _drive_default, variant_on=("series", "y4"), bits=4)
    else:
        _on_off(case, _drive_default, variant_off=("y4",), bits=8)


def test_forced_series_at_a_small_shape():
    """CA_VARX_SERIES far below the automatic pick: a stream of a few blocks behind a moment role of a few."""
    _on_off(make_case(seed=45, N=260, G=97, C=3, K=1), _drive_default)


def test_two_ranks_on_one_device_over_the_host_reduction():
    """Cell-sharded: the moment role takes max |psi| of ALL ranks (the slots the fit's collective carries) like the moments' own launches; replicas bit-identical."""
    case = make_case(seed=31, N=2400, G=640, C=5, K=1)
    _on_off(case, _drive_default, group=dict(devices=[0, 0], transport="host"))


def test_iterate_in_several_calls_and_in_one():
    """ca_iterate carries the forward half of the next train pass from call to call: split or whole, riding or not, the same bits."""
    case = make_case(seed=46, N=1000, G=333, C=4, K=1)
    eps = np.stack([eps_for(1, 333, 300 + i) for i in range(9)])

    def several(eng, G):
        eng.gamma_init(eps_for(1, G, 0))
        return [np.asarray([eng.iterate(2, eps[:5]), eng.iterate(2, eps[4:9])])]

    def one(eng, G):
        eng.gamma_init(eps_for(1, G, 0))
        return [np.asarray([eng.iterate(4, eps)])]

    _on_off(case, several)
    _on_off(case, one)
