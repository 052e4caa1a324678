"""The series form's cell launch with its passes taken off the memory round trips (CA_VAR_CELL_LEAN, clonealign_amd/csrc/ca_poly.hip k_poly_cell<CP, true>): no
read of the zero exponent bound, the cell's constant c_n prefetched a pass ahead with the other epilogue operands, psi of the prior term taken from the register
that already holds it, the 4- and 8-lane reductions through the DPP network instead of the LDS crossbar, the powers x^k without a branch per step.  No sum gets a
new operand or a new order, so a fit with the switch on and one with it off must agree to the last bit -- ELBO traces, every state array, and the passes each
gave to the series form and to the sweeps."""
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


def _on_off(case, drive, variant_on=("series",), variant_off=()):
    """The same fit with the lean cell passes and with the launch as it was: bit-equal traces and states, equal pass counts; returns the lean engine's info."""
    from clonealign_amd.engine import HipEngine
    G = case["Y"].shape[1]
    res = []
    for off in ((), ("cell_lean",)):
        eng = HipEngine(**case, variant_on=variant_on, variant_off=tuple(variant_off) + off)
        try:
            i0 = eng.info()
            assert i0["fwd_series"] == 1, i0
            assert i0["cell_lean"] == (0 if off else 1), (off, i0["cell_lean"])
            traces = drive(eng, G)
            res.append((traces, eng.get_state(), eng.info()))
        finally:
            eng.close()
    (ta, sa, ia), (tb, sb, ib) = res
    assert len(ta) == len(tb)
    for x, y in zip(ta, tb):
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (x, y)
    assert set(sa) == set(sb)
    for n in sb:
        assert np.array_equal(sa[n], sb[n], equal_nan=True), n
    assert (ia["series_passes"], ia["series_fallbacks"]) == (ib["series_passes"], ib["series_fallbacks"]), (ia, ib)
    assert ia["series_passes"] > 0
    return ia


def test_eight_lanes_partial_last_group_and_blocks_without_a_pass():
    """C = 8: eight lanes per cell, all of them live.  41 groups of 32 cells, the last one of 21: most of the cell blocks have no pass at all (the prefetch's guard)."""
    i = _on_off(make_case(seed=41, N=1301, G=700, C=8, K=1), _drive_default)
    assert i["series_fallbacks"] == 0


def test_four_lanes_with_one_padding_lane():
    """C = 3: four lanes per cell (xor 2 and 1 only), one of them padding that enters the maxima as -inf and the sums as 0."""
    i = _on_off(make_case(seed=45, N=515, G=97, C=3, K=1), _drive_default)
    assert i["series_fallbacks"] == 0


def test_eight_lanes_with_three_padding_lanes():
    """C = 5: eight lanes per cell, three padding lanes in every reduction."""
    i = _on_off(make_case(seed=47, N=2600, G=1300, C=5, K=1), _drive_default)
    assert i["series_fallbacks"] == 0


@pytest.mark.parametrize("C", [8, 4])
def test_two_passes_in_some_blocks_and_one_in_others(C):
    """The carried prefetch: N = (cell blocks x cells per pass) + 5 groups + 7 cells, so that five blocks make two full passes, one a full and a partial one and the
    rest one -- 16 551 cells at C = 8 and 33 095 at C = 4 on 256 CUs (two cell blocks per CU, as the engine picks them)."""
    from clonealign_amd.engine import HipEngine
    probe = HipEngine(**make_case(seed=1, N=64, G=32, C=3, K=1))
    try:
        n_cu = probe.info()["n_cu"]
    finally:
        probe.close()
    cpb = 256 // C                     # cells per pass: 256 threads, C (a power of two here) lanes per cell
    N = 2 * n_cu * cpb + 5 * cpb + 7
    i = _on_off(make_case(seed=48 + C, N=N, G=96, C=C, K=1), _drive_default)
    assert i["N"] == N and i["series_fallbacks"] == 0


def test_two_or_three_bins():
    """The multi-bin gather of the backward moments."""
    case = make_case(seed=42, N=900, G=300, C=5, K=1)
    W = _wide(case, 0.45)      # max|psi| ~ 3.3, W range ~ 2.5: product ~ 8 -> two or three bins
    i = _on_off(case, lambda e, G: _drive_default(e, G, W))
    assert i["series_fallbacks"] == 0


def test_three_or_four_bins():
    case = make_case(seed=43, N=900, G=300, C=6, K=1)
    W = _wide(case, 0.7)       # max|psi| ~ 3.3, W range ~ 4: product ~ 13 -> three or four bins
    i = _on_off(case, lambda e, G: _drive_default(e, G, W))
    assert i["series_fallbacks"] == 0


def test_wide_exponent_range_takes_the_slab_path():
    """Thirteen or so bins: past the four a thread keeps in registers (NBR) and the four whose tables sit in LDS (CA_PL_NBL) -- those paths keep their loads."""
    case = make_case(seed=33, N=600, G=200, C=4, K=1)
    W = _wide(case, 2.5)       # max|psi| ~ 3.2, W range ~ 14: product ~ 45 -> a dozen bins
    i = _on_off(case, lambda e, G: _drive_default(e, G, W))
    assert i["series_fallbacks"] == 0
