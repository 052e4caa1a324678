"""The series form's cell launch gathering its backward moments by fp64 MFMA per wave (CA_VAR_CELL_MFMA, clonealign_amd/csrc/ca_poly.hip
k_poly_cell<CP, LEAN, true>): each wave multiplies the powers of its own cells by coef x exp(x v_b) on the matrix cores, keeps the tiles over the block's
passes, and the four waves' tiles are added in wave order at the block's end.  tests/test_gpu_series_grad.py holds the default (switch on) to float64 for every
bin count, clone count and pass pattern; here:

* states with a SMALL max|psi| and a WIDE range of loadings, against float64 by the same probe: the rows k = 16 .. 21 of the gather (its second row tile) only
  matter there (see WIDE below);
* the thread-owned chain (switch off) stays under the same float64 check, with the same tolerances;
* the lean and the plain passes feed the gather the same operands in the same order: bit-equal states and gradients with the switch on;
* the sums have one order, whatever the waves' timing: two fresh engines agree to the bit."""
import numpy as np
import pytest

from tests import _series_ref as sr
from tests._cases import eps_for
from tests.test_gpu_series_grad import TAIL_VARS, TRAIN_VARS, _check, _n_cu, _probe

pytestmark = pytest.mark.gpu

# The moment Q_k enters a gene's gradient as dv^k / k! Q_k, dv = v_g - v_b.  The bin geometry bounds max|psi| dv by CA_PL_A = 2, not dv: with nb = ceil(max|psi| width / 4)
# bins, dv reaches width / (2 nb).  Every state of tests/_series_ref.SPECS has max|psi| >= 1, hence dv <= 2, and there a WRONG Q_16 (the second row tile of the MFMA
# gather reading the rows of the first, say: Q_0 in its place) shifts an element by at most 2^16 / 16! = 3e-9 of its scale, far below TOL.  The states below have
# dv = 4 (one bin) and dv = 3.67 / 3.75 (three and four bins): the same mistake is 4^16 / 16! = 2e-4, 3.7^16 / 16! = 6e-5 of scale, a hundred times TOL -- while the
# series itself is as exact as anywhere, its argument max|psi| dv staying within CA_PL_A.  Small max|psi| beside wide loadings is what a fit looks like early on (the
# benchmark's state: max|psi| 0.48, W over a range of 4).  Same fields as _series_ref.SPECS; the states are built by _series_ref.build_state from these entries.
WIDE = {
    "wide_one_bin_c3":    dict(N=77, G=33, C=3, xmax=0.25, w=(-4.0, 4.0), grid=None, nb=1),       # CP = 4, one bin, dv = 4
    "wide_one_bin_c8":    dict(N=130, G=64, C=8, xmax=0.25, w=(-4.0, 4.0), grid=None, nb=1),      # CP = 8, the first column tile alone, more than one wave's cells
    "wide_three_bins_c4": dict(N=130, G=97, C=4, xmax=0.5, w=(-11.0, 11.0), grid=None, nb=3),     # CP = 4: three of the one tile's four bins, dv = 3.67
    "wide_four_bins_c8":  dict(N=300, G=130, C=8, xmax=0.5, w=(-15.0, 15.0), grid=None, nb=4),    # CP = 8: the second column tile full, dv = 3.75
}


@pytest.mark.parametrize("name", list(WIDE))
def test_small_psi_and_wide_loadings_match_float64(name, monkeypatch):
    """The default form where the high moments weigh in: every gradient against float64 per element, the probe and the tolerances of tests/test_gpu_series_grad.py."""
    monkeypatch.setitem(sr.SPECS, name, WIDE[name])
    fig = _probe(name)
    assert len(fig) == 2 * (len(TRAIN_VARS) + len(TAIL_VARS) + 2), sorted(fig)
    _check(name, fig)


@pytest.mark.parametrize("name", ["one_bin", "two_bins", "four_bins", "five_bins", "two_pass_c8", "two_pass_c4"])
def test_the_thread_owned_chain_matches_float64_too(name, monkeypatch):
    """Switch off: k_poly_cell<CP, true, false>, the launch as it was, against float64 with the tolerances of the default form."""
    from clonealign_amd.engine import HipEngine
    seen = []
    real = HipEngine.info

    def info(self):
        i = real(self)
        seen.append((i["fwd_series"], i["cell_mfma"]))
        return i

    _n_cu()                                      # (its little engine runs now and is cached: from here on only the probed engine answers)
    monkeypatch.setattr(HipEngine, "info", info)
    fig = _probe(name, variant_off=("cell_mfma",))
    assert seen and all(x == (1, 0) for x in seen), seen          # the probed engine: the series form, ca_info.cell_mfma == 0
    assert len(fig) == 2 * (len(TRAIN_VARS) + len(TAIL_VARS) + 2), sorted(fig)
    _check(name + "/cell_mfma_off", fig)


def _fit(name, n_iter, variant_off=()):
    """A fresh engine on the case's state: ELBO of iterate(n_iter), state, stored gradients."""
    from clonealign_amd.engine import HipEngine
    spec = sr.SPECS[name]
    case, S0 = sr.build_state(name, _n_cu() if spec["N"] is None else None)
    G = case["Y"].shape[1]
    eps = np.stack([eps_for(1, G, 900 + i) for i in range(2 * n_iter)])
    eng = HipEngine(**case, variant_on=("series",), variant_off=variant_off)
    try:
        info = eng.info()
        assert info["fwd_series"] == 1 and info["cell_mfma"] == 1 and info["cell_lean"] == int("cell_lean" not in variant_off), info
        for n in sr.VAR_NAMES:
            eng.set(n, S0[n])
        i0 = eng.info()
        e = eng.iterate(n_iter, eps)
        i1 = eng.info()
        assert i1["series_passes"] > i0["series_passes"] and i1["series_fallbacks"] == i0["series_fallbacks"], (i0, i1)   # every pass in the series form
        return e, eng.get_state(), eng.last_gradients()
    finally:
        eng.close()


def _same_bits(a, b):
    assert set(a) == set(b)
    for n in a:
        assert np.asarray(a[n]).shape == np.asarray(b[n]).shape and np.array_equal(a[n], b[n], equal_nan=True), n


@pytest.mark.parametrize("name", ["two_pass_c8", "five_bins", "two_pass_c4"])
def test_lean_and_plain_passes_feed_the_gather_the_same_bits(name):
    """two_pass_c8: three bins, the second column tile half filled; five_bins: a bin past the register bins, the chain between its barriers beside the
    tiles; two_pass_c4: the four-lane column map (four bins in one tile, four steps per pass)."""
    ea, sa, ga = _fit(name, 2)
    eb, sb, gb = _fit(name, 2, variant_off=("cell_lean",))
    assert ea == eb, (ea, eb)
    _same_bits(sa, sb)
    _same_bits(ga, gb)


def test_two_fresh_engines_agree_to_the_bit():
    ea, sa, ga = _fit("two_pass_c8", 3)
    eb, sb, gb = _fit("two_pass_c8", 3)
    assert ea == eb, (ea, eb)
    _same_bits(sa, sb)
    _same_bits(ga, gb)
