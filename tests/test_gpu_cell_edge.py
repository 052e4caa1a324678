"""The series form's cell launch with what stands around its passes taken off their critical path (CA_VAR_CELL_EDGE, clonealign_amd/csrc/ca_poly.hip
k_poly_cell<CP, true, true, true>): every load of a block's head issued before the first wait (the first prefetch, the header, the tables of all CA_PL_NBL bins
whatever the bin count, alpha -- log softmax(alpha) as a copy per wave through the DPP network), the block end as one parking step (the waves' sums and tiles left
in LDS at once, the finishing adds shared between two waves), and the q(z) half of the epilogue beside bin 0 instead of behind the bins' loop.  No sum gets a new
operand or a new order, so a fit with the switch on and one with it off must agree to the last bit -- ELBO traces, every state array, and the passes each gave to
the series form and to the sweeps.  Bit equality with a twin that had the same bug would prove nothing: the last test holds the gradients the switched-on form
applies to float64, element by element."""
import numpy as np
import pytest

from tests import _series_ref as sr
from tests._cases import eps_for, make_case

pytestmark = pytest.mark.gpu


def _wide(case, sigma, seed=2):
    """Loadings spread so that max|psi| (max W - min W) needs several bins (the loadings of tests/test_gpu_cell_lean.py)."""
    G = case["Y"].shape[1]
    return np.random.default_rng(seed).normal(0, sigma, size=(G, 1)).astype(np.float32).astype(np.float64)


def _drive_default(eng, G, W=None, first_bins=None, final=False):
    from clonealign_amd.rng import EpsStream
    eps = np.stack([eps_for(1, G, 40 + i) for i in range(9)])
    out = []
    if W is not None:
        eng.gamma_init(eps_for(1, G, 0))
        eng.set("W", W)
    else:
        if first_bins is not None:      # the state the fresh fit's first pass runs at: W = 0, a range of zero width
            first_bins.append(sr.expected_bins(eng.get_state()))
        out.append(np.asarray(eng.run(EpsStream(7, 1, G), 5, 1e-12)))
    out.append(np.asarray([eng.iterate(4, eps)]))
    out.append(np.asarray(eng.run(EpsStream(9, 1, G), 3, 1e-12)))
    if final:                           # the second draw's block sums
        out.append(np.asarray(eng.final_elbo(EpsStream(11, 1, G), 4)))
    return out


def _fit(case, drive, off, variant_on, group):
    from clonealign_amd.engine import HipEngine, HipGroupEngine
    G = case["Y"].shape[1]
    eng = HipGroupEngine(**case, variant_on=variant_on, variant_off=tuple(off), **group) if group else HipEngine(**case, variant_on=variant_on, variant_off=tuple(off))
    try:
        i0 = eng.rank_info(0) if group else eng.info()
        assert i0["fwd_series"] == 1 and i0["cell_lean"] == 1 and i0["cell_mfma"] == 1, i0
        assert i0["cell_edge"] == (0 if off else 1), (off, i0["cell_edge"])
        traces = drive(eng, G)
        infos = [eng.rank_info(r) for r in range(len(group["devices"]))] if group else [eng.info()]
        return traces, eng.get_state(), infos      # (a group's get_state also checks that the ranks' replicas are bit-identical)
    finally:
        eng.close()


def _on_off(case, drive, variant_on=("series",), group=None):
    """The same fit with the switch on and with the launch as it was: bit-equal traces and states, equal pass counts; returns the switched-on engine's info."""
    (ta, sa, ia), (tb, sb, ib) = _fit(case, drive, (), variant_on, group), _fit(case, drive, ("cell_edge",), variant_on, group)
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


def test_blocks_without_a_pass_ragged_last_pass_zero_width_range_and_second_draw():
    """C = 8.  41 groups of 32 cells, the last one of 21: most cell blocks have no pass (the hoisted prefetch's guard, a block end with all-zero tiles).  A fresh
    fit: its first pass runs at W = 0, one bin of a zero-width range.  final_elbo after the fit: the second draw's block sums."""
    bins = []
    i = _on_off(make_case(seed=41, N=1301, G=700, C=8, K=1), lambda e, G: _drive_default(e, G, first_bins=bins, final=True))
    assert i["series_fallbacks"] == 0
    assert bins == [1, 1], bins


@pytest.mark.parametrize("N,G,C", [(515, 97, 3), (2600, 1300, 5)])
def test_padding_lanes(N, G, C):
    """C = 3: four lanes per cell, one of them padding; C = 5: eight lanes, three padding -- log softmax(alpha) and the q(z) half see -inf and 0.0 lanes."""
    i = _on_off(make_case(seed=45 + C, N=N, G=G, C=C, K=1), _drive_default)
    assert i["series_fallbacks"] == 0


@pytest.mark.parametrize("C", [8, 4])
def test_one_and_two_passes_per_block(C):
    """N = (cell blocks x cells per pass) + 5 groups + 7 cells: five blocks make two full passes, one a full and a partial one, the rest one -- 16 551 cells at
    C = 8 and 33 095 at C = 4 on 256 CUs.  The q(z) half must belong to the pass's own cells, the head's prefetch to the first pass alone."""
    from tests.test_gpu_series_grad import _n_cu
    cpb = 256 // C
    N = 2 * _n_cu() * cpb + 5 * cpb + 7
    i = _on_off(make_case(seed=48 + C, N=N, G=96, C=C, K=1), _drive_default)
    assert i["N"] == N and i["series_fallbacks"] == 0


@pytest.mark.parametrize("sigma,N,G,C", [(0.45, 900, 300, 5), (0.7, 900, 300, 6), (2.5, 600, 200, 4)])
def test_two_to_four_bins_then_a_dozen(sigma, N, G, C):
    """Two or three bins, three or four (tables staged past nb, the second column tile), about a dozen (bins past CA_PL_NBL read from memory, the slab path's
    barriers in front of the block end)."""
    case = make_case(seed=42, N=N, G=G, C=C, K=1)
    W = _wide(case, sigma)
    i = _on_off(case, lambda e, G_: _drive_default(e, G_, W))
    assert i["series_fallbacks"] == 0


def test_two_ranks_on_one_device_over_the_host_reduction():
    """Cell-sharded: a pass orders its launches differently around the cell launch (the rig of tests/test_gpu_gene_ride.py)."""
    case = make_case(seed=31, N=2400, G=640, C=5, K=1)
    _on_off(case, _drive_default, group=dict(devices=[0, 0], transport="host"))


@pytest.mark.parametrize("name", ["one_bin", "wide_three_bins_c4"])
def test_applied_gradients_match_float64_per_element(name, monkeypatch):
    """Independent of the switch's twin: the gradients the switched-on form applies against float64, the probe and the tolerances of
    tests/test_gpu_series_grad.py, at a state with a padding lane (C = 3, one bin) and at one with three bins whose high moments weigh in."""
    from clonealign_amd.engine import HipEngine
    from tests.test_gpu_cell_mfma import WIDE
    from tests.test_gpu_series_grad import TAIL_VARS, TRAIN_VARS, _check, _n_cu, _probe
    if name in WIDE:
        monkeypatch.setitem(sr.SPECS, name, WIDE[name])
    seen = []
    real = HipEngine.info

    def info(self):
        i = real(self)
        seen.append((i["fwd_series"], i["cell_edge"]))
        return i

    _n_cu()                                      # (its little engine runs now and is cached: from here on only the probed engine answers)
    monkeypatch.setattr(HipEngine, "info", info)
    fig = _probe(name)
    assert seen and all(x == (1, 1) for x in seen), seen          # the probed engine: the series form, ca_info.cell_edge == 1
    assert len(fig) == 2 * (len(TRAIN_VARS) + len(TAIL_VARS) + 2), sorted(fig)
    _check(name + "/cell_edge", fig)
