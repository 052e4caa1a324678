"""The series form's way back as ONE launch (CA_VAR_GENE_RIDE, clonealign_amd/csrc/ca_polygene.hip.h): the reduction of the backward moments, the per-gene pass, the
pending monitor pass's tail and the count-matrix stream's column sums as blocks of k_poly_tail, the moment table handed from the reducer blocks to the gene blocks
through tagged words; with the switch off, k_poly_red and k_poly_gene as launches of their own and the column jobs behind the cell launch's cell blocks.  A
cell-sharded fit keeps the two launches either way (its collective sits between them) and carries the column jobs on the reduction launch.  Scheduling only: every
order calls the same bodies, every sum keeps its operands and its order, so a fit with the switch on and one with it off must agree to the last bit -- ELBO traces,
every state array, and the passes each gave to the series form and to the sweeps.
(The gene blocks' bounded wait has no test that provokes it; its error path -- sticky word, block leaves, comm_check reports CA_ERR_STATE -- is read in the code.)"""
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


def _fit(case, drive, off, variant_on=("series", "y4"), group=None, probe=None, tune=None):
    """One fit with `off` switched off: (traces, state, infos).  `tune`: the lab knob that keeps (series_side = 7) or moves (8) the column jobs whatever the
    engine's size rule says -- at these sizes the rule moves them."""
    from clonealign_amd.engine import HipEngine, HipGroupEngine
    G = case["Y"].shape[1]
    if group:
        eng = HipGroupEngine(**case, variant_on=variant_on, variant_off=tuple(off), tune=tune, **group)
    else:
        eng = HipEngine(**case, variant_on=variant_on, variant_off=tuple(off), tune=tune)
    try:
        i0 = eng.rank_info(0) if group else eng.info()
        assert i0["fwd_series"] == 1, i0
        assert i0["gene_ride"] == (0 if (off or group) else 1), (off, i0["gene_ride"])   # (a cell-sharded fit keeps the two launches: 0 either way)
        traces = drive(eng, G)
        if probe is not None:
            probe(eng)
        infos = [eng.rank_info(r) for r in range(len(group["devices"]))] if group else [eng.info()]
        return traces, eng.get_state(), infos      # (a group's get_state also checks that the ranks' replicas are bit-identical)
    finally:
        eng.close()


def _same(a, b):
    (ta, sa, ia), (tb, sb, ib) = a, b
    assert len(ta) == len(tb)
    for x, y in zip(ta, tb):
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (x, y)
    assert set(sa) == set(sb)
    for n in sb:
        assert np.array_equal(sa[n], sb[n], equal_nan=True), n
    for x, y in zip(ia, ib):
        assert (x["series_passes"], x["series_fallbacks"]) == (y["series_passes"], y["series_fallbacks"]), (x, y)
        assert x["series_passes"] > 0


def _on_off(case, drive, variant_on=("series", "y4"), group=None, probe=None, tune=None):
    """The same fit with the merged way back and with the launches of their own: bit-equal traces and states, equal pass counts; returns the merged engine's info."""
    on = _fit(case, drive, (), variant_on, group, probe, tune)
    off = _fit(case, drive, ("gene_ride",), variant_on, group)
    _same(on, off)
    return on[2][0]


def test_one_bin():
    """A fresh fit: W starts at zero and stays small -- one bin.  G is a multiple of neither 256 nor 64: the last gene block and the last column wave are partial;
    six slab rows: the column jobs' form for few rows."""
    i = _on_off(make_case(seed=41, N=1301, G=700, C=8, K=1), _drive_default)
    assert i["series_fallbacks"] == 0 and i["y_stream_bits"] == 4


def test_two_or_three_bins():
    """Five clones in eight lanes (CP = 8, C < CP); two or three bins of 22 x 5 outputs: more than one reducer block's worth per bin count."""
    case = make_case(seed=42, N=900, G=300, C=5, K=1)
    W = _wide(case, 0.45)      # max|psi| ~ 3.3, W range ~ 2.5: product ~ 8 -> two or three bins
    i = _on_off(case, lambda e, G: _drive_default(e, G, W))
    assert i["series_fallbacks"] == 0


def test_wide_exponent_range_reads_the_table_from_memory():
    """Thirteen or so bins: past the four whose tables sit in LDS (NBL) -- the gene blocks read tabQ from global memory behind the hand-over; CP = 4."""
    case = make_case(seed=33, N=600, G=200, C=4, K=1)
    W = _wide(case, 2.5)       # max|psi| ~ 3.2, W range ~ 14: product ~ 45 -> a dozen bins
    i = _on_off(case, lambda e, G: _drive_default(e, G, W))
    assert i["series_fallbacks"] == 0


def test_sixty_four_slab_rows_and_more():
    """The column jobs' main form: 65 row groups of the stream -- one whole trip of four rows per row lane and a ragged tail.
    (The slab-row count is probed on the fit with the switch on only: it is a property of the shape, the same for both.)"""
    case = make_case(seed=47, N=64 * 256 + 16, G=576, C=4, K=1)
    eps = np.stack([eps_for(1, 576, 500 + i) for i in range(5)])
    rows = []

    def drive(eng, G):
        eng.gamma_init(eps_for(1, G, 0))
        return [np.asarray([eng.iterate(2, eps)])]

    _on_off(case, drive, probe=lambda eng: rows.append(eng.ystream_parts()["yt_part"].shape[0]))
    assert rows and rows[0] >= 64 and rows[0] % 64 != 0, rows


def test_a_pass_handed_to_the_sweeps_and_back():
    """W blown up by hand: the guard gives those passes to the sweeps -- no merged launch is queued, the column sums come with the sweeps' own finisher --; W back:
    the series form and its merged way back take over again.  (variant_on = ("series",) as in the case of tests/test_gpu_mom_ride.py this one mirrors: the handed-over
    passes ride the stream on the sweeps, which the forced 4-bit image is not this test's business to constrain; the engine picks the image.)"""
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

    _on_off(case, drive, variant_on=("series",))
    for p0, p1, p2 in seen:
        assert p0["series_fallbacks"] == 0 and p0["series_passes"] >= 4, p0
        assert p1["series_fallbacks"] > 0, p1
        assert p2["series_passes"] > p1["series_passes"], (p1, p2)


def test_columns_left_behind_the_cell_blocks():
    """What the engine's size rule picks from 65 537 cells up (the headline shape): the merged launch without column jobs, the column jobs behind the cell launch's
    blocks as with the switch off -- here forced at a small size by the lab knob; and the knob that forces the move gives the same bits too."""
    case = make_case(seed=41, N=1301, G=700, C=8, K=1)
    kept = _fit(case, _drive_default, (), tune={"series_side": 7})
    moved = _fit(case, _drive_default, (), tune={"series_side": 8})
    off = _fit(case, _drive_default, ("gene_ride",))
    _same(kept, off)
    _same(moved, off)


def test_the_same_fit_three_times():
    """The hand-over's timing decides nothing: three fits with the switch on, the same bits every time."""
    case = make_case(seed=42, N=900, G=300, C=5, K=1)
    W = _wide(case, 0.45)
    runs = [_fit(case, lambda e, G: _drive_default(e, G, W), ()) for _ in range(3)]
    _same(runs[0], runs[1])
    _same(runs[0], runs[2])


def test_two_ranks_on_one_device_over_the_host_reduction():
    """Cell-sharded: reduction and per-gene pass stay two launches (gene_ride reports 0), the column jobs ride on k_poly_red; bit-equal to the switch off.
    (variant_on = ("series",), devices and transport as in the group case of tests/test_gpu_mom_ride.py, which this one mirrors.)"""
    case = make_case(seed=31, N=2400, G=640, C=5, K=1)
    _on_off(case, _drive_default, variant_on=("series",), group=dict(devices=[0, 0], transport="host"))
