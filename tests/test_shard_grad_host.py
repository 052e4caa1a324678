"""CPU side of tests/test_gpu_shard_grad.py: the slicing, the preconditions of its states and the bars it borrows -- no GPU, no engine."""
import numpy as np
import pytest

from clonealign_amd.sharding import cell_range
from tests import _loop_ref as lr
from tests import _series_ref as sr
from tests import _shard_rig as rig
from tests import test_gpu_loop_grad as lg
from tests import test_gpu_series_grad as sg
from tests import test_gpu_shard_grad as shg


def _shapes_and_worlds():
    out = {(shg.spec(n)["shape"]["N"], w) for n, w in shg.SWEEP_CASES}
    out |= {(sr.SPECS[n]["N"], w) for n, w, _ in shg.SERIES_CASES}
    out |= {(shg.spec(shg.STEADY_CASE[0])["shape"]["N"], shg.STEADY_CASE[1]), (shg.spec(shg.RUN_SWEEP_CASE[0])["shape"]["N"], shg.RUN_SWEEP_CASE[1]),
            (sr.SPECS[shg.RUN_SERIES_CASE[0]]["N"], shg.RUN_SERIES_CASE[1]), (shg.GROUP_SHAPE["N"], 2)}
    return sorted(out)


def test_every_cell_is_in_exactly_one_rank_for_every_shape_used():
    pairs = _shapes_and_worlds()
    assert (333, 2) in pairs and (333, 3) in pairs and (40, 3) in pairs and (300, 3) in pairs
    for N, world in pairs:
        assert N is not None
        rs = rig.ranges(N, world)
        assert rs[0][0] == 0 and rs[-1][1] == N and all(a[1] == b[0] for a, b in zip(rs, rs[1:])), (N, world, rs)
        sizes = [hi - lo for lo, hi in rs]
        assert min(sizes) >= 1 and max(sizes) - min(sizes) <= 1, (N, world, sizes)
        count = np.zeros(N, dtype=np.int64)
        whole = {"psi": np.arange(N, dtype=np.float64).reshape(N, 1), "gamma_logits": np.arange(3 * N, dtype=np.float64).reshape(N, 3), "W": np.arange(7.0)}
        for lo, hi in rs:
            count[lo:hi] += 1
            assert np.array_equal(rig.shard_value("psi", whole["psi"], lo, hi)[:, 0], np.arange(lo, hi))
            assert rig.shard_value("gamma_logits", whole["gamma_logits"], lo, hi).shape == (hi - lo, 3)
            assert rig.shard_value("W", whole["W"], lo, hi) is whole["W"]          # replicated: whole on every rank
        assert np.array_equal(count, np.ones(N, dtype=np.int64)), (N, world)
        # the ranks' slices put back together are the whole array (what the GPU file assembles the stepped state with)
        assert np.array_equal(np.concatenate([rig.shard_value("gamma_logits", whole["gamma_logits"], lo, hi) for lo, hi in rs], 0), whole["gamma_logits"])
    assert [hi - lo for lo, hi in rig.ranges(40, 3)] == [13, 13, 14]                   # every shard smaller than one 16-cell block
    assert [hi - lo for lo, hi in rig.ranges(333, 2)] == [166, 167] and [hi - lo for lo, hi in rig.ranges(333, 3)] == [111, 111, 111]


def test_shard_case_slices_what_is_indexed_by_cell_and_nothing_else():
    case, _st = lr.build_state("generic", 5, N=50, G=20, C=3, K=2, P=1, extra=True)
    sh = rig.shard_case(case, 10, 25)
    for k in rig.SHARDED_INPUTS:
        assert sh[k].shape[0] == 15 and np.array_equal(sh[k], case[k][10:25]), k
    for k in case:
        if k not in rig.SHARDED_INPUTS:
            assert sh[k] is case[k], k
    assert set(rig.CELL_VARS) | set(shg.REPLICATED) == set(sr.VAR_NAMES)


EXTREMES = [c for c in shg.SERIES_CASES if c[2] in ("extremes_first", "extremes_last")]
assert len(EXTREMES) == 2


@pytest.mark.parametrize("name,world,where", EXTREMES, ids=[shg.series_id(*c) for c in EXTREMES])
def test_extreme_states_keep_the_whole_bin_count_and_leave_the_other_ranks_fewer(name, world, where):
    """What a rank-local maximum cannot pass: the whole state has the bin count it is named for, a rank WITHOUT the extremes would take fewer for its own cells."""
    consts = sr.poly_constants()
    case, st = shg.series_state(name, world, where)
    _case0, st0 = sr.build_state(name)
    N = case["Y"].shape[0]
    assert np.array_equal(st["psi"].astype(np.float32).astype(np.float64), st["psi"])            # still float32-exact
    assert sr.expected_bins(st, consts) == sr.expected_bins(st0, consts) == sr.SPECS[name]["nb"] > 1
    holder = 0 if where == "extremes_first" else world - 1
    for r in range(world):
        lo, hi = cell_range(N, r, world)
        own = sr.expected_bins({"psi": st["psi"][lo:hi], "W": st["W"]}, consts)
        if r == holder:
            assert own == sr.SPECS[name]["nb"], (r, own)
            assert np.abs(st["psi"][lo:hi]).max() == np.abs(st0["psi"]).max()
        else:
            assert own < sr.SPECS[name]["nb"], (r, own)
            assert np.array_equal(st["psi"][lo:hi], 0.25 * st0["psi"][lo:hi])
    for n in sr.VAR_NAMES:
        if n != "psi":
            assert np.array_equal(st[n], st0[n]), n


@pytest.mark.parametrize("name,world,where", shg.SERIES_CASES, ids=[shg.series_id(*c) for c in shg.SERIES_CASES])
def test_series_states_have_the_bin_count_they_are_named_for_and_a_covered_first_pass(name, world, where):
    xmax, vlo, vhi, sb = shg.series_preconditions(name, world, where)
    assert sb > 0 and sr.poly_covers(xmax, vlo, vhi, 0, sb)
    if name == "bins_32":        # the one state whose later passes the look ahead hands to the sweeps, on every rank alike
        assert not sr.poly_covers(xmax, vlo, vhi, 1, sb)
    elif where == "xadd_probe":
        # the pass one step on is still the series form's; its geometry is what xadd decides
        assert sr.poly_covers(xmax, vlo, vhi, 1, sb) and not sr.poly_covers(xmax, vlo, vhi, 2, sb)
        consts = sr.poly_constants()
        assert (xmax, vlo, vhi) == (2.0 ** -6, -72.0, 72.0)
        _v, d_stale, nb_stale = sr.bin_geometry(xmax, vlo, vhi, consts)                 # the slots one step back, no xadd
        _v, d_est, nb_est = sr.bin_geometry(xmax + sb, vlo, vhi, consts)                # ... plus one step's bound: what poly_xsrc hands over
        stepped = xmax + 0.1 * 0.99                                                      # Adam's first step is lr x g / (|g| + eps): 0.1 for every cell but a zero gradient's
        assert nb_stale == 1 and nb_est == 27 and stepped * d_est / 2 <= consts["CA_PL_A"]
        assert stepped * d_stale / 2 > 4 * consts["CA_PL_A"]                             # the stale geometry: |x dv| four times what the series is built for
    else:
        assert sr.poly_covers(xmax, vlo, vhi, 2, sb)


def test_every_sharded_case_has_its_bars_in_the_unsharded_files():
    for name, _w in shg.SWEEP_CASES + [shg.STEADY_CASE, shg.RUN_SWEEP_CASE]:
        fam = shg.family(name)
        assert fam in lg.MODEL, fam
        if name != shg.TINY:
            assert name in lg.CASES and lg.family(name) == fam
        for n in sr.VAR_NAMES:
            assert 0.0 <= lg.bar(fam, n) <= lg.HARD, (fam, n)
    assert shg.GROUP_FAMILY in lg.MODEL and "handover/bins_32" in lg.MODEL
    for n in sr.VAR_NAMES:
        if n != "beta":
            assert 0.0 < shg.series_bar(n) == sg.TOL[n] <= lg.HARD, n
    assert shg.series_bar("beta") == 0.0 and "elbo" in sg.TOL
    assert shg.series_bar("W", handed=True) == lg.bar("handover/bins_32", "W") and shg.series_bar("v", handed=True) == sg.TOL["v"]
    for name, _w, _where in shg.SERIES_CASES + [shg.RUN_SERIES_CASE]:
        assert name in sr.SPECS and sr.SPECS[name]["N"] is not None, name


def test_the_small_state_is_held_to_bars_its_own_operand_model_stays_under():
    """40 x 95 x 3 borrows cell16/generic's bars (same kernels, same G): the documented operand roundings at THAT state, from the reference alone, fit under them."""
    case, S0, eps, fc = shg.sweep_problem(shg.TINY)
    assert case["Y"].shape == (40, 95) and case["L"].shape[1] == 3
    ref, sc = lr.ref_gradients(fc, S0, eps[0])
    mod = lr.operand_model(fc, S0, eps[0], shg.TINY_SPEC["model"])
    for n in sr.VAR_NAMES:
        r = sr.worst_ratio(mod[n], ref[n], sc[n])
        assert r <= lg.bar(shg.family(shg.TINY), n), (n, r, lg.bar(shg.family(shg.TINY), n))


def test_logit_ratio_takes_off_the_float32_floor_and_nothing_else():
    """A state out of gamma init holds posteriors below float32's range (the ``set`` states hold none): there an engine that stores d logits = 0 is right, and
    ``worst_ratio`` alone would put it at per cent of the element's own scale.  ``logit_ratio`` lets exactly that through; an error of 1e-6 of scale still shows."""
    from oracle.fused_numpy import FusedModel
    from scipy.special import logsumexp
    from tests._cases import eps_for
    case = shg._group_case()
    G = case["Y"].shape[1]
    m = FusedModel(**case, dtype="float64")
    m.gamma_init(eps_for(1, G, 0))
    st = {n: np.asarray(getattr(m, n), dtype=np.float64).astype(np.float32).astype(np.float64) for n in sr.VAR_NAMES}
    gamma = np.exp(st["gamma_logits"] - logsumexp(st["gamma_logits"], 1, keepdims=True))
    assert (gamma < shg.F32_MIN).sum() > 50
    ref, sc = lr.ref_gradients(lr.fit_constants(case), st, eps_for(1, G, 1))
    flushed = np.where(gamma < shg.F32_MIN, 0.0, ref["gamma_logits"])
    assert sr.worst_ratio(flushed, ref["gamma_logits"], sc["gamma_logits"]) > 1e-4
    assert shg.logit_ratio(flushed, ref["gamma_logits"], sc["gamma_logits"], st["gamma_logits"]) == 0.0
    wrong = ref["gamma_logits"] + 1e-6 * sc["gamma_logits"]
    r = shg.logit_ratio(wrong, ref["gamma_logits"], sc["gamma_logits"], st["gamma_logits"])
    assert 0.99e-6 <= r <= 1.01e-6, r
    for name, _w in shg.SWEEP_CASES:          # the set states: nothing below the floor, logit_ratio is worst_ratio to 1e-30
        _case, S0, _eps, _fc = shg.sweep_problem(name)
        g0 = np.exp(S0["gamma_logits"] - logsumexp(S0["gamma_logits"], 1, keepdims=True))
        assert g0.min() > shg.F32_MIN * 2.0 ** 20, name


def test_a_step_of_the_series_run_case_cannot_move_a_nonzero_float32():
    """learning_rate = 2^-100 (the series form needs a step bound, none exists at 0): Adam's step is at most the bound, far below half an ulp of any float32 the
    states hold but an exact zero."""
    b = sr.poly_step_bound(lr=shg.RUN_SERIES_LR)
    assert 0.0 < 2 * b < 2.0 ** -90
    _case, S0, _eps, _fc = shg.series_problem(*shg.RUN_SERIES_CASE)
    for n in sr.VAR_NAMES:
        a = np.abs(S0[n][S0[n] != 0.0])
        assert a.size == 0 or a.min() * 2.0 ** -25 > 2 * b, n
