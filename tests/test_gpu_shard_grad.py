"""The gradients every rank of a CELL-SHARDED fit applies, against float64, element by element, on one GPU: what tests/test_gpu_loop_grad.py (sweeps) and
tests/test_gpu_series_grad.py (series form) hold for one handle, for W handles (``rank = r, world = W``) on W host threads joined by the host all-reduce hook
(tests/_shard_rig.py), and for the device group (``HipGroupEngine``: host reduction, and the peer-to-peer all-reduce with the backward sweep's column sums
folded into its launch).

REFERENCE: the WHOLE, unsharded problem through tests/_loop_ref.py (sweeps) and tests/_series_ref.py (series form), per-element scales as they are.  psi and
gamma_logits are compared on the rank's cells [lo, hi); loc, ls, W, beta, v, alpha_unconstr whole on EVERY rank, and those must be bit-identical across the
ranks.  The call's ELBO is compared on every rank and must be equal across the ranks.

PROTOCOL (the two unsharded files'): every rank ``set``s all eight variables to S0 (psi and gamma_logits as its slice); ``iterate(1, eps[0:2])``;
``last_gradients()`` and ``get_state()`` (= S1, assembled from the ranks' slices; the replicated variables are asserted equal on all ranks); compare; a second
``iterate(1, eps[2:4])`` from S1 and the same again.  Every rank makes the same sequence of calls; workers only collect arrays, every assert runs on the main
thread after the join.

MAPPING for a sharded handle, from ca_iterate / train_pass / train_bwd / fused_pass (clonealign_hip.hip, ca_eng_loop.inc), ``iterate(1, [e0, e1])``:
* ``bwd_mfma = 1`` and ``fused_sweep = 1`` (S = 1 up to 16 clones, mc_samples = 2, the series form): the unsharded sequence -- ``fused_pass(0, 0)`` at S0
  (C16 / S2: made by ``train_pass``, whose forward half asks for ``bwd_mfma`` when sharded), ``train_from_lookahead(0)``, the monitor pass ``fused_pass(1, 1)``
  at S1, ``flush_mon_tail``:
    loc, ls, W, beta, psi at (S0, e0);  gamma_logits at (S1, e1);  v, alpha_unconstr at S1;  the ELBO at (S1, e1).
  What differs is where the sums become global: the pending monitor pass's LOCAL cell sums travel in the next train pass's collective (``merged``), the last
  one's in ``flush_mon_tail``'s (3 + C)-double collective; alpha_unconstr is made of red[3 + c] = the sum of gamma over ALL ranks' cells.
* ``bwd_mfma = 0`` and ``fused_sweep = 1`` (the vector unit's way back, K = 0): ``can_carry`` is off and ca_iterate makes NO first ``fused_pass(0, 0)``;
  ``train_pass`` is the plain ``run_pass(0, TRAIN)`` (k_cell_par stores d logits at (S0, e0)), the monitor pass is still ``fused_pass(1, 1)`` at S1, whose cell
  epilogue rewrites d logits: the buffers end where the fused loop's do --
    loc, ls, W, beta, psi at (S0, e0);  gamma_logits at (S1, e1);  v, alpha_unconstr at S1.
  (include/clonealign_hip.h did not say that a sharded handle's train pass is a plain pass here; added there.)
* plain passes (``fused_sweep = 0``): as unsharded, one collective per pass -- gamma_logits at (S0, e0), the train pass's.
STEADY STATE: ``iterate(2, four draws)`` at learning_rate = 0: ``fused_pass(1, 2)`` carries the first monitor pass and the second train pass's draw through a
pending, merged tail: loc, ls, W, beta, psi at (S0, e2), gamma_logits at (S0, e3), v and alpha at S0, the ELBO at (S0, e3); the state comes back bit for bit.
``ca_run`` (run_loop, clonealign_hip.hip), ``run(six draws, max_iter = 2, rel_tol = 0)``: gamma init with e0 (the logits change: S' is the state read back after
the call, every other variable as set); ``monitor_pass(1, 2)`` -> trace[0] at (S', e1), flushed (``cell_sums_global``: the next train pass's collective skips
the 3 + C cell sums); train pass e2; ``monitor_pass(3, 4)`` -> trace[1] at (S', e3); train pass e4; the last monitor pass has no next train pass and is the
plain ``run_pass(5, ELBO)`` -> trace[2] at (S', e5); k_cell_par stores no d logits in that mode.  So after the call:
    loc, ls, W, beta, psi at (S', e4);  gamma_logits at (S', e4) (the look-ahead half of ``fused_pass(3, 4)``);  v, alpha_unconstr at S'.
A STOPPED ``run`` (``run(eight draws, 3, rel_tol = 1e30)`` ends after iteration 1) leaves the next train pass's backward half queued ahead with no update behind
it: its collective has made Y^T psi global (``ycache_valid`` cleared), a gated update is cancelled.  ``iterate(1, [e8, e9])`` afterwards: the two-draw mapping at S'.
Sweeps: learning_rate = 0 (the state is asserted unchanged but for the logits).  The series form does not exist at learning_rate = 0 (its look ahead rests on
ca_adam_step_bound, which has no bound to give there: ``fwd_series = 0``), so its ``run`` case takes learning_rate = 2^-100: a step of at most 8e-31 leaves every
non-zero float32 as it is and moves an exact 0 (psi[0]) by that much -- asserted: no variable but the logits moves by more than 2^-90.

SERIES FORM, sharded.  The look ahead decides as it does unsharded (the ranges it waits for are those of the first pass after the ``set``, published from the
GLOBAL max |psi|; the steps are Adam steps since): the (series, fallback) counts per call are ``poly_covers`` at steps (0, 1) and (1, 2), asserted per rank and
equal on all ranks.  What differs is the geometry: the first pass after a ``set`` refreshes the slots by a collective of their own (xadd = 0), every later pass
takes the slots one Adam step back plus ``xadd = steps x poly_step_bound`` -- never the exact-range geometry; in float64 that is worth <= 3e-14
(tests/test_series_ref_host.py).  The two "extremes" states hold max |psi| in ONE rank's cells: the whole state keeps its bin count, the other ranks' own
slices would take fewer bins (asserted on the CPU, tests/test_shard_grad_host.py): a rank that used its own maximum would bin differently from its peers and
the summed backward moments Q would mix geometries.  The "xadd_probe" state is the one a stale ``xadd`` cannot pass: max |psi| = 2^-6, so small that one Adam step
(0.1 per cell) multiplies it by seven, against loadings +-72 -- the slots one step back say one bin where the stepped state needs five.

BARS: the unsharded files' own objects -- ``bar(family, variable)`` and ``HARD`` of tests/test_gpu_loop_grad.py, ``TOL`` of tests/test_gpu_series_grad.py
(a series engine's train pass handed to the sweeps: ``bar("handover/bins_32", .)``).  Sharding changes the order of float64 sums and the series form's geometry,
no operand rounding.  ONE CORRECTION of the metric, for gamma_logits alone (``logit_ratio``): a state that came out of gamma init (``run``, the group) holds
posteriors below float32's range, where the engine's exact 0 is right and the element's own scale is as small as the element; the float32 floor
(2^-126 times the element's |f| + .., 2e-34 here) is taken off the difference before the ratio.  The ``set`` states hold no such element
(tests/test_shard_grad_host.py).  The 40 x 95 x 3 state has no case of its own there: it runs the cell16 kernels (asserted through ``info()``) at the same G and is held to
``cell16/generic``; tests/test_shard_grad_host.py checks on the CPU that its operand model stays under those bars.  The group's cases start from no ``set``
state: three Adam steps from psi0 x 3 on the 333 x 95 x 8 problem, held to ``cell16/generic`` and ``TOL``.
profiles/r17_shard_grad.txt holds the printed figures of one full run.
"""
import functools

import numpy as np
import pytest

from clonealign_amd.sharding import cell_range
from tests import _loop_ref as lr
from tests import _series_ref as sr
from tests import _shard_rig as rig
from tests import test_gpu_loop_grad as lg
from tests import test_gpu_series_grad as sg
from tests._cases import eps_for

pytestmark = pytest.mark.gpu

TRAIN_VARS = lg.TRAIN_VARS                      # loc, ls, W, beta, psi
TAIL_VARS = lg.TAIL_VARS                        # v, alpha_unconstr
REPLICATED = tuple(n for n in sr.VAR_NAMES if n not in rig.CELL_VARS)

# ------------------------------------------------------------------------------------------------------------------ the cases
TINY = "tiny-generic"                           # 40 x 95 x 3 over three ranks: 13, 13 and 14 cells, every shard smaller than one 16-cell block
TINY_SPEC = dict(group="cell16", kind="generic", shape=dict(N=40, G=95, C=3, K=1), model=lg.MC, opts={}, seed=5,
                 expect=dict(lg.FUSED_MC, **lg.U8_RIDE, fwd_block_cells=16, fwd_blocks_big=0, fwd_balanced=0))
SWEEP_CASES = ([(n, w) for n in ("cell16-generic", "cell16-wide", "cell16-peaked") for w in (2, 3)]
               + [(n, 2) for n in ("cell16-exact", "d2-k1p1-generic", "c16-c16-generic", "s2-fuse-generic", "plain-s3-generic", "plain-c18-generic",
                                   "valu_bwd-generic", "valu-k0-generic", "frac_c11-generic", "storage-u16-generic", "storage-u8_overflow-generic")]
               + [(TINY, 3)])
# name of the state (tests/_series_ref.py), world, where max |psi| lives (None: as built)
SERIES_CASES = [("one_bin", 2, None), ("five_bins", 2, None), ("nine_bins", 2, None), ("five_bins", 3, None), ("bins_32", 2, None), ("equal_0_x8", 2, None),
                ("five_bins", 2, "extremes_first"), ("five_bins", 3, "extremes_last"), ("five_bins", 2, "xadd_probe")]
NB_OF = {"xadd_probe": 1}                       # the bin count of a variant that is not its state's
STEADY_CASE, RUN_SWEEP_CASE, RUN_SERIES_CASE = ("cell16-generic", 2), ("cell16-generic", 2), ("one_bin", 2, None)
RUN_SERIES_LR = 2.0 ** -100
GROUP_SHAPE = dict(lg.R8)                       # 333 x 95 x 8, K = 1
GROUP_FAMILY = "cell16/generic"


def spec(name):
    return TINY_SPEC if name == TINY else lg.CASES[name]


def family(name):
    s = spec(name)
    return f"{s['group']}/{s['kind']}"


@functools.lru_cache(maxsize=None)
def sweep_problem(name):
    """(constructor arguments of the whole problem, S0, eps [4, S, G], fit constants): made once, shared, left unchanged."""
    if name == TINY:
        case, st = lr.build_state(TINY_SPEC["kind"], TINY_SPEC["seed"], **TINY_SPEC["shape"])
        eps = np.stack([eps_for(1, TINY_SPEC["shape"]["G"], 900 + i) for i in range(4)])
    else:
        case, st, eps = lg.build(name)
    return case, st, eps, lr.fit_constants(case)


def series_state(name, world, where):
    """(case, S0) of a series case.  extremes_first: psi of the cells of ranks >= 1 times 0.25 (float32-exact), so that +-max |psi| sit in rank 0 alone;
    extremes_last: psi of the cells of every rank but the last times 0.25; xadd_probe: psi times 2^-8, W times 32 (below)."""
    case, st = sr.build_state(name)
    st = {n: np.array(a, copy=True) for n, a in st.items()}
    N = case["Y"].shape[0]
    if where == "extremes_first":
        st["psi"][cell_range(N, 1, world)[0]:] *= 0.25
    elif where == "extremes_last":
        st["psi"][:cell_range(N, world - 1, world)[0]] *= 0.25
    elif where == "xadd_probe":
        # max |psi| = 2^-6 against loadings over [-72, 72]: ONE bin covers S0 (0.0156 x 144 / 4 < 1), and one Adam step (0.1 for every cell) makes |psi| seven times
        # what it was.  The pass after the step takes max |psi| from one step back: plus xadd (one step's bound, 0.727) that is 27 bins; WITHOUT xadd it is still one
        # bin, 72 wide each way, against |psi| = 0.115: |x dv| up to 8.3 where the series is built for 2 (tests/test_shard_grad_host.py has the arithmetic).
        # (Loadings of +-81 would show a stale xadd five times as clearly -- ELBO 1.2e-6 instead of 2.1e-7 of its magnitude -- but then the LAST monitor pass, two
        #  steps on and handed to the matrix-core sweeps, measured 1.95e-7 against the series form's ELBO bar of 1.18e-7, which is not a sweep's bar: +-72 it is.)
        st["psi"] *= 2.0 ** -8
        st["W"] *= 32.0
    else:
        assert where is None, where
    return case, st


def series_id(name, world, where):
    return f"{name}-w{world}" + (f"-{where}" if where else "")


@functools.lru_cache(maxsize=None)
def series_problem(name, world, where):
    case, st = series_state(name, world, where)
    G = case["Y"].shape[1]
    return case, st, np.stack([eps_for(1, G, 900 + i) for i in range(6)]), sr.fit_constants(case["Y"], case["L"])


def series_bar(n, handed=False):
    """TOL of the series file; beta has no element on the series form's shapes (bar 0); a train pass the look ahead gave to the sweeps: the hand-over bars."""
    if n == "beta":
        return 0.0
    if handed and n in TRAIN_VARS:
        return lg.bar("handover/bins_32", n)
    return sg.TOL[n]


# ------------------------------------------------------------------------------------------------------------------ what a rank does: collect
def _set_all(eng, S0, lo, hi):
    for n in sr.VAR_NAMES:
        eng.set(n, rig.shard_value(n, S0[n], lo, hi))


def _two_calls(S0, eps):
    def body(eng, rank, lo, hi, ar):
        rec = {"range": (lo, hi), "info": [eng.info()], "calls": []}
        _set_all(eng, S0, lo, hi)
        for it in (1, 2):
            elbo = eng.iterate(1, eps[2 * it - 2:2 * it])
            rec["calls"].append((elbo, eng.last_gradients(), eng.get_state()))
            rec["info"].append(eng.info())
        return rec
    return body


def _steady(S0, eps):
    def body(eng, rank, lo, hi, ar):
        rec = {"range": (lo, hi), "info": [eng.info()]}
        _set_all(eng, S0, lo, hi)
        elbo = eng.iterate(2, eps[:4])
        rec["calls"] = [(elbo, eng.last_gradients(), eng.get_state())]
        return rec
    return body


def _run(S0, eps):
    def body(eng, rank, lo, hi, ar):
        rec = {"range": (lo, hi), "info": [eng.info()]}
        _set_all(eng, S0, lo, hi)
        trace = eng.run(eps[:6], 2, 0.0)
        rec["calls"] = [(trace, eng.last_gradients(), eng.get_state())]
        rec["info"].append(eng.info())
        return rec
    return body


def _stopped_run_then_call(S0, eps):
    def body(eng, rank, lo, hi, ar):
        rec = {"range": (lo, hi), "info": [eng.info()]}
        _set_all(eng, S0, lo, hi)
        trace = eng.run(eps[:8], 3, 1e30)          # (stops after its first iteration: any mean |relative change| is below 1e30)
        elbo = eng.iterate(1, eps[8:10])
        rec["calls"] = [((trace, elbo), eng.last_gradients(), eng.get_state())]
        rec["info"].append(eng.info())
        return rec
    return body


# ------------------------------------------------------------------------------------------------------------------ the main thread: compare
def whole_state(recs, k):
    """The state after call k, assembled from the ranks' slices; the replicated variables are those of every rank (asserted)."""
    st = {}
    for n in sr.VAR_NAMES:
        if n in rig.CELL_VARS:
            st[n] = np.concatenate([r["calls"][k][2][n] for r in recs], 0)
        else:
            st[n] = recs[0]["calls"][k][2][n]
            for r in recs[1:]:
                assert np.array_equal(r["calls"][k][2][n], st[n]), ("replicated variable differs between ranks", n)
    return st


F32_MIN = 2.0 ** -126      # the smallest normal float32


def logit_ratio(test, ref, scale, logits):
    """``worst_ratio`` for d gamma_logits = gamma (f - fbar), less what float32 cannot hold.  The engine's gamma is a float32: below F32_MIN it is flushed or has
    lost its bits, and so is a product below F32_MIN.  Against a float64 gamma of 1e-60 -- a state that came out of gamma init has such clones, the ``set`` states
    of the unsharded files have none: their logits differ by 60 at most, exp(-60) = 9e-27 -- the engine's exact 0 is as good as float32 gets, but relative to the
    element's own scale gamma (|f| + ..) it is |f - fbar| / (|f| + ..), per cent.  So from every |difference| the float32 floor is taken off first:
    F32_MIN (|f| + ..) + F32_MIN, with (|f| + ..) = scale / gamma.  2e-34 at these shapes: nothing a kernel can be wrong by and still have a finite ELBO."""
    from scipy.special import logsumexp
    test, ref, scale = (np.asarray(a, dtype=np.float64) for a in (test, ref, scale))
    gl = np.asarray(logits, dtype=np.float64)
    gamma = np.exp(gl - logsumexp(gl, 1, keepdims=True))
    with np.errstate(divide="ignore", invalid="ignore"):
        floor = F32_MIN * (1.0 + np.where(gamma > 0.0, scale / gamma, 0.0))
    assert np.isfinite(floor).all()
    d = np.abs(test - ref)
    d = np.where(np.isfinite(d), np.maximum(d - floor, 0.0), np.inf)
    return sr.worst_ratio(d, np.zeros_like(d), scale)


def compare(fig, key, recs, k, plan, logit_state):
    """fig[key + (rank, variable)] = worst |engine - reference| / scale over ALL elements, for every rank and variable; ``plan[variable] = (reference, scale)`` of
    the whole problem; ``logit_state``: the state gamma_logits' plan is at (``logit_ratio``).  The replicated gradients are asserted bit-identical across the ranks."""
    for r, rec in enumerate(recs):
        lo, hi = rec["range"]
        g = rec["calls"][k][1]
        for n in sr.VAR_NAMES:
            ref, sc = plan[n]
            if n in rig.CELL_VARS:
                ref, sc = ref[n][lo:hi], sc[n][lo:hi]
            else:
                ref, sc = ref[n], sc[n]
                assert np.array_equal(g[n], recs[0]["calls"][k][1][n]), ("replicated gradient differs between ranks", key, r, n)
            assert g[n].shape == ref.shape, (key, r, n, g[n].shape, ref.shape)
            fig[key + (r, n)] = logit_ratio(g[n], ref, sc, logit_state["gamma_logits"][lo:hi]) if n == "gamma_logits" else sr.worst_ratio(g[n], ref, sc)


def report(tag, fig, bar_of):
    """One line per figure, then the assertion: every figure under its bar."""
    bad = {}
    for k in sorted(fig):
        b = bar_of(k)
        print(f"shard_grad {tag} " + " ".join(f"rank{x}" if i == len(k) - 2 else str(x) for i, x in enumerate(k)) + f" {fig[k]:.3e} (bar {b:.2e})")
        if not fig[k] <= b:
            bad[k] = (fig[k], b)
    assert not bad, (tag, bad)


def check_info(tag, recs, world, expect):
    for r, rec in enumerate(recs):
        i = rec["info"][0]
        got = {k: i[k] for k in expect}
        assert got == expect, (tag, r, got, expect)
        assert i["transport_name"] == "host", (tag, r, i["transport_name"])
        lo, hi = cell_range(sum(x["info"][0]["N"] for x in recs), r, world)
        assert (lo, hi) == rec["range"] and i["N"] == hi - lo, (tag, r, rec["range"], i["N"])
        assert i["fold_gsum"] == 0 and i["yfin_split"] == 0, (tag, r, i)       # (both are off on a sharded handle)
    assert len(recs) == world


def _elbo(case, st, e):
    from oracle.fused_numpy import FusedModel
    return sr.state_for(FusedModel, case, st).elbo(e)


# ------------------------------------------------------------------------------------------------------------------ sweeps
def sweep_engine_kw(name):
    return dict(spec(name)["opts"])


@pytest.mark.parametrize("name,world", SWEEP_CASES, ids=[f"{n}-w{w}" for n, w in SWEEP_CASES])
def test_sharded_sweeps_apply_the_float64_gradient_per_element_on_every_rank(name, world):
    case, S0, eps, fc = sweep_problem(name)
    tag = f"{name}-w{world}"
    recs = rig.sharded_engines(case, world, _two_calls(S0, eps), engine_kw=sweep_engine_kw(name))
    plain = recs[0]["info"][0]["fused_sweep"] == 0
    fig, st = {}, S0
    for it in (1, 2):
        e0, e1 = eps[2 * it - 2], eps[2 * it - 1]
        nxt = whole_state(recs, it - 1)
        at0, at1 = lr.ref_gradients(fc, st, e0), lr.ref_gradients(fc, nxt, e1)
        plan = {n: at1 if (n in TAIL_VARS or (n == "gamma_logits" and not plain)) else at0 for n in sr.VAR_NAMES}
        compare(fig, (f"it{it}",), recs, it - 1, plan, st if plain else nxt)
        want = _elbo(case, nxt, e1)
        for r, rec in enumerate(recs):
            got = rec["calls"][it - 1][0]
            assert got == recs[0]["calls"][it - 1][0], ("the ELBO differs between ranks", tag, it, r)
            fig[(f"it{it}", r, "elbo")] = abs(got - want) / abs(want) if np.isfinite(got) else np.inf
        st = nxt
    assert len(fig) == world * 2 * (len(sr.VAR_NAMES) + 1), sorted(fig)          # no rank, iteration or variable left out
    fam = family(name)
    try:
        report(tag, fig, lambda k: lg.HARD if k[-1] == "elbo" else lg.bar(fam, k[-1]))
    finally:
        check_info(tag, recs, world, spec(name)["expect"])


def test_sharded_steady_state_sweep_applies_the_float64_gradient():
    """``iterate(2, four draws)`` at learning_rate = 0 (module docstring, STEADY STATE): the sweep that carries a monitor pass and the next train pass's draw
    through a pending tail whose local sums travel in that train pass's collective."""
    name, world = STEADY_CASE
    case, S0, eps, fc = sweep_problem(name)
    recs = rig.sharded_engines(case, world, _steady(S0, eps), engine_kw=dict(sweep_engine_kw(name), learning_rate=0.0))
    after = whole_state(recs, 0)
    for n in sr.VAR_NAMES:
        assert np.array_equal(after[n].reshape(S0[n].shape), S0[n]), n            # no step moved anything: every pass of the call was at S0
    at2, at3 = lr.ref_gradients(fc, S0, eps[2]), lr.ref_gradients(fc, S0, eps[3])
    fig = {}
    compare(fig, ("steady",), recs, 0, {n: at2 if n in TRAIN_VARS else at3 for n in sr.VAR_NAMES}, S0)
    want = _elbo(case, S0, eps[3])
    for r, rec in enumerate(recs):
        assert rec["calls"][0][0] == recs[0]["calls"][0][0], ("the ELBO differs between ranks", r)
        fig[("steady", r, "elbo")] = abs(rec["calls"][0][0] - want) / abs(want)
    assert len(fig) == world * (len(sr.VAR_NAMES) + 1), sorted(fig)
    fam = family(name)
    try:
        report(f"steady {name}-w{world}", fig, lambda k: lg.HARD if k[-1] == "elbo" else lg.bar(fam, k[-1]))
    finally:
        check_info("steady", recs, world, dict(spec(name)["expect"], fused_sweep=1, bwd_mfma=1))


def _check_run(tag, recs, world, case, S0, eps, ref_gradients, bar_of, moved):
    """``run(six draws, 2, 0)`` (module docstring, ca_run): the trace against the oracle at each value's draw, the buffers at the state read back."""
    after = whole_state(recs, 0)
    for n in sr.VAR_NAMES:
        if n != "gamma_logits":
            assert np.abs(after[n].reshape(S0[n].shape) - S0[n]).max(initial=0.0) <= moved, (tag, n)
    assert not np.array_equal(after["gamma_logits"], S0["gamma_logits"])           # gamma init has run
    at4 = ref_gradients(after, eps[4])
    fig = {}
    compare(fig, ("run",), recs, 0, {n: at4 for n in sr.VAR_NAMES}, after)
    want = [_elbo(case, after, eps[2 * i + 1]) for i in range(3)]
    for r, rec in enumerate(recs):
        trace = rec["calls"][0][0]
        assert trace.shape == (3,), (tag, r, trace)
        assert np.array_equal(trace, recs[0]["calls"][0][0]), ("the ELBO trace differs between ranks", tag, r)
        for i in range(3):
            fig[("run", r, f"elbo{i}")] = abs(trace[i] - want[i]) / abs(want[i]) if np.isfinite(trace[i]) else np.inf
    assert len(fig) == world * (len(sr.VAR_NAMES) + 3), sorted(fig)
    report(tag, fig, bar_of)


def test_sharded_run_on_the_sweeps_leaves_the_float64_gradient_and_trace():
    name, world = RUN_SWEEP_CASE
    case, S0, eps4, fc = sweep_problem(name)
    eps = np.concatenate([eps4, np.stack([eps_for(1, eps4.shape[2], 904 + i) for i in range(2)])])
    recs = rig.sharded_engines(case, world, _run(S0, eps), engine_kw=dict(sweep_engine_kw(name), learning_rate=0.0))
    fam = family(name)
    try:
        _check_run(f"run {name}-w{world}", recs, world, case, S0, eps, lambda st, e: lr.ref_gradients(fc, st, e),
                   lambda k: lg.HARD if k[-1].startswith("elbo") else lg.bar(fam, k[-1]), moved=0.0)
    finally:
        check_info("run", recs, world, dict(spec(name)["expect"]))


def _check_stopped_run(tag, recs, world, case, S0, eps, ref_gradients, bar_of, moved):
    """``run(eight draws, 3, 1e30)`` stops after iteration 1 with the NEXT train pass's backward half queued ahead (train_bwd_speculative: its collective has made
    Y^T psi global, no update follows -- and where the update was queued behind it, gated, it is cancelled); ``iterate(1, [e8, e9])`` then starts from a state
    whose count-matrix products must be made again and whose max |psi| slots are refreshed.  Trace at (S', e1), (S', e3); then the two-draw mapping at S'."""
    after = whole_state(recs, 0)
    for n in sr.VAR_NAMES:
        if n != "gamma_logits":
            assert np.abs(after[n].reshape(S0[n].shape) - S0[n]).max(initial=0.0) <= moved, (tag, n)
    at8, at9 = ref_gradients(after, eps[8]), ref_gradients(after, eps[9])
    fig = {}
    compare(fig, ("stopped",), recs, 0, {n: at8 if n in TRAIN_VARS else at9 for n in sr.VAR_NAMES}, after)
    want = [_elbo(case, after, eps[1]), _elbo(case, after, eps[3]), _elbo(case, after, eps[9])]
    for r, rec in enumerate(recs):
        trace, elbo = rec["calls"][0][0]
        assert trace.shape == (2,), (tag, r, trace)
        assert np.array_equal(trace, recs[0]["calls"][0][0][0]) and elbo == recs[0]["calls"][0][0][1], ("the ELBOs differ between ranks", tag, r)
        for i, got in enumerate((trace[0], trace[1], elbo)):
            fig[("stopped", r, f"elbo{i}")] = abs(got - want[i]) / abs(want[i]) if np.isfinite(got) else np.inf
    assert len(fig) == world * (len(sr.VAR_NAMES) + 3), sorted(fig)
    report(tag, fig, bar_of)


def _ten_draws(G):
    return np.stack([eps_for(1, G, 900 + i) for i in range(10)])


def test_sharded_call_after_a_stopped_run_applies_the_float64_gradient_on_the_sweeps():
    name, world = RUN_SWEEP_CASE
    case, S0, eps4, fc = sweep_problem(name)
    eps = _ten_draws(eps4.shape[2])
    recs = rig.sharded_engines(case, world, _stopped_run_then_call(S0, eps), engine_kw=dict(sweep_engine_kw(name), learning_rate=0.0))
    fam = family(name)
    _check_stopped_run(f"stopped {name}-w{world}", recs, world, case, S0, eps, lambda st, e: lr.ref_gradients(fc, st, e),
                       lambda k: lg.HARD if k[-1].startswith("elbo") else lg.bar(fam, k[-1]), moved=0.0)


def test_sharded_call_after_a_stopped_run_applies_the_float64_gradient_on_the_series_form():
    name, world, where = RUN_SERIES_CASE
    case, S0, _eps, fc = series_problem(name, world, where)
    eps = _ten_draws(case["Y"].shape[1])
    recs = rig.sharded_engines(case, world, _stopped_run_then_call(S0, eps), engine_kw=dict(variant_on=("series",), learning_rate=RUN_SERIES_LR))
    try:
        _check_stopped_run(f"stopped {series_id(name, world, where)}", recs, world, case, S0, eps, lambda st, e: sr.ref_gradients(fc, st, e[0]),
                           lambda k: sg.TOL["elbo"] if k[-1].startswith("elbo") else series_bar(k[-1]), moved=2.0 ** -90)
    finally:
        check_info("stopped series", recs, world, SERIES_INFO)
        for r, rec in enumerate(recs):
            assert rec["info"][1]["series_fallbacks"] == 0 and rec["info"][1]["series_passes"] >= 4, (r, rec["info"][1])


# ------------------------------------------------------------------------------------------------------------------ series form
SERIES_INFO = dict(fwd_series=1, fused_sweep=1, fwd_cell=1, fwd_mfma=1, bwd_mfma=1, update_merge=1, y_storage_name="u8", y_ride=1)


def series_preconditions(name, world, where):
    """CPU: the state has the bin count it is named for; returns (max |psi| of the WHOLE state, min W, max W, one step's bound)."""
    case, S0, _eps, _fc = series_problem(name, world, where)
    consts = sr.poly_constants()
    assert sr.expected_bins(S0, consts) == NB_OF.get(where, sr.SPECS[name]["nb"]), (name, where, sr.expected_bins(S0, consts))
    psi, W = S0["psi"].reshape(-1), S0["W"].reshape(-1)
    return float(np.abs(psi).max()), float(W.min()), float(W.max()), sr.poly_step_bound()


@pytest.mark.parametrize("name,world,where", SERIES_CASES, ids=[series_id(*c) for c in SERIES_CASES])
def test_sharded_series_form_applies_the_float64_gradient_per_element_on_every_rank(name, world, where):
    case, S0, eps, fc = series_problem(name, world, where)
    tag = series_id(name, world, where)
    xmax, vlo, vhi, sb = series_preconditions(name, world, where)
    consts = sr.poly_constants()
    assert sr.poly_covers(xmax, vlo, vhi, 0, sb, consts), tag                      # the first pass after a set decides at the exact (global) ranges
    # passes of call 1: Adam steps 0 and 1 since the ranges the look ahead decides from; of call 2: 1 and 2 -- on every rank alike (module docstring)
    want = [[sr.poly_covers(xmax, vlo, vhi, s, sb, consts) for s in steps] for steps in ((0, 1), (1, 2))]
    recs = rig.sharded_engines(case, world, _two_calls(S0, eps), engine_kw=dict(variant_on=("series",)))
    fig, st = {}, S0
    for it in (1, 2):
        e0, e1 = eps[2 * it - 2], eps[2 * it - 1]
        nxt = whole_state(recs, it - 1)
        at0, at1 = sr.ref_gradients(fc, st, e0[0]), sr.ref_gradients(fc, nxt, e1[0])
        compare(fig, (f"it{it}",), recs, it - 1, {n: at0 if n in TRAIN_VARS else at1 for n in sr.VAR_NAMES}, nxt)
        elbo = _elbo(case, nxt, e1)
        for r, rec in enumerate(recs):
            got = rec["calls"][it - 1][0]
            assert got == recs[0]["calls"][it - 1][0], ("the ELBO differs between ranks", tag, it, r)
            fig[(f"it{it}", r, "elbo")] = abs(got - elbo) / abs(elbo) if np.isfinite(got) else np.inf
        st = nxt
    assert len(fig) == world * 2 * (len(sr.VAR_NAMES) + 1), sorted(fig)
    handed = {f"it{it}": not want[it - 1][0] for it in (1, 2)}                     # the call's train pass went to the sweeps (bins_32's second)
    assert not handed["it1"], tag
    try:
        report(tag, fig, lambda k: series_bar(k[-1], handed[k[0]]))
    finally:
        check_info(tag, recs, world, SERIES_INFO)
        for r, rec in enumerate(recs):
            for it in (1, 2):
                i0, i1 = rec["info"][it - 1], rec["info"][it]
                got = (i1["series_passes"] - i0["series_passes"], i1["series_fallbacks"] - i0["series_fallbacks"])
                assert got == (sum(want[it - 1]), 2 - sum(want[it - 1])), (tag, r, it, got, want[it - 1])


def test_sharded_run_on_the_series_form_leaves_the_float64_gradient_and_trace():
    name, world, where = RUN_SERIES_CASE
    case, S0, eps, fc = series_problem(name, world, where)
    xmax, vlo, vhi, _sb = series_preconditions(name, world, where)
    sb = sr.poly_step_bound(lr=RUN_SERIES_LR)
    consts = sr.poly_constants()
    want = [sr.poly_covers(xmax, vlo, vhi, s, sb, consts) for s in (0, 1)]          # fused_pass(1, 2) at the exact ranges, fused_pass(3, 4) one step on
    assert want == [True, True]
    recs = rig.sharded_engines(case, world, _run(S0, eps), engine_kw=dict(variant_on=("series",), learning_rate=RUN_SERIES_LR))
    try:
        _check_run(f"run {series_id(name, world, where)}", recs, world, case, S0, eps, lambda st, e: sr.ref_gradients(fc, st, e[0]),
                   lambda k: sg.TOL["elbo"] if k[-1].startswith("elbo") else series_bar(k[-1]), moved=2.0 ** -90)
    finally:
        check_info("run series", recs, world, SERIES_INFO)
        for r, rec in enumerate(recs):
            i0, i1 = rec["info"]
            assert (i1["series_passes"] - i0["series_passes"], i1["series_fallbacks"] - i0["series_fallbacks"]) == (2, 0), (r, i0, i1)


# ------------------------------------------------------------------------------------------------------------------ the device group
def _group_case():
    case, _st = lr.build_state("generic", 5, **GROUP_SHAPE)
    case = dict(case)
    case["psi0"] = case["psi0"] * 3.0            # (so that the exponents are not all near zero)
    return case


def _group_probe(case, transport, variant_on):
    """No ``set`` on a group: gamma_init, three iterations, S = get_state(), ``iterate(1, [e0, e1])``, every rank's buffers, the state after."""
    from clonealign_amd.engine import HipGroupEngine
    G = case["Y"].shape[1]
    grp = HipGroupEngine(**case, devices=[0, 0], transport=transport, variant_on=variant_on, comm_timeout_ms=rig.COMM_TIMEOUT_MS)
    try:
        grp.gamma_init(eps_for(1, G, 0))
        grp.iterate(3, np.stack([eps_for(1, G, 700 + i) for i in range(6)]))
        S = grp.get_state()
        eps = np.stack([eps_for(1, G, 900 + i) for i in range(2)])
        elbo = grp.iterate(1, eps)
        infos = [grp.rank_info(r) for r in range(2)]
        grads = [grp.rank_last_gradients(r) for r in range(2)]
        return S, eps, elbo, infos, grads, grp.get_state(), grp.group_info()
    finally:
        grp.close()


def _check_group(tag, out, case, ref_gradients, bar_of, expect, transport):
    S, eps, elbo, infos, grads, after, ginfo = out
    N = case["Y"].shape[0]
    recs = [{"range": cell_range(N, r, 2), "info": [infos[r]], "calls": [(elbo, grads[r], None)]} for r in range(2)]
    at0, at1 = ref_gradients(S, eps[0]), ref_gradients(after, eps[1])
    fig = {}
    compare(fig, ("group",), recs, 0, {n: at0 if n in TRAIN_VARS else at1 for n in sr.VAR_NAMES}, after)
    want = _elbo(case, after, eps[1])
    fig[("group", 0, "elbo")] = abs(elbo - want) / abs(want)
    assert len(fig) == 2 * len(sr.VAR_NAMES) + 1, sorted(fig)
    try:
        report(tag, fig, bar_of)
    finally:
        assert ginfo["world"] == 2 and ginfo["transport_name"] == transport, ginfo
        for r in range(2):
            got = {k: infos[r][k] for k in expect}
            assert got == expect and infos[r]["transport_name"] == transport and infos[r]["N"] == recs[r]["range"][1] - recs[r]["range"][0], (tag, r, got, infos[r])


GROUP_SWEEP_INFO = dict(lg.FUSED_MC, **lg.U8_RIDE, fwd_block_cells=16)


def test_group_over_the_host_transport_applies_the_float64_gradient_on_the_sweeps():
    case = _group_case()
    fc = lr.fit_constants(case)
    out = _group_probe(case, "host", ())
    _check_group("group host sweeps", out, case, lambda st, e: lr.ref_gradients(fc, st, e),
                 lambda k: lg.HARD if k[-1] == "elbo" else lg.bar(GROUP_FAMILY, k[-1]), GROUP_SWEEP_INFO, "host")


def test_group_over_the_host_transport_applies_the_float64_gradient_on_the_series_form():
    case = _group_case()
    fc = sr.fit_constants(case["Y"], case["L"])
    out = _group_probe(case, "host", ("series",))
    _check_group("group host series", out, case, lambda st, e: sr.ref_gradients(fc, st, e[0]),
                 lambda k: sg.TOL["elbo"] if k[-1] == "elbo" else series_bar(k[-1]), SERIES_INFO, "host")


def test_group_over_the_peer_to_peer_transport_applies_the_float64_gradient():
    """The one case that reaches the column sums of the backward slabs and the psi.(YW) partial sum folded INSIDE the all-reduce's launch (ca_ar_ride), per element.
    Two ranks of one process on one device: the rig of tests/test_gpu_group.py, which may skip on its documented limit and on nothing else."""
    from tests.test_gpu_group import _rig_or_skip
    case = _group_case()
    fc = lr.fit_constants(case)
    out = _rig_or_skip(lambda: _group_probe(case, "p2p", ("p2p_same_device",)))
    _check_group("group p2p sweeps", out, case, lambda st, e: lr.ref_gradients(fc, st, e),
                 lambda k: lg.HARD if k[-1] == "elbo" else lg.bar(GROUP_FAMILY, k[-1]), GROUP_SWEEP_INFO, "p2p")
