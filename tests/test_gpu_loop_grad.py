"""The gradients the SWEEP forms of the fused loop apply, against float64, element by element: every row of DESIGN.md section 5's table but the series form's
(tests/test_gpu_series_grad.py), and the series form's handed-over passes.

``HipEngine.gradients()`` goes through the call-by-call passes; inside ``iterate`` / ``run`` the loop runs other kernels (k_fwd_cell_mix_ys, k_fwd_bal_ys,
k_fwd_cell<D, TL>, the two-operand-set sweeps of 9-16 clones and of mc_samples = 2, k_bwd_mfma as the loop launches it, k_update_merged or k_final_gene +
k_adam_cell).  The update launches store the gradient they apply and ``HipEngine.last_gradients()`` reads those buffers without running anything.

PROTOCOL per case (the one of tests/test_gpu_series_grad.py): ``set`` all eight variables to S0; ``iterate(1, eps[0:2])``; ``last_gradients()`` and ``get_state()``
(= S1); compare; a second ``iterate(1, eps[2:4])`` from S1 and the same again: the second call runs the merged update's riding prologue, the lagged fixed-point
exponents of the int8 stream and the look-ahead pick-up, which the first runs after a ``set``.

MAPPING, from ca_iterate / train_pass / monitor_pass (clonealign_hip.hip, ca_eng_loop.inc), for ``iterate(1, [e0, e1])`` (two draws: nothing carried):
* fused loop, S = 1 (<= 8 clones and 9-16 clones alike: ``fused_pass(0, 0)`` at S0, ``train_from_lookahead(0)``, ``fused_pass(1, 1)`` at S1) and mc_samples = 2
  (``train_pass``: ``fused_pass(0, 1)`` of the pass's two samples, then ``train_from_lookahead``; the monitor pass ``fused_pass(2, 3)``; s2_fuse changes nothing here
  because the last monitor pass has no next train pass):
    loc, ls, W, beta, psi  at (S0, e0)  -- k_update_merged, or k_final_gene (+ its psi blocks) where the merged form is off: both store at the same points;
    gamma_logits           at (S1, e1)  -- every fused cell epilogue stores d logits, the monitor pass's last;
    v, alpha_unconstr      at S1        -- the O(K + C) body of the monitor pass's tail (flush_mon_tail), stored whether or not it steps.
  K = 0 and D >= 5 at S = 1 and up to 8 clones run this fused loop too (``fused_sweep = 1``), with the vector unit's kernels in it.
* plain passes (``run_pass``, ``fused_sweep = 0``: mc_samples >= 3, more than 16 clones, 9-16 clones with S >= 2 or fractional copy numbers, the fused form
  switched off):
    loc, ls, W, beta, psi  at (S0, e0)  -- k_final_gene;
    gamma_logits           at (S0, e0)  -- k_cell_par / k_cell store d logits in CA_MODE_TRAIN only: the monitor pass (CA_MODE_ELBO) leaves the train pass's;
    v, alpha_unconstr      at S1        -- k_final_small of the monitor pass.
  (include/clonealign_hip.h said "stored by every cell epilogue" for gamma_logits; corrected there.)
Every case asserts the kernels it is named for through ``info()``: sweep forms, block shape, balanced sweep, stream, storage, update form.  ``info()`` has no
field for ``s2_fuse`` nor for ``yfin_ride``: those two cases differ from their twins in the switch alone, and a switch that did nothing would not show here
(tests/test_gpu_parity.py's bitwise twin tests are what holds the switches themselves).

BARS.  Hard: |engine - reference| <= 2e-5 x scale for EVERY element (the project's gradient bound, tests/test_gpu_parity.py, here per element).  Per family and
variable: min(2e-5, 8 x model ratio), the model ratio being ``worst_ratio(operand_model, reference, scale)`` over the family's cases at (S0, e0)
(tests/_loop_ref.py: the documented operand roundings) -- computed on the CPU from the reference alone (MODEL below; tests/test_loop_ref_host.py recomputes
the whole table).  A FAMILY is a kernel group AND a kind of state ("cell32/peaked"): over all kinds of a group the "wide" states' float32 exponent sets every
figure, and a bar of that size lets a coef carried in two bf16 parts through at the generic and peaked states, where it is the largest error by far.
The call's ELBO (the monitor pass's, at (S1, e1)) is compared too, against the float64 oracle at 2e-5 of its magnitude: the per-cell exponent shift the cell
epilogue adds back to log Z is the same for every clone of a cell and so cancels in EVERY gradient (d logits = gamma (f - fbar)) -- a wrong shift there shows
in the ELBO alone.
ONE DEVIATION from the plain rule, for v and alpha_unconstr alone (K and C elements): their only rounding is the float32 store, the model draws it once per
element (3e-10 ... 4e-8 in MODEL), and 8 x one draw says nothing about another draw: their model ratio is taken at least at 2^-24, the format's half ulp
(bar 4.8e-7).  The vector unit's float32 ACCUMULATORS are part of its model (tests/_loop_ref.py; DESIGN.md section 3 documents them).
THE "exact" KIND (tests/_loop_ref.py::build_state) is there for one defect: coef carried in two bf16 parts where three are specified.  At every other
state the forward sweep's own split error (2^-17 per product, as large as the missing third part) stands in the model and, times 8, hides it: the model with
coef cut to two parts stays under those bars in most cases.  In the exact state E = 1, mu L is one bf16 part and Z an integer: the model is left with the
float32 roundings alone (psi: 3.2e-8 ... 3.6e-8) and a two-part coef stands at 3.3e-6 ... 3.7e-6 of psi's scale (its model on the CPU, all five cases).  8 x 3e-8
is below what the sweeps' float32 accumulators are worth, which no matrix-core model here carries and the issue puts at sqrt(G) x 2^-24; so the bar of an
exact family is max(8 x model, sqrt(terms) x 2^-24), terms = G for psi and gamma_logits, N for the per-gene variables (``accumulation``): 5.8e-7 for psi at
G = 95, 1.0e-6 at G = 300 -- from the number format and the shape, a third to a fifth of what the defect gives.  One case per instantiation of k_bwd_mfma:
up to 8 clones (cell16), two exponent dimensions (d2-k1p1), three (d34-k2p1), C16 (c16-c16), S2 (s2-fuse).  One Adam step takes a state out of the kind (W moves by
0.1 at every gene, with its own sign), so these cases run at learning_rate = 0: S1 = S0 bit for bit, and the second call -- riding prologue, look-ahead pick-up
-- is held to the same bars at the same state with other draws.
STEADY STATE.  ``iterate(1, two draws)`` never runs ``fused_pass(m, next)`` with two DIFFERENT draws, nor mc_samples = 2's four-draw sweep
(``fused_pass(2m, 2m + 1, .., trainA)``, what ``s2_fuse`` switches on): its last monitor pass has no next train pass.  ``iterate(2, four draws)`` does, but from a
state (S1) no call returns.  test_steady_state_sweeps_apply_the_float64_gradient runs it at learning_rate = 0, where every pass is at S0 (asserted: the state
comes back unchanged, bit for bit): loc, ls, W, beta, psi at (S0, e2) come out of the look-ahead half of that sweep, gamma_logits at (S0, e3), v and alpha at S0.
profiles/r16_loop_grad.txt holds model and measured ratios per case and variable.
"""
import numpy as np
import pytest

from tests import _loop_ref as lr
from tests import _series_ref as sr
from tests._cases import eps_for

pytestmark = pytest.mark.gpu

TRAIN_VARS = ("loc", "ls", "W", "beta", "psi")
TAIL_VARS = ("v", "alpha_unconstr")
HARD = 2e-5
MARGIN = 8.0

MC = ("mfma", "mfma")
U8_RIDE = dict(y_storage_name="u8", y_mfma=2, y_stream_bits=8, y_ride=1)
FUSED_MC = dict(fused_sweep=1, fwd_cell=1, fwd_mfma=1, bwd_mfma=1, fwd_series=0, update_merge=1)
PLAIN_MC = dict(fused_sweep=0, fwd_cell=0, bwd_mfma=1, fwd_series=0, update_merge=0, y_ride=0)
VALU = dict(fwd_mfma=0, bwd_mfma=0, fwd_series=0, fwd_cell=0, update_merge=0, y_ride=0)
R8 = dict(N=333, G=95, C=8, K=1)        # ragged N and G
C5 = dict(N=700, G=1100, C=5, K=1)


EXACT_OPTS = dict(learning_rate=0.0)      # an exact state stays exact: both iterations of the protocol at S0 (module docstring)


def _case(group, shape, kinds=("generic",), model=MC, opts=None, expect=None, frac=False, overflow=False, seed=5):
    return [(f"{group}-{tag}-{k}" if tag else f"{group}-{k}", dict(group=group, shape=shape, kind=k, model=model, opts=dict(opts or {}, **(EXACT_OPTS if k == "exact" else {})), expect=expect or {}, frac=frac,
                                                                overflow=overflow, seed=seed))
            for tag in [shape.pop("tag", "")] for k in kinds]


ALL = ("generic", "wide", "peaked", "zero_L")
ALLX = ALL + ("exact",)      # ... and the state whose only operand with anything to lose is coef (tests/_loop_ref.py): one per k_bwd_mfma instantiation
CASES = dict(
    # 16-cell four-wave blocks with the int8 stream riding: k_fwd_cell_mix_ys<1, 1>
    _case("cell16", dict(R8), ALLX, expect=dict(FUSED_MC, **U8_RIDE, fwd_block_cells=16, fwd_blocks_big=0, fwd_balanced=0))
    # 32-cell blocks
    + _case("cell32", dict(C5), ALL, opts=dict(tune=dict(fc_tl=2)), expect=dict(FUSED_MC, **U8_RIDE, fwd_block_cells=32, fwd_blocks_big=0, fwd_balanced=0))
    # two block sizes in one launch: 3 blocks of 64 cells, the rest in 32-cell blocks (k_fwd_cell_mix; the stream does not ride on this shape of launch)
    + _case("cell_mix", dict(C5), ALL, opts=dict(tune=dict(fc_tl=4, fc_nbig=3)), expect=dict(FUSED_MC, y_storage_name="u8", y_mfma=2, y_ride=0, fwd_block_cells=64, fwd_blocks_big=3, fwd_balanced=0))
    # 96-cell blocks with the stream riding, forced at 2011 cells (21 blocks, the last one ragged)
    + _case("cell96", dict(N=2011, G=300, C=8, K=1), ALL, opts=dict(tune=dict(fc_tl=6)),
            expect=dict(FUSED_MC, **U8_RIDE, fwd_block_cells=96, fwd_blocks_big=0, fwd_balanced=0))
    # the balanced sweep k_fwd_bal_ys: 270 tiles = 256 + 14 left over in sixteen gene chunks, ragged last tile (the smallest of tests/test_gpu_scale.py's BAL_SHAPES)
    + _case("balanced", dict(N=4316, G=3100, C=8, K=1), ALL, expect=dict(FUSED_MC, **U8_RIDE, fwd_balanced=1, fwd_block_cells=16, fwd_blocks_big=0))
    # D = 2
    + _case("d2", dict(N=520, G=300, C=6, K=1, P=1, tag="k1p1"), ALLX, expect=dict(FUSED_MC, **U8_RIDE, fwd_block_cells=16, fwd_blocks_big=0, fwd_balanced=0))
    + _case("d2", dict(N=257, G=161, C=2, K=2, tag="k2"), expect=dict(FUSED_MC, y_storage_name="u8", y_mfma=0, y_stream_bits=0, y_ride=0, fwd_block_cells=32, fwd_blocks_big=0, fwd_balanced=0))   # K = 2: the vector stream, a launch of its own
    # D = 3, 4: k_fwd_cell<D, TL>, k_bwd_mfma<3, D>
    + _case("d34", dict(N=200, G=90, C=4, K=2, P=1, tag="k2p1"), ALLX, expect=dict(FUSED_MC, y_storage_name="u8", y_mfma=0, y_stream_bits=0, y_ride=0, fwd_block_cells=32, fwd_blocks_big=0, fwd_balanced=0))
    + _case("d34", dict(N=530, G=333, C=7, K=2, P=2, tag="k2p2"), ("generic", "wide"), expect=dict(FUSED_MC, y_storage_name="u8", y_mfma=0, y_stream_bits=0, y_ride=0, fwd_block_cells=32, fwd_blocks_big=0, fwd_balanced=0))
    # 9-16 clones: the two-operand-set sweep, coef in three bf16 parts
    + _case("c16", dict(N=333, G=95, C=16, K=1, tag="c16"), ALLX, expect=dict(FUSED_MC, **U8_RIDE, fwd_block_cells=32, fwd_blocks_big=0, fwd_balanced=0))
    + _case("c16", dict(N=700, G=1100, C=11, K=1, tag="c11"), expect=dict(FUSED_MC, **U8_RIDE, fwd_block_cells=32, fwd_blocks_big=0, fwd_balanced=0))
    # mc_samples = 2, with the four-draw sweep and without
    + _case("s2", dict(N=333, G=95, C=8, K=1, S=2, tag="fuse"), ALLX, expect=dict(FUSED_MC, **U8_RIDE, fwd_block_cells=96, fwd_blocks_big=0, fwd_balanced=0))
    + _case("s2", dict(N=333, G=95, C=8, K=1, S=2, tag="nofuse"), opts=dict(variant_off=("s2_fuse",)), expect=dict(FUSED_MC, **U8_RIDE, fwd_block_cells=96, fwd_blocks_big=0, fwd_balanced=0))
    # plain passes on the matrix cores
    + _case("plain", dict(N=700, G=1100, C=5, K=1, S=3, tag="s3"), ALL, expect=dict(PLAIN_MC, fwd_mfma=1, y_storage_name="u8", y_mfma=2, y_stream_bits=8))
    + _case("plain", dict(N=333, G=95, C=18, K=1, tag="c18"), expect=dict(PLAIN_MC, fwd_mfma=1, y_storage_name="u8", y_mfma=2, y_stream_bits=8))
    + _case("plain", dict(N=333, G=95, C=11, K=1, S=2, tag="c11s2"), expect=dict(PLAIN_MC, fwd_mfma=1, y_storage_name="u8", y_mfma=2, y_stream_bits=8))
    # a plain pass with no matrix-core way forward (D = 3 at S = 2) and the extra log-likelihood term
    + _case("plain_d3", dict(N=200, G=90, C=4, K=2, P=1, S=2, extra=True), model=("valu", "mfma"), expect=dict(PLAIN_MC, fwd_mfma=0, y_storage_name="u8", y_mfma=0))
    # vector-unit fallbacks
    + _case("valu", dict(N=200, G=90, C=4, K=3, P=2, tag="d5"), model="valu", expect=dict(VALU, fused_sweep=1))
    + _case("valu", dict(N=257, G=70, C=4, K=0, tag="k0"), model="valu", expect=dict(VALU, fused_sweep=1))
    + _case("valu", dict(N=100, G=40, C=3, K=0, P=1, tag="k0p1"), model="valu", expect=dict(VALU, fused_sweep=1))
    + _case("valu", dict(R8, tag="fused_off"), model=("valu", "mfma"), opts=dict(variant_off=("fused",)), expect=dict(fused_sweep=0, fwd_cell=0, fwd_mfma=0, bwd_mfma=1, fwd_series=0, update_merge=0, y_ride=0, y_mfma=2))
    + _case("valu_bwd", dict(R8), model=("mfma", "valu"), opts=dict(variant_off=("bwd_mfma",)), expect=dict(fused_sweep=1, fwd_cell=1, fwd_mfma=1, bwd_mfma=0, fwd_series=0, update_merge=1, **U8_RIDE, fwd_block_cells=16, fwd_blocks_big=0, fwd_balanced=0))
    + _case("valu_fwd", dict(R8), model=("valu", "mfma"), opts=dict(variant_off=("fwd_mfma",)), expect=dict(fused_sweep=1, fwd_cell=0, fwd_mfma=0, bwd_mfma=1, fwd_series=0, update_merge=0, y_ride=0, y_mfma=2, y_stream_bits=8))
    # fractional copy numbers: the two-part form at C <= 8, the vector unit's way back beyond eight clones
    + _case("frac", dict(R8), ALL, model="mfma_frac", frac=True, expect=dict(FUSED_MC, **U8_RIDE, fwd_block_cells=16, fwd_blocks_big=0, fwd_balanced=0))
    + _case("frac_c11", dict(N=333, G=95, C=11, K=1), model="valu", frac=True, expect=dict(VALU, fused_sweep=0, y_storage_name="u8", y_mfma=2))
    # storage and stream
    + _case("storage", dict(R8, tag="u16"), opts=dict(y_storage="u16"), expect=dict(FUSED_MC, y_storage_name="u16", y_mfma=0, y_stream_bits=0, fwd_block_cells=32))
    + _case("storage", dict(R8, tag="f32"), opts=dict(y_storage="f32"), expect=dict(FUSED_MC, y_storage_name="f32", y_mfma=0, y_stream_bits=0, fwd_block_cells=32))
    + _case("storage", dict(R8, tag="u8_overflow"), overflow=True, expect=dict(FUSED_MC, **U8_RIDE, fwd_block_cells=16, fwd_blocks_big=0, fwd_balanced=0))
    + _case("storage", dict(R8, tag="vector_stream"), opts=dict(variant_off=("y_mfma1",)), expect=dict(FUSED_MC, y_storage_name="u8", y_mfma=0, y_stream_bits=0, y_ride=1, fwd_block_cells=32, fwd_blocks_big=0))
    + _case("storage", dict(R8, tag="two_launch_update"), opts=dict(variant_off=("update_merge",)), expect=dict(FUSED_MC, **U8_RIDE, fwd_block_cells=16, fwd_blocks_big=0, fwd_balanced=0, update_merge=0))
    + _case("storage", dict(R8, tag="yfin_launch"), opts=dict(variant_off=("yfin_ride",)), expect=dict(FUSED_MC, **U8_RIDE, fwd_block_cells=16, fwd_blocks_big=0, fwd_balanced=0))
)

# worst_ratio(operand_model, reference, scale) at (S0, e0), the largest over each family's cases (family = group/kind): the CPU's figures (model_ratios
# below; no engine involved; tests/test_loop_ref_host.py recomputes every row)
MODEL = {
    "cell16/generic": {"W": 6.244e-08, "v": 9.576e-09, "psi": 4.479e-07, "beta": 0.000e+00, "alpha_unconstr": 8.200e-09, "loc": 8.014e-08, "ls": 9.428e-08, "gamma_logits": 8.171e-08},
    "cell16/wide": {"W": 6.284e-07, "v": 3.107e-10, "psi": 2.689e-06, "beta": 0.000e+00, "alpha_unconstr": 8.200e-09, "loc": 3.507e-07, "ls": 3.292e-07, "gamma_logits": 1.179e-07},
    "cell16/peaked": {"W": 4.956e-08, "v": 9.576e-09, "psi": 5.394e-07, "beta": 0.000e+00, "alpha_unconstr": 5.518e-09, "loc": 1.088e-07, "ls": 1.445e-07, "gamma_logits": 1.284e-07},
    "cell16/zero_L": {"W": 5.471e-08, "v": 9.576e-09, "psi": 4.452e-07, "beta": 0.000e+00, "alpha_unconstr": 8.200e-09, "loc": 8.973e-08, "ls": 9.488e-08, "gamma_logits": 8.045e-08},
    "cell32/generic": {"W": 6.790e-08, "v": 1.215e-08, "psi": 1.578e-07, "beta": 0.000e+00, "alpha_unconstr": 5.466e-09, "loc": 1.340e-07, "ls": 1.246e-07, "gamma_logits": 1.716e-08},
    "cell32/wide": {"W": 7.418e-07, "v": 5.466e-09, "psi": 1.052e-06, "beta": 0.000e+00, "alpha_unconstr": 5.466e-09, "loc": 5.723e-07, "ls": 5.940e-07, "gamma_logits": 2.963e-08},
    "cell32/peaked": {"W": 5.495e-08, "v": 1.215e-08, "psi": 1.504e-07, "beta": 0.000e+00, "alpha_unconstr": 7.341e-09, "loc": 1.183e-07, "ls": 1.222e-07, "gamma_logits": 2.884e-08},
    "cell32/zero_L": {"W": 5.696e-08, "v": 1.215e-08, "psi": 1.602e-07, "beta": 0.000e+00, "alpha_unconstr": 5.466e-09, "loc": 1.666e-07, "ls": 1.441e-07, "gamma_logits": 1.778e-08},
    "cell_mix/generic": {"W": 6.790e-08, "v": 1.215e-08, "psi": 1.578e-07, "beta": 0.000e+00, "alpha_unconstr": 5.466e-09, "loc": 1.340e-07, "ls": 1.246e-07, "gamma_logits": 1.716e-08},
    "cell_mix/wide": {"W": 7.418e-07, "v": 5.466e-09, "psi": 1.052e-06, "beta": 0.000e+00, "alpha_unconstr": 5.466e-09, "loc": 5.723e-07, "ls": 5.940e-07, "gamma_logits": 2.963e-08},
    "cell_mix/peaked": {"W": 5.495e-08, "v": 1.215e-08, "psi": 1.504e-07, "beta": 0.000e+00, "alpha_unconstr": 7.341e-09, "loc": 1.183e-07, "ls": 1.222e-07, "gamma_logits": 2.884e-08},
    "cell_mix/zero_L": {"W": 5.696e-08, "v": 1.215e-08, "psi": 1.602e-07, "beta": 0.000e+00, "alpha_unconstr": 5.466e-09, "loc": 1.666e-07, "ls": 1.441e-07, "gamma_logits": 1.778e-08},
    "cell96/generic": {"W": 4.922e-08, "v": 2.498e-08, "psi": 1.894e-07, "beta": 0.000e+00, "alpha_unconstr": 5.023e-09, "loc": 5.782e-08, "ls": 6.453e-08, "gamma_logits": 4.985e-08},
    "cell96/wide": {"W": 7.544e-07, "v": 1.210e-09, "psi": 1.921e-06, "beta": 0.000e+00, "alpha_unconstr": 5.023e-09, "loc": 5.179e-07, "ls": 5.110e-07, "gamma_logits": 7.620e-08},
    "cell96/peaked": {"W": 5.367e-08, "v": 2.498e-08, "psi": 2.645e-07, "beta": 0.000e+00, "alpha_unconstr": 2.754e-09, "loc": 7.940e-08, "ls": 6.310e-08, "gamma_logits": 6.184e-08},
    "cell96/zero_L": {"W": 5.718e-08, "v": 2.498e-08, "psi": 1.891e-07, "beta": 0.000e+00, "alpha_unconstr": 5.023e-09, "loc": 6.834e-08, "ls": 7.608e-08, "gamma_logits": 5.016e-08},
    "balanced/generic": {"W": 4.320e-08, "v": 2.630e-08, "psi": 7.124e-08, "beta": 0.000e+00, "alpha_unconstr": 5.211e-09, "loc": 1.072e-07, "ls": 9.791e-08, "gamma_logits": 1.323e-08},
    "balanced/wide": {"W": 5.696e-07, "v": 2.954e-09, "psi": 9.096e-07, "beta": 0.000e+00, "alpha_unconstr": 5.211e-09, "loc": 4.471e-07, "ls": 4.150e-07, "gamma_logits": 2.244e-08},
    "balanced/peaked": {"W": 4.265e-08, "v": 2.630e-08, "psi": 1.092e-07, "beta": 0.000e+00, "alpha_unconstr": 6.976e-09, "loc": 9.236e-08, "ls": 8.953e-08, "gamma_logits": 1.704e-08},
    "balanced/zero_L": {"W": 5.324e-08, "v": 2.630e-08, "psi": 7.421e-08, "beta": 0.000e+00, "alpha_unconstr": 5.211e-09, "loc": 1.121e-07, "ls": 1.154e-07, "gamma_logits": 1.370e-08},
    "d2/generic": {"W": 8.602e-08, "v": 2.583e-08, "psi": 3.116e-07, "beta": 2.705e-07, "alpha_unconstr": 2.309e-09, "loc": 2.104e-07, "ls": 2.055e-07, "gamma_logits": 5.554e-08},
    "d2/wide": {"W": 7.643e-07, "v": 4.538e-09, "psi": 1.788e-06, "beta": 3.365e-07, "alpha_unconstr": 1.612e-09, "loc": 5.703e-07, "ls": 5.925e-07, "gamma_logits": 6.461e-08},
    "d2/peaked": {"W": 1.040e-07, "v": 2.498e-08, "psi": 2.744e-07, "beta": 3.059e-07, "alpha_unconstr": 1.008e-08, "loc": 2.203e-07, "ls": 2.017e-07, "gamma_logits": 7.829e-08},
    "d2/zero_L": {"W": 8.573e-08, "v": 2.498e-08, "psi": 2.624e-07, "beta": 2.365e-07, "alpha_unconstr": 1.612e-09, "loc": 2.687e-07, "ls": 3.140e-07, "gamma_logits": 5.618e-08},
    "d34/generic": {"W": 1.432e-07, "v": 4.161e-08, "psi": 4.549e-07, "beta": 2.508e-07, "alpha_unconstr": 5.811e-09, "loc": 2.433e-07, "ls": 2.415e-07, "gamma_logits": 7.960e-08},
    "d34/wide": {"W": 4.308e-06, "v": 2.152e-08, "psi": 4.741e-06, "beta": 1.769e-06, "alpha_unconstr": 5.811e-09, "loc": 3.747e-06, "ls": 3.752e-06, "gamma_logits": 1.004e-07},
    "d34/peaked": {"W": 1.360e-07, "v": 2.681e-08, "psi": 5.592e-07, "beta": 2.208e-07, "alpha_unconstr": 3.558e-09, "loc": 2.731e-07, "ls": 2.386e-07, "gamma_logits": 1.327e-07},
    "d34/zero_L": {"W": 1.537e-07, "v": 2.681e-08, "psi": 4.716e-07, "beta": 1.573e-07, "alpha_unconstr": 5.811e-09, "loc": 2.608e-07, "ls": 2.567e-07, "gamma_logits": 9.657e-08},
    "c16/generic": {"W": 5.506e-08, "v": 1.215e-08, "psi": 3.995e-07, "beta": 0.000e+00, "alpha_unconstr": 1.126e-08, "loc": 1.596e-07, "ls": 1.638e-07, "gamma_logits": 9.572e-08},
    "c16/wide": {"W": 4.719e-07, "v": 3.107e-10, "psi": 2.725e-06, "beta": 0.000e+00, "alpha_unconstr": 5.045e-09, "loc": 4.073e-07, "ls": 4.340e-07, "gamma_logits": 1.178e-07},
    "c16/peaked": {"W": 8.993e-08, "v": 9.576e-09, "psi": 4.329e-07, "beta": 0.000e+00, "alpha_unconstr": 9.715e-09, "loc": 1.328e-07, "ls": 1.156e-07, "gamma_logits": 1.593e-07},
    "c16/zero_L": {"W": 5.072e-08, "v": 9.576e-09, "psi": 3.970e-07, "beta": 0.000e+00, "alpha_unconstr": 5.045e-09, "loc": 1.885e-07, "ls": 1.615e-07, "gamma_logits": 9.548e-08},
    "s2/generic": {"W": 1.029e-07, "v": 9.576e-09, "psi": 4.280e-07, "beta": 0.000e+00, "alpha_unconstr": 8.200e-09, "loc": 2.008e-07, "ls": 2.708e-07, "gamma_logits": 6.761e-08},
    "s2/wide": {"W": 1.429e-06, "v": 3.107e-10, "psi": 3.041e-06, "beta": 0.000e+00, "alpha_unconstr": 8.200e-09, "loc": 7.473e-07, "ls": 1.173e-06, "gamma_logits": 9.011e-08},
    "s2/peaked": {"W": 7.844e-08, "v": 9.576e-09, "psi": 3.929e-07, "beta": 0.000e+00, "alpha_unconstr": 5.518e-09, "loc": 2.187e-07, "ls": 2.631e-07, "gamma_logits": 9.912e-08},
    "s2/zero_L": {"W": 9.954e-08, "v": 9.576e-09, "psi": 4.318e-07, "beta": 0.000e+00, "alpha_unconstr": 8.200e-09, "loc": 2.088e-07, "ls": 2.277e-07, "gamma_logits": 6.968e-08},
    "plain/generic": {"W": 1.131e-07, "v": 1.215e-08, "psi": 3.259e-07, "beta": 0.000e+00, "alpha_unconstr": 6.869e-09, "loc": 2.958e-07, "ls": 4.239e-07, "gamma_logits": 9.807e-08},
    "plain/wide": {"W": 9.011e-07, "v": 5.466e-09, "psi": 1.156e-06, "beta": 0.000e+00, "alpha_unconstr": 5.466e-09, "loc": 6.985e-07, "ls": 6.983e-07, "gamma_logits": 2.684e-08},
    "plain/peaked": {"W": 4.020e-08, "v": 1.215e-08, "psi": 9.358e-08, "beta": 0.000e+00, "alpha_unconstr": 7.341e-09, "loc": 1.006e-07, "ls": 9.542e-08, "gamma_logits": 1.541e-08},
    "plain/zero_L": {"W": 3.440e-08, "v": 1.215e-08, "psi": 1.134e-07, "beta": 0.000e+00, "alpha_unconstr": 5.466e-09, "loc": 1.223e-07, "ls": 1.273e-07, "gamma_logits": 1.167e-08},
    "plain_d3/generic": {"W": 2.767e-08, "v": 2.681e-08, "psi": 8.632e-08, "beta": 5.486e-08, "alpha_unconstr": 5.811e-09, "loc": 5.606e-08, "ls": 3.628e-08, "gamma_logits": 2.015e-08},
    "valu/generic": {"W": 1.194e-07, "v": 3.360e-08, "psi": 1.558e-07, "beta": 2.115e-07, "alpha_unconstr": 1.087e-08, "loc": 3.276e-07, "ls": 3.359e-07, "gamma_logits": 3.651e-08},
    "valu_bwd/generic": {"W": 1.105e-07, "v": 9.576e-09, "psi": 4.479e-07, "beta": 0.000e+00, "alpha_unconstr": 8.200e-09, "loc": 5.085e-07, "ls": 4.996e-07, "gamma_logits": 8.171e-08},
    "valu_fwd/generic": {"W": 1.994e-08, "v": 9.576e-09, "psi": 7.893e-08, "beta": 0.000e+00, "alpha_unconstr": 8.200e-09, "loc": 4.942e-08, "ls": 4.448e-08, "gamma_logits": 3.651e-08},
    "frac/generic": {"W": 3.575e-07, "v": 9.576e-09, "psi": 8.998e-07, "beta": 0.000e+00, "alpha_unconstr": 8.200e-09, "loc": 1.465e-06, "ls": 1.418e-06, "gamma_logits": 9.601e-08},
    "frac/wide": {"W": 1.729e-06, "v": 3.107e-10, "psi": 3.437e-06, "beta": 0.000e+00, "alpha_unconstr": 8.200e-09, "loc": 1.319e-06, "ls": 1.318e-06, "gamma_logits": 1.474e-07},
    "frac/peaked": {"W": 9.438e-07, "v": 9.576e-09, "psi": 2.283e-06, "beta": 0.000e+00, "alpha_unconstr": 5.518e-09, "loc": 1.540e-06, "ls": 1.576e-06, "gamma_logits": 1.268e-07},
    "frac/zero_L": {"W": 4.578e-07, "v": 9.576e-09, "psi": 1.668e-06, "beta": 0.000e+00, "alpha_unconstr": 8.200e-09, "loc": 1.398e-06, "ls": 1.423e-06, "gamma_logits": 9.458e-08},
    "frac_c11/generic": {"W": 2.316e-07, "v": 9.576e-09, "psi": 9.371e-08, "beta": 0.000e+00, "alpha_unconstr": 6.869e-09, "loc": 7.816e-07, "ls": 7.638e-07, "gamma_logits": 4.030e-08},
    "storage/generic": {"W": 6.244e-08, "v": 9.576e-09, "psi": 4.479e-07, "beta": 0.000e+00, "alpha_unconstr": 8.200e-09, "loc": 1.072e-07, "ls": 1.369e-07, "gamma_logits": 8.171e-08},
    "cell16/exact": {"W": 1.016e-08, "v": 6.216e-09, "psi": 3.606e-08, "beta": 0.000e+00, "alpha_unconstr": 5.518e-09, "loc": 3.714e-08, "ls": 2.220e-16, "gamma_logits": 1.558e-09},
    "d2/exact": {"W": 1.672e-08, "v": 5.714e-09, "psi": 3.324e-08, "beta": 1.721e-08, "alpha_unconstr": 1.008e-08, "loc": 4.186e-08, "ls": 8.882e-16, "gamma_logits": 9.537e-10},
    "d34/exact": {"W": 1.108e-08, "v": 1.646e-08, "psi": 3.226e-08, "beta": 1.259e-08, "alpha_unconstr": 3.558e-09, "loc": 5.000e-08, "ls": 3.331e-16, "gamma_logits": 1.410e-09},
    "c16/exact": {"W": 1.341e-08, "v": 6.216e-09, "psi": 3.519e-08, "beta": 0.000e+00, "alpha_unconstr": 9.715e-09, "loc": 3.526e-08, "ls": 6.661e-16, "gamma_logits": 1.537e-09},
    "s2/exact": {"W": 1.016e-08, "v": 6.216e-09, "psi": 3.606e-08, "beta": 0.000e+00, "alpha_unconstr": 5.518e-09, "loc": 3.714e-08, "ls": 2.220e-16, "gamma_logits": 1.558e-09},
    "handover/bins_32": {"W": 3.367e-06, "v": 4.895e-09, "psi": 6.624e-06, "beta": 0.000e+00, "alpha_unconstr": 9.405e-09, "loc": 2.920e-06, "ls": 2.929e-06, "gamma_logits": 1.238e-07},
    "handover/too_wide": {"W": 2.235e-06, "v": 3.827e-08, "psi": 5.301e-06, "beta": 0.000e+00, "alpha_unconstr": 9.405e-09, "loc": 1.727e-06, "ls": 1.727e-06, "gamma_logits": 1.561e-07},
}


def family(name):
    return f"{CASES[name]['group']}/{CASES[name]['kind']}"


def build(name):
    """(constructor arguments, S0, eps [4, S, G]) of a case."""
    c = CASES[name]
    case, st = lr.build_state(c["kind"], c["seed"], **c["shape"])
    if c["frac"]:
        case["L"] = case["L"] + np.random.default_rng(5).random(case["L"].shape) * 0.9 * (case["L"] > 0)     # arbitrary fractions, not bf16-exact
    if c["overflow"]:
        Y, rng = case["Y"], np.random.default_rng(0)
        for _ in range(12):
            Y[rng.integers(0, Y.shape[0]), rng.integers(1, Y.shape[1])] = float(rng.integers(256, 5000))
        Y[3, 5], Y[3, 6], Y[200, 5] = 256.0, 70000.0, 300.0
    S, G = c["shape"].get("S", 1), c["shape"]["G"]
    return case, st, np.stack([eps_for(S, G, 900 + i) for i in range(4)])


def model_ratios(name):
    """{variable: worst_ratio(operand model, reference, scale)} of a case at (S0, e0): CPU only."""
    case, st, eps = build(name)
    fc = lr.fit_constants(case)
    ref, sc = lr.ref_gradients(fc, st, eps[0])
    mod = lr.operand_model(fc, st, eps[0], CASES[name]["model"])
    return {n: sr.worst_ratio(mod[n], ref[n], sc[n]) for n in sr.VAR_NAMES}


FLOOR = 2.0 ** -24      # v, alpha_unconstr alone (module docstring): the float32 store of a K- or C-element gradient, half an ulp of at most its scale


def accumulation(fam, n):
    """sqrt(terms) x 2^-24: what a float32 sum of ``terms`` summands is worth and no model here carries for the matrix-core sweeps -- psi and gamma_logits are
    sums over the G genes, the per-gene variables over the N cells (the largest N or G of the family's cases)."""
    dims = [CASES[c]["shape"] for c in CASES if family(c) == fam]
    return np.sqrt(max(d["G" if n in ("psi", "gamma_logits") else "N"] for d in dims)) * FLOOR


def bar(fam, n):
    m = MODEL[fam][n]
    if n in TAIL_VARS:
        return min(HARD, MARGIN * max(m, FLOOR))
    if fam.endswith("/exact"):      # (module docstring: the one kind of state whose model has no operand error for the factor 8 to stand on)
        return min(HARD, max(MARGIN * m, accumulation(fam, n)))
    return min(HARD, MARGIN * m)


def probe(name, engine_kw=None, check_info=True):
    """One engine, two iterations: ({(iteration, variable): worst |engine - reference| / scale over all elements}, info)."""
    from clonealign_amd.engine import HipEngine
    from oracle.fused_numpy import FusedModel
    c = CASES[name]
    case, S0, eps = build(name)
    fc = lr.fit_constants(case)
    eng = HipEngine(**case, **(c["opts"] if engine_kw is None else engine_kw))
    fig = {}
    try:
        info = eng.info()
        if check_info:
            got = {k: info[k] for k in c["expect"]}
            assert got == c["expect"], (name, got, c["expect"])
        plain = info["fused_sweep"] == 0
        for n in sr.VAR_NAMES:
            eng.set(n, S0[n])
        st = S0
        for it in (1, 2):
            e0, e1 = eps[2 * it - 2], eps[2 * it - 1]
            elbo = eng.iterate(1, eps[2 * it - 2:2 * it])
            g, nxt = eng.last_gradients(), eng.get_state()
            want = sr.state_for(FusedModel, case, nxt).elbo(e1)          # the call's ELBO is the monitor pass's: (S1, e1)
            fig[(it, "elbo")] = abs(elbo - want) / abs(want) if np.isfinite(elbo) else np.inf
            ref0, sc0 = lr.ref_gradients(fc, st, e0)
            ref1, sc1 = lr.ref_gradients(fc, nxt, e1)
            for n in sr.VAR_NAMES:
                ref, sc = (ref1, sc1) if (n in TAIL_VARS or (n == "gamma_logits" and not plain)) else (ref0, sc0)
                assert g[n].shape == ref[n].shape, (n, g[n].shape, ref[n].shape)
                fig[(it, n)] = sr.worst_ratio(g[n], ref[n], sc[n])
            st = nxt
        return fig, info
    finally:
        eng.close()


def check(name, fig):
    group = family(name)
    for (it, n), r in sorted(fig.items()):
        print(f"loop_grad {name} it{it} {n} {r:.3e} " + (f"(bar {HARD:.2e})" if n == "elbo" else f"(bar {bar(group, n):.2e}, model {MODEL[group][n]:.2e})"))
    assert len(fig) == 2 * (len(sr.VAR_NAMES) + 1), sorted(fig)        # no variable and no iteration left out
    bad = {k: (r, HARD if k[1] == "elbo" else bar(group, k[1])) for k, r in fig.items() if not r <= (HARD if k[1] == "elbo" else bar(group, k[1]))}
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", list(CASES))
def test_sweep_forms_apply_the_float64_gradient_per_element(name):
    fig, _info = probe(name)
    check(name, fig)


STEADY = ("cell16-generic", "d34-k2p1-generic", "c16-c16-generic", "s2-fuse-generic", "s2-fuse-exact", "s2-nofuse-generic")


@pytest.mark.parametrize("name", STEADY)
def test_steady_state_sweeps_apply_the_float64_gradient(name):
    """The sweep of a monitor pass and the NEXT train pass's draws (module docstring, STEADY STATE): ``iterate(2, [e0 .. e3])`` at learning_rate = 0."""
    from clonealign_amd.engine import HipEngine
    c = CASES[name]
    case, S0, eps = build(name)
    fc = lr.fit_constants(case)
    eng = HipEngine(**case, **dict(c["opts"], learning_rate=0.0))
    try:
        info = eng.info()
        got = {k: info[k] for k in c["expect"]}
        assert got == c["expect"], (name, got, c["expect"])
        assert info["fused_sweep"] == 1, info
        for n in sr.VAR_NAMES:
            eng.set(n, S0[n])
        eng.iterate(2, eps)
        g, nxt = eng.last_gradients(), eng.get_state()
    finally:
        eng.close()
    for n in sr.VAR_NAMES:
        assert np.array_equal(nxt[n].reshape(S0[n].shape), S0[n]), n             # no step moved anything: every pass of the call was at S0
    ref2, sc2 = lr.ref_gradients(fc, S0, eps[2])
    ref3, sc3 = lr.ref_gradients(fc, S0, eps[3])
    fig = {}
    for n in sr.VAR_NAMES:
        ref, sc = (ref2, sc2) if n in TRAIN_VARS else (ref3, sc3)
        assert g[n].shape == ref[n].shape, (n, g[n].shape, ref[n].shape)
        fig[n] = sr.worst_ratio(g[n], ref[n], sc[n])
    fam = family(name)
    for n, r in sorted(fig.items()):
        print(f"loop_grad steady {name} {n} {r:.3e} (bar {bar(fam, n):.2e}, model {MODEL[fam][n]:.2e})")
    bad = {n: (r, bar(fam, n)) for n, r in fig.items() if not r <= bar(fam, n)}
    assert not bad, (name, bad)


def test_every_bar_is_at_most_the_projects_gradient_bound():
    assert set(MODEL) == {family(n) for n in CASES} | {"handover/bins_32", "handover/too_wide"}
    for group, row in MODEL.items():
        assert set(row) == set(sr.VAR_NAMES), group
        for n in sr.VAR_NAMES:
            assert 0.0 <= bar(group, n) <= HARD, (group, n)


# ------------------------------------------------------------------------------------------------------------------ the series form's handed-over passes
def _too_wide():
    """bins_32's problem in a state no 32 bins cover: max |psi| = 8 against loadings over [-8.5, 8.5] (8 x 17 = 136 > 128, ca_poly_covers) -- the sweeps from the start."""
    case, st = sr.build_state("bins_32")
    G = case["Y"].shape[1]
    W = lr.f32(np.random.default_rng(3).uniform(-8.5, 8.5, size=G))
    W[G // 2], W[G - 1] = -8.5, 8.5
    st["W"] = W.reshape(G, 1)
    return case, st


@pytest.mark.parametrize("stream", ["picked", "y4"])
@pytest.mark.parametrize("state", ["bins_32", "too_wide"])
def test_passes_the_series_form_hands_to_the_sweeps_apply_the_float64_gradient(state, stream):
    """A series engine whose look ahead (ca_poly_covers) gives a pass to the sweeps runs the 4-bit riding body of k_fwd_cell_mix_ys and k_bwd_mfma for it:
    bins_32's second train pass (tests/test_gpu_series_grad.py leaves exactly that one uncompared) and both train passes of a state too wide from the start.
    The TRAIN variables of exactly those passes, per element.  "picked": the 1-byte image the pick rule takes for these counts (more than 1 in 256 is >= 15);
    "y4": the 4-bit image forced, the handed-over pass on its riding body."""
    from clonealign_amd.engine import HipEngine
    case, S0 = sr.build_state("bins_32") if state == "bins_32" else _too_wide()
    G = case["Y"].shape[1]
    consts, sb = sr.poly_constants(), sr.poly_step_bound()
    psi0, W0 = S0["psi"].reshape(-1), S0["W"].reshape(-1)
    xmax, vlo, vhi = float(np.abs(psi0).max()), float(W0.min()), float(W0.max())
    fc = lr.fit_constants(case)
    eps = np.stack([eps_for(1, G, 900 + i) for i in range(4)])
    eng = HipEngine(**case, variant_on=("series",) + (("y4",) if stream == "y4" else ()))
    fig = {}
    try:
        info = eng.info()
        assert (info["fwd_series"], info["fwd_cell"], info["fwd_mfma"], info["bwd_mfma"], info["y_ride"], info["y_storage_name"]) == (1, 1, 1, 1, 1, "u8"), info
        assert info["y_stream_bits"] == (4 if stream == "y4" else 8), info
        for n in sr.VAR_NAMES:
            eng.set(n, S0[n])
        st, steps_before = S0, 0
        for it in (1, 2):
            i0 = eng.info()
            eng.iterate(1, eps[2 * it - 2:2 * it])
            i1 = eng.info()
            want = [sr.poly_covers(xmax, vlo, vhi, steps_before, sb, consts), sr.poly_covers(xmax, vlo, vhi, steps_before + 1, sb, consts)]
            rise, fell = i1["series_passes"] - i0["series_passes"], i1["series_fallbacks"] - i0["series_fallbacks"]
            assert (rise, fell) == (sum(want), 2 - sum(want)), (state, it, rise, fell, want)
            g, nxt = eng.last_gradients(), eng.get_state()
            if not want[0]:                               # the train pass of this call was the sweeps'
                ref, sc = lr.ref_gradients(fc, st, eps[2 * it - 2])
                for n in TRAIN_VARS:
                    assert g[n].shape == ref[n].shape, n
                    fig[(it, n)] = sr.worst_ratio(g[n], ref[n], sc[n])
            st, steps_before = nxt, 1
    finally:
        eng.close()
    for (it, n), r in sorted(fig.items()):
        print(f"loop_grad handover-{state}-{stream} it{it} {n} {r:.3e} (bar {bar('handover/' + state, n):.2e}, model {MODEL['handover/' + state][n]:.2e})")
    assert len(fig) == len(TRAIN_VARS) * (1 if state == "bins_32" else 2), sorted(fig)      # bins_32: the second train pass alone; too wide: both
    bad = {k: (r, bar("handover/" + state, k[1])) for k, r in fig.items() if not r <= bar("handover/" + state, k[1])}
    assert not bad, (state, bad)


def handover_model_ratios(state):
    case, st = sr.build_state("bins_32") if state == "bins_32" else _too_wide()
    fc = lr.fit_constants(case)
    e0 = eps_for(1, case["Y"].shape[1], 900)
    ref, sc = lr.ref_gradients(fc, st, e0)
    mod = lr.operand_model(fc, st, e0, "mfma")
    return {n: sr.worst_ratio(mod[n], ref[n], sc[n]) for n in sr.VAR_NAMES}
