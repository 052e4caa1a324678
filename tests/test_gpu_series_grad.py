"""The gradients the SERIES form applies (clonealign_amd/csrc/ca_poly.hip, ca_polymom.hip.h), against float64, element by element.

``HipEngine.gradients()`` goes through the plain kernels; the series form runs only inside ``iterate`` / ``run``.  But the update launches store the gradient
they apply (ca_final_gene_step: loc, ls, W; ca_psi_adam_body_at: psi; the cell epilogue: d gamma_logits; the O(K + C) body: v, alpha_unconstr), and
``HipEngine.last_gradients()`` reads those buffers without running anything.  After ``iterate(1, eps[0:2])`` from a state S0 they hold gradients that went
through k_poly_B / the riding moment role, k_poly_cell, k_poly_red and k_poly_gene.  Which state and draw each buffer belongs to, from ca_iterate's code:

* ``iterate(1, [e0, e1])`` with exactly two draws carries no half over.  It queues fused_pass(e0, e0) at S0 (the first series pass: decided from S0's exact
  ranges, zero steps), the train pass (backward half and update with e0: loc, ls, W, psi <- gradient at (S0, e0), then the step to S1), and the monitor pass
  fused_pass(e1, e1) at S1 -- its own draw in both halves (the second series pass: S0's ranges plus one step's bound); ca_iterate ends with flush_mon_tail.
* the monitor pass's cell epilogue rewrites d gamma_logits: that buffer belongs to (S1, e1).  (With one draw more than 2 n it would belong to the carried draw.)
* the O(K + C) body runs once more as the monitor pass's tail (apply = 0) and stores g_v and g_a unconditionally: after the call they belong to S1 as well
  (neither depends on the draw; g_a is made of the monitor pass's sum of gamma over the cells).  The returned ELBO is the one at (S1, e1).

Every comparison is ``|engine - reference| <= tol * scale`` for EVERY element, the scale being the sum of the magnitudes of the element's summands
(tests/_series_ref.py).  A second ``iterate(1, eps[2:4])`` repeats the comparison from S1: after a ``set`` the first pass takes k_poly_xmax and the moments' own
launches, the passes after an update take max|psi| from the merged update and ride on the count-matrix stream's launch.

TOLERANCES: 8 x the largest |engine - reference| / scale observed on an MI355X over all cases, per variable (profiles/r13_series_grad.txt has the table per
case).  What limits agreement is float32 on the way in and out (mu and coef stored as float, the gradients stored as float), not the series (<= 3e-14 in
float64, tests/test_series_ref_host.py).

Measured (largest ratio over all elements and both iterations; elbo relative to |ELBO|):

case                              loc           ls            W          psi            v alpha_uncons gamma_logits         elbo
one_bin                      4.49e-08     4.25e-08     5.34e-08     6.14e-08     2.81e-09     2.35e-09     1.03e-09     1.12e-09
two_bins                     4.16e-08     4.38e-08     8.46e-08     7.37e-08     1.77e-08     6.87e-10     8.11e-10     2.42e-09
four_bins                    4.50e-08     5.28e-08     9.19e-08     7.50e-08     3.81e-09     1.95e-09     5.61e-10     1.25e-10
five_bins                    4.62e-08     4.56e-08     1.48e-07     8.71e-08     1.38e-09     5.07e-09     1.23e-09     5.21e-10
nine_bins                    4.33e-08     4.15e-08     7.89e-08     1.08e-07     2.29e-08     2.00e-09     1.04e-09     1.34e-09
bins_32                      3.97e-08     4.92e-08     9.20e-08     7.40e-08     2.34e-08     5.88e-09     1.51e-07     1.42e-08
equal_0_x3                   3.91e-08     4.22e-08     3.00e-08     3.13e-08     3.64e-08     1.08e-09     9.98e-10     2.13e-09
equal_0_x8                   4.66e-08     4.03e-08     3.66e-08     4.21e-08     5.44e-08     9.38e-10     1.41e-09     4.79e-09
equal_0_x11                  3.49e-08     4.56e-08     5.76e-08     5.20e-08     1.27e-08     1.75e-09     1.18e-09     4.39e-09
equal_p_x3                   3.74e-08     3.60e-08     1.45e-08     5.07e-08     6.68e-09     5.52e-10     1.20e-09     9.77e-10
equal_p_x8                   3.47e-08     3.73e-08     3.40e-08     4.31e-08     8.53e-09     4.99e-09     3.89e-09     3.34e-09
equal_p_x11                  3.68e-08     2.99e-08     4.61e-08     4.51e-08     2.60e-09     4.25e-09     4.38e-09     1.47e-08
two_pass_c8                  4.33e-08     5.50e-08     7.99e-08     1.02e-07     7.42e-09     5.77e-09     1.54e-09     3.90e-09
two_pass_c4                  4.89e-08     4.68e-08     8.39e-08     1.19e-07     1.89e-08     1.82e-09     1.88e-09     2.43e-09
five_bins/as_they_were       4.62e-08     4.56e-08     1.48e-07     8.71e-08     1.38e-09     5.07e-09     1.23e-09     5.21e-10
largest                      4.89e-08     5.50e-08     1.48e-07     1.19e-07     5.44e-08     5.88e-09     1.51e-07     1.47e-08
tol = 8 x largest            3.91e-07     4.40e-07     1.19e-06     9.52e-07     4.35e-07     4.71e-08     1.21e-06     1.18e-07

bins_32: its monitor passes and its second train pass fall to the matrix-core sweeps, as ca_poly_covers predicts (hence gamma_logits at 1.5e-7).  Before the
zero-width geometry was fixed (one bin centred 0.5 above the common loading) psi of the equal_* cases stood at 0 / 2.0e-4 / 3.5e-1 (W = 0, max|psi| = 3 / 8 /
11) and 3.0e-8 / 7.9e-6 / 2.0e-2 (W = 0.75).
"""
import numpy as np
import pytest

from tests import _series_ref as sr
from tests._cases import eps_for

pytestmark = pytest.mark.gpu

TRAIN_VARS = ("loc", "ls", "W", "psi")          # stored by the train pass's update launches: (state before the step, the train draw)
TAIL_VARS = ("v", "alpha_unconstr")              # stored last by the monitor pass's tail: the state after the step
OBSERVED = {"loc": 4.889e-08, "ls": 5.503e-08, "W": 1.482e-07, "psi": 1.190e-07, "v": 5.441e-08, "alpha_unconstr": 5.883e-09, "gamma_logits": 1.507e-07,
            "elbo": 1.473e-08}
TOL = {n: 8.0 * r for n, r in OBSERVED.items()}
assert max(TOL.values()) <= 2e-5      # the project's own gradient bound (tests/test_gpu_parity.py), here per element: anything above it is a finding

_N_CU = []


def _n_cu():
    if not _N_CU:
        from clonealign_amd.engine import HipEngine
        from tests._cases import make_case
        probe = HipEngine(**make_case(seed=1, N=64, G=32, C=3, K=1))
        try:
            _N_CU.append(probe.info()["n_cu"])
        finally:
            probe.close()
    return _N_CU[0]


def _probe(name, variant_off=()):
    """One engine, two iterations, every figure: {(phase, variable): worst |engine - reference| / scale}.  Asserts the preconditions and the path taken."""
    from clonealign_amd.engine import HipEngine
    from oracle.fused_numpy import FusedModel
    spec = sr.SPECS[name]
    case, S0 = sr.build_state(name, _n_cu() if spec["N"] is None else None)
    G = case["Y"].shape[1]
    consts = sr.poly_constants()
    # the inputs are what the case is named for (a check of the test's own arrays, on the CPU)
    assert sr.expected_bins(S0, consts) == spec["nb"], (name, sr.expected_bins(S0, consts))
    psi0, W0 = S0["psi"].reshape(-1), S0["W"].reshape(-1)
    assert psi0[0] == 0.0 and psi0.max() == -psi0.min() == np.float32(spec["xmax"])
    xmax, vlo, vhi, sb = float(np.abs(psi0).max()), float(W0.min()), float(W0.max()), sr.poly_step_bound()
    assert sr.poly_covers(xmax, vlo, vhi, 0, sb, consts), name                     # the first pass after a set decides at the exact ranges
    fc = sr.fit_constants(case["Y"], case["L"])
    eps = np.stack([eps_for(1, G, 900 + i) for i in range(4)])
    eng, ora = HipEngine(**case, variant_on=("series",), variant_off=variant_off), FusedModel(**case, dtype="float64")
    fig = {}

    def compare(phase, names, got, st, e):
        ref, sc = sr.ref_gradients(fc, st, e[0])
        for n in names:
            assert got[n].shape == ref[n].shape, (n, got[n].shape)
            fig[(phase, n)] = sr.worst_ratio(got[n], ref[n], sc[n])

    def load(st):
        for n in sr.VAR_NAMES:
            setattr(ora, n, np.asarray(st[n], dtype=np.float64).copy())

    try:
        info = eng.info()
        assert info["fwd_series"] == 1 and info["mom_ride"] == int("mom_ride" not in variant_off) and info["cell_lean"] == int("cell_lean" not in variant_off), info
        for n in sr.VAR_NAMES:
            eng.set(n, S0[n])
        st = S0
        steps_before = 0        # Adam steps between the ranges the look ahead decides from (S0's, queued by the first pass after the set) and the pass
        for it in (1, 2):
            i0 = eng.info()
            e = eng.iterate(1, eps[2 * it - 2:2 * it])
            i1 = eng.info()
            # passes of this call: iteration 1 -- the forward half at the exact ranges, then the monitor pass one step on; iteration 2 -- one and two steps on
            want = [sr.poly_covers(xmax, vlo, vhi, steps_before, sb, consts), sr.poly_covers(xmax, vlo, vhi, steps_before + 1, sb, consts)]
            rise, fell = i1["series_passes"] - i0["series_passes"], i1["series_fallbacks"] - i0["series_fallbacks"]
            assert (rise, fell) == (sum(want), 2 - sum(want)), (name, it, rise, fell, want)
            if it == 1:
                assert want[0] and rise >= 1            # the train pass of S0 ran the series form
            g = eng.last_gradients()
            nxt = eng.get_state()
            if want[0]:                                 # (a train pass the look ahead gave to the matrix-core sweeps is not this file's subject: tests/test_gpu_parity.py)
                compare(f"it{it}", TRAIN_VARS, g, st, eps[2 * it - 2])
            compare(f"it{it}", TAIL_VARS + ("gamma_logits",), g, nxt, eps[2 * it - 1])
            load(nxt)
            eo = ora.elbo(eps[2 * it - 1])
            fig[(f"it{it}", "elbo")] = abs(e - eo) / abs(eo)
            st = nxt
            steps_before = 1
        return fig
    finally:
        eng.close()


def _check(name, fig):
    for (phase, n), r in sorted(fig.items()):
        print(f"series_grad {name} {phase} {n} {r:.3e}")
    bad = {k: r for k, r in fig.items() if not r <= TOL[k[1]]}
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", list(sr.SPECS))
def test_series_train_pass_gradients_match_float64_per_element(name):
    fig = _probe(name)
    # every phase and variable was compared (the 32-bin state's second train pass alone may fall to the sweeps: ca_poly_covers one step on)
    need = 2 * (len(TRAIN_VARS) + len(TAIL_VARS) + 2) - (len(TRAIN_VARS) if name == "bins_32" else 0)
    assert len(fig) == need, sorted(fig)
    _check(name, fig)


def test_the_launches_as_they_were_match_float64_too():
    """k_poly_cell<CP, false> and the moments' own launches (CA_VAR_CELL_LEAN and CA_VAR_MOM_RIDE off) against float64, not only against their twins."""
    fig = _probe("five_bins", variant_off=("cell_lean", "mom_ride"))
    assert len(fig) == 2 * (len(TRAIN_VARS) + len(TAIL_VARS) + 2)
    _check("five_bins/as_they_were", fig)
