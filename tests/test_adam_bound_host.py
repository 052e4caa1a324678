"""How far ONE TF1-Adam step can move a variable: the bound both look-aheads of the engine rest on -- the int8 count-matrix stream's lagged fixed-point exponents
(ca_engine::ys_step_bound) and the series form's range look-ahead (poly_step_bound -> ca_poly_covers, and in sharded fits the max |psi| every rank's bin geometry
is built from).  No GPU: a float64 TF1 Adam is fed the gradient sequences that make its step LARGEST -- a constant prefix (v settles, the bias correction runs
out), then gradients growing geometrically (m follows them faster than sqrt(v) does) -- and no step may exceed either bound, restated from the sources
(tests/_series_ref.py: adam_step_bound, step_bound_margins).

Measured here at the defaults (lr 0.1, beta1 0.9, beta2 0.999): the rigorous bound is 0.7270 (ys_step_bound carries 2 % on top: 0.742; poly_step_bound 1e-4);
the largest step over all sequences comes within 1 % of it (printed by the test).  max(lr, lr (1 - beta1) / sqrt(1 - beta2)) = 0.316, which poly_step_bound used
to return with the comment "no Adam step moves a variable further", is passed within 20 steps of growth by beta2 / beta1 behind 500 constant gradients (7 at a factor of 1.5)."""
import math

import numpy as np
import pytest

from tests import _series_ref as sr

LR, B1, B2, AEPS = 0.1, 0.9, 0.999, 1e-8
PREFIXES = (0, 50, 500, 5000)
FACTORS = (B2 / B1, 1.2, 1.5, 2.0, 3.0, 10.0)


def adam_steps(grads, lr=LR, b1=B1, b2=B2, aeps=AEPS):
    """|step| of every TF1 Adam update (epsilon outside the bias correction, oracle/literal_torch.py) along one scalar gradient sequence, float64."""
    m = v = 0.0
    p1 = p2 = 1.0
    out = np.empty(len(grads))
    for i, g in enumerate(grads):
        p1 *= b1
        p2 *= b2
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        out[i] = abs(lr * math.sqrt(1.0 - p2) / (1.0 - p1) * m / (math.sqrt(v) + aeps))
    return out


def sequence(prefix, factor, sign, grow_sign):
    n_grow = min(400, int(140.0 / math.log10(factor)))      # (g^2 stays finite in float64)
    return np.concatenate([np.full(prefix, float(sign)), grow_sign * sign * factor ** np.arange(1, n_grow + 1)])


def test_the_restated_bounds_are_the_sources():
    mp, my = sr.step_bound_margins()
    assert mp >= 1.0 and my >= 1.0
    b = sr.adam_step_bound(LR, B1, B2)
    assert abs(b - 0.727) < 1e-3, b                          # (the figure the sources' comments state)
    assert sr.poly_step_bound() == b * mp and abs(sr.ys_step_bound() - b * my) <= 1e-7
    assert sr.adam_step_bound(0.1, 0.9, 0.8) < 0             # beta1^2 >= beta2: no bound, and both uses know (ys: no lagged exponents; poly: no step counted on)


@pytest.mark.parametrize("prefix", PREFIXES)
def test_no_adam_step_exceeds_the_bound_the_look_aheads_use(prefix):
    bounds = {"poly_step_bound": sr.poly_step_bound(LR, B1, B2), "ys_step_bound": sr.ys_step_bound(LR, B1, B2)}
    old = max(LR, LR * (1.0 - B1) / math.sqrt(1.0 - B2))
    worst, first_over_old = 0.0, {}
    for factor in FACTORS:
        for sign in (1.0, -1.0):
            for grow_sign in (1.0, -1.0):
                st = adam_steps(sequence(prefix, factor, sign, grow_sign))
                worst = max(worst, float(st.max()))
                over = np.nonzero(st[prefix:] > old)[0]
                if over.size:
                    first_over_old[(round(factor, 3), sign, grow_sign)] = int(over[0]) + 1
                for name, b in bounds.items():
                    assert st.max() <= b, (name, b, prefix, factor, sign, grow_sign, float(st.max()), int(st.argmax()))
    print(f"adam_bound prefix {prefix}: largest step {worst:.4f}; bounds {bounds}; growth steps until a step passes {old:.3f}, by factor: "
          f"{ {k[0]: v for k, v in first_over_old.items() if k[1:] == (1.0, 1.0)} }")
    if prefix >= 500:
        # the sequences are sharp enough to tell a bound from a non-bound: behind a settled prefix the step passes 0.316 within 25 steps of growth by beta2 / beta1
        assert worst > old * 1.3, worst
        assert first_over_old[(round(B2 / B1, 3), 1.0, 1.0)] <= 25
    if prefix >= 5000:
        assert worst > 0.95 * sr.adam_step_bound(LR, B1, B2), worst          # (the bias correction has run out: within 5 % of the rigorous bound)


def test_other_adam_settings_keep_their_bound():
    for lr, b1, b2 in ((0.01, 0.9, 0.999), (0.1, 0.5, 0.9), (0.3, 0.0, 0.99), (0.1, 0.95, 0.9999)):
        b = sr.adam_step_bound(lr, b1, b2)
        assert b > 0
        for prefix in (0, 500):
            for factor in ((b2 / b1) if b1 > 0 else 4.0, 2.0, 10.0):
                for gs in (1.0, -1.0):
                    st = adam_steps(sequence(prefix, factor, 1.0, gs), lr, b1, b2)
                    assert st.max() <= b * (1 + 1e-12), (lr, b1, b2, prefix, factor, gs, float(st.max()), b)
