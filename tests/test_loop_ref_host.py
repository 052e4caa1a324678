"""Host checks of the float64 reference the loop's gradient test compares against (tests/_loop_ref.py).  No GPU.

* against autodiff of the literal model (oracle/literal_torch.py, float64) for every (K, P, S, extra) combination tests/test_gpu_loop_grad.py uses and every kind
  of state: each element within 1e-10 x its scale;
* L = 0 entries: torch's xlogy has no finite derivative at (0, 0), the literal model's autodiff gives NaN there; the hand gradients of oracle/fused_numpy.py (held
  to the literal model in tests/test_oracle.py) stand in, same bound;
* at K = 1, P = 0, S = 1 against tests/_series_ref.py: gradients within 1e-13 x scale, scales within 1e-13 relative;
* the operand model differs from the reference by what its roundings are worth and no more (a bound from the number formats, not from an engine)."""
import numpy as np
import pytest

from tests import _loop_ref as lr
from tests import _series_ref as sr
from tests._cases import eps_for

# (K, P, S, extra) of tests/test_gpu_loop_grad.py's families, at shapes small enough for the literal model's [S, G, C, N] tensors
COMBOS = {
    "k1": dict(K=1), "k1p1": dict(K=1, P=1), "k2": dict(K=2), "k2p1": dict(K=2, P=1), "k2p2": dict(K=2, P=2), "k3p2": dict(K=3, P=2), "k0": dict(K=0), "k0p1": dict(K=0, P=1),
    "k1s2": dict(K=1, S=2), "k1s3": dict(K=1, S=3), "k2p1s2x": dict(K=2, P=1, S=2, extra=True), "k1x": dict(K=1, extra=True),
}


def _literal(case, st):
    import torch
    from oracle.literal_torch import LiteralModel
    m = LiteralModel(**case)
    for n in sr.VAR_NAMES:
        setattr(m, n, torch.tensor(np.asarray(st[n], dtype=np.float64), dtype=torch.float64))
    return m


@pytest.mark.parametrize("kind", lr.STATE_KINDS)
@pytest.mark.parametrize("combo", list(COMBOS))
def test_reference_gradients_agree_with_autodiff(combo, kind):
    kw = COMBOS[combo]
    case, st = lr.build_state(kind, 40 + list(COMBOS).index(combo), N=53, G=37, C=9 if combo == "k1" else 4, **kw)
    S, G = kw.get("S", 1), 37
    for a in st.values():
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))
    fc = lr.fit_constants(case)
    eps = eps_for(S, G, 5)
    gr, sc = lr.ref_gradients(fc, st, eps)
    if kind == "zero_L":
        from oracle.fused_numpy import FusedModel
        assert (case["L"] == 0).any() and not np.any((case["L"][None] == 0) & (case["Y"][:, :, None] > 0))
        go, _ = sr.state_for(FusedModel, case, st).gradients(eps)
    else:
        go = {n: g.numpy() for n, g in _literal(case, st).gradients(eps)[0].items()}
    assert set(gr) == set(sr.VAR_NAMES)
    for n in sr.VAR_NAMES:
        assert gr[n].shape == sc[n].shape == go[n].shape, (n, gr[n].shape, go[n].shape)
        assert (sc[n] >= np.abs(gr[n]) * (1 - 1e-12)).all(), n                     # a scale is never below the magnitude of what it scales
        r = sr.worst_ratio(go[n], gr[n], sc[n])
        assert r <= 1e-10, (combo, kind, n, r)
    if kw["K"] == 0:
        assert fc["D"] == 0 and gr["beta"].shape == (G, kw.get("P", 0)) and not gr["beta"].any()   # K = 0 switches the covariates off too


def test_fractional_copy_numbers_agree_with_autodiff():
    case, st = lr.build_state("generic", 77, N=53, G=37, C=5, K=1)
    case["L"] = case["L"] + np.random.default_rng(5).random(case["L"].shape) * 0.9
    eps = eps_for(1, 37, 5)
    gr, sc = lr.ref_gradients(lr.fit_constants(case), st, eps)
    go = _literal(case, st).gradients(eps)[0]
    for n in sr.VAR_NAMES:
        assert sr.worst_ratio(go[n].numpy(), gr[n], sc[n]) <= 1e-10, n


@pytest.mark.parametrize("name", ["five_bins", "bins_32", "equal_p_x8"])
def test_reference_reproduces_the_series_reference(name):
    case, st = sr.build_state(name, n_cu=1)
    eps = eps_for(1, case["Y"].shape[1], 5)
    g1, s1 = sr.ref_gradients(sr.fit_constants(case["Y"], case["L"]), st, eps[0])
    g2, s2 = lr.ref_gradients(lr.fit_constants(case), st, eps)
    for n in sr.VAR_NAMES:
        assert g1[n].shape == g2[n].shape, n
        assert sr.worst_ratio(g2[n], g1[n], s1[n]) <= 1e-13, (n, sr.worst_ratio(g2[n], g1[n], s1[n]))
        assert sr.worst_ratio(s2[n], s1[n], s1[n]) <= 1e-13, n


@pytest.mark.parametrize("family", ["mfma", "mfma_frac", "valu"])
def test_operand_model_is_worth_its_roundings(family):
    """Float32 operands are good to 2^-24, the matrix cores' split products to 2^-16 (two 8-bit parts, the lo * lo product dropped): the model may differ from the
    reference by a few of those per element and must differ at all (or it models nothing)."""
    case, st = lr.build_state("wide", 9, N=70, G=40, C=4, K=2, P=1)
    if family == "mfma_frac":
        case["L"] = case["L"] + np.random.default_rng(5).random(case["L"].shape) * 0.9
    fc = lr.fit_constants(case)
    eps = eps_for(1, 40, 3)
    g, sc = lr.ref_gradients(fc, st, eps)
    m = lr.operand_model(fc, st, eps, family)
    top = 2.0 ** -16 if family != "valu" else 2.0 ** -20        # (|eta| <= 32: the float32 exponent alone is worth 32 x 2^-24 = 2^-19 in E)
    for n in ("W", "psi", "beta", "loc", "ls", "gamma_logits"):
        r = sr.worst_ratio(m[n], g[n], sc[n])
        assert 0.0 < r <= top, (family, n, r)
    for n in ("v", "alpha_unconstr"):
        assert sr.worst_ratio(m[n], g[n], sc[n]) <= 2.0 ** -24, n   # no sweep behind them: the float32 store alone


def _groups():
    from tests import test_gpu_loop_grad as t
    return sorted(t.MODEL)


@pytest.mark.parametrize("fam", _groups())
def test_the_bars_of_the_gpu_test_are_the_operand_models_figures(fam):
    """tests/test_gpu_loop_grad.py's MODEL table is what ``operand_model`` gives on the CPU for each family's cases (family = kernel group / kind of state) -- no
    engine has a say in it.  Every row is recomputed from every case that makes it (the balanced sweep's four 4316 x 3100 x 8 cases take 6 s each)."""
    from tests import test_gpu_loop_grad as t
    if fam.startswith("handover/"):
        rows = [t.handover_model_ratios(fam.split("/")[1])]
    else:
        names = [n for n in t.CASES if t.family(n) == fam]
        assert names, fam
        rows = [t.model_ratios(n) for n in names]
    for n in sr.VAR_NAMES:
        got, want = max(r[n] for r in rows), t.MODEL[fam][n]
        assert abs(got - want) <= 2e-3 * want + 1e-14, (fam, n, got, want)      # (1e-14: the exact states' ls stands at float64's own rounding, 1e-16)
        if n in ("v", "alpha_unconstr"):           # the two variables of K and C elements: the model taken at least at the float32 store's half ulp
            assert t.bar(fam, n) == min(2e-5, 8.0 * max(want, 2.0 ** -24))
        elif fam.endswith("/exact"):               # no operand error in the model: at least what a float32 sum of G (psi, d logits) or N terms is worth
            dims = [t.CASES[c]["shape"] for c in t.CASES if t.family(c) == fam]
            terms = max(d["G" if n in ("psi", "gamma_logits") else "N"] for d in dims)
            assert t.bar(fam, n) == min(2e-5, max(8.0 * want, np.sqrt(terms) * 2.0 ** -24))
        else:
            assert t.bar(fam, n) == min(2e-5, 8.0 * want)


def test_the_exact_state_is_what_it_is_named_for():
    """E = 1, mu L in one bf16 part, Z an integer (tests/_loop_ref.py::build_state): the matrix-core model is left with float32 roundings alone, and the same
    model with coef cut to two bf16 parts stands above the exact families' psi bar in every case that carries the kind."""
    from tests import test_gpu_loop_grad as t
    names = [n for n in t.CASES if t.CASES[n]["kind"] == "exact"]
    assert sorted(t.CASES[n]["group"] for n in names) == ["c16", "cell16", "d2", "d34", "s2"]
    parts = lr.bf16_parts
    for name in names:
        case, st, eps = t.build(name)
        fc = lr.fit_constants(case)
        mu = lr.f32(lr.softplus(st["loc"] + np.exp(st["ls"]) * eps[0]))
        M = mu[:, :, None] * fc["L"][None]
        assert np.array_equal(M, lr.bf16(M)) and np.array_equal(mu, np.broadcast_to(st["loc"], mu.shape)), name
        ref, sc = lr.ref_gradients(fc, st, eps[0])
        try:
            lr.bf16_parts = lambda a, n: parts(a, min(n, 2))
            two = lr.operand_model(fc, st, eps[0], "mfma")
        finally:
            lr.bf16_parts = parts
        r = sr.worst_ratio(two["psi"], ref["psi"], sc["psi"])
        assert r > 2.0 * t.bar(t.family(name), "psi"), (name, r, t.bar(t.family(name), "psi"))
