"""Host checks of the float64 reference the series form's GPU test compares against (tests/_series_ref.py), and of the series algorithm's own accuracy claim
("remainder below 1e-11", ca_poly.hip) with the constants ca_poly.h defines.  No GPU.

Measured here (float64, numpy): the restated algorithm misses the direct contraction by at most 3e-14 of scale (q' at four bins; 4e-15 at 32), over two decades inside
the claim.  With the centre of a zero-width range half a bin off its genes (delta = 1, vlo = the common loading: the geometry before this test existed) the same
restatement misses Z of a cell with psi = 8 by 4e-6 and with psi = 11 by 1e-2: ``test_a_zero_width_bin_must_be_centred_on_its_genes`` keeps that on record."""
import numpy as np
import pytest

from tests import _series_ref as sr
from tests._cases import eps_for

HOST_STATES = [n for n in sr.SPECS if not n.startswith("two_pass")] + ["two_pass_c8"]


def _state(name):
    return sr.build_state(name, n_cu=1)      # (two_pass_*: 231 cells here; the device's CU count sets the number on the GPU)


def test_constants_and_geometry_are_what_the_states_were_built_for():
    c = sr.poly_constants()
    assert c["CA_PL_R"] >= 1 and c["CA_PL_A"] > 0 and c["CA_PL_NB"] >= 32 and sr.genes_per_partial() == 32, c
    for name in HOST_STATES:
        _case, st = _state(name)
        assert sr.expected_bins(st, c) == sr.SPECS[name]["nb"], name
        psi, W = st["psi"].reshape(-1), st["W"].reshape(-1)
        assert psi[0] == 0.0 and psi.max() == -psi.min() == np.float32(sr.SPECS[name]["xmax"]), name
        for a in st.values():
            assert np.array_equal(a, a.astype(np.float32).astype(np.float64)), name
        vlo, delta, nb = sr.bin_geometry(float(np.abs(psi).max()), float(W.min()), float(W.max()), c)
        # the bound the expansion rests on: |x| times the largest distance of a gene from its bin's centre
        b = sr.bin_of(W, vlo, delta, nb)
        dv = W - (vlo + (b + 0.5) * delta)
        assert np.abs(psi).max() * np.abs(dv).max() <= c["CA_PL_A"] * (1 + 1e-12), (name, np.abs(psi).max() * np.abs(dv).max())
    assert any(sr.SPECS[n]["G"] % sr.genes_per_partial() == 1 for n in HOST_STATES)
    # genes exactly on vlo, on vhi (the clamp) and on every interior boundary of the four-bin state
    _case, st = _state("four_bins")
    W = st["W"].reshape(-1)
    assert all((W == e).any() for e in (-2.0, -1.0, 0.0, 1.0, 2.0))


@pytest.mark.parametrize("name", ["five_bins", "equal_p_x8"])
def test_reference_gradients_agree_with_the_oracle(name):
    from oracle.fused_numpy import FusedModel
    case, st = _state(name)
    G = case["Y"].shape[1]
    ora = sr.state_for(FusedModel, case, st)
    fc = sr.fit_constants(case["Y"], case["L"])
    eps = eps_for(1, G, 5)
    go, _elbo = ora.gradients(eps)
    gr, sc = sr.ref_gradients(fc, st, eps[0])
    assert set(gr) == set(FusedModel.VAR_NAMES)
    for n in FusedModel.VAR_NAMES:
        assert gr[n].shape == sc[n].shape == go[n].shape, n
        assert (sc[n] >= np.abs(gr[n]) * (1 - 1e-12)).all(), n          # a scale is never below the magnitude of what it scales
        r = sr.worst_ratio(go[n], gr[n], sc[n])
        assert r <= 1e-12, (n, r)


def _contraction_inputs(name):
    case, st = _state(name)
    fc = sr.fit_constants(case["Y"], case["L"])
    p = sr.forward_parts(fc, st, eps_for(1, case["Y"].shape[1], 6)[0])
    return p["x"], p["v"], p["M"], p["coef"], fc["L"], p["mu"]


@pytest.mark.parametrize("name", HOST_STATES)
def test_series_algorithm_in_float64_meets_its_claim(name):
    """B, Horner, Q, q and q' with CA_PL_R / CA_PL_A / CA_PL_NB as ca_poly.h has them: within 1e-11 of scale of the direct sums, element by element."""
    x, v, M, coef, L, mu = _contraction_inputs(name)
    ref, sc = sr.direct_contraction(x, v, M, coef, L, mu)
    got, geo = sr.series_contraction(x, v, M, coef, L, mu)
    assert geo["nb"] == sr.SPECS[name]["nb"], geo["nb"]
    if geo["nb"] > 1:
        assert set(geo["bin"]) == set(range(geo["nb"])) or geo["nb"] == 32, sorted(set(geo["bin"]))   # (97 genes cannot fill 32 bins: most of them, and both ends)
        assert geo["bin"].min() == 0 and geo["bin"].max() == geo["nb"] - 1
    worst = {k: sr.worst_ratio(got[k], ref[k], sc[k]) for k in ("Z", "dZ", "dmu", "dV")}
    print(name, "bins", geo["nb"], {k: f"{r:.2e}" for k, r in worst.items()})
    for k, r in worst.items():
        assert r <= 1e-11, (name, k, r)


def test_a_zero_width_bin_must_be_centred_on_its_genes():
    """What the tests above rest on at zero width: with the one bin's centre at the common loading + 0.5 the form evaluates exp(0.5 x) sum_{k <= R} (-0.5 x)^k / k!
    and nothing bounds |0.5 x| by CA_PL_A -- a cell with psi = 8 loses six digits of Z, one with psi = 11 all but two.  Centred on the genes it is exact."""
    off_centre = lambda xmax, mn, mx, c: (mn, 1.0, 1) if mx == mn else sr.bin_geometry(xmax, mn, mx, c)  # noqa: E731
    for name, least in (("equal_0_x8", 1e-6), ("equal_p_x11", 1e-3)):
        x, v, M, coef, L, mu = _contraction_inputs(name)
        ref, sc = sr.direct_contraction(x, v, M, coef, L, mu)
        bad, _ = sr.series_contraction(x, v, M, coef, L, mu, geometry=off_centre)
        good, _ = sr.series_contraction(x, v, M, coef, L, mu)
        assert sr.worst_ratio(bad["Z"], ref["Z"], sc["Z"]) >= least, name
        assert sr.worst_ratio(good["Z"], ref["Z"], sc["Z"]) <= 1e-14, name
