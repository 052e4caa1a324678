"""The Python side of the scoring calls: the engine lease closes what it built and nothing else, unnamed clones are named beyond the 26 letters, and
``assignment_support`` returns ``assign_cells``'s answer bit for bit.  No GPU: a fake engine class stands in for ``HipEngine`` and falls to the host forms."""
import numpy as np
import pytest

from clonealign_amd import api
from clonealign_amd import engine as engine_mod

N, G, C = 12, 9, 3


class FakeEngine:
    """What ``HipEngine`` is to the lease -- a constructor on (Y, L, psi0, loc0, K), ``N``, ``G`` and ``close`` -- without a scoring method."""
    built = []

    def __init__(self, Y, L, psi0, loc0, K, **opts):
        self.N, self.G = Y.shape
        self.closed = 0
        FakeEngine.built.append(self)

    def close(self):
        self.closed += 1


@pytest.fixture
def fake(monkeypatch):
    FakeEngine.built = []
    monkeypatch.setattr(engine_mod, "HipEngine", FakeEngine)
    return FakeEngine


def problem(n=N, g=G, c=C, K=1, seed=0):
    rng = np.random.default_rng(seed)
    L = rng.integers(1, 5, size=(g, c)).astype(np.float64)
    Y = rng.poisson(2.0, size=(n, g)).astype(np.int32)
    Y[:, 0] += 1
    ml = {"mu": rng.lognormal(0.0, 0.3, g), "alpha": rng.dirichlet(np.ones(c) * 3.0)}
    if K:
        ml["W"] = rng.normal(size=(g, K)) * 0.2
    return {"ml_params": ml}, Y, L, np.log(rng.dirichlet(np.ones(c), size=n))


BLOCKS = ["a"] * 4 + ["b"] * 5
# (name, call(fit, Y, L, **kw), keywords of a refusal that fires only once the engine exists); None: a copy-number table whose first clone has
# E = 0 in every gene, which the host form of every call refuses.
BAD_EXTRA = {"extra_loglik": np.zeros((N, C + 1))}
CALLS = [
    ("clone_loglik", lambda f, Y, L, **kw: api.clone_loglik(f, Y, L, **kw), None),
    ("assign_cells", lambda f, Y, L, **kw: api.assign_cells(f, Y, L, **kw), BAD_EXTRA),
    ("clone_loglik_by_block", lambda f, Y, L, **kw: api.clone_loglik_by_block(f, Y, L, BLOCKS, **kw), None),
    ("assignment_support", lambda f, Y, L, **kw: api.assignment_support(f, Y, L, BLOCKS, **kw), BAD_EXTRA),
    ("clone_pair_loglik", lambda f, Y, L, **kw: api.clone_pair_loglik(f, Y, L, **kw), None),
    ("detect_doublets", lambda f, Y, L, **kw: api.detect_doublets(f, Y, L, **kw), None),
    ("clone_loglik_dm", lambda f, Y, L, **kw: api.clone_loglik_dm(f, Y, L, concentration=(10.0, 100.0), **kw), None),
    ("estimate_concentration", lambda f, Y, L, **kw: api.estimate_concentration(f, Y, L, grid=(10.0, 100.0, 1000.0), refine=1, **kw), BAD_EXTRA),
    ("assign_cells_dm", lambda f, Y, L, **kw: api.assign_cells_dm(f, Y, L, 50.0, **kw), BAD_EXTRA),
    ("assign_cells_dm auto", lambda f, Y, L, **kw: api.assign_cells_dm(f, Y, L, "auto", grid=(10.0, 100.0, 1000.0), refine=1, **kw), BAD_EXTRA),
    ("project_cells", lambda f, Y, L, **kw: api.project_cells(f, Y, L, max_iter=3, **kw), {"tol": 0.0}),
    ("clone_evidence", lambda f, Y, L, **kw: api.clone_evidence(f, Y, L, max_iter=3, **kw), {"psi_start": np.zeros(N + 1)}),
    ("assign_cells_marginal", lambda f, Y, L, **kw: api.assign_cells_marginal(f, Y, L, max_iter=3, **kw), BAD_EXTRA),
    ("heldout_evidence", lambda f, Y, L, **kw: api.heldout_evidence({"k1": f, "k0": problem(K=0)[0]}, Y, L, max_iter=3, **kw), BAD_EXTRA),
]


@pytest.mark.parametrize("name,call,late", CALLS, ids=[c[0] for c in CALLS])
def test_the_lease_closes_the_engine_it_built_and_only_that(fake, name, call, late):
    fit, Y, L, _lp = problem()
    call(fit, Y, L)                                                  # clean: one throwaway engine, closed once
    assert [e.closed for e in fake.built] == [1]
    fake.built.clear()
    with pytest.raises(ValueError):                                  # a refusal after the engine exists closes it all the same
        if late is None:
            dead = L.copy()
            dead[:, 0] = 0.0
            call(fit, Y, dead)
        else:
            call(fit, Y, L, **late)
    assert [e.closed for e in fake.built] == [1]
    fake.built.clear()
    with pytest.raises(ValueError, match="rows .genes."):            # a refusal before the engine exists builds none
        call(fit, Y, L[:-1])
    assert fake.built == []
    mine = FakeEngine(Y, L, None, None, 0)                           # the caller's engine is used and never closed, whether the call returns or raises
    fake.built.clear()
    call(fit, Y, L, engine=mine)
    with pytest.raises(ValueError):
        bad = L.copy()
        bad[:, 0] = 0.0
        call(fit, Y, bad, engine=mine)
    assert mine.closed == 0 and fake.built == []


def test_the_lease_refuses_an_engine_of_another_shape_for_its_method():
    fit, Y, L, _lp = problem()

    class Other:
        N, G = N + 1, G

        def clone_loglik(self, *a, **k):
            raise AssertionError("not to be called")
    with pytest.raises(ValueError, match=f"the engine holds a {N + 1} x {G} matrix but Y is {N} x {G}"):
        api.clone_loglik(fit, Y, L, engine=Other())


@pytest.mark.parametrize("c", [26, 27])
def test_unnamed_clones_are_numbered_beyond_the_letters(fake, c):
    fit, Y, L, _lp = problem(n=6, g=5, c=c)
    letters = [f"clone_{ch}" for ch in "abcdefghijklmnopqrstuvwxyz"]
    want = letters if c == 26 else letters + ["clone_27"]
    pairs = c * (c - 1) // 2
    for out in (api.assign_cells(fit, Y, L), api.detect_doublets(fit, Y, L, weights=(0.5,)), api.project_cells(fit, Y, L, max_iter=2)):
        assert list(out["clone_names"]) == want
        assert set(out["clone"]) <= set(want) | {"unassigned", "doublet"}
        assert out["clone_probs"].shape == (6, c)
    assert api.detect_doublets(fit, Y, L, weights=(0.5,))["pair_probs"].shape == (6, pairs)
    named = dict(fit, clone_names=[f"k{i}" for i in range(c)])       # names the fit carries win, at any count
    assert list(api.assign_cells(named, Y, L)["clone_names"]) == [f"k{i}" for i in range(c)]


def test_assignment_support_returns_assign_cells_bit_for_bit(fake):
    fit, Y, L, lp = problem(n=40, g=9)
    Y[3, 2] = 5
    L[2, 1] = 0.0                                                    # a -inf entry takes part
    a = api.assign_cells(fit, Y, L, extra_loglik=lp)
    s = api.assignment_support(fit, Y, L, BLOCKS, extra_loglik=lp)
    for k in ("clone_probs", "loglik", "clone_loglik"):
        assert a[k].tobytes() == s[k].tobytes(), k
    assert list(a["clone"]) == list(s["clone"]) and list(a["clone_names"]) == list(s["clone_names"])
    # and the margins use the sum in the other association, ll + (log alpha + extra): equal to the first up to rounding only
    t = a["clone_loglik"] + (np.log(fit["ml_params"]["alpha"])[None, :] + lp)
    top = np.sort(np.where(np.isneginf(t), -np.inf, t), axis=1)
    np.testing.assert_array_equal(s["margin"], top[:, -1] - top[:, -2])
