"""The Python side of the handle-free generative calls (``simulate_counts``, ``predictive_stats``, ``predictive_moments``): the one operand check they share
hands the library what it reads and refuses in the caller's name.  No GPU, no library."""
import numpy as np
import pytest

from clonealign_amd.engine import _model_operands

N, G, C, D = 5, 4, 3, 2
CALLERS = ("simulate_counts", "predictive_stats", "predictive_moments")


def operands(seed=0):
    rng = np.random.default_rng(seed)
    return rng.lognormal(size=(G, C)), rng.normal(size=(G, D)), rng.normal(size=(N, D)), rng.integers(0, C, N), rng.integers(0, 100, N)


@pytest.mark.parametrize("what", CALLERS)
def test_refusals_carry_the_callers_name(what):
    E, V, U, clone, total = operands()
    with pytest.raises(ValueError) as e:
        _model_operands(what, E[:, 0], V, U, clone, total)
    assert str(e.value) == f"{what}: E is ({G},); expected (genes, clones)"
    for u, v in ((U, None), (None, V)):
        with pytest.raises(ValueError) as e:
            _model_operands(what, E, v, u, clone, total)
        assert str(e.value) == f"{what}: U and V go together (both, or neither)"
    for u, v in ((U[:-1], V), (U, V[:-1]), (U[:, :1], V), (U[:, 0], V)):
        with pytest.raises(ValueError) as e:
            _model_operands(what, E, v, u, clone, total)
        assert str(e.value) == f"{what}: U is {u.shape} and V is {v.shape}; expected ({N}, D) and ({G}, D)"


def test_what_the_library_reads():
    E, V, U, clone, total = operands()
    Ef = np.asfortranarray(E)                                        # not C-contiguous
    assert not Ef.flags.c_contiguous
    out = _model_operands("x", Ef, V[:, ::-1], U.astype(np.float32), clone.astype(np.int64)[::-1], list(total))
    E2, V2, U2, clone2, total2 = out[:5]
    assert out[5:] == (N, G, C, D)
    for a, dt, shape in ((E2, np.float64, (G, C)), (V2, np.float64, (G, D)), (U2, np.float64, (N, D)), (clone2, np.int32, (N,)), (total2, np.int64, (N,))):
        assert a.dtype == dt and a.shape == shape and a.flags.c_contiguous
    assert np.array_equal(E2, E) and np.array_equal(V2, V[:, ::-1]) and np.array_equal(U2, U.astype(np.float32))
    assert np.array_equal(clone2, clone[::-1]) and np.array_equal(total2, total)


def test_scalar_total_is_every_cells():
    E, V, U, clone, _ = operands()
    total = _model_operands("x", E, V, U, clone, 3000)[4]
    assert total.dtype == np.int64 and total.shape == (N,) and total.flags.c_contiguous and np.all(total == 3000)


def test_without_factors():
    E, _, _, clone, total = operands()
    out = _model_operands("x", E, None, None, clone, total)
    assert out[1] is None and out[2] is None and out[5:] == (N, G, C, 0)
    out = _model_operands("x", E, np.zeros((G, 0)), np.zeros((N, 0)), clone, total)     # factors with no columns: the same call
    assert out[1] is None and out[2] is None and out[8] == 0
