"""The host's share of the 2-bit / 4-bit loop image (CA_VAR_Y2), without a GPU: ca_y2_plan -- the per-segment sort of the genes by their counts >= 3 (ties by index),
the escape list's length for N2 narrow blocks and the rule that picks N2 -- against its numpy restatement (tests/_y2_ref.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import _y2_ref as ref


def _plan(c3, c15, counts, force):
    from clonealign_amd import engine
    lib = engine.load_library()
    Gp = c3.size
    perm = np.zeros(Gp, np.uint16)
    pos = np.zeros(Gp, np.uint16)
    n_esc = C.c_int64(-1)
    c3 = np.ascontiguousarray(c3, np.int32)
    c15 = np.ascontiguousarray(c15, np.int32)
    fn = lib.ca_y2_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    n2 = fn(c3.ctypes.data, c15.ctypes.data, Gp, counts, force, perm.ctypes.data, pos.ctypes.data, C.byref(n_esc))
    return n2, n_esc.value, perm, pos


def _counts(seed, Gp, N, sigma, many_ties):
    rng = np.random.default_rng(seed)
    mu = rng.lognormal(-1.5, sigma, Gp)
    c3 = rng.binomial(N, np.minimum(mu * mu / 8.0, 0.9)).astype(np.int32)
    c15 = rng.binomial(c3, 0.05).astype(np.int32)
    if many_ties:
        c3 //= 50
        c15 = np.minimum(c15, c3)
    c3[Gp - 300:] = 0          # padded genes
    c15[Gp - 300:] = 0
    return c3, c15


@pytest.mark.parametrize("seed,Gp,sigma,many_ties", [(1, 1024, 1.6, False), (2, 5120, 1.0, False), (3, 2048, 1.6, True), (4, 1024, 0.1, True)])
@pytest.mark.parametrize("force", [0, 5, 6])
def test_plan_is_the_restatement(seed, Gp, sigma, many_ties, force):
    N = 20000
    c3, c15 = _counts(seed, Gp, N, sigma, many_ties)
    counts = N * (Gp - 300)
    got = _plan(c3, c15, counts, force)
    want = ref.plan_counts(c3, c15, counts, force)
    assert got[:2] == want[:2], (got[:2], want[:2])
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    for s in range(0, Gp, 512):                                   # a permutation of the segment, and its inverse
        assert np.array_equal(np.sort(got[2][s:s + 512]), np.arange(512))
        assert np.array_equal(got[3][s + got[2][s:s + 512].astype(np.int64)], np.arange(512))


def test_rule_takes_the_largest_candidate_inside_the_budget():
    Gp = 1024
    c3 = np.zeros(Gp, np.int32)
    c15 = np.zeros(Gp, np.int32)
    # per segment: 256 quiet genes, 64 genes with 100 counts >= 3, 64 with 1000, 128 with 5000 (a tenth of them >= 15)
    for s in (0, 512):
        c3[s + 256:s + 320] = 100
        c3[s + 320:s + 384] = 1000
        c3[s + 384:s + 512] = 5000
    c15[:] = c3 // 10
    e15 = int(c15.sum())
    e5 = e15 + 2 * 64 * 90                       # blocks 0..4 narrow: the 100-count genes' other nine tenths
    e6 = e5 + 2 * 64 * 900
    assert _plan(c3, c15, 256 * e6, 0)[:2] == (6, e6)
    assert _plan(c3, c15, 256 * e6 - 1, 0)[:2] == (5, e5)
    assert _plan(c3, c15, 256 * e5 - 1, 0)[:2] == (0, e15)
    assert _plan(c3, c15, 1, 6)[:2] == (6, e6)  # forced: whatever the budget
    assert ref.plan_counts(c3, c15, 256 * e6 - 1)[:2] == (5, e5)


def test_identical_histograms_keep_the_order():
    c3 = np.full(1024, 37, np.int32)
    c15 = np.full(1024, 2, np.int32)
    _, _, perm, pos = _plan(c3, c15, 10**9, 0)
    assert np.array_equal(perm, np.tile(np.arange(512), 2)) and np.array_equal(pos, perm)
