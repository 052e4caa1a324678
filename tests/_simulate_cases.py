"""The parity cases of ca_simulate_counts, shared by tests/test_simulate_host.py (the restatement is insensitive to the grouping of the sums on them) and
tests/test_gpu_simulate.py (the device equals the restatement on them).  Same seeds in both, by construction."""
import functools

import numpy as np

#        name            N     G      C   D  what it is there for
CASES = {"ragged":      (33,   77,    2,  0),   # ragged tails of every tile
         "mixed":       (300,  1234,  8,  1),   # copy number 0 in places; totals 0 .. 6000 with 0 and 1, one cell of 200 000 (several work items)
         "pow2_plus_1": (64,   2049,  20, 2),   # one gene past a power of two, K = 1 and P = 1, twenty clones
         "large_g":     (16,   20000, 4,  1),   # two-level search table, counters on the global row
         "two_level":   (8,    6000,  3,  1),   # two-level search table beside an LDS histogram
         "few_genes":   (5,    3,     2,  0),   # fewer genes than lanes
         "steep":       (24,   300,   3,  2)}   # |eta| up to 700: the shift by the maximum matters


@functools.lru_cache(maxsize=None)
def make(name):
    """(E, V, U, clone, total, seed) of a case; arrays are read-only (the reference made from them is shared)."""
    N, G, C, D = CASES[name]
    seed = 1000 + sorted(CASES).index(name)
    rng = np.random.default_rng(seed)
    E = rng.lognormal(0.0, 1.0, (G, 1)) * rng.integers(1, 5, (G, C)).astype(np.float64)
    V = rng.normal(size=(G, D)) * 0.5 if D else None
    U = rng.normal(size=(N, D)) if D else None
    clone = rng.integers(0, C, N).astype(np.int32)
    total = np.full(N, 3000, dtype=np.int64)
    if name == "mixed":
        E[rng.random((G, C)) < 0.1] = 0.0                            # 10 % of the genes have copy number 0 in some clone
        total = rng.integers(0, 6001, N).astype(np.int64)
        total[:4] = (0, 1, 200_000, 2)
    elif name == "few_genes":
        total[:] = 1000
    elif name == "steep":
        V = rng.uniform(-1.0, 1.0, (G, D))
        U = rng.uniform(-350.0, 350.0, (N, D))                       # eta in [-700, 700]
        U[0], V[0] = (350.0, 350.0), (1.0, 1.0)                      # ... and 700 itself
        U[1], V[1] = (350.0, -350.0), (-1.0, 1.0)                    # ... and -700
        total = rng.integers(1, 4000, N).astype(np.int64)
    out = (E, V, U, clone, total)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out + (seed,)
