"""Time of ca_copy_number_profile (the expression side of the likelihood profile over the copy-number matrix) beside ca_predictive_moments, whose cell phase
it shares.
   python tools/copy_number_profile_time.py [cells genes clones blocks repeats subset]      (default 100000 5000 8 23 5 2000)

The inputs are tools/predictive_moments_time.py's: K = 1 with sd(W) = 0.5, no covariates, the benchmark's library sizes; the candidates are 0 .. 6 (J = 7, the
bucket of 8 accumulators); the blocks are `blocks` contiguous runs of genes.  Reported, in milliseconds, from ONE process, two warm-up calls, medians:
  (a) ca_predictive_moments_kernel_ms and the wall time of the call (the yardstick next to it);
  (b) ca_copy_number_profile_kernel_ms (HIP events around the launches: the cell phase, the accumulation and its finish) and the call time, per-gene mode;
  (c) the same in block mode;
  (d) the numpy restatement (api._copy_number_profile_host) on the first `subset` cells, both modes, one run each.
Before timing, both modes are checked against the restatement on 256 cells."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clonealign_amd import api, engine  # noqa: E402

N, G, C, B, reps, sub = (int(a) for a in (sys.argv[1:7] + ["100000", "5000", "8", "23", "5", "2000"][len(sys.argv) - 1:])[:6])
rng = np.random.default_rng(7)
L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
mu = rng.lognormal(-1.0, 1.0, G)
E = mu[:, None] * L
W = rng.normal(size=(G, 1)) * 0.5
z = rng.integers(0, C, N).astype(np.int32)
psi = rng.normal(size=(N, 1))
total = rng.poisson(0.5 * E.sum(0)[z]).astype(np.int64)
kappa = np.arange(7.0)
blocks = (np.arange(G) * B // G).astype(np.int32)
out = {"N": N, "G": G, "C": C, "K": 1, "J": int(kappa.shape[0]), "blocks": B, "mean_total": float(total.mean()), "repeats": reps,
       "build": engine.load_library().ca_build_id().decode()}

m = min(N, 256)
for name, bl in (("per_gene", None), ("per_block", blocks)):
    got = engine.copy_number_profile(E, W, psi[:m], z[:m], total[:m], mu, kappa, blocks=bl)
    want = api._copy_number_profile_host(E, W, psi[:m], z[:m], total[:m], mu, kappa, bl)
    out[f"{name}_vs_numpy_max_rel"] = float((np.abs(got - want) / np.abs(want).max(2, keepdims=True)).max())   # (relative to the entry's largest candidate)
    assert np.isfinite(got).all() and out[f"{name}_vs_numpy_max_rel"] <= 1e-9


def timed(call, kernel_ms, warm=2):
    for _ in range(warm):
        call()
    kern, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(kernel_ms())
    return round(float(np.median(kern)), 3), round(float(np.median(wall)), 1)


out["a_moments_kernel_ms"], out["a_moments_call_ms"] = timed(lambda: engine.predictive_moments(E, W, psi, z, total), engine.predictive_moments_kernel_ms)
out["b_per_gene_kernel_ms"], out["b_per_gene_call_ms"] = timed(lambda: engine.copy_number_profile(E, W, psi, z, total, mu, kappa), engine.copy_number_profile_kernel_ms)
out["c_per_block_kernel_ms"], out["c_per_block_call_ms"] = timed(lambda: engine.copy_number_profile(E, W, psi, z, total, mu, kappa, blocks=blocks),
                                                                 engine.copy_number_profile_kernel_ms)
s = min(N, sub)
out["d_numpy_subset_cells"] = s
for name, bl in (("per_gene", None), ("per_block", blocks)):
    t0 = time.perf_counter()
    api._copy_number_profile_host(E, W, psi[:s], z[:s], total[:s], mu, kappa, bl)
    out[f"d_numpy_{name}_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
print(json.dumps(out, indent=1))
