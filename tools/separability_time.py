"""Time of ca_clone_separability (clone separability in closed form) at the headline shape, in ONE process.
   python tools/separability_time.py [cells genes clones repeats boot_replicates host_cells]      (default 100000 5000 8 5 32 2048)
Writes profiles/r18_separability.txt (JSON) and prints it.

K = 1 with sd(W) = 0.5, no covariates.  Reported, in milliseconds:
  (a) ca_clone_separability_kernel_ms (HIP events around every launch: log e, the right-hand side, the product, the merge, the epilogue) and the wall time of
      the whole call, which ends with the five outputs (4 N C C + N C float64) in the caller's arrays; two warm-up calls, median and min / max;
  (b) the float64 FLOP/s of the product, 2 N G ncol_padded over ALL the call's kernels (the product has no time of its own: the events are summed), beside
      ca_reweighted_kernel_ms of a bootstrap call with ``boot_replicates`` replicates on the same device and its 2 N G R (2 C + 1) flops -- the same MFMA
      kernel, there with the resident rows as a second left operand;
  (c) the numpy restatement (api._clone_separability_host) on the first ``host_cells`` cells, and that time EXTRAPOLATED to all cells (labelled as such).
Before timing, the call is checked against the restatement on those cells under the parity bars of tests/test_gpu_separability.py."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clonealign_amd import api, engine  # noqa: E402

N, G, C, reps, R, host_cells = (int(a) for a in (sys.argv[1:7] + ["100000", "5000", "8", "5", "32", "2048"][len(sys.argv) - 1:])[:6])
rng = np.random.default_rng(7)
L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
mu = rng.lognormal(-2.7, 1.0, G)
E = mu[:, None] * L
W = rng.normal(size=(G, 1)) * 0.5
psi = rng.normal(size=(N, 1))
ncol = C + 4 * C * (C - 1)
ncolp = (ncol + 15) // 16 * 16


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(min(v)), 3), "max": round(float(max(v)), 3)}


out = {"N": N, "G": G, "C": C, "K": 1, "columns": ncol, "columns_padded": ncolp, "repeats": reps, "build": engine.load_library().ca_build_id().decode()}
m = min(N, host_cells)
t0 = time.perf_counter()
want = api._clone_separability_host(E, W, psi[:m], with_scale=True)
host_ms = (time.perf_counter() - t0) * 1e3
got = engine.clone_separability(E, W, psi)
bars = [1e-10 * np.maximum(1.0, np.abs(want[0])), 1e-10, 1e-10 * want[5], 1e-10 * want[6], 1e-10 * want[7]]
for k in range(5):
    assert (np.abs(got[k][:m] - want[k]) <= bars[k]).all(), k
out["checked_cells"] = m

kern, wall = [], []
for i in range(reps + 2):
    t0 = time.perf_counter()
    engine.clone_separability(E, W, psi)
    if i >= 2:
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(engine.clone_separability_kernel_ms())
flop = 2.0 * N * G * ncolp
out["a_separability"] = {"kernels_ms": stats(kern), "call_ms": stats(wall), "output_megabytes": round((4 * N * C * C + N * C) * 8 / 2 ** 20, 1)}
out["b_product"] = {"flop": flop, "tflops_over_all_kernels": round(flop / (float(np.median(kern)) * 1e-3) / 1e12, 2)}

# the bootstrap's products on the same device: a resident matrix of the same shape
z = rng.integers(0, C, N)
Y = np.empty((N, G), dtype=np.int32)
for lo in range(0, N, 10_000):
    Y[lo:lo + 10_000] = rng.poisson(mu[None, :] * L[:, z[lo:lo + 10_000]].T)
Y[:, 0] += 1
w = api.bootstrap_gene_weights(G, R, seed=1)
eng = engine.HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, y_storage="u8")
try:
    bk = []
    for i in range(reps + 2):
        eng.clone_loglik_reweighted(E, psi, W, w, log_prior=np.zeros((N, C)))
        if i >= 2:
            bk.append(engine.reweighted_kernel_ms())
finally:
    eng.close()
bflop = 2.0 * N * G * R * (C + 1) + 2.0 * N * G * R * C
out["b_bootstrap_R%d" % R] = {"kernels_ms": stats(bk), "flop": bflop, "tflops_over_all_kernels": round(bflop / (float(np.median(bk)) * 1e-3) / 1e12, 2)}
out["c_numpy_restatement"] = {"cells": m, "ms": round(host_ms, 1), "EXTRAPOLATED_ms_for_all_cells": round(host_ms * N / m, 1)}
text = json.dumps(out, indent=1)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "r18_separability.txt"), "w") as f:
    f.write(text + "\n")
print(text)
