"""Time of ca_predictive_stats (replicate rows drawn and reduced on the device) beside the routes it replaces.
   python tools/predictive_time.py [cells genes clones n_rep repeats]      (default 100000 5000 8 20 5)

K = 1 with sd(W) = 0.5, no covariates; library sizes as the benchmark's matrix has them (bench.py: Poisson counts with rates lognormal(-1, 1) x L x 0.5, so
a row sum is Poisson with the summed rate).  Reported, in milliseconds:
  (a) ca_predictive_kernel_ms for n_rep replicates, with and without the per-clone gene totals (HIP events around the launches; two warm-up calls, median);
  (b) n_rep x ca_simulate_kernel_ms for the same inputs: what k_simulate takes to DRAW the same rows, before any of them is copied or scored;
  (c) the wall time of the route without this entry point, per replicate: simulate_counts, then the upload (an engine), then clone_loglik;
  (d) the wall time of one whole predictive_check call (observed matrix = a replicate at draw 1000).
Before timing, replicate 0 is checked against the rows of simulate_counts (totals exact, ll against float64 numpy on 256 cells)."""
import json
import os
import sys
import time

import numpy as np
from scipy.special import gammaln

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clonealign_amd import api, engine  # noqa: E402
from clonealign_amd.engine import HipEngine  # noqa: E402

N, G, C, n_rep, reps = (int(a) for a in (sys.argv[1:6] + ["100000", "5000", "8", "20", "5"][len(sys.argv) - 1:])[:5])
rng = np.random.default_rng(7)
L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
mu = rng.lognormal(-1.0, 1.0, G)
E = mu[:, None] * L
W = rng.normal(size=(G, 1)) * 0.5
z = rng.integers(0, C, N).astype(np.int32)
psi = rng.normal(size=(N, 1))
total = rng.poisson(0.5 * E.sum(0)[z]).astype(np.int64)
out = {"N": N, "G": G, "C": C, "K": 1, "n_rep": n_rep, "mean_total": float(total.mean()), "repeats": reps}

# the replicate of draw 0 is the matrix simulate_counts returns
rows = engine.simulate_counts(E, W, psi, z, total, seed=1, draw=0)
ll, T = engine.predictive_stats(E, W, psi, z, total, seed=1, draw0=0, n_rep=1)
assert all(np.array_equal(T[0][:, c], rows[z == c].sum(0, dtype=np.int64)) for c in range(C))
m = min(N, 256)
eta = psi[:m] @ W.T
x = eta - eta.max(1, keepdims=True)
logp = np.log(E[:, z[:m]].T) + x - np.log((E[:, z[:m]].T * np.exp(x)).sum(1, keepdims=True))
y = rows[:m].astype(np.float64)
want = gammaln(total[:m] + 1.0) - gammaln(y + 1.0).sum(1) + (y * logp).sum(1)
scale = gammaln(total[:m] + 1.0) + gammaln(y + 1.0).sum(1) + np.abs(y * logp).sum(1)
out["ll_vs_numpy_max_over_scale"] = float((np.abs(ll[:m, 0] - want) / scale).max())
assert out["ll_vs_numpy_max_over_scale"] <= 1e-10


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


buf = (np.zeros((N, n_rep)), np.zeros((n_rep, G, C), dtype=np.int64))
k, w = timed(lambda: engine.predictive_stats(E, W, psi, z, total, seed=1, n_rep=n_rep, out=buf), engine.predictive_kernel_ms)
out["a_predictive_kernel_ms"], out["a_predictive_call_ms"] = k, w
k, w = timed(lambda: engine.predictive_stats(E, W, psi, z, total, seed=1, n_rep=n_rep, gene_totals=False, out=(buf[0], None)), engine.predictive_kernel_ms)
out["a_predictive_kernel_ms_without_totals"], out["a_predictive_call_ms_without_totals"] = k, w
k, w = timed(lambda: engine.predictive_stats(E, W, psi, z, total, seed=1, n_rep=1, gene_totals=False), engine.predictive_kernel_ms)
out["predictive_kernel_ms_one_replicate_without_totals"] = k
k, w = timed(lambda: engine.simulate_counts(E, W, psi, z, total, seed=1, out=rows), engine.simulate_kernel_ms)
out["simulate_kernel_ms_one_replicate"], out["simulate_call_ms_one_replicate"] = k, w
out["b_n_rep_x_simulate_kernel_ms"] = round(n_rep * k, 1)
out["a_over_b"] = round(out["a_predictive_kernel_ms"] / (n_rep * k), 3)

# (c) one replicate by the route without the entry point: rows to the host, an engine for the upload, the scorer
wall = []
for r in range(2):
    t0 = time.perf_counter()
    engine.simulate_counts(E, W, psi, z, total, seed=1, draw=r, out=rows)
    eng = HipEngine(rows, L, np.zeros((N, 0)), None, 0)
    try:
        eng.clone_loglik(E, psi, W, const=True)
    finally:
        eng.close()
    wall.append((time.perf_counter() - t0) * 1e3)
out["c_route_per_replicate_ms"] = round(min(wall), 1)
out["c_route_n_rep_replicates_ms"] = round(n_rep * min(wall), 1)

# (d) the public call
names = [f"clone_{i}" for i in range(C)]
fit = {"ml_params": {"mu": mu, "W": W, "psi": psi}, "clone_names": names, "clone": np.asarray(names, dtype=object)[z]}
engine.simulate_counts(E, W, psi, z, total, seed=1, draw=1000, out=rows)
t0 = time.perf_counter()
res = api.predictive_check(fit, rows, L, n_rep=n_rep, seed=1)
out["d_predictive_check_call_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
out["d_z_of_data_drawn_from_the_model"] = round(res["z"], 3)
print(json.dumps(out, indent=1))
