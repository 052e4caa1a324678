"""Time of ca_predictive_moments (the replicates' moments in closed form) beside ca_predictive_stats, the Monte Carlo it replaces for the totals.
   python tools/predictive_moments_time.py [cells genes clones n_rep repeats]      (default 100000 5000 8 20 5)

The inputs are tools/predictive_time.py's: K = 1 with sd(W) = 0.5, no covariates, the benchmark's library sizes.  Reported, in milliseconds, from ONE process:
  (a) ca_predictive_moments_kernel_ms (HIP events around the launches: log E, the cell phase, the gene phase and its finish) and the wall time of the whole
      call, which ends with all five outputs in the caller's arrays; two warm-up calls, median;
  (b) ca_predictive_kernel_ms and the call time of ca_predictive_stats at n_rep replicates with the totals, the same inputs;
  (c) the wall time of one whole predictive_moments call (observed matrix = a replicate at draw 1000) and of dosage_response on its result.
Before timing, the call is checked against float64 numpy on 256 cells (cell values) and against the replicates' own mean (totals)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clonealign_amd import api, engine  # noqa: E402

N, G, C, n_rep, reps = (int(a) for a in (sys.argv[1:6] + ["100000", "5000", "8", "20", "5"][len(sys.argv) - 1:])[:5])
rng = np.random.default_rng(7)
L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
mu = rng.lognormal(-1.0, 1.0, G)
E = mu[:, None] * L
W = rng.normal(size=(G, 1)) * 0.5
z = rng.integers(0, C, N).astype(np.int32)
psi = rng.normal(size=(N, 1))
total = rng.poisson(0.5 * E.sum(0)[z]).astype(np.int64)
out = {"N": N, "G": G, "C": C, "K": 1, "n_rep": n_rep, "mean_total": float(total.mean()), "repeats": reps, "build": engine.load_library().ca_build_id().decode()}

mean, var, Tm, Tv, Tc = engine.predictive_moments(E, W, psi, z, total)
m = min(N, 256)
eta = psi[:m] @ W.T
x = eta - eta.max(1, keepdims=True)
w = E[:, z[:m]].T * np.exp(x)
p = w / w.sum(1, keepdims=True)
lp = np.log(E[:, z[:m]].T) + x - np.log(w.sum(1, keepdims=True))
h = (p * lp).sum(1, keepdims=True)
out["cell_mean_vs_numpy_max_over_scale"] = float((np.abs(mean[:m] - total[:m] * h[:, 0]) / (total[:m] * (p * np.abs(lp)).sum(1))).max())
out["cell_var_vs_numpy_max_over_scale"] = float((np.abs(var[:m] - total[:m] * (p * (lp - h) ** 2).sum(1)) / (total[:m] * (p * lp * lp).sum(1))).max())
assert max(out["cell_mean_vs_numpy_max_over_scale"], out["cell_var_vs_numpy_max_over_scale"]) <= 1e-10
assert abs(Tm.sum() - total.sum()) <= 1e-9 * total.sum()            # the p of a cell sum to 1


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


k, wl = timed(lambda: engine.predictive_moments(E, W, psi, z, total), engine.predictive_moments_kernel_ms)
out["a_moments_kernel_ms"], out["a_moments_call_ms"] = k, wl
buf = (np.zeros((N, n_rep)), np.zeros((n_rep, G, C), dtype=np.int64))
k, wl = timed(lambda: engine.predictive_stats(E, W, psi, z, total, seed=1, n_rep=n_rep, out=buf), engine.predictive_kernel_ms)
out["b_predictive_kernel_ms"], out["b_predictive_call_ms"] = k, wl
sd = np.sqrt(Tv / n_rep)
out["b_replicate_mean_minus_T_mean_worst_se"] = round(float((np.abs(buf[1].mean(0) - Tm)[Tv > 0] / sd[Tv > 0]).max()), 2)

# (c) the public calls
names = [f"clone_{i}" for i in range(C)]
fit = {"ml_params": {"mu": mu, "W": W, "psi": psi}, "clone_names": names, "clone": np.asarray(names, dtype=object)[z]}
rows = engine.simulate_counts(E, W, psi, z, total, seed=1, draw=1000)
t0 = time.perf_counter()
res = api.predictive_moments(fit, rows, L)
out["c_predictive_moments_call_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
t0 = time.perf_counter()
dr = api.dosage_response(fit, rows, L, moments=res)
out["c_dosage_response_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
zc, zg = res["z_cell"], res["z_gene_clone"]
out["c_z_cell_mean_sd"] = [round(float(np.nanmean(zc)), 3), round(float(np.nanstd(zc)), 3)]
out["c_z_gene_clone_mean_sd"] = [round(float(np.nanmean(zg)), 3), round(float(np.nanstd(zg)), 3)]
out["c_kappa_median"] = round(float(np.nanmedian(dr["kappa"])), 4)
print(json.dumps(out, indent=1))
