"""Time of ca_project_cells (per-cell MAP psi and clone posterior of cells outside the fit) beside ca_clone_loglik at the same shape in the same process.
   python tools/project_cells_time.py [cells genes clones repeats logmean]      (default 100000 5000 8 7 -2.7: 80 % zeros, an overflow list in u8 storage)

u8 storage, K = 1, no covariates, at the full cell count and at an eighth of it (where the 512-gene chunks are what fills the device).  Kernel time: the
engine's own profile (HIP events around the launches; the sweep is kernel class "ypass", the rounds' launches -- k_proj_mom and k_proj_step -- class "other",
as is k_clone_ll_z of ca_clone_loglik with D = 1); call time: a host clock around the whole call, which ends in a device synchronise.  ``max_iter = 0`` is
one k_proj_mom launch and one k_proj_step launch over every cell: the cost of a round before any cell has frozen.  Two warm-up calls of each, then
``repeats`` timed calls, alternating the cases; medians are reported.  The numpy restatement's wall time (one call, 2000 cells, scaled) stands beside them."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clonealign_amd.api import _project_cells_host  # noqa: E402
from clonealign_amd.engine import HipEngine  # noqa: E402

N, G, C, reps = (int(a) for a in (sys.argv[1:5] + ["100000", "5000", "8", "7"][len(sys.argv) - 1:])[:4])
logmean = float(sys.argv[5]) if len(sys.argv) > 5 else -2.7
rng = np.random.default_rng(7)
L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
mu = rng.lognormal(logmean, 1.0, G)                                # -2.7: 80 % zeros, like the benchmark matrix
W = rng.normal(size=(G, 1)) * 0.5
z = rng.integers(0, C, N)
psi = rng.normal(size=(N, 1))
Y = np.empty((N, G), dtype=np.int32)
for lo in range(0, N, 10_000):
    sl = slice(lo, lo + 10_000)
    Y[sl] = rng.poisson(mu[None, :] * L[:, z[sl]].T * np.exp(psi[sl] @ W.T))
Y[:, 0] += 1
hot = rng.choice(N * G, 5000, replace=False)
Y.reshape(-1)[hot] = rng.integers(256, 60000, size=hot.size)
E = mu[:, None] * L
lp = np.zeros((N, C)) + np.log(1.0 / C)
out = {"N": N, "G": G, "C": C, "K": 1, "zero_fraction": round(float((Y == 0).mean()), 4), "repeats": reps, "cases": {}}
for n in (N, N // 8):
    eng = HipEngine(Y[:n], L, np.zeros((n, 0)), np.zeros(G), 0, profile=True, y_storage="u8")
    try:
        res = {}
        calls = {"project_cells": lambda: res.update(eng.project_cells(E, W, 1, log_prior=lp[:n])),
                 "project_cells max_iter=0": lambda: eng.project_cells(E, W, 1, log_prior=lp[:n], max_iter=0),
                 "clone_loglik D=1": lambda: eng.clone_loglik(E, psi[:n], W),
                 "clone_loglik D=0": lambda: eng.clone_loglik(E)}
        for fn in calls.values():
            fn(); fn()
        sweep, other, nother, wall = ({k: [] for k in calls} for _ in range(4))
        for _ in range(reps):
            for k, fn in calls.items():
                eng.kernel_times(reset=True)
                t0 = time.perf_counter()
                fn()
                wall[k].append((time.perf_counter() - t0) * 1e3)
                kt = eng.kernel_times()
                sweep[k].append(kt["ypass"][0]); other[k].append(kt["other"][0]); nother[k].append(kt["other"][1])
    finally:
        eng.close()
    rows = {k: {"sweep_ms_median": round(float(np.median(sweep[k])), 4), "other_ms_median": round(float(np.median(other[k])), 4),
                "other_launches": int(np.median(nother[k])), "call_ms_median": round(float(np.median(wall[k])), 3)} for k in calls}
    rows["project_cells"].update(rounds_max=int(res["rounds"].max()), rounds_mean=round(float(res["rounds"].mean()), 2),
                                 converged=round(float(res["converged"].mean()), 4))
    one = rows["project_cells max_iter=0"]["other_ms_median"]
    rows["one_round_before_freezing_ms (k_proj_mom + k_proj_step)"] = one
    rows["one_round_over_k_clone_ll_z"] = round(one / rows["clone_loglik D=1"]["other_ms_median"], 3)
    m = min(n, 2000)
    t0 = time.perf_counter()
    _project_cells_host(Y[:m], E, W, 1, 0, None, lp[:m], None)
    rows["numpy_restatement_ms_scaled"] = round((time.perf_counter() - t0) * 1e3 * n / m, 1)
    out["cases"][f"{n} cells"] = rows
print(json.dumps(out, indent=1))
