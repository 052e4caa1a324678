"""Time of ca_clone_evidence (clone evidence with psi integrated out: Newton mode, Laplace value and quadrature per (cell, clone)) beside ca_project_cells at the
same shape in the same process.
   python tools/clone_evidence_time.py [cells genes clones repeats nodes]      (default 100000 5000 8 5 8: 80 % zeros, an overflow list in u8 storage)

u8 storage, K = 1, no covariates.  Kernel time: the engine's own profile (HIP events around the launches; the sweep is kernel class "ypass", every launch of
ca_k_evidence.hip.h and of the rounds of ca_project_cells class "other"); call time: a host clock around the whole call, which ends in a device synchronise.
The split of the "other" time of a call into Newton rounds and quadrature comes from three calls of the same engine:
   a = max_iter = 0 with ONE node, b = max_iter = 0 with the rule's ``nodes`` nodes, c = the full call.
The quadrature pass is linear in the nodes, so quadrature = (b - a) * nodes / (nodes - 1), one Newton round before any pair has frozen (k_ev_mom with all
moments + k_ev_step, plus k_ev_init) = a - quadrature / nodes, and the Newton rounds of the full call = c - quadrature.  ``project_cells max_iter=0`` is one
k_proj_mom + k_proj_step over every cell: a Newton round here spends C exp where that spends one.  Two warm-up calls of each, then ``repeats`` timed calls,
alternating the cases; medians are reported."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clonealign_amd.api import gauss_hermite_rule  # noqa: E402
from clonealign_amd.engine import HipEngine  # noqa: E402

N, G, C, reps, Q = (int(a) for a in (sys.argv[1:6] + ["100000", "5000", "8", "5", "8"][len(sys.argv) - 1:])[:5])
rng = np.random.default_rng(7)
L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
mu = rng.lognormal(-2.7, 1.0, G)                                   # 80 % zeros, like the benchmark matrix
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
nd, wt = gauss_hermite_rule(1, Q)
out = {"N": N, "G": G, "C": C, "K": 1, "nodes": Q, "zero_fraction": round(float((Y == 0).mean()), 4), "repeats": reps}
eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, profile=True, y_storage="u8")
try:
    res, prj = {}, {}
    calls = {"clone_evidence": lambda: res.update(eng.clone_evidence(E, W, 1, nodes=nd, weights=wt)),
             "clone_evidence max_iter=0": lambda: eng.clone_evidence(E, W, 1, nodes=nd, weights=wt, max_iter=0),
             "clone_evidence max_iter=0 one node": lambda: eng.clone_evidence(E, W, 1, max_iter=0),
             "project_cells": lambda: prj.update(eng.project_cells(E, W, 1, log_prior=lp, max_iter=50)),
             "project_cells max_iter=0": lambda: eng.project_cells(E, W, 1, log_prior=lp, max_iter=0)}
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
rows["clone_evidence"].update(rounds_max=int(res["rounds"].max()), rounds_mean=round(float(res["rounds"].mean()), 2),
                              converged=round(float(res["converged"].mean()), 6))
rows["project_cells"].update(rounds_max=int(prj["rounds"].max()), rounds_mean=round(float(prj["rounds"].mean()), 2))
a, b, c = (rows[k]["other_ms_median"] for k in ("clone_evidence max_iter=0 one node", "clone_evidence max_iter=0", "clone_evidence"))
quad = (b - a) * Q / (Q - 1) if Q > 1 else 0.0
one = a - quad / max(Q, 1)
pm = rows["project_cells max_iter=0"]["other_ms_median"]
out["cases"] = rows
out["split_ms"] = {"sweep": rows["clone_evidence"]["sweep_ms_median"], "newton_rounds": round(c - quad, 4), "quadrature": round(quad, 4)}
out["one_newton_round_before_freezing_ms"] = round(one, 4)
out["one_proj_round_ms (k_proj_mom + k_proj_step)"] = pm
out["newton_round_over_C_proj_rounds"] = round(one / (C * pm), 3)
print(json.dumps(out, indent=1))
