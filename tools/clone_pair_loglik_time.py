"""Time of the pair-mixture log-likelihood, ca_clone_pair_loglik, beside ca_clone_loglik at the same shape on the same engine in the same process.
   python tools/clone_pair_loglik_time.py [cells genes clones repeats logmean weights]      (default 100000 5000 8 7 -2.7 3: 80 % zeros, u8 storage with an overflow list)

Cases: ``pair D=1`` (the new kernel k_pair_ll: one float64 log per cell, non-zero count, pair and weight), ``pair D=0`` (the table route: k_clone_ll against a
table of M W columns), ``clone_loglik D=1`` and ``clone_loglik D=0``.  Kernel time: the engine's own profile (HIP events around the launches).  A pair call runs
ca_clone_loglik's launches and then its own; k_clone_ll and k_pair_ll share the kernel class "ypass", so the pair part's time is reported as the DIFFERENCE of
the medians of that class between the pair call and ca_clone_loglik with the same D (``pair_part_ms``), and its ratio to ca_clone_loglik's whole kernel time
with D = 1 (sweep + contraction).  Call time: a host clock around the whole call, which ends in a device synchronise (tables, uploads, finishing launches and
the read-back of N x M W doubles included).  Two warm-up calls of each, then ``repeats`` timed calls, alternating the cases; medians are reported."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clonealign_amd.engine import HipEngine  # noqa: E402

N, G, C, reps = (int(a) for a in (sys.argv[1:5] + ["100000", "5000", "8", "7"][len(sys.argv) - 1:])[:4])
logmean = float(sys.argv[5]) if len(sys.argv) > 5 else -2.7
W = int(sys.argv[6]) if len(sys.argv) > 6 else 3
weights = np.linspace(0.3, 0.7, W) if W > 1 else np.array([0.5])
rng = np.random.default_rng(7)
L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
mu = rng.lognormal(logmean, 1.0, G)                                # -2.7: 80 % zeros, like the benchmark matrix
z = rng.integers(0, C, N)
Y = np.empty((N, G), dtype=np.int32)
for lo in range(0, N, 10_000):
    Y[lo:lo + 10_000] = rng.poisson(mu[None, :] * L[:, z[lo:lo + 10_000]].T)
Y[:, 0] += 1
hot = rng.choice(N * G, 5000, replace=False)
Y.reshape(-1)[hot] = rng.integers(256, 60000, size=hot.size)
nnz = int((Y != 0).sum())
E = mu[:, None] * L
U, V = rng.normal(size=(N, 1)) * 0.5, rng.normal(size=(G, 1)) * 0.3
M = C * (C - 1) // 2

out = {"N": N, "G": G, "C": C, "pairs": M, "weights": W, "slots": M * W, "zero_fraction": round(1 - nnz / (N * G), 4), "nonzeros": nnz, "repeats": reps, "cases": {}}
eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, profile=True, y_storage="u8")
try:
    calls = {"pair D=1": lambda: eng.clone_pair_loglik(E, U, V, weights=weights, want_ll=False),
             "pair D=0": lambda: eng.clone_pair_loglik(E, weights=weights, want_ll=False),
             "clone_loglik D=1": lambda: eng.clone_loglik(E, U, V),
             "clone_loglik D=0": lambda: eng.clone_loglik(E)}
    for fn in calls.values():
        fn(); fn()
    ypass, other, wall = ({k: [] for k in calls} for _ in range(3))
    for _ in range(reps):
        for k, fn in calls.items():
            eng.kernel_times(reset=True)
            t0 = time.perf_counter()
            fn()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            kt = eng.kernel_times()
            ypass[k].append(kt["ypass"][0])
            other[k].append(kt["other"][0])
finally:
    eng.close()
for k in calls:
    out["cases"][k] = {"ypass_ms_median": round(float(np.median(ypass[k])), 4), "ypass_ms_min_max": [round(min(ypass[k]), 4), round(max(ypass[k]), 4)],
                       "other_ms_median": round(float(np.median(other[k])), 4), "call_ms_median": round(float(np.median(wall[k])), 3)}
cs = out["cases"]
ll1 = cs["clone_loglik D=1"]["ypass_ms_median"] + cs["clone_loglik D=1"]["other_ms_median"]
for D in (1, 0):
    row = cs[f"pair D={D}"]
    row["pair_part_ms"] = round(row["ypass_ms_median"] - cs[f"clone_loglik D={D}"]["ypass_ms_median"], 4)
    row["pair_part_over_clone_loglik_D1_kernels"] = round(row["pair_part_ms"] / ll1, 3)
    row["call_over_clone_loglik_D1_call"] = round(row["call_ms_median"] / cs["clone_loglik D=1"]["call_ms_median"], 3)
cs["pair D=1"]["fp64_log_G_per_s"] = round(nnz * M * W / (cs["pair D=1"]["pair_part_ms"] * 1e-3) / 1e9, 2)
out["clone_loglik_D1_kernels_ms"] = round(ll1, 4)
print(json.dumps(out, indent=1))
