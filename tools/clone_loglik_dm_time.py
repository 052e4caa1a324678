"""Time of the Dirichlet-multinomial log-likelihood, ca_clone_loglik_dm, beside ca_clone_loglik at the same shape on the same engine in the same process.
   python tools/clone_loglik_dm_time.py [cells genes clones repeats logmean concentrations]      (default 100000 5000 8 7 -2.7 8: 80 % zeros, u8 storage with an overflow list, 64 slots)

Cases: ``dm D=1`` and ``dm D=0`` (the kernel k_dm_ll on both: one float64 transcendental per cell, non-zero count, clone and concentration), ``clone_loglik D=1``
and ``clone_loglik D=0``.  Kernel time: the engine's own profile (HIP events around the launches).  A dm call runs ca_clone_loglik's launches and then its own;
k_clone_ll and k_dm_ll share the kernel class "ypass", so the dm part's time is reported as the DIFFERENCE of the medians of that class between the dm call and
ca_clone_loglik with the same D (``dm_part_ms``), and its ratio to ca_clone_loglik's whole kernel time with D = 1 (sweep + contraction).  Call time: a host
clock around the whole call, which ends in a device synchronise (tables, uploads, finishing launches and the read-back of N x C K doubles included).  Two
warm-up calls of each, then ``repeats`` timed calls, alternating the cases; medians are reported.  ``small_count_fraction``: the share of the non-zero counts
that take the product route (integers up to 8); the others cost two lgamma."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clonealign_amd.engine import HipEngine  # noqa: E402

N, G, C, reps = (int(a) for a in (sys.argv[1:5] + ["100000", "5000", "8", "7"][len(sys.argv) - 1:])[:4])
logmean = float(sys.argv[5]) if len(sys.argv) > 5 else -2.7
K = int(sys.argv[6]) if len(sys.argv) > 6 else 8
phi = np.geomspace(10.0, 10.0 ** 4.5, K) if K > 1 else np.array([100.0])
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
small = int(((Y > 0) & (Y <= 8)).sum())
E = mu[:, None] * L
U, V = rng.normal(size=(N, 1)) * 0.5, rng.normal(size=(G, 1)) * 0.3

out = {"N": N, "G": G, "C": C, "concentrations": K, "slots": C * K, "zero_fraction": round(1 - nnz / (N * G), 4), "nonzeros": nnz,
       "small_count_fraction": round(small / nnz, 4), "repeats": reps, "cases": {}}
eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, profile=True, y_storage="u8")
try:
    calls = {"dm D=1": lambda: eng.clone_loglik_dm(E, U, V, concentration=phi, want_ll=False),
             "dm D=0": lambda: eng.clone_loglik_dm(E, concentration=phi, want_ll=False),
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
    row = cs[f"dm D={D}"]
    row["dm_part_ms"] = round(row["ypass_ms_median"] - cs[f"clone_loglik D={D}"]["ypass_ms_median"], 4)
    row["dm_part_over_clone_loglik_D1_kernels"] = round(row["dm_part_ms"] / ll1, 3)
    row["call_over_clone_loglik_D1_call"] = round(row["call_ms_median"] / cs["clone_loglik D=1"]["call_ms_median"], 3)
    row["terms_G_per_s"] = round(nnz * C * K / (row["dm_part_ms"] * 1e-3) / 1e9, 2)
out["clone_loglik_D1_kernels_ms"] = round(ll1, 4)
print(json.dumps(out, indent=1))
