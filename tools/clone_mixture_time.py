"""Time of the per-cell clone mixture, ca_clone_mixture, beside ca_clone_loglik and ca_clone_pair_loglik at the same shape on the same engine in the same process.
   python tools/clone_mixture_time.py [cells genes clones repeats logmean max_iter tol]      (default 100000 5000 8 5 -2.7 50 1e-3: 80 % zeros, u8 storage with an overflow list, K = 1)

The rows are PLANTED mixtures: Dirichlet(0.5) weights over the clones, a sixth of the rows pure and a sixth two-clone, Poisson counts at the mixed rate; a few
thousand entries are raised above 255 so that the overflow list is in play (those rows are far from the model and are the ones that stay at ``max_iter``).
Cases: ``mixture D=1`` (uniform start), ``evaluate D=1`` (``max_iter = 0``: the list and one evaluation), ``mixture D=0``, ``pair D=1`` (three weights),
``clone_loglik D=1`` and ``clone_loglik D=0``.  Kernel time: the engine's own profile (HIP events around the launches).  A mixture call runs ca_clone_loglik's
launches and then its own -- k_mix_list in the kernel class "ypass", k_mix_rounds in "other" -- so the mixture part is reported as the DIFFERENCE of the
medians of ypass + other between the mixture call and ca_clone_loglik with the same D (``mixture_part_ms``; ``list_ms`` and ``rounds_ms`` are the two classes'
differences).  Call time: a host clock around the whole call, which ends in a device synchronise.  Per cell: rounds, LIST PASSES = 2 rounds + 1 (every round
is one evaluation and one line-search pass over the list, and the returned point is evaluated once more; a start replaced by the uniform one adds a pass),
and the share of cells that stopped at ``max_iter`` with ``bound > tol``.  Two warm-up calls of each, then ``repeats`` timed calls, alternating the cases;
medians are reported."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clonealign_amd.engine import HipEngine  # noqa: E402

N, G, C, reps = (int(a) for a in (sys.argv[1:5] + ["100000", "5000", "8", "5"][len(sys.argv) - 1:])[:4])
logmean = float(sys.argv[5]) if len(sys.argv) > 5 else -2.7
max_iter = int(sys.argv[6]) if len(sys.argv) > 6 else 50
tol = float(sys.argv[7]) if len(sys.argv) > 7 else 1e-3
rng = np.random.default_rng(7)
L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
mu = rng.lognormal(logmean, 1.0, G)                                # -2.7: 80 % zeros, like the benchmark matrix
E = mu[:, None] * L
PI = rng.dirichlet(np.full(C, 0.5), size=N)
PI[: N // 6] = np.eye(C)[rng.integers(0, C, N // 6)]
two = np.arange(N // 6, N // 3)
a, b = rng.integers(0, C, two.size), rng.integers(1, C, two.size)
w2 = rng.uniform(0.2, 0.8, two.size)
PI[two] = 0.0
PI[two, a], PI[two, (a + b) % C] = w2, 1.0 - w2
U, V = rng.normal(size=(N, 1)) * 0.5, rng.normal(size=(G, 1)) * 0.3
Y = np.empty((N, G), dtype=np.int32)
for lo in range(0, N, 10_000):                                      # the model's own rows: sum_c pi_c E_gc exp(eta_ng) / Z_nc, at the depth of E
    ex = np.exp(U[lo:lo + 10_000] @ V.T)
    Y[lo:lo + 10_000] = rng.poisson(ex * ((PI[lo:lo + 10_000] * (E.sum(0)[None, :] / (ex @ E))) @ E.T))
Y[:, 0] += 1
hot = rng.choice(N * G, 5000, replace=False)
Y.reshape(-1)[hot] = rng.integers(256, 60000, size=hot.size)
hot_rows = np.zeros(N, dtype=bool)
hot_rows[hot // G] = True
nnz = int((Y != 0).sum())
weights = (0.3, 0.5, 0.7)

out = {"N": N, "G": G, "C": C, "slots": C + C * (C + 1) // 2, "max_iter": max_iter, "tol_nats": tol, "zero_fraction": round(1 - nnz / (N * G), 4), "nonzeros": nnz,
       "rows_with_a_raised_entry": int(hot_rows.sum()), "repeats": reps, "cases": {}}
eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, profile=True, y_storage="u8")
res = {}
try:
    calls = {"mixture D=1": lambda: eng.clone_mixture(E, U, V, max_iter=max_iter, tol=tol, want_ll=False),
             "evaluate D=1": lambda: eng.clone_mixture(E, U, V, max_iter=0, want_ll=False),
             "mixture D=0": lambda: eng.clone_mixture(E, max_iter=max_iter, tol=tol, want_ll=False),
             "pair D=1": lambda: eng.clone_pair_loglik(E, U, V, weights=weights, want_ll=False),
             "clone_loglik D=1": lambda: eng.clone_loglik(E, U, V),
             "clone_loglik D=0": lambda: eng.clone_loglik(E)}
    for k, fn in calls.items():
        fn()
        res[k] = fn()
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
    out["cases"][k] = {"ypass_ms_median": round(float(np.median(ypass[k])), 4), "other_ms_median": round(float(np.median(other[k])), 4),
                       "call_ms_median": round(float(np.median(wall[k])), 3)}
cs = out["cases"]
ll1 = cs["clone_loglik D=1"]["ypass_ms_median"] + cs["clone_loglik D=1"]["other_ms_median"]
for k, D in (("mixture D=1", 1), ("evaluate D=1", 1), ("mixture D=0", 0)):
    row, ref = cs[k], cs[f"clone_loglik D={D}"]
    row["list_ms"] = round(row["ypass_ms_median"] - ref["ypass_ms_median"], 4)
    row["rounds_ms"] = round(row["other_ms_median"] - ref["other_ms_median"], 4)
    row["mixture_part_ms"] = round(row["list_ms"] + row["rounds_ms"], 4)
    row["mixture_part_over_clone_loglik_D1_kernels"] = round(row["mixture_part_ms"] / ll1, 3)
    row["call_over_clone_loglik_D1_call"] = round(row["call_ms_median"] / cs["clone_loglik D=1"]["call_ms_median"], 3)
    r = res[k]
    rd = r["rounds"].astype(np.int64)
    row["rounds_median_max"] = [int(np.median(rd)), int(rd.max())]
    row["list_passes_per_cell_median_max_mean"] = [int(np.median(2 * rd + 1)), int((2 * rd + 1).max()), round(float((2 * rd + 1).mean()), 2)]
    row["share_at_max_iter"] = round(float((~r["converged"]).mean()), 5)
    row["share_at_max_iter_rows_without_a_raised_entry"] = round(float((~r["converged"])[~hot_rows].mean()), 5)
    if max_iter > 0 and k != "evaluate D=1":
        row["mean_abs_weight_error"] = round(float(np.abs(r["weights"] - PI)[~hot_rows].mean()), 5)
        row["ns_per_entry_and_list_pass"] = round(row["rounds_ms"] * 1e6 / (nnz * float((2 * rd + 1).mean())), 3)
cs["pair D=1"]["pair_part_ms"] = round(cs["pair D=1"]["ypass_ms_median"] - cs["clone_loglik D=1"]["ypass_ms_median"], 4)
out["clone_loglik_D1_kernels_ms"] = round(ll1, 4)
print(json.dumps(out, indent=1))
