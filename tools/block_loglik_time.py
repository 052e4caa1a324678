"""Time of the log-likelihood sweep by block of genes, ca_clone_loglik_by_block, beside ca_clone_loglik and the route it replaces, in one process.
   python tools/block_loglik_time.py [cells genes clones repeats blocks logmean]      (default 100000 5000 8 5 23 -2.7: 80 % zeros, u8 storage, K = 1)

Cases, all on ONE u8 engine with D = 1 (a K = 1 fit) and the lgamma constant:
  clone_loglik          the plain sweep (k_clone_ll + k_clone_ll_z)
  by_block contiguous   ``blocks`` blocks of consecutive genes of equal size (a chromosome-sorted gene axis)
  by_block interleaved  the labels ``g % blocks`` (every gene is a run of its own: the slowest labelling there is)
and then the route the call replaces for the leave-one-block-out likelihoods: per block one engine on the matrix without the block's columns (a host
copy of the columns, an upload, ca_clone_loglik, the engine closed), timed once.
Kernel time: the engine's own profile (HIP events around the launches; the sweep is kernel class "ypass", the contraction Z class "other"; a by-block
call launches each once per batch of cells, the sums are reported with the number of batches); call time: a host clock around the whole call, which ends
in a device synchronise (table and run-list building, uploads, the finishing launches and the read-back included).  Two warm-up calls of each case, then
``repeats`` timed calls, alternating the cases; medians are reported."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clonealign_amd.engine import HipEngine  # noqa: E402

N, G, C, reps, B = (int(a) for a in (sys.argv[1:6] + ["100000", "5000", "8", "5", "23"][len(sys.argv) - 1:])[:5])
logmean = float(sys.argv[6]) if len(sys.argv) > 6 else -2.7
rng = np.random.default_rng(7)
L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
mu = rng.lognormal(logmean, 1.0, G)                                # -2.7: 80 % zeros, like the benchmark matrix
z = rng.integers(0, C, N)
Y = np.empty((N, G), dtype=np.int32)
for lo in range(0, N, 10_000):
    Y[lo:lo + 10_000] = rng.poisson(mu[None, :] * L[:, z[lo:lo + 10_000]].T)
Y[:, 0] += 1
hot = rng.choice(N * G, 5000, replace=False)
Y.reshape(-1)[hot] = rng.integers(256, 60000, size=hot.size)       # an overflow list beside the u8 matrix
E = mu[:, None] * L
U, V = rng.normal(size=(N, 1)) * 0.5, rng.normal(size=(G, 1)) * 0.3
contiguous = (np.arange(G) * B // G).astype(np.int32)
interleaved = (np.arange(G) % B).astype(np.int32)

out = {"N": N, "G": G, "C": C, "D": 1, "blocks": B, "storage": "u8", "zero_fraction": round(float((Y == 0).mean()), 4), "repeats": reps, "cases": {}}
eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, profile=True, y_storage="u8")
try:
    assert eng.info()["y_storage_name"] == "u8"
    calls = {"clone_loglik": lambda: eng.clone_loglik(E, U, V),
             "by_block contiguous": lambda: eng.clone_loglik_by_block(E, U, V, contiguous, B),
             "by_block interleaved": lambda: eng.clone_loglik_by_block(E, U, V, interleaved, B)}
    for fn in calls.values():
        fn(); fn()
    kern, other, wall, batches = ({k: [] for k in calls} for _ in range(4))
    for _ in range(reps):
        for k, fn in calls.items():
            eng.kernel_times(reset=True)
            t0 = time.perf_counter()
            fn()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            kt = eng.kernel_times()
            kern[k].append(kt["ypass"][0])
            other[k].append(kt["other"][0])
            batches[k].append(kt["ypass"][1])
finally:
    eng.close()
for k in calls:
    out["cases"][k] = {"sweep_ms_median": round(float(np.median(kern[k])), 4), "sweep_ms_min_max": [round(min(kern[k]), 4), round(max(kern[k]), 4)],
                       "contraction_ms_median": round(float(np.median(other[k])), 4), "call_ms_median": round(float(np.median(wall[k])), 3),
                       "cell_batches": int(batches[k][0])}
plain = out["cases"]["clone_loglik"]
for k in calls:
    out["cases"][k]["sweep_over_plain_sweep"] = round(out["cases"][k]["sweep_ms_median"] / plain["sweep_ms_median"], 3)
    out["cases"][k]["call_over_plain_call"] = round(out["cases"][k]["call_ms_median"] / plain["call_ms_median"], 3)

# the route the call replaces: an engine per block on the matrix without the block's columns
t_copy = t_engine = t_call = 0.0
for b in range(B):
    keep = np.flatnonzero(contiguous != b)
    t0 = time.perf_counter()
    Yb = np.ascontiguousarray(Y[:, keep])
    t1 = time.perf_counter()
    sub = HipEngine(Yb, L[keep], np.zeros((N, 0)), np.zeros(keep.size), 0, y_storage="u8")
    t2 = time.perf_counter()
    try:
        sub.clone_loglik(E[keep], U, V[keep])
    finally:
        t3 = time.perf_counter()
        sub.close()
    t_copy, t_engine, t_call = t_copy + (t1 - t0), t_engine + (t2 - t1), t_call + (t3 - t2)
    del Yb
out["cases"]["engine per block"] = {"engines": B, "host_column_copy_ms": round(t_copy * 1e3, 1), "engine_create_ms": round(t_engine * 1e3, 1),
                                    "clone_loglik_call_ms": round(t_call * 1e3, 1), "total_ms": round((t_copy + t_engine + t_call) * 1e3, 1),
                                    "total_over_by_block_contiguous_call": round((t_copy + t_engine + t_call) * 1e3 / out["cases"]["by_block contiguous"]["call_ms_median"], 1)}
print(json.dumps(out, indent=1))
