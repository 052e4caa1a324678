"""Time of ca_simulate_counts (count rows drawn from a fitted model on the device) beside its numpy restatement.
   python tools/simulate_time.py [cells genes clones repeats total]      (default 100000 5000 8 7 5000)

K = 1 with sd(W) = 0.5, no covariates, library sizes uniform in [0.8, 1.2] x total, at the full cell count and at an eighth of it.  Kernel time: HIP
events around the k_simulate launches (ca_simulate_kernel_ms); call time: a host clock around the whole call, which ends with every row in the caller's
array -- the difference is mostly the copy of cells x genes x 4 bytes to the host.  Two warm-up calls, then ``repeats`` timed calls; medians.  The
restatement's wall time (one call on 200 cells, scaled) stands beside them."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clonealign_amd import engine  # noqa: E402
from clonealign_amd.api import _simulate_counts_host  # noqa: E402

N, G, C, reps, tot = (int(a) for a in (sys.argv[1:6] + ["100000", "5000", "8", "7", "5000"][len(sys.argv) - 1:])[:5])
rng = np.random.default_rng(7)
E = rng.lognormal(-2.7, 1.0, (G, 1)) * rng.integers(1, 5, size=(G, C)).astype(np.float64)
W = rng.normal(size=(G, 1)) * 0.5
z = rng.integers(0, C, N).astype(np.int32)
psi = rng.normal(size=(N, 1))
total = rng.integers(int(0.8 * tot), int(1.2 * tot) + 1, N).astype(np.int64)
out = {"N": N, "G": G, "C": C, "K": 1, "mean_total": float(total.mean()), "repeats": reps, "cases": {}}
for n in (N, N // 8):
    buf = np.zeros((n, G), dtype=np.int32)
    call = lambda: engine.simulate_counts(E, W, psi[:n], z[:n], total[:n], seed=1, out=buf)  # noqa: E731
    call(); call()
    kern, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(engine.simulate_kernel_ms())
    assert np.array_equal(buf.sum(1), total[:n])
    m = min(n, 200)
    t0 = time.perf_counter()
    ref, flagged = _simulate_counts_host(E, W, psi[:m], z[:m], total[:m], seed=1)
    host_ms = (time.perf_counter() - t0) * 1e3 * n / m
    assert np.array_equal(ref, buf[:m]) and flagged.sum() == 0
    k, w, draws = float(np.median(kern)), float(np.median(wall)), int(total[:n].sum())
    out["cases"][f"{n} cells"] = {"draws": draws, "kernel_ms_median": round(k, 3), "draws_per_second": round(draws / (k * 1e-3), 0), "call_ms_median": round(w, 1),
                                  "call_minus_kernel_ms (copy of the rows to the host)": round(w - k, 1), "row_bytes": int(n) * G * 4,
                                  "host_GB_per_s_of_rows_over_call": round(n * G * 4 / (w * 1e-3) / 1e9, 2),
                                  "numpy_restatement_ms_scaled": round(host_ms, 1), "restatement_over_kernel": round(host_ms / k, 1),
                                  "restatement_over_call": round(host_ms / w, 1), "kernel_over_k_proj_mom_round_1.55ms": round(k / 1.55, 2)}
print(json.dumps(out, indent=1))
