"""Time of the bootstrap's device call, ca_clone_loglik_reweighted, beside the route it replaces, at the headline shape, in ONE process.
   python tools/bootstrap_time.py [cells genes clones replicates repeats logmean]      (default 100000 5000 8 100 5 -2.7: K = 1, u8 storage with an overflow list, 80 % zeros)
Writes profiles/r17_bootstrap.txt (JSON) and prints it.

  (a) the new call: its kernels by HIP events (ca_reweighted_kernel_ms: event pairs around the launches, no copy) and the whole call by a host clock that ends
      in the call's last synchronise (tables, uploads, the read-back of votes / shares / reads; ll is not asked for); with the engine's profile on, in calls
      of their own, the split by kernel class: "ypass" = the product against the resident rows (and the side pass over the genes with a zero of E),
      "other" = the builder, the product against exp(eta - m), finish and reduce;
  (b) the ca_clone_loglik sweep (const = 0) in the same process: its kernels by the engine's profile, times R -- the FLOOR of the route the call replaces, as
      if the resampled matrices were already resident;
  (c) three replicates of that route in full -- the host copy of the resampled columns, a throwaway engine for the upload, clone_loglik -- timed by a host
      clock and EXTRAPOLATED to R (labelled as such);
  (d) the products' useful float64 FLOP/s, 2 N G R (C + 1) + 2 N G R C over the two products' kernel classes, beside the rate of a bare loop of the same MFMA
      on the same device (tools/mfma_f64_rate.bin, built from tools/mfma_f64_rate.hip by the line in its header; "not measured" when it is not built).
Two warm-up calls of each, then ``repeats`` timed calls, alternating (a) and (b); medians and min / max."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clonealign_amd import api  # noqa: E402
from clonealign_amd.engine import HipEngine, reweighted_kernel_ms  # noqa: E402

N, G, C, R, reps = (int(a) for a in (sys.argv[1:6] + ["100000", "5000", "8", "100", "5"][len(sys.argv) - 1:])[:5])
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
Y.reshape(-1)[hot] = rng.integers(256, 60000, size=hot.size)
E = mu[:, None] * L
U, V = rng.normal(size=(N, 1)) * 0.5, rng.normal(size=(G, 1)) * 0.3
w = api.bootstrap_gene_weights(G, R, seed=1)
lp = np.zeros((N, C))


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(min(v)), 3), "max": round(float(max(v)), 3)}


out = {"N": N, "G": G, "C": C, "K": 1, "R": R, "storage": "u8", "zero_fraction": round(float((Y == 0).mean()), 4), "repeats": reps}
eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, y_storage="u8")
try:
    new = lambda: eng.clone_loglik_reweighted(E, U, V, w, log_prior=lp)    # noqa: E731
    old = lambda: eng.clone_loglik(E, U, V, const=False)                    # noqa: E731
    for fn in (new, old):
        fn(); fn()
    a_kern, a_call, b_call = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        new()
        a_call.append((time.perf_counter() - t0) * 1e3)
        a_kern.append(reweighted_kernel_ms())
        t0 = time.perf_counter()
        old()
        b_call.append((time.perf_counter() - t0) * 1e3)
    # the split by kernel class, and the sweep's kernels, with the engine's profile on (event pairs around every launch: calls of their own)
    eng.set_profile(0x1F)
    a_y, a_o, b_k = [], [], []
    for _ in range(max(reps // 2, 2)):
        eng.kernel_times(reset=True)
        new()
        kt = eng.kernel_times()
        a_y.append(kt["ypass"][0]); a_o.append(kt["other"][0])
        eng.kernel_times(reset=True)
        old()
        kt = eng.kernel_times()
        b_k.append(kt["ypass"][0] + kt["other"][0])
finally:
    eng.close()
out["a_new_call"] = {"kernels_ms": stats(a_kern), "call_ms": stats(a_call), "profiled_product_rows_ms": stats(a_y), "profiled_other_ms": stats(a_o)}
out["b_clone_loglik_sweep"] = {"kernels_ms_one": stats(b_k), "call_ms_one": stats(b_call), "kernels_ms_times_R": round(float(np.median(b_k)) * R, 1),
                               "call_ms_times_R": round(float(np.median(b_call)) * R, 1)}
out["a_below_b_kernels"] = bool(np.median(a_kern) < np.median(b_k) * R)
# (c) the route in full, three replicates
full = []
for r in range(3):
    t0 = time.perf_counter()
    idx = np.repeat(np.arange(G), w[r].astype(np.int64))
    Yr = np.ascontiguousarray(Y[:, idx])
    e2 = HipEngine(Yr, L[idx], np.zeros((N, 0)), np.zeros(idx.size), 0, y_storage="u8")
    try:
        e2.clone_loglik(E[idx], U, V[idx], const=False)
    finally:
        e2.close()
    full.append((time.perf_counter() - t0) * 1e3)
out["c_full_route"] = {"ms_per_replicate": stats(full), "EXTRAPOLATED_ms_for_R": round(float(np.median(full)) * R, 1)}
# (d) useful FLOP/s of the products beside the bare MFMA loop
flop = 2.0 * N * G * R * (C + 1) + 2.0 * N * G * R * C
out["d_products"] = {"useful_flop": flop, "tflops_over_all_kernels": round(flop / (float(np.median(a_kern)) * 1e-3) / 1e12, 2),
                     "tflops_rows_product_alone": round(2.0 * N * G * R * (C + 1) / (float(np.median(a_y)) * 1e-3) / 1e12, 2)}
rate_bin = os.path.join(ROOT, "tools", "mfma_f64_rate.bin")
if os.path.exists(rate_bin):
    out["d_products"]["bare_mfma_loop"] = json.loads(subprocess.run([rate_bin], check=True, capture_output=True, text=True, timeout=120).stdout.strip().splitlines()[-1])
else:
    out["d_products"]["bare_mfma_loop"] = "not measured (tools/mfma_f64_rate.bin is not built)"
text = json.dumps(out, indent=1)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "r17_bootstrap.txt"), "w") as f:
    f.write(text + "\n")
print(text)
