"""Time of the two post-fit sweeps over the resident count matrix, ca_logexpr_sums and ca_fit_mse, in one process.
   python tools/logexpr_time.py [cells genes clones repeats logmean]      (default 100000 5000 8 7 -2.7: u8 storage, 80 % zeros, an overflow list;
   logmean -2.2 gives 71 % zeros)

Kernel time: the engine's own profile (HIP events around the sweep's launch, kernel class "ypass"); call time: a host clock around the whole call, which
ends in a device synchronise (list building, uploads, the prepare and finishing launches and the read-back included).  Two warm-up calls of each,
then ``repeats`` timed calls, alternating the two; medians are reported, and the stored bytes of the matrix over the kernel time."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clonealign_amd.engine import HipEngine  # noqa: E402

N, G, C, reps = (int(a) for a in (sys.argv[1:5] + ["100000", "5000", "8", "7"][len(sys.argv) - 1:])[:4])
logmean = float(sys.argv[5]) if len(sys.argv) > 5 else -2.7
rng = np.random.default_rng(7)
L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
mu = rng.lognormal(logmean, 1.0, G)                                # -2.7: 80 % zeros, like the benchmark matrix
z = rng.integers(0, C, N)
Y = np.empty((N, G), dtype=np.int32)
for lo in range(0, N, 10_000):
    Y[lo:lo + 10_000] = rng.poisson(mu[None, :] * L[:, z[lo:lo + 10_000]].T)
Y[:, 0] += 1
hot = rng.choice(N * G, 5000, replace=False)
Y.reshape(-1)[hot] = rng.integers(256, 100000, size=hot.size)
zeros = float((Y == 0).mean())
groups = z.astype(np.int32)
groups[rng.choice(N, N // 20, replace=False)] = C                  # an "unassigned" group beside the clones
E = mu[:, None] * L

eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, profile=True)
try:
    info = eng.info()
    calls = {"logexpr_sums": lambda: eng.logexpr_sums(groups, C + 1), "fit_mse": lambda: eng.fit_mse(z.astype(np.int32), E, per_gene=True)}
    for fn in calls.values():
        fn(); fn()
    kern = {k: [] for k in calls}
    wall = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            eng.kernel_times(reset=True)
            t0 = time.perf_counter()
            fn()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            ms, n = eng.kernel_times()["ypass"]
            assert n == 1, n
            kern[k].append(ms)
finally:
    eng.close()
width = {"u8": 1, "u16": 2, "f32": 4}[info["y_storage_name"]]
seg = 64 * 16 // width                                            # columns of one gene segment: a row is padded to whole segments
bytes_stored = N * (-(-G // seg) * seg) * width
out = {"N": N, "G": G, "C": C, "storage": info["y_storage_name"], "zero_fraction": round(zeros, 4), "stored_bytes": bytes_stored, "repeats": reps}
for k in calls:
    km, wm = float(np.median(kern[k])), float(np.median(wall[k]))
    out[k] = {"kernel_ms_median": round(km, 4), "kernel_ms_min_max": [round(min(kern[k]), 4), round(max(kern[k]), 4)], "call_ms_median": round(wm, 3),
              "stored_TB_per_s": round(bytes_stored / (km * 1e-3) / 1e12, 4)}
    if k == "logexpr_sums":
        nz = int((Y[groups >= 0] != 0).sum())
        out[k]["nonzero_counts"] = nz
        out[k]["ns_per_1e3_nonzero"] = round(km * 1e6 / (nz / 1e3), 5)
print(json.dumps(out))
