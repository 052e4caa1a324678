"""Time of the log-likelihood sweep over the resident count matrix, ca_clone_loglik, beside ca_fit_mse at the same shape in the same process.
   python tools/clone_loglik_time.py [cells genes clones repeats logmean]      (default 100000 5000 8 7 -2.7: 80 % zeros, an overflow list in u8 storage)

Cases: u8 storage with D = 0 (with and without the lgamma constant) and D = 1, u16 and f32 storage with D = 0, and ca_fit_mse on the u8 engine.
Kernel time: the engine's own profile (HIP events around the launches; the sweep is kernel class "ypass", the contraction Z of D > 0 class "other"); call
time: a host clock around the whole call, which ends in a device synchronise (table building, uploads, the finishing launch and the read-back of N x C
doubles included).  Two warm-up calls of each, then ``repeats`` timed calls, alternating the cases of one engine; medians are reported, the stored bytes of
the matrix over the sweep's time, and the sweep's float64 multiply-adds (cells x genes x table columns) over its time."""
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
Y.reshape(-1)[hot] = rng.integers(256, 60000, size=hot.size)       # (u16 storage holds them too)
zeros = float((Y == 0).mean())
E = mu[:, None] * L
U, V = rng.normal(size=(N, 1)) * 0.5, rng.normal(size=(G, 1)) * 0.3
idx = z.astype(np.int32)


def cols(D):
    n = C + D
    return 8 if n <= 8 else 16 if n <= 16 else 32 * -(-n // 32)


out = {"N": N, "G": G, "C": C, "zero_fraction": round(zeros, 4), "repeats": reps, "cases": {}}
for storage in ("u8", "u16", "f32"):
    eng = HipEngine(Y, L, np.zeros((N, 0)), np.zeros(G), 0, profile=True, y_storage=storage)
    try:
        assert eng.info()["y_storage_name"] == storage
        calls = {f"{storage} D=0": (lambda: eng.clone_loglik(E), 0)}
        if storage == "u8":
            calls["u8 D=0 no const"] = (lambda: eng.clone_loglik(E, const=False), 0)
            calls["u8 D=1"] = (lambda: eng.clone_loglik(E, U, V), 1)
            calls["u8 fit_mse"] = (lambda: eng.fit_mse(idx, E, per_gene=True), None)
        for fn, _ in calls.values():
            fn(); fn()
        kern, other, wall = ({k: [] for k in calls} for _ in range(3))
        for _ in range(reps):
            for k, (fn, _D) in calls.items():
                eng.kernel_times(reset=True)
                t0 = time.perf_counter()
                fn()
                wall[k].append((time.perf_counter() - t0) * 1e3)
                kt = eng.kernel_times()
                assert kt["ypass"][1] == 1, kt
                kern[k].append(kt["ypass"][0])
                other[k].append(kt["other"][0])
    finally:
        eng.close()
    width = {"u8": 1, "u16": 2, "f32": 4}[storage]
    seg = 64 * 16 // width                                        # columns of one gene segment: a row is padded to whole segments
    stored = N * (-(-G // seg) * seg) * width
    for k, (_fn, D) in calls.items():
        km = float(np.median(kern[k]))
        row = {"sweep_ms_median": round(km, 4), "sweep_ms_min_max": [round(min(kern[k]), 4), round(max(kern[k]), 4)],
               "call_ms_median": round(float(np.median(wall[k])), 3), "stored_bytes": stored, "stored_TB_per_s": round(stored / (km * 1e-3) / 1e12, 4)}
        if D is not None:
            row["table_columns"] = cols(D)
            row["fp64_fma_T_per_s"] = round(N * G * cols(D) / (km * 1e-3) / 1e12, 3)
            if D > 0:
                row["contraction_ms_median"] = round(float(np.median(other[k])), 4)
        out["cases"][k] = row
fm = out["cases"]["u8 fit_mse"]["sweep_ms_median"]
for k, row in out["cases"].items():
    row["sweep_over_fit_mse_sweep"] = round(row["sweep_ms_median"] / fm, 3)
print(json.dumps(out, indent=1))
