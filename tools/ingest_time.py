"""Ingestion at the C ABI, from HOST memory: what clonealign() hands over is an N x G column-major double matrix
(R/clonealign.R:212-222; R/inference-tflow.R:355,401,403 re-feed it to every sess$run), here once per fit.

  python tools/ingest_time.py [cells genes clones] [--tag before|after]

For float64 column-major (R), int32 column-major and int32 row-major host matrices of the same counts:
  ca_create (HipEngine(...)) wall time, against the same engine built from a DEVICE pointer (no host bytes to move) -- the
  difference is the ingestion; then ca_run(200) + 20 final ELBOs.  Beside it the box's own copy rates for the same bytes:
  pinned hipMemcpy (the roof of any upload) and pageable hipMemcpy (what a single full-size copy gets).

  python tools/ingest_time.py --sparse [cells genes clones]

The sparse leg (profiles/r07_sparse_ingest.txt): ca_create_sparse of the synth_data.make_problem matrix as CSR (int32 indices; values
in the narrowest exact dtype -- uint8, or uint16 when some count exceeds 255 -- and in float64) and as CSC with int32 indices and float64 values (R's dgCMatrix), against ca_create of the same matrix as float64
column-major (R's dense matrix) and int32 row-major.  Every form must give the same storage and the same 20-iteration trace."""
import argparse
import ctypes
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
import synth_data as synth  # noqa: E402
from clonealign_amd.engine import HipEngine, build_id  # noqa: E402
from clonealign_amd.hostprep import safe_inverse_softplus  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("shape", nargs="*", type=int, default=[100_000, 5_000, 8])
ap.add_argument("--tag", default="")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--sparse", action="store_true")
args = ap.parse_args()
N, G, C = args.shape


def sparse_leg():
    import scipy.sparse as sps
    print(f"== ingest_time --sparse {args.tag}: {N} x {G} x {C}, build {build_id()}")
    prob = synth.make_problem(N, G, C, seed=20240)
    Yh, L = prob["Y"], prob["L"]
    psi0 = np.random.default_rng(1).normal(size=(N, 1))
    csr = sps.csr_matrix(Yh)
    nnz = csr.nnz
    # the narrowest exact value dtype (uint8 when every count is below 256, else uint16: what engine.sparse_counts would pick)
    csr_small = sps.csr_matrix((csr.data.astype(np.uint8 if csr.data.max() <= 255 else np.uint16), csr.indices, csr.indptr), shape=csr.shape)
    csr_f64 = sps.csr_matrix((csr.data.astype(np.float64), csr.indices, csr.indptr), shape=csr.shape)
    csc_f64 = csr_f64.tocsc()
    print(f"nnz {nnz} ({nnz / (N * G) * 100:.1f} % of the counts); max count {int(csr.data.max())}")
    forms = [("dense float64 col-major (R)", np.asfortranarray(Yh.astype(np.float64)), "col"), ("dense int32 row-major", Yh, "row"),
             (f"CSR int32 idx, {csr_small.data.dtype} val", csr_small, "row"), ("CSR int32 idx, float64 val", csr_f64, "row"),
             ("CSC int32 idx, float64 val (dgCMatrix)", csc_f64, "row")]
    ref = None
    for name, Y, lay in forms:
        Lx = np.asfortranarray(L) if lay == "col" else L
        ts, eng = [], None
        for _ in range(args.reps):
            if eng is not None:
                eng.close()
            t0 = time.perf_counter()
            eng = HipEngine(Y, Lx, psi0, None, 1, layout=lay)
            eng.synchronize()
            ts.append(time.perf_counter() - t0)
        if sps.issparse(Y):
            hb = Y.data.nbytes + Y.indices.nbytes + Y.indptr.nbytes
        else:
            hb = Y.nbytes
        tr = eng.run(None, 20, 1e-12)
        st = (eng.info()["y_storage_name"], tr.tolist())
        ref = st if ref is None else ref
        print(f"{name:40s} {hb / 1e9:5.2f} GB host: ca_create{'_sparse' if sps.issparse(Y) else ''} {min(ts) * 1e3:7.1f} ms "
              f"(median {float(np.median(ts)) * 1e3:.1f}); storage {st[0]}; same 20-iteration trace as the first form: {st == ref}")
        eng.close()


if args.sparse:
    sparse_leg()
    sys.exit(0)
print(f"== ingest_time {args.tag}: {N} x {G} x {C}, build {build_id()}")
Yd, aux = synth.make_problem_torch(N, G, C, seed=20243, device="cuda:0")
rm = Yd.sum(1, keepdim=True).to(torch.float64) / G
col = torch.zeros(G, dtype=torch.float64, device="cuda:0")
for b0 in range(0, N, 8192):
    col += (Yd[b0:b0 + 8192].to(torch.float64) / rm[b0:b0 + 8192]).sum(0)
loc0 = safe_inverse_softplus(np.maximum(col.cpu().numpy() / N, 1e-6))
psi0 = np.random.default_rng(1).normal(size=(N, 1))
Yh = Yd.cpu().numpy()                                   # int32 row-major
forms = {
    "float64 col-major (R)": (np.asfortranarray(Yh.astype(np.float64)), "col"),
    "int32 col-major": (np.asfortranarray(Yh), "col"),
    "int32 row-major": (Yh, "row"),
}

# --- the box's copy rates for these byte counts
def rate(host_t, reps=3):
    dev = torch.empty_like(host_t, device="cuda:0")
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev.copy_(host_t, non_blocking=True)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return host_t.numel() * host_t.element_size() / min(ts) / 1e9, min(ts) * 1e3


for nbytes in (N * G * 4, N * G * 8):
    pg = torch.empty(nbytes // 4, dtype=torch.int32)
    pg.fill_(1)
    t0 = time.perf_counter()
    pn = torch.empty(nbytes // 4, dtype=torch.int32).pin_memory()
    t_pin = time.perf_counter() - t0
    pn.fill_(1)
    r_pin, ms_pin = rate(pn)
    r_pg, ms_pg = rate(pg)
    print(f"{nbytes / 1e9:.1f} GB: pinned copy {r_pin:6.1f} GB/s ({ms_pin:6.1f} ms; pinning the buffer itself took {t_pin * 1e3:.0f} ms)   "
          f"pageable copy {r_pg:6.1f} GB/s ({ms_pg:6.1f} ms)")
    del pg, pn

# --- the engine from a device pointer: everything but the host bytes
def build(**kw):
    ts, eng = [], None
    for _ in range(args.reps):
        if eng is not None:
            eng.close()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng = HipEngine(**kw)
        eng.synchronize()
        ts.append(time.perf_counter() - t0)
    return eng, min(ts) * 1e3, float(np.median(ts)) * 1e3


eng, t_dev, t_dev_med = build(Y=None, L=aux["L"], psi0=psi0, loc0=loc0, K=1, y_device_ptr=Yd.data_ptr(), y_device_dtype=np.int32, shape=(N, G))
ref = None
print(f"ca_create from a DEVICE int32 pointer: {t_dev:7.1f} ms (median {t_dev_med:.1f}) -- scan + conversion + fit constants, no host bytes")
eng.close()
for name, (Y, lay) in forms.items():
    L = np.asfortranarray(aux["L"]) if lay == "col" else aux["L"]
    eng, t_min, t_med = build(Y=Y, L=L, psi0=psi0, loc0=loc0, K=1, layout=lay)
    gb = Y.nbytes / 1e9
    t0 = time.perf_counter()
    tr = eng.run(None, 200, 1e-6)
    fin = eng.final_elbo(None, 20)
    t_fit = (time.perf_counter() - t0) * 1e3
    st = (tr[-1], eng.get("mu")[:4].tolist())
    if ref is None:
        ref = st
    same = st[0] == ref[0] and st[1] == ref[1]
    print(f"{name:24s} {gb:4.1f} GB host: ca_create {t_min:7.1f} ms (median {t_med:.1f}) = {gb / (t_min * 1e-3):5.1f} GB/s of host bytes end to end; "
          f"ingestion over the device-pointer build {t_min - t_dev:7.1f} ms = {gb / max((t_min - t_dev) * 1e-3, 1e-9):5.1f} GB/s;  "
          f"ca_run(200) + 20 final ELBOs {t_fit:6.1f} ms; storage {eng.info()['y_storage_name']}; same fit as the first form: {same}")
    eng.close()
