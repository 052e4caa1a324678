"""Where a pass of the series form's cell launch (ca_series::k_poly_cell) spends its cycles, from the phase stamps wave 0 of the first 64 cell blocks leaves in a
timing-lab build (CA_LAB_CELL_PH, tools/lab/ca_lab_hooks.inc):
    make -C clonealign_amd/csrc lab
    CLONEALIGN_HIP_LIB=build_ab/libclonealign_hip_lab.so python tools/cell_stamps.py [--cells N --genes G --clones C] [--variant-off cell_lean,cell_mfma]
One fit, a few iterations, the stamps of the LAST cell launch; shader clock cycles per phase over every stamped pass.  The stamps cost a clock read and a store by
one thread each, so the phases compare between builds of the same stamps, not with a product build's kernel time."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = ("bins: exp and Horner over the gene bins", "powers x^k into LDS", "cell epilogue and d/dF", "wait at the first barrier",
          "gather of the backward moments", "wait at the second barrier")
# CA_VAR_CELL_MFMA: the gather is the wave's own matrix product, a pass has no barrier to wait at (past four bins the slab chain and its two barriers are inside
# the one phase), and the pass ends at stamp 4
PHASES_MFMA = PHASES[:3] + ("moments: the wave's fp64 MFMA gather",)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100_000)
    ap.add_argument("--genes", type=int, default=5_000)
    ap.add_argument("--clones", type=int, default=8)
    ap.add_argument("--variant-off", default="")
    args = ap.parse_args()
    import torch  # noqa: F401  (first: its HIP runtime)
    from clonealign_amd import engine as E
    import synth_data as synth
    from tests._cases import eps_for
    N, G, Cn = args.cells, args.genes, args.clones
    Yd, aux = synth.make_problem_torch(N, G, Cn, seed=20243, device="cuda:0")
    psi0 = np.random.default_rng(1).normal(size=(N, 1))
    loc0 = np.zeros(G) + 0.5
    off = tuple(v for v in args.variant_off.split(",") if v)
    eng = E.HipEngine(None, aux["L"], psi0, loc0, 1, y_device_ptr=Yd.data_ptr(), y_device_dtype=np.int32, shape=(N, G), variant_on=("series",), variant_off=off)
    eps = np.stack([eps_for(1, G, 10 + i) for i in range(12)])
    eng.iterate(5, eps)
    eng.synchronize()
    info = eng.info()
    lib = E.load_library()
    st = np.zeros((64, 8, 8), dtype=np.uint64)
    assert lib.ca_lab_read_cell_stamps(st.ctypes.data_as(C.c_void_p), st.size) == 0
    eng.close()
    print(f"# {N} x {G} x {Cn}; build {E.build_id()}; cell_lean {info['cell_lean']}; cell_mfma {info['cell_mfma']}; series passes {info['series_passes']}; cycles of the shader clock, wave 0 of cell blocks 0..63")
    phases, last = (PHASES_MFMA, 4) if info["cell_mfma"] else (PHASES, 6)
    live = (st[:, :, 0] > 0) & (st[:, :, last] > st[:, :, 0])
    d = np.diff(st.astype(np.int64), axis=2)[:, :, :last]       # [block][pass][phase]
    whole = (st[:, :, last].astype(np.int64) - st[:, :, 0].astype(np.int64))
    print(f"# stamped passes: {int(live.sum())} (passes per block: {sorted(set(live.sum(1).tolist()))})")
    print("# phase: median / mean / p10 / p90 over the stamped passes; then the median per pass index 0, 1, 2, ...")
    for j, nm in enumerate(phases):
        a = d[:, :, j][live]
        per = [int(np.median(d[:, p, j][live[:, p]])) for p in range(8) if live[:, p].any()]
        print(f"{nm:44s} {int(np.median(a)):7d} {a.mean():9.1f} {int(np.percentile(a, 10)):7d} {int(np.percentile(a, 90)):7d}   {per}")
    a = whole[live]
    per = [int(np.median(whole[:, p][live[:, p]])) for p in range(8) if live[:, p].any()]
    print(f"{'whole pass':44s} {int(np.median(a)):7d} {a.mean():9.1f} {int(np.percentile(a, 10)):7d} {int(np.percentile(a, 90)):7d}   {per}")


if __name__ == "__main__":
    main()
