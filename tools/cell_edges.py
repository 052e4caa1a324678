"""What stands around the passes of the series form's cell launch (ca_series::k_poly_cell): the block-level stamps EVERY block of the launch leaves in a timing-lab
build (CA_LAB_CELL_EDGE, tools/lab/ca_lab_hooks.inc) --
    make -C clonealign_amd/csrc lab
    CLONEALIGN_HIP_LIB=build_ab/libclonealign_hip_lab.so python tools/cell_edges.py [--cells N --genes G --clones C] [--variant-off cell_edge]
One fit, a few iterations, the stamps of the LAST cell launch, on the 100 MHz clock all compute units share (10 ns a tick), relative to the launch's earliest stamp.
Cell blocks: start, first pass begins (head done), last pass ends, return (behind a block barrier of the lab's own).  Finisher blocks (the count-matrix stream's row
jobs, and its column jobs where they ride here): start and return.  The stamps cost a clock read and a store by one thread each: they compare between lab builds
and say which part ends the launch, not what a product build's kernel takes."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TICK_US = 0.01


def _row(name, a):
    a = np.asarray(a, dtype=np.float64) * TICK_US
    return f"{name:34s} median {np.median(a):7.2f}  p90 {np.percentile(a, 90):7.2f}  min {a.min():7.2f}  max {a.max():7.2f}  (us, {a.size} blocks)"


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
    st = np.zeros((4096, 8), dtype=np.uint64)
    assert lib.ca_lab_read_cell_edges(st.ctypes.data_as(C.c_void_p), st.size) == 0
    eng.close()
    st = st.astype(np.int64)
    kind = st[:, 4]
    cell = np.flatnonzero((kind == 1) & (st[:, 3] > 0))
    fin = np.flatnonzero(((kind == 2) | (kind == 3)) & (st[:, 3] > 0))
    t0 = min(st[cell, 0].min(), st[fin, 0].min() if fin.size else st[cell, 0].min())
    print(f"# {N} x {G} x {Cn}; build {E.build_id()}; cell_lean {info['cell_lean']}; cell_mfma {info['cell_mfma']}; cell_edge {info.get('cell_edge', 0)}; "
          f"gene_ride {info['gene_ride']}; series passes {info['series_passes']}; {cell.size} cell blocks, {fin.size} finisher blocks "
          f"({int((kind[fin] == 3).sum())} of column jobs); us on the shared 100 MHz clock")
    ran = cell[st[cell, 2] - st[cell, 1] > 0] if cell.size else cell
    print(_row("head (start -> first pass)", st[cell, 1] - st[cell, 0]))
    print(_row("passes (first begins -> last ends)", st[ran, 2] - st[ran, 1]))
    print(_row("block end (last pass -> return)", st[cell, 3] - st[cell, 2]))
    print(_row("cell block, whole", st[cell, 3] - st[cell, 0]))
    print(_row("cell block start after t0", st[cell, 0] - t0))
    ce = st[cell, 3] - t0
    print(f"cell blocks return: first {ce.min() * TICK_US:.2f} us (block {cell[ce.argmin()]}), last {ce.max() * TICK_US:.2f} us (block {cell[ce.argmax()]})")
    last_blk, last_t, last_kind = cell[ce.argmax()], ce.max(), "cell"
    if fin.size:
        print(_row("finisher block, whole", st[fin, 3] - st[fin, 0]))
        fs, fe = st[fin, 0] - t0, st[fin, 3] - t0
        print(f"finisher blocks: first starts {fs.min() * TICK_US:.2f} us (block {fin[fs.argmin()]}), last starts {fs.max() * TICK_US:.2f} us, "
              f"last returns {fe.max() * TICK_US:.2f} us (block {fin[fe.argmax()]})")
        if fe.max() > last_t:
            last_blk, last_t, last_kind = fin[fe.argmax()], fe.max(), "finisher (column job)" if kind[fin[fe.argmax()]] == 3 else "finisher (row job)"
        print(f"finishers behind the last cell block's return: {(fe.max() - ce.max()) * TICK_US:+.2f} us")
    print(f"the launch ends with block {last_blk} ({last_kind}) at {last_t * TICK_US:.2f} us")


if __name__ == "__main__":
    main()
