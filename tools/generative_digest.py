#!/usr/bin/env python3
"""tools/generative_digest.py -- one SHA-256 per output array of the handle-free generative calls (engine.simulate_counts, engine.predictive_stats,
engine.predictive_moments) over fixed cases, in a fixed order: two builds of the library with the same ABI return the same bits exactly when their outputs
are the same, line for line.
   python tools/generative_digest.py                                   (the tree's library)
   CLONEALIGN_HIP_LIB=build_ab/parent/libclonealign_hip.so python tools/generative_digest.py

The first line is the library's build id.  Then: the seven cases of tests/_simulate_cases.py (simulate_counts at draw = 5; predictive_stats at draw0 = 5,
n_rep = 3, with and without the totals; predictive_moments); one case split in two calls with cell_offset; predictive_moments without factors on a case
that has them (the host path); no cells; and inputs with exactly one fault each -- the code and the message."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _simulate_cases as cases  # noqa: E402
from clonealign_amd import engine  # noqa: E402

MOMENTS = ("cell_mean", "cell_var", "T_mean", "T_var", "T_cum3")


def sha(a):
    if a is None:
        return "none"
    a = np.ascontiguousarray(a)
    return f"{a.dtype.str}{list(a.shape)} " + hashlib.sha256(a.tobytes()).hexdigest()


def emit(case, call, *arrays):
    for i, a in enumerate(arrays):
        print(f"{case} | {call}{'' if len(arrays) == 1 else f'[{i}]'} | {sha(a)}")


def run(case, E, V, U, clone, total, seed, **split):
    emit(case, "simulate_counts", engine.simulate_counts(E, V, U, clone, total, seed, draw=5, **split))
    emit(case, "predictive_stats", *engine.predictive_stats(E, V, U, clone, total, seed, draw0=5, n_rep=3, **split))
    emit(case, "predictive_stats without totals", *engine.predictive_stats(E, V, U, clone, total, seed, draw0=5, n_rep=3, gene_totals=False, **split))
    if not split:
        for name, a in zip(MOMENTS, engine.predictive_moments(E, V, U, clone, total)):
            emit(case, f"predictive_moments.{name}", a)


def refusal(label, call, thunk):
    try:
        thunk()
        print(f"refusal {label} | {call} | no refusal")
    except engine.EngineError as e:
        print(f"refusal {label} | {call} | code {e.code}: {e}")
    except ValueError as e:
        print(f"refusal {label} | {call} | ValueError: {e}")


def refusals():
    """Inputs with exactly one fault each, through every call the fault can reach."""
    E, V, U, clone, total, seed = cases.make("steep")

    def edit(a, at, value):
        a = np.array(a, dtype=np.float64 if a.dtype.kind == "f" else a.dtype)
        a[at] = value
        return a

    faults = [("E negative", dict(E=edit(E, (3, 1), -1.0))), ("E not finite", dict(E=edit(E, (0, 0), np.inf))), ("V not finite", dict(V=edit(V, (2, 1), np.nan))),
              ("U not finite", dict(U=edit(U, (4, 0), np.inf))), ("clone out of range", dict(clone=edit(clone, 2, E.shape[1]))),
              ("clone negative", dict(clone=edit(clone, 0, -1))), ("total negative", dict(total=edit(total, 1, -1))), ("total 2^31", dict(total=edit(total, 1, 2 ** 31))),
              ("a clone without expression", dict(E=edit(E, (slice(None), int(clone[0])), 0.0))), ("33 factors", dict(V=np.zeros((E.shape[0], 33)), U=np.zeros((len(clone), 33)))),
              ("U without V", dict(V=None)), ("E one-dimensional", dict(E=E[:, 0]))]
    for label, kv in faults:
        a = dict(dict(E=E, V=V, U=U, clone=clone, total=total), **kv)
        refusal(label, "simulate_counts", lambda: engine.simulate_counts(seed=seed, **a))
        refusal(label, "predictive_stats", lambda: engine.predictive_stats(seed=seed, n_rep=2, **a))
        refusal(label, "predictive_moments", lambda: engine.predictive_moments(**a))
    a = dict(E=E, V=V, U=U, clone=clone, total=total, seed=seed)
    refusal("draw 2^48", "simulate_counts", lambda: engine.simulate_counts(draw=2 ** 48, **a))
    refusal("cell_offset negative", "simulate_counts", lambda: engine.simulate_counts(cell_offset=-1, **a))
    refusal("cell_offset 2^48", "predictive_stats", lambda: engine.predictive_stats(cell_offset=2 ** 48, **a))
    refusal("n_rep 0", "predictive_stats", lambda: engine.predictive_stats(n_rep=0, **a))
    refusal("draw0 + n_rep above 2^48", "predictive_stats", lambda: engine.predictive_stats(draw0=2 ** 48 - 1, n_rep=2, **a))
    refusal("out of the wrong shape", "simulate_counts", lambda: engine.simulate_counts(out=np.zeros((1, 1), dtype=np.int32), **a))


def main():
    print(f"build id {engine.build_id()}")
    for name in cases.CASES:
        run(name, *cases.make(name))
    E, V, U, clone, total, seed = cases.make("mixed")
    for lo, hi in ((0, 101), (101, len(clone))):
        run(f"mixed cells {lo}:{hi}", E, V, U[lo:hi], clone[lo:hi], total[lo:hi], seed, cell_offset=lo)
    for name, a in zip(MOMENTS, engine.predictive_moments(E, None, None, clone, total)):
        emit("mixed without factors", f"predictive_moments.{name}", a)
    run("no cells", E, V, U[:0], clone[:0], total[:0], seed)
    refusals()


if __name__ == "__main__":
    main()
