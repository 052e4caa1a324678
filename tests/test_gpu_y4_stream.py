"""The 4-bit image's own stream launch (k_ys_mfma<true> / k_ys_mfma_ovf<true>): a cell step's first 128 escape entries are loaded when the
step starts and the rest in a loop; fix(W_g) and fix(psi_n) come from LDS; the column side is summed per step in LDS int64.  Every sum is an
exact integer, so the oracle is the same engine on the 1-byte image (variant_off=("y4",)), compared bit for bit."""
import numpy as np
import pytest

from tests.test_gpu_y4 import _case, _same

pytestmark = pytest.mark.gpu


def _stream_matrix(N, G, seed, dtype):
    """Poisson(0.3) counts with: steps without any escape, one step where about a third of the counts escape (far more entries than the
    128 loaded ahead), one cell whose every gene escapes (a whole segment's worth in one step), scattered escapes elsewhere."""
    rng = np.random.default_rng(seed)
    Y = np.minimum(rng.poisson(0.3, size=(N, G)), 14).astype(np.int64)
    flat = rng.choice(Y.size, Y.size // 500, replace=False)
    Y.flat[flat] = rng.integers(15, 300 if dtype != np.uint8 else 256, size=flat.size)
    Y[64:2048, :] = np.minimum(Y[64:2048, :], 14)                     # whole cell steps (and strips) with no escape
    dense = rng.random((64, G)) < 0.35
    Y[2048:2112][dense] = rng.integers(15, 256, size=int(dense.sum()))   # one step: thousands of entries per segment
    Y[5000, :] = 200                                                  # one cell: every gene of every segment escapes
    Y[N - 3, : G // 2] = 40                                           # and a cell of the last, partial strip
    Y[:, 0] += 1
    Y[0, :] += 1
    return Y.astype(dtype)


def test_y4_stream_multi_step_strips():
    """27001 x 5000: 10 segments, strips of 128 cells (two cell steps each: cdiv(N, 256) x 10 > 4 x 256 CUs, cdiv(N, 512) x 10 is not),
    53 row groups; N is not a multiple of 64, the last row group's third strip ends past N and its fourth starts past it.  u16 counts
    with some above 255: the overflow list's extra blocks ride in the same launch."""
    _same(_case(_stream_matrix(27001, 5000, 31, np.uint16), C=5), n_iter=2)


def test_y4_stream_one_step_strips():
    """Strips of 64 cells (one step each) over many row groups, G not a multiple of the 512-gene segment, u8 counts (no overflow list)."""
    _same(_case(_stream_matrix(6001, 1700, 32, np.uint8)))
