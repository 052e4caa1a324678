"""The piece loop of the 4-bit image's own stream launch (ca_ys_mfma_body<DEPTH, true, true>): how a 64 x 64 piece goes through LDS, in which
order the column products wait for their transposed reads, and how one cell step hands over to the next (psi's digits and the first pieces of
the next step are in flight while the escapes and the flush of this one run; past a strip's last step the loads are out of the resource's
range).  None of this may change a sum: they are exact integers, so the oracle is the same engine on the 1-byte image (variant_off=("y4",))
and the comparison is np.array_equal.  The own launch is forced with variant_on=("y4",).

The inputs are made so that a cell order that is permuted on one side only cannot pass: the counts depend on the cell's index within its
64-step, and psi0 and W are spread over several orders of magnitude (all four base-256 digits of the fixed-point images in use).

Strips are 64 cells (one cell step) wherever cdiv(N, 256) x (segments) fits four blocks per CU, which is every small shape; the last case is
the smallest that gets strips of two steps, where the hand-over between steps runs."""
import numpy as np
import pytest

from tests._cases import eps_for, make_case

pytestmark = pytest.mark.gpu


def _counts(N, G, seed, dtype=np.uint16):
    """y = (n % 64) % 7 + (g % 5) over a random background of 0..2: at most 12, every cell of a 64-step different from its neighbours."""
    rng = np.random.default_rng(seed)
    Y = rng.integers(0, 3, size=(N, G), dtype=np.uint8).astype(dtype)
    Y += ((np.arange(N) % 64) % 7).astype(dtype)[:, None]
    Y += (np.arange(G) % 5).astype(dtype)[None, :]
    return Y


def _spread(rng, shape, top):
    return rng.normal(size=shape) * top * 10.0 ** rng.uniform(-4.0, 0.0, size=shape)


def _bit_identical(Y, C=4, seed=3, n_iter=3):
    """gradients(), n_iter iterations and get_params() of the 4-bit own launch against the 1-byte image, bit for bit."""
    from clonealign_amd.engine import HipEngine
    N, G = Y.shape
    c = make_case(N=8, G=G, C=C, K=1, seed=seed)
    rng = np.random.default_rng(seed)
    kw = dict(Y=Y, L=c["L"], psi0=_spread(rng, (N, 1), 2.0), loc0=c["loc0"], K=1, S=1)
    W0 = _spread(rng, (G, 1), 0.5)
    a = HipEngine(**kw, variant_on=("y4",))
    b = HipEngine(**kw, variant_off=("y4",), variant_on=("y4",))
    try:
        ia, ib = a.info(), b.info()
        assert ia["y_stream_bits"] == 4 and ib["y_stream_bits"] == 8, (ia["y_stream_bits"], ib["y_stream_bits"])
        for e in (a, b):
            e.set("W", W0.reshape(np.asarray(e.get("W")).shape))
        e0 = eps_for(1, G, 5)
        ga, ea = a.gradients(e0)
        gb, eb = b.gradients(e0)
        assert ea == eb, (ea, eb)
        for k in gb:
            assert np.array_equal(ga[k], gb[k]), k
        eps = np.stack([eps_for(1, G, 20 + i)[0] for i in range(2 * n_iter)])[:, None, :]
        ca, cb = a.iterate(n_iter, eps), b.iterate(n_iter, eps)
        assert ca == cb, (ca, cb)
        pa, pb = a.get_params(), b.get_params()
        for k in pb:
            assert np.array_equal(pa[k], pb[k]), k
    finally:
        a.close()
        b.close()


def test_transit_three_steps_last_with_two_rows():
    """130 x 70: three cell steps, the last with 2 live rows; one segment, genes past G padded; the row group's fourth wave has no step."""
    _bit_identical(_counts(130, 70, 1))


def test_transit_single_step_two_segments():
    """64 x 513: one cell step and nothing behind it; the second segment holds one gene."""
    _bit_identical(_counts(64, 513, 2))


def test_transit_escape_loop_beyond_128():
    """1000 x 1030: one 64-cell step with 250 entries >= 15 in one segment (the loop past the 128 entries loaded ahead), 40 in another step,
    none elsewhere."""
    Y = _counts(1000, 1030, 3)
    rng = np.random.default_rng(30)
    pos = rng.choice(64 * 512, 250, replace=False)
    Y[128 + pos // 512, pos % 512] = rng.integers(15, 256, size=250)
    assert (Y[128:192, :512] >= 15).sum() >= 200
    pos = rng.choice(64 * 512, 40, replace=False)
    Y[640 + pos // 512, 512 + pos % 512] = rng.integers(15, 300, size=40)
    _bit_identical(Y)


def test_transit_escapes_at_the_corners():
    """Cell 0 and cell 63 of a step, gene 0 and gene 511 of a segment: 14 (no escape), 15, 16, 255 and 300 (also on the overflow list)."""
    Y = _counts(200, 1030, 4)
    for k, v in enumerate((14, 15, 16, 255, 300)):
        step, seg = k % 3, k % 2
        for n in (64 * step, 64 * step + 63):
            for g in (512 * seg, 512 * seg + 511):
                Y[n, g] = v
    _bit_identical(Y)


def test_transit_waves_without_a_step():
    """300 x 600: the last row group (cells 256 ..) has one wave with 44 live rows and three waves with no step at all."""
    Y = _counts(300, 600, 5)
    Y[299, 599] = 77
    Y[256, 0] = 300
    _bit_identical(Y)


def test_transit_two_step_strips():
    """26306 x 5000, the smallest size with strips of two cell steps (cdiv(N, 256) x 10 segments > four blocks on each of 256 CUs): the
    step-to-step hand-over.  The last row group has a full strip, a strip whose second step has 2 live rows, and two waves with no step.
    Escapes in the first and in the second step of a strip, in the last one's partial step, and more than 128 in one step."""
    N, G = 26306, 5000
    Y = _counts(N, G, 6, dtype=np.uint8)
    rng = np.random.default_rng(60)
    flat = rng.integers(0, N * G, size=N * G // 2000)
    Y.flat[flat] = rng.integers(15, 256, size=flat.size)
    pos = rng.choice(64 * 512, 300, replace=False)
    Y[64 + pos // 512, 1024 + pos % 512] = rng.integers(15, 256, size=300)   # second step of the first strip
    Y[N - 1, :700] = 41                                                      # the last, partial step
    _bit_identical(Y, C=5, n_iter=2)
