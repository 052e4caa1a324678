"""The one-copy stream's 4-bit loop image (CA_VAR_Y4): min(y, 15) in a nibble, the stored counts from 15 up as their exact excess in an
escape list.  Integer sums are order-free, so every gradient, ELBO and parameter is the 1-byte image's bit for bit: the oracle of every
test here is the same engine with variant_off=("y4",), compared with np.array_equal.  The default picks the 4-bit image for the series
form only; the small shapes here force it (variant_on "y4"), which also runs the stream as its own launch where the sweeps would carry it."""
import numpy as np
import pytest
import scipy.sparse as sps

from tests._cases import eps_for, make_case

pytestmark = pytest.mark.gpu


def _low(N, G, seed, lam=0.4):
    """Counts mostly below 15 (a few escapes), like the benchmark's matrix."""
    rng = np.random.default_rng(seed)
    Y = rng.poisson(lam, size=(N, G)).astype(np.float64)
    flat = rng.choice(Y.size, Y.size // 400, replace=False)
    Y.flat[flat] = rng.integers(15, 300, size=flat.size)
    Y[:, 0] += 1
    Y[0, :] += 1
    return Y


def _case(Y, C=4, seed=3):
    N, G = Y.shape
    c = make_case(N=8, G=G, C=C, K=1, seed=seed)
    rng = np.random.default_rng(seed)
    return dict(Y=Y, L=c["L"], psi0=rng.normal(size=(N, 1)), loc0=c["loc0"], K=1, S=1)


def _same(case, bits=4, n_iter=3, variant_off=(), variant_on=("y4",), info=None, Ymat=None, after=None, b_off=()):
    from clonealign_amd.engine import HipEngine
    G = case["Y"].shape[1]
    kw = dict(case)
    if Ymat is not None:
        kw["Y"] = Ymat
    a = HipEngine(**kw, variant_off=variant_off, variant_on=variant_on)
    b = HipEngine(**kw, variant_off=tuple(variant_off) + ("y4",) + tuple(b_off), variant_on=variant_on)
    try:
        ia, ib = a.info(), b.info()
        assert ia["y_stream_bits"] == bits and ib["y_stream_bits"] == 8, (ia["y_stream_bits"], ib["y_stream_bits"])
        assert ia["y_storage_name"] == "u8" and ia["y_bytes_per_elem"] == 1
        for k, v in (info or {}).items():
            assert ia[k] == v, (k, ia[k])
        e0 = eps_for(1, G, 5)
        ga, ea = a.gradients(e0)
        gb, eb = b.gradients(e0)
        assert ea == eb
        for k in gb:
            assert np.array_equal(ga[k], gb[k]), k
        eps = np.stack([eps_for(1, G, 20 + i)[0] for i in range(2 * n_iter)])[:, None, :]
        ca, cb = a.iterate(n_iter, eps), b.iterate(n_iter, eps)
        assert ca == cb, (ca, cb)
        pa, pb = a.get_params(), b.get_params()
        for k in pb:
            assert np.array_equal(pa[k], pb[k]), k
        for k, v in (after or {}).items():
            assert v(a.info()[k]), (k, a.info()[k])
        return ia
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("N,G", [(4133, 1030), (1000, 333)])
def test_y4_ragged(N, G):
    _same(_case(_low(N, G, N)))


def test_y4_boundary_counts():
    """Counts of exactly 14, 15, 16, 255 and 256 (the last on the > 255 overflow list), a strip with every gene of a segment escaping,
    and strips with no escape at all."""
    N, G = 3000, 1100
    rng = np.random.default_rng(9)
    Y = rng.poisson(0.3, size=(N, G)).astype(np.float64)
    Y[:, 0] += 1
    Y[0, :] += 1
    for v, rows in ((14, slice(10, 40)), (15, slice(40, 70)), (16, slice(70, 100)), (255, slice(100, 130)), (256, slice(130, 160))):
        cols = rng.choice(G, 50, replace=False)
        Y[rows, cols[:, None]] = v
    Y[200, :] = 200                                          # every gene of every segment of one cell escapes
    Y[300:303, :] = rng.integers(15, 1000, size=(3, G))     # and of three more, some above 255
    Y[1000:, :] = np.minimum(Y[1000:, :], 14)               # no escapes in the later strips
    _same(_case(Y))


def test_y4_series_default():
    """The series form picks the 4-bit image by default, and its passes run in the series form."""
    Y = _low(40000, 2100, 1)
    _same(_case(Y, C=5), variant_on=("series",), info={"fwd_series": 1}, after={"series_passes": lambda v: v > 0, "series_fallbacks": lambda v: v == 0})


def test_y4_no_overflow_list():
    """Escapes up to 255 only: no overflow list, the stream's launch without its extra blocks."""
    rng = np.random.default_rng(12)
    Y = rng.poisson(0.4, size=(7000, 2100)).astype(np.float64)
    flat = rng.choice(Y.size, Y.size // 400, replace=False)
    Y.flat[flat] = rng.integers(15, 256, size=flat.size)
    Y[:, 0] += 1
    Y[0, :] += 1
    assert Y.max() <= 255
    _same(_case(Y, C=5), variant_on=("series",), info={"fwd_series": 1})


def test_y4_sweeps_keep_riding():
    """Without the series form the default keeps the 1-byte image riding on the sweep; forced, the 4-bit image's stream is a launch of its own."""
    from clonealign_amd.engine import HipEngine
    Y = _low(33000, 2048, 2)
    case = _case(Y, C=5)
    e = HipEngine(**case, variant_off=("series",))
    try:
        assert (e.info()["y_stream_bits"], e.info()["y_ride"]) == (8, 1)
    finally:
        e.close()
    # (the oracle then runs the same launch sequence: the stream a launch of its own, not riding -- the two place the finishing sums differently)
    _same(case, variant_off=("series",), info={"y_ride": 0}, b_off=("y_ride",))


def test_y4_balanced_sweep_shape():
    """The balanced small-problem sweep carries the 1-byte image by default; forced, the 4-bit image's stream runs beside the plain sweep."""
    from clonealign_amd.engine import HipEngine
    Y = _low(12500, 5000, 4)
    case = _case(Y, C=5)
    e = HipEngine(**case, variant_off=("series",))
    try:
        assert (e.info()["y_stream_bits"], e.info()["fwd_balanced"] >= 1) == (8, True)
    finally:
        e.close()
    _same(case, variant_off=("series",), info={"y_ride": 0}, b_off=("y_ride",))


def test_y4_sparse_csr():
    Y = _low(5000, 1500, 6)
    case = _case(Y)
    _same(case, Ymat=sps.csr_matrix(Y))


def test_y4_pick_rule():
    """More than 1 in 256 stored counts >= 15: the 1-byte image, also in the series form; CA_VARX_Y4 forces the 4-bit one, still exact."""
    rng = np.random.default_rng(8)
    Y = rng.poisson(0.5, size=(3000, 1030)).astype(np.float64)
    flat = rng.choice(Y.size, Y.size // 20, replace=False)
    Y.flat[flat] = rng.integers(15, 255, size=flat.size)
    Y[:, 0] += 1
    Y[0, :] += 1
    from clonealign_amd.engine import HipEngine
    case = _case(Y)
    e = HipEngine(**case, variant_on=("series",))
    try:
        assert (e.info()["y_stream_bits"], e.info()["fwd_series"]) == (8, 1)
    finally:
        e.close()
    _same(case, variant_on=("series", "y4"))
